"""Seeded per-scenario noise and the ensemble statistics on the device
(cmpc_noise_step, cmpc_noise_uniforms, cmpc_score_ensemble; include/cmpc.h,
DESIGN.md §3.17).

  1. device uniforms equal the host's bit for bit (partial waves, B = 1, the
     step and scenario0 edges);
  2. device normals against the long-double model of tests/noise_ref.py, and
     numpy reproducing out and the AR(1) state bit for bit from the device's z;
  3. guard zones around out, w and u; every optional array left out in turn;
  4. a batch of 70 equals the batches of 33 and 37;
  5. the closed loop: bit-identical without noise and with zero sigmas, equal
     to the hand-written loop of tests/noise_loop.py with noise in force,
     reproducible from the seed, and an input disturbance stays unmeasured;
  6. score_ensemble after that run and on synthetic bound records.
"""
import functools

import numpy as np
import pytest

import cmpc
import golden_cases as GC
import noise_ref as R
from noise_loop import NoiseLoop
from test_gpu_scores import loop_inputs

pytestmark = pytest.mark.gpu

SEED = 20261020
SENTINEL = np.array([0x5EA1ED0FF1CEB0B0], dtype=np.uint64).view(np.float64)[0]   # a finite double
GUARD = 64
# The float64 numpy model that forms cos(2 pi u2) is 3.08 units of eps r from
# the long-double model (tests/test_noise.py); a device evaluation is allowed
# 8 x that (DESIGN.md §3.16's margin of a device evaluation over a host one).
# The device's own worst case, MI355X, seed 20261020, step 3, B = 4096, n = 5:
# 1.146 units (the host entry point: 1.141), DESIGN.md §3.17.
DEVICE_UNITS_BOUND = 8 * 3.09


@pytest.fixture(autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()
    yield


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to("cuda:0")


def stream_ptr():
    import torch
    return torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream


def guarded(m, fill=None):
    """A device buffer of GUARD + m + GUARD sentinels; `fill` (m values) goes
    in the middle.  Returns (buffer, address of the middle)."""
    a = np.full(m + 2 * GUARD, SENTINEL)
    if fill is not None:
        a[GUARD:GUARD + m] = np.asarray(fill).reshape(-1)
    t = dev(a)
    return t, t.data_ptr() + 8 * GUARD


def middle(t, m):
    a = t.cpu().numpy()
    assert np.array_equal(R.bits(a[:GUARD]), R.bits(np.full(GUARD, SENTINEL))), "guard below"
    assert np.array_equal(R.bits(a[GUARD + m:]), R.bits(np.full(GUARD, SENTINEL))), "guard above"
    return a[GUARD:GUARD + m].copy()


# ---- 1. uniforms ------------------------------------------------------------------------

@pytest.mark.parametrize("B", [70, 1])
@pytest.mark.parametrize("n", [1, 4, 5, 9])
def test_gpu_uniforms_equal_the_hosts(B, n):
    npair = (n + 1) // 2
    for step in (0, 1, 2 ** 32 - 1):
        for scenario0 in (0, 2 ** 32 - B):
            buf, p = guarded(B * npair * 2)
            key = cmpc.noise_key(SEED, 1, scenario0)
            cmpc.noise_uniforms_ptr(0, stream_ptr(), key, step, B, n, p)
            u = middle(buf, B * npair * 2).reshape(B, npair, 2)
            ref = cmpc.noise_uniforms_host(SEED, step, B, n, stream=1, scenario0=scenario0)
            assert np.array_equal(R.bits(u), R.bits(ref)), (step, scenario0)


def test_gpu_uniforms_tensor_entry_point():
    import torch
    out = torch.zeros(70, 3, 2, dtype=torch.float64, device="cuda:0")
    u = cmpc.noise_uniforms(SEED, 5, out, stream=9, scenario0=100).cpu().numpy()
    assert np.array_equal(R.bits(u), R.bits(cmpc.noise_uniforms_host(SEED, 5, 70, 6, stream=9, scenario0=100)))


# ---- 2. normals and the element update --------------------------------------------------

def test_gpu_normals_against_the_long_double_model():
    import torch
    B, n, step = 4096, 5, 3
    out = torch.zeros(B, n, dtype=torch.float64, device="cuda:0")
    z = cmpc.noise_step(SEED, step, out).cpu().numpy()
    u = cmpc.noise_uniforms_host(SEED, step, B, n)
    z_ld, r = R.normals_ld(u, n)
    units = R.error_units(z, z_ld, r)
    host = R.error_units(cmpc.noise_step_host(SEED, step, B, n), z_ld, r)
    print(f"distance to the long-double model in eps r: device {units:.3f}, host {host:.3f}")
    assert units <= DEVICE_UNITS_BOUND, units
    assert (z[r == 0] == 0).all()


@pytest.mark.parametrize("n", [4, 5])
def test_gpu_element_update_from_the_devices_own_normals(n):
    """Given the device's z, numpy reproduces out and the AR(1) state bit for
    bit over 5 steps (zero sigmas, rho = +-1 and negative zeros among them)."""
    import torch
    B = 70
    rng = np.random.default_rng(11 + n)
    sigma = rng.uniform(0.0, 3.0, (B, n))
    sigma[::5] = 0.0
    rho = rng.uniform(-1.0, 1.0, (B, n))
    rho[1::7], rho[2::7] = 1.0, -1.0
    base = rng.normal(size=(B, n))
    base[::10] = -0.0
    w = rng.normal(size=(B, n))
    w[::5] = 0.0
    d_sigma, d_rho, d_base, d_w = dev(sigma), dev(rho), dev(base), dev(w)
    z_t = torch.zeros(B, n, dtype=torch.float64, device="cuda:0")
    out = torch.zeros(B, n, dtype=torch.float64, device="cuda:0")
    for k in range(5):
        z = cmpc.noise_step(SEED, k, z_t, stream=1, scenario0=7).cpu().numpy()
        o = cmpc.noise_step(SEED, k, out, sigma=d_sigma, base=d_base, stream=1, scenario0=7).cpu().numpy()
        assert np.array_equal(R.bits(o), R.bits(R.step_model(z, sigma, None, None, base)[1])), k
        o = cmpc.noise_step(SEED, k, out, sigma=d_sigma, rho=d_rho, w=d_w, base=d_base, stream=1,
                            scenario0=7).cpu().numpy()
        w, ref = R.step_model(z, sigma, rho, w, base)
        assert np.array_equal(R.bits(d_w.cpu().numpy()), R.bits(w)), k
        assert np.array_equal(R.bits(o), R.bits(ref)), k
        assert np.array_equal(R.bits(o[::5]), R.bits(base[::5])), k       # sigma 0, w 0: base bit for bit


# ---- 3. guard zones, optional arrays, refusals ------------------------------------------

@pytest.mark.parametrize("B", [1, 63, 64, 70])
@pytest.mark.parametrize("n", [4, 5])
def test_gpu_noise_stays_inside_its_buffers(B, n):
    m = B * n
    rng = np.random.default_rng(B * 10 + n)
    sigma, rho, base, w0 = (rng.uniform(0.1, 0.9, m) for _ in range(4))
    d_sigma, d_rho, d_base = dev(sigma), dev(rho), dev(base)
    key = cmpc.noise_key(SEED, 2, 5)
    z = cmpc.noise_step_host(SEED, 4, B, n, stream=2, scenario0=5)
    # every optional array left out in turn (rho out: w is not touched)
    for has_sigma, has_rho, has_base in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)):
        out, p_out = guarded(m)
        wb, p_w = guarded(m, w0)
        cmpc.noise_step_ptr(0, stream_ptr(), key, 4, B, n, d_sigma.data_ptr() if has_sigma else 0,
                            d_rho.data_ptr() if has_rho else 0, p_w, d_base.data_ptr() if has_base else 0, p_out)
        o, w = middle(out, m), middle(wb, m)
        rw, ro = R.step_model(z, sigma.reshape(B, n) if has_sigma else None, rho.reshape(B, n) if has_rho else None,
                              w0.reshape(B, n), base.reshape(B, n) if has_base else None)
        # (the host's z and the device's differ by rounding: compared to 1e-12, the
        # bit-for-bit comparisons are tests 1, 2 and 4)
        np.testing.assert_allclose(o.reshape(B, n), ro, rtol=0, atol=1e-12)
        np.testing.assert_allclose(w.reshape(B, n), rw, rtol=0, atol=1e-12)
        if not has_rho:
            assert np.array_equal(R.bits(w), R.bits(w0))
    u, p_u = guarded(B * ((n + 1) // 2) * 2)
    cmpc.noise_uniforms_ptr(0, stream_ptr(), key, 4, B, n, p_u)
    middle(u, B * ((n + 1) // 2) * 2)


def test_gpu_noise_pointer_refusals():
    import torch
    B, n = 4, 3
    key = cmpc.noise_key(SEED)
    good = torch.zeros(B * n + 1, dtype=torch.float64, device="cuda:0")
    host = np.zeros(B * n)
    with pytest.raises(RuntimeError, match="out is not"):
        cmpc.noise_step_ptr(0, stream_ptr(), key, 0, B, n, 0, 0, 0, 0, host.ctypes.data)
    with pytest.raises(RuntimeError, match="out is not"):
        cmpc.noise_step_ptr(0, stream_ptr(), key, 0, B, n, 0, 0, 0, 0, good.data_ptr() + 4)
    with pytest.raises(RuntimeError, match="sigma is not"):
        cmpc.noise_step_ptr(0, stream_ptr(), key, 0, B, n, host.ctypes.data, 0, 0, 0, good.data_ptr())
    with pytest.raises(RuntimeError, match="w is not"):
        cmpc.noise_step_ptr(0, stream_ptr(), key, 0, B, n, 0, good.data_ptr(), host.ctypes.data, 0, good.data_ptr())
    with pytest.raises(RuntimeError, match="u is not"):
        cmpc.noise_uniforms_ptr(0, stream_ptr(), key, 0, B, n, host.ctypes.data)
    with pytest.raises(RuntimeError, match="no such HIP device"):
        cmpc.noise_step_ptr(10 ** 6, stream_ptr(), key, 0, B, n, 0, 0, 0, 0, good.data_ptr())
    with pytest.raises(ValueError, match="contiguous float64"):
        cmpc.noise_step(SEED, 0, good[:B * n].view(B, n), sigma=torch.zeros(B, n, device="cuda:0"))
    cmpc.noise_step_ptr(0, stream_ptr(), key, 0, B, n, 0, 0, 0, 0, good.data_ptr() + 8)
    torch.cuda.synchronize()


# ---- 4. split invariance ----------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 4])
def test_gpu_split_invariance(n):
    import torch
    rng = np.random.default_rng(5)
    sigma, rho = rng.uniform(0.1, 2.0, (70, n)), rng.uniform(-0.95, 0.95, (70, n))
    base = rng.normal(size=(70, n))
    parts = ((0, 70), (0, 33), (33, 70))
    d = [dict(sigma=dev(sigma[a:b]), rho=dev(rho[a:b]), base=dev(base[a:b]),
              w=torch.zeros(b - a, n, dtype=torch.float64, device="cuda:0"),
              out=torch.zeros(b - a, n, dtype=torch.float64, device="cuda:0"),
              u=torch.zeros(b - a, (n + 1) // 2, 2, dtype=torch.float64, device="cuda:0")) for a, b in parts]
    for k in range(5):
        o, w, u = [], [], []
        for (a, _), t in zip(parts, d):
            o.append(cmpc.noise_step(SEED, k, t["out"], sigma=t["sigma"], rho=t["rho"], w=t["w"], base=t["base"],
                                     stream=1, scenario0=a).cpu().numpy())
            w.append(t["w"].cpu().numpy())
            u.append(cmpc.noise_uniforms(SEED, k, t["u"], stream=1, scenario0=a).cpu().numpy())
        for whole, first, second in (o, w, u):
            assert np.array_equal(R.bits(whole), R.bits(np.concatenate([first, second]))), k


# ---- 5. the closed loop -----------------------------------------------------------------

NAME, LOOP_B, LOOP_N = "coop-par", 6, 20
N_OUT = 4


def noise_settings(cfg):
    no, ni = N_OUT, len(cmpc.plant_default(cfg.plant)[1])
    rng = np.random.default_rng(31)
    sigma_y = 2e-4 * (1.0 + np.arange(no))
    sigma_u = rng.uniform(1e-3, 4e-3, (LOOP_B, ni))      # per scenario
    sigma_u[:, 1] = 0.0                                  # an input without a disturbance
    rho_u = np.full(ni, 0.8)
    return sigma_y, sigma_u, rho_u


@functools.lru_cache(maxsize=None)
def loop_run(kind, steps=LOOP_N):
    """One closed-loop run (module docstring, 5); returns host records, all
    read-only: y, meas, u (steps, B, .), u_lin at step 0, and for the scored
    run the downloaded record, the ensemble statistics and its thresholds."""
    from cmpc.driver import ClosedLoop
    cfg, arr, Kl, x0, u_def, lim, sched, yo = loop_inputs(NAME, LOOP_B, LOOP_N)
    S = cfg.S
    M = cmpc.reference_observer_gain(cfg)
    sigma_y, sigma_u, rho_u = noise_settings(cfg)
    X0, U0 = np.tile(x0, (LOOP_B, 1)), np.tile(u_def, (LOOP_B, 1))
    res = {}
    if kind == "hand":
        loop = NoiseLoop(cfg, arr, [M] * S, X0, U0, Kl, SEED, sigma_y, sigma_u, rho_u, scenario0=1000, y_offset=yo,
                         limits=tuple(lim), schedule=sched)
        loop.initialize()
        rows = [loop.step() for _ in range(steps)]
        loop.close()
        res["y"], res["meas"], res["u"] = (np.stack([r[i] for r in rows]) for i in range(3))
        res["u_lin0"] = rows[0][3]
    else:
        loop = ClosedLoop(cfg, arr, [M] * S, X0, U0, Kl, y_offset=yo, limits=tuple(lim))
        loop.set_setpoint_schedule(sched)
        if kind == "zero":
            loop.set_noise(SEED, np.zeros(N_OUT), np.zeros_like(sigma_u), rho_u)
        elif kind in ("noise", "again"):
            loop.set_noise(SEED, sigma_y, sigma_u, rho_u, scenario0=1000)
        elif kind == "other seed":
            loop.set_noise(SEED + 1, sigma_y, sigma_u, rho_u, scenario0=1000)
        elif kind == "input only":
            loop.set_noise(SEED, None, sigma_u, rho_u, scenario0=1000)
        else:
            assert kind == "none"
        if kind == "noise":
            loop.enable_scores(band=np.full((S, cfg.ny), 1e-3))
        loop.initialize()
        ys, ms, us = [], [], []
        for k in range(steps):
            _, y = loop.step()
            ys.append(y.cpu().numpy().copy())
            ms.append(None if loop.last_measurement is None else loop.last_measurement.cpu().numpy().copy())
            us.append(loop.u_ctrl.cpu().numpy().copy())
            if k == 0:
                res["u_lin0"] = loop.u_lin.cpu().numpy().copy()
        res["y"], res["u"] = np.stack(ys), np.stack(us)
        res["meas"] = None if ms[0] is None else np.stack(ms)
        if kind == "noise":
            rec = loop.ctx.score_download()
            res["dims"] = loop.ctx.dims
            res["thr"] = np.median(rec, axis=1)                 # (some values above, some equal, some below)
            plans = loop.ctx.download()
            res["ens"] = loop.score_ensemble(res["thr"])
            res["ens0"] = loop.score_ensemble()
            res["rec"] = rec
            assert np.array_equal(R.bits(loop.ctx.score_download()), R.bits(rec))     # the record is only read
            for a, b in zip(plans, loop.ctx.download()):
                assert np.array_equal(a, b)
        loop.close()
    for a in res.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return res


def test_gpu_closed_loop_without_noise_is_unchanged():
    """(a) no set_noise call and set_noise with all sigmas zero: the same y and
    u_ctrl bit for bit (a zero sigma reproduces its base exactly)."""
    a, z = loop_run("none"), loop_run("zero")
    assert a["meas"] is None
    assert np.array_equal(R.bits(a["y"]), R.bits(z["y"]))
    assert np.array_equal(R.bits(a["u"]), R.bits(z["u"]))
    assert np.array_equal(R.bits(z["meas"]), R.bits(z["y"]))


def test_gpu_closed_loop_equals_the_hand_written_loop():
    """(b) y, last_measurement and u_ctrl, bit for bit over the 20 steps."""
    a, h = loop_run("noise"), loop_run("hand")
    for k in ("y", "meas", "u"):
        assert np.array_equal(R.bits(a[k]), R.bits(h[k])), k
    # the noise is there: the measurement differs from y, and the run from the noiseless one
    assert (a["meas"] != a["y"]).all()
    assert not np.array_equal(a["y"], loop_run("none")["y"])


def test_gpu_closed_loop_is_reproducible_from_the_seed():
    """(c) the same seed twice: bit-identical; another seed: another
    measurement at step 0."""
    a, b, c = loop_run("noise"), loop_run("again"), loop_run("other seed", 1)
    for k in ("y", "meas", "u"):
        assert np.array_equal(R.bits(a[k]), R.bits(b[k])), k
    assert (a["meas"][0] != c["meas"][0]).all()
    assert np.array_equal(R.bits(a["y"][0]), R.bits(c["y"][0]))       # (y(x0) is the true output)


def test_gpu_input_disturbance_is_unmeasured():
    """(d) sigma_u only: the controller's linearisation input at step 0 is the
    noiseless run's (its own offset is untouched), while the plant moves."""
    a, d = loop_run("none"), loop_run("input only", 3)
    assert np.array_equal(R.bits(a["u_lin0"]), R.bits(d["u_lin0"]))
    assert np.array_equal(R.bits(a["u"][0]), R.bits(d["u"][0]))
    assert d["meas"] is None
    assert not np.array_equal(a["y"][1], d["y"][1])


def test_gpu_set_noise_argument_refusals():
    from cmpc.driver import ClosedLoop
    cfg, arr, Kl, x0, u_def, lim, sched, yo = loop_inputs(NAME, LOOP_B, LOOP_N)
    M = cmpc.reference_observer_gain(cfg)
    loop = ClosedLoop(cfg, arr, [M] * cfg.S, np.tile(x0, (LOOP_B, 1)), np.tile(u_def, (LOOP_B, 1)), Kl)
    try:
        ni = len(u_def)
        for kw, err, match in ((dict(sigma_y=np.ones(3)), ValueError, "sigma must be"),
                               (dict(sigma_y=-np.ones(N_OUT)), RuntimeError, "sigma must be finite"),
                               (dict(sigma_u=np.ones(ni), rho_u=np.full(ni, 1.5)), RuntimeError, "rho must be"),
                               (dict(rho_u=np.zeros(ni)), ValueError, "rho_u needs sigma_u"),
                               (dict(sigma_y=np.ones(N_OUT), scenario0=2 ** 32 - 1), RuntimeError, "scenario0 \\+ B")):
            with pytest.raises(err, match=match):
                loop.set_noise(SEED, **kw)
            assert loop._noise is None and loop.last_measurement is None      # nothing was allocated
        loop.set_noise(SEED, sigma_y=np.ones(N_OUT))
        assert loop.last_measurement is not None
        loop.set_noise(SEED)
        assert loop._noise is None and loop.last_measurement is None
    finally:
        loop.close()


# ---- 6. score_ensemble ------------------------------------------------------------------

def assert_ensemble(ens, rec, thr, dims):
    """The statistics against the record (len, B*S) on the host.

    min, max, argmax and count are exact in any order of combination: equal to
    numpy's.  mean and std are sums of B terms in some fixed order; with
    eps = 2^-52 (twice the unit roundoff, which covers the second-order terms)
    any order of recursive summation has |fl(sum t) - sum t| <= (B - 1) eps
    sum |t|.  So with the long-double mean m as the reference,
      |mean - m| <= dm = (B - 1) eps sum|x| / B + eps |m|      (the sum, the division).
    The centred sum uses the device's own mean m' = m + delta, |delta| <= dm:
    sum (x - m')^2 = sum (x - m)^2 + B delta^2 exactly, each term carries the
    roundings of its difference and its square (a factor within 1 +- 2 eps),
    and the sum (B - 1) eps of the terms' total, so for var = sum / B
      |var' - var| <= dv = dm^2 + (B + 1) eps (var + dm^2),
    and std = sqrt(var') with |sqrt a - sqrt b| <= min(sqrt|a - b|, |a - b| /
    sqrt b), plus eps std for the division and the root.  No measured constant."""
    eps = np.finfo(np.float64).eps
    ld = np.longdouble
    S, B = dims.S, dims.B
    X = rec.reshape(rec.shape[0], B, S)
    Xl = X.astype(ld)
    m = Xl.sum(axis=1) / ld(B)                                    # (len, S)
    var = ((Xl - m[:, None, :]) ** 2).sum(axis=1) / ld(B)
    dm = ((B - 1) * eps * np.abs(Xl).sum(axis=1) / B + eps * np.abs(m)).astype(np.float64)
    dv = dm ** 2 + (B + 1) * eps * (var.astype(np.float64) + dm ** 2)
    sd = np.sqrt(var).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ds = np.minimum(np.sqrt(dv), np.where(sd > 0, dv / sd, np.inf)) + eps * sd
    count = (X > thr[:, None, None]).sum(axis=1) if thr is not None else np.zeros(m.shape, np.int64)
    for name, sl in cmpc.score_fields(dims).items():
        e = ens[name]
        assert np.array_equal(e["min"], X.min(axis=1)[sl].T), name
        assert np.array_equal(e["max"], X.max(axis=1)[sl].T), name
        assert np.array_equal(e["argmax"], X.argmax(axis=1)[sl].T), name       # (numpy: the first, the lowest)
        assert np.array_equal(e["count"], count[sl].T), name
        err_m = np.abs(e["mean"].astype(ld) - m[sl].T).astype(np.float64)
        err_s = np.abs(e["std"].astype(ld) - np.sqrt(var)[sl].T).astype(np.float64)
        assert (err_m <= dm[sl].T).all(), (name, err_m.max(), dm[sl].max())
        assert (err_s <= ds[sl].T).all(), (name, err_s.max(), ds[sl].max())


def test_gpu_score_ensemble_after_the_closed_loop():
    r = loop_run("noise")
    assert (r["rec"][cmpc.score_fields(r["dims"])["n"]] == LOOP_N).all()             # (a live record)
    assert_ensemble(r["ens"], r["rec"], r["thr"], r["dims"])
    assert_ensemble(r["ens0"], r["rec"], None, r["dims"])
    assert r["ens"]["ise"]["std"].min() > 0 and r["ens"]["ise"]["count"].sum() > 0


@pytest.mark.parametrize("B", [1, 70, 257])
def test_gpu_score_ensemble_on_a_bound_record(B):
    """A synthetic record bound with cmpc_score_bind: S = 2, planted ties of the
    maximum and of the minimum, a planted extreme, thresholds that equal values
    of their rows, a constant row."""
    import torch
    cfg = GC.case("coop-par", p=50)[0]
    with cmpc.Context(cfg, B) as ctx:
        dims, S = ctx.dims, cfg.S
        n = cmpc.score_len(dims)
        rng = np.random.default_rng(100 + B)
        rec = rng.normal(size=(n, B, S)) * 10.0 ** rng.integers(-3, 4, size=(n, 1, 1))
        rec[3] = 7.25                                              # a constant row: std 0, argmax 0
        if B > 1:
            rec[1, [B - 1, B // 2, 5 % B], 0] = 1e6                # ties of the maximum: the lowest wins
            rec[2, [B - 1, 3 % B], 1] = -1e6                       # ties of the minimum
            rec[4, B // 3, 1] = 1e150                              # an extreme
            rec[5, :, 0] = 1e8 + rng.normal(size=B)                # a large mean under a small spread
        thr = rng.normal(size=n)
        thr[6] = rec[6, B // 2, 0]                                 # equal to a value: not counted (x > thr)
        thr[1] = np.inf
        thr[7] = -np.inf
        rec = np.ascontiguousarray(rec.reshape(n, B * S))
        buf, p = guarded(rec.size, rec)
        ctx.score_enable(N_OUT, Ts=0.05)
        ctx.score_bind(p)
        plans = ctx.download()
        torch.cuda.synchronize()
        ens = ctx.score_ensemble(thr)
        ens0 = ctx.score_ensemble()
        assert np.array_equal(R.bits(middle(buf, rec.size)), R.bits(rec.reshape(-1)))     # the record is only read
        for a, b in zip(plans, ctx.download()):
            assert np.array_equal(a, b)
        assert_ensemble(ens, rec, thr, dims)
        assert_ensemble(ens0, rec, None, dims)
        by_name = ctx.score_ensemble({"ise": 0.5})
        f = cmpc.score_fields(dims)
        X = rec.reshape(n, B, S)
        assert np.array_equal(by_name["ise"]["count"], (X[f["ise"]] > 0.5).sum(axis=1).T)
        assert (by_name["iae"]["count"] == 0).all()
        ctx.score_bind(0)


def test_gpu_score_ensemble_needs_scores():
    cfg = GC.case("coop-par", p=50)[0]
    with cmpc.Context(cfg, 2) as ctx:
        with pytest.raises(RuntimeError, match="not enabled"):
            ctx.score_ensemble()
        ctx.score_enable(N_OUT, Ts=0.05)
        with pytest.raises(RuntimeError, match="not a number"):
            ctx.score_ensemble(np.full(cmpc.score_len(ctx.dims), np.nan))
        with pytest.raises(ValueError, match="no score field"):
            ctx.score_ensemble({"nope": 1.0})
        ens = ctx.score_ensemble()                                 # the record after a reset
        assert (ens["last_out"]["max"] == -1).all() and (ens["ise"]["mean"] == 0).all()
