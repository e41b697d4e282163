"""Exact ensemble quantiles and the per-step envelope on the device
(cmpc_score_quantiles, cmpc_envelope_*; include/cmpc.h).

  1. cmpc_score_quantiles on a guarded bound record filled from
     tests/quantile_cases.py: equal to the sort of tests/quantile_ref.py and to
     cmpc_quantiles_host bit for bit, for one block, partial waves, several
     blocks and a grid-stride loop's second lap;
  2. levels 0 and 1 against cmpc_score_ensemble's min, max and argmax;
  3. after a closed loop with scores and noise, ClosedLoop.score_quantiles
     against the model on the downloaded record;
  4. the envelope of that loop against numpy on y and u_ctrl downloaded after
     every step; the loop is bit-identical with the envelope on and off;
  5. cmpc_envelope_step alone: B = 1, no levels, no u_control, bound rows;
  6. the refusals.
"""
import functools

import numpy as np
import pytest

import cmpc
import golden_cases as GC
import quantile_cases as QC
import quantile_ref as QR
from test_gpu_noise import LOOP_B, LOOP_N, N_OUT, NAME, SEED, noise_settings
from test_gpu_scores import loop_inputs

pytestmark = pytest.mark.gpu

SENTINEL = np.array([0x5EA1ED0FF1CEB0B0], dtype=np.uint64).view(np.float64)[0]   # a finite double
GUARD = 64


@pytest.fixture(autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()
    yield


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to("cuda:0")


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
    assert np.array_equal(QR.bits(a[:GUARD]), QR.bits(np.full(GUARD, SENTINEL))), "guard below"
    assert np.array_equal(QR.bits(a[GUARD + m:]), QR.bits(np.full(GUARD, SENTINEL))), "guard above"
    return a[GUARD:GUARD + m].copy()


def by_rows(q, dims):
    """Context.score_quantiles' {field: {k: (n_levels, S, rows)}} as {k: (n_levels, len, S)}."""
    out = {}
    for k in ("lo", "hi", "arg", "value"):
        a = np.zeros((next(iter(q.values()))[k].shape[0], cmpc.score_len(dims), dims.S), dtype=q["n"][k].dtype)
        for name, sl in cmpc.score_fields(dims).items():
            a[:, sl, :] = q[name][k].transpose(0, 2, 1)
        out[k] = a
    return out


def assert_equals_model(got, X, levels, finite=None):
    """got {k: (n_levels, len, S)} against the sort of X (len, B, S); on the
    rows `finite` the value is numpy.quantile's bit for bit."""
    ref = QR.model(X, levels)
    assert QR.same(got["lo"], ref["lo"])
    assert QR.same(got["hi"], ref["hi"])
    assert np.array_equal(got["arg"], ref["arg"])
    assert QR.same(got["value"], ref["value"])
    if finite is not None and finite.any():
        want = np.quantile(X[finite], np.asarray(levels), axis=1)
        assert np.array_equal(QR.bits(got["value"][:, finite]), QR.bits(want))


# ---- 1, 2. a bound record ---------------------------------------------------------------

# 16389: past 64 blocks x 256 threads, so the grid-stride loop takes a second lap
@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 257, 16389])
def test_gpu_score_quantiles_on_a_bound_record(B):
    import torch
    cfg = GC.case("coop-par", p=50)[0]
    with cmpc.Context(cfg, B) as ctx:
        dims, S = ctx.dims, cfg.S
        assert S == 2
        n = cmpc.score_len(dims)
        X, finite = QC.record(n, B, S)
        rec = np.ascontiguousarray(X.reshape(n, B * S))
        buf, p = guarded(rec.size, rec)
        ctx.score_enable(N_OUT, Ts=0.05)
        ctx.score_bind(p)
        plans = ctx.download()
        torch.cuda.synchronize()
        calls = QC.LEVEL_CALLS if B <= 257 else (QC.ALL8, (0.95,))
        for levels in calls:
            got = by_rows(ctx.score_quantiles(levels), dims)
            assert_equals_model(got, X, levels, finite)
            host = cmpc.quantiles_host(X, levels)
            for k in ("lo", "hi", "value"):
                assert np.array_equal(QR.bits(got[k]), QR.bits(host[k])), (k, levels)    # NaN canonical on both
            assert np.array_equal(got["arg"], host["arg"]), levels
        # levels 0 and 1 against the ensemble statistics, on the NaN-free rows
        ens = ctx.score_ensemble()
        q = ctx.score_quantiles((0.0, 1.0))
        f_rows = np.flatnonzero(finite)
        for name, sl in cmpc.score_fields(dims).items():
            keep = [r - sl.start for r in f_rows if sl.start <= r < sl.stop]
            assert np.array_equal(q[name]["lo"][0][:, keep], ens[name]["min"][:, keep]), name
            assert np.array_equal(q[name]["lo"][1][:, keep], ens[name]["max"][:, keep]), name
            for r in keep:
                for s in range(S):
                    assert X[sl.start + r, q[name]["arg"][1][s, r], s] == ens[name]["max"][s, r], (name, r, s)
        # the record is only read, and nothing outside it is written
        assert np.array_equal(QR.bits(middle(buf, rec.size)), QR.bits(rec.reshape(-1)))
        for a, b in zip(plans, ctx.download()):
            assert np.array_equal(a, b)
        ctx.score_bind(0)


def test_gpu_score_quantiles_repeat_and_change_levels():
    """The work buffer serves calls with other level counts in any order (its
    layout follows the call's level count; nothing is carried between calls)."""
    cfg = GC.case("coop-par", p=50)[0]
    B = 300
    with cmpc.Context(cfg, B) as ctx:
        dims = ctx.dims
        n = cmpc.score_len(dims)
        X, finite = QC.record(n, B, cfg.S)
        d_rec = dev(X.reshape(-1))
        ctx.score_enable(N_OUT, Ts=0.05)
        ctx.score_bind(d_rec.data_ptr())
        for levels in (QC.ALL8, (0.5,), (0.05, 0.5, 0.95), QC.ALL8, (1.0,)):
            assert_equals_model(by_rows(ctx.score_quantiles(levels), dims), X, levels, finite)
        ctx.score_bind(0)


# ---- 3, 4. the closed loop --------------------------------------------------------------

ENV_STEPS, ENV_RUN = 8, 10
ENV_LEVELS = (0.05, 0.5, 0.95)


@functools.lru_cache(maxsize=None)
def loop_run(envelope, steps):
    """The closed loop of tests/test_gpu_noise.py (LOOP_B scenarios, scores and
    noise on); y and u_ctrl are downloaded after every step.  Read-only."""
    from cmpc.driver import ClosedLoop
    cfg, arr, Kl, x0, u_def, lim, sched, yo = loop_inputs(NAME, LOOP_B, LOOP_N)
    S = cfg.S
    M = cmpc.reference_observer_gain(cfg)
    sigma_y, sigma_u, rho_u = noise_settings(cfg)
    X0, U0 = np.tile(x0, (LOOP_B, 1)), np.tile(u_def, (LOOP_B, 1))
    loop = ClosedLoop(cfg, arr, [M] * S, X0, U0, Kl, y_offset=yo, limits=tuple(lim))
    res = {}
    try:
        loop.set_setpoint_schedule(sched)
        loop.set_noise(SEED, sigma_y, sigma_u, rho_u, scenario0=1000)
        loop.enable_scores(band=np.full((S, cfg.ny), 1e-3))
        if envelope:
            y0 =cmpc.plant_output(cfg.plant, x0)
            # a threshold per channel: the outputs' initial values, 0 for the inputs
            res["thr"] = np.concatenate([np.asarray(y0, dtype=np.float64)[:N_OUT], np.zeros(cfg.nu_tot)])
            loop.enable_envelope(ENV_STEPS, ENV_LEVELS, res["thr"])
        loop.initialize()
        ys, us = [], []
        for _ in range(steps):
            _, y = loop.step()
            ys.append(y.cpu().numpy().copy())
            us.append(loop.u_ctrl.cpu().numpy().copy())
        res["y"], res["u"] = np.stack(ys), np.stack(us)
        res["dims"] = loop.ctx.dims
        res["rec"] = loop.ctx.score_download()
        res["q"] = loop.score_quantiles(QC.ALL8)
        res["q95"] = loop.score_quantiles((0.95,))
        assert np.array_equal(QR.bits(loop.ctx.score_download()), QR.bits(res["rec"]))    # the record is only read
        if envelope:
            res["t"], res["env"] = loop.envelope()
    finally:
        loop.close()
    for a in res.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return res


def test_gpu_score_quantiles_after_the_closed_loop():
    r = loop_run(False, LOOP_N)
    dims = r["dims"]
    rec = r["rec"]
    assert (rec[cmpc.score_fields(dims)["n"]] == LOOP_N).all()                   # (a live record)
    X = rec.reshape(rec.shape[0], dims.B, dims.S)
    finite = np.isfinite(X).all(axis=(1, 2))
    assert finite.all()
    assert_equals_model(by_rows(r["q"], dims), X, QC.ALL8, finite)
    assert_equals_model(by_rows(r["q95"], dims), X, (0.95,), finite)
    assert r["q"]["ise"]["value"].shape == (8, dims.S, dims.ny)
    assert (r["q"]["ise"]["value"][1] > r["q"]["ise"]["value"][0]).any()         # (the ensemble is spread)


def moments_bound(X):
    """tests/test_gpu_noise.py's assert_ensemble bound restated for X (B, C):
    with eps = 2^-52, any order of recursive summation of B terms t has
    |fl(sum t) - sum t| <= (B - 1) eps sum |t|, so against the long-double mean m
      |mean - m| <= dm = (B - 1) eps sum|x| / B + eps |m|;
    the centred sum uses the device's own mean m' = m + delta, |delta| <= dm:
    sum (x - m')^2 = sum (x - m)^2 + B delta^2, each term within 1 +- 2 eps, the
    sum (B - 1) eps of the total, so for var = sum / B
      |var' - var| <= dv = dm^2 + (B + 1) eps (var + dm^2),
    and |sqrt a - sqrt b| <= min(sqrt|a - b|, |a - b| / sqrt b), plus eps std for
    the division and the root.  Returns (m, sd, dm, ds) per column."""
    eps = np.finfo(np.float64).eps
    ld = np.longdouble
    B = X.shape[0]
    Xl = X.astype(ld)
    m = Xl.sum(axis=0) / ld(B)
    var = ((Xl - m[None, :]) ** 2).sum(axis=0) / ld(B)
    dm = ((B - 1) * eps * np.abs(Xl).sum(axis=0) / B + eps * np.abs(m)).astype(np.float64)
    dv = dm ** 2 + (B + 1) * eps * (var.astype(np.float64) + dm ** 2)
    sd = np.sqrt(var)
    sdf = sd.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ds = np.minimum(np.sqrt(dv), np.where(sdf > 0, dv / sdf, np.inf)) + eps * sdf
    return m, sd, dm, ds


def assert_envelope_row(e, k, X, thr, levels):
    """Row k of one group of ClosedLoop.envelope() against X (B, channels)."""
    assert np.array_equal(e["min"][k], X.min(axis=0))
    assert np.array_equal(e["max"][k], X.max(axis=0))
    assert np.array_equal(e["argmax"][k], X.argmax(axis=0))                      # (numpy: the first, the lowest)
    count = (X > thr[None, :]).sum(axis=0) if thr is not None else np.zeros(X.shape[1], np.int64)
    assert np.array_equal(e["count"][k], count)
    m, sd, dm, ds = moments_bound(X)
    err_m = np.abs(e["mean"][k].astype(np.longdouble) - m).astype(np.float64)
    err_s = np.abs(e["std"][k].astype(np.longdouble) - sd).astype(np.float64)
    assert (err_m <= dm).all(), (err_m, dm)
    assert (err_s <= ds).all(), (err_s, ds)
    if len(levels):
        ref = QR.model(X[None], levels)                                          # (n_levels, 1, channels)
        assert QR.same(e["lo"][k], ref["lo"][:, 0])
        assert QR.same(e["hi"][k], ref["hi"][:, 0])
        assert np.array_equal(QR.bits(e["value"][k]), QR.bits(np.quantile(X, np.asarray(levels), axis=0)))


def test_gpu_envelope_of_the_closed_loop():
    r = loop_run(True, ENV_RUN)
    t, env = r["t"], r["env"]
    assert t.shape == (ENV_STEPS,) and np.array_equal(t, np.arange(ENV_STEPS) * 0.05)   # 10 steps, 8 rows
    no = r["y"].shape[2]
    assert no == N_OUT and env["y"]["mean"].shape == (ENV_STEPS, no)
    assert env["u"]["lo"].shape == (ENV_STEPS, len(ENV_LEVELS), r["u"].shape[2])
    for k in range(ENV_STEPS):
        assert_envelope_row(env["y"], k, r["y"][k], r["thr"][:no], ENV_LEVELS)
        assert_envelope_row(env["u"], k, r["u"][k], r["thr"][no:], ENV_LEVELS)
    assert (env["y"]["std"][-1] > 0).any() and (env["u"]["hi"][-1, -1] > env["u"]["lo"][-1, 0]).any()   # (it is spread)


def test_gpu_closed_loop_is_unchanged_by_the_envelope():
    on, off = loop_run(True, ENV_RUN), loop_run(False, LOOP_N)
    for k in ("y", "u"):
        assert np.array_equal(QR.bits(on[k]), QR.bits(off[k][:ENV_RUN])), k


# ---- 5. cmpc_envelope_step alone --------------------------------------------------------

@pytest.mark.parametrize("B", [1, 70])
def test_gpu_envelope_step_alone(B):
    """B = 1; no levels; no u_control (its columns stay zero); steps past t_cap
    are dropped; bound, guarded rows; reset."""
    import torch
    cfg = GC.case("coop-par", p=50)[0]
    nu = cfg.nu_tot
    rng = np.random.default_rng(50 + B)
    with cmpc.Context(cfg, B) as ctx:
        ys = rng.normal(size=(4, B, N_OUT))
        us = rng.integers(0, 3, size=(4, B, nu)).astype(np.float64)              # ties
        d_y, d_u = [dev(a) for a in ys], [dev(a) for a in us]
        thr = np.concatenate([np.zeros(N_OUT), np.ones(nu)])
        # (a) three levels, thresholds, rows bound into a guarded buffer, t_cap = 3 of 4 steps
        ctx.envelope_enable(N_OUT, 3, ENV_LEVELS, thr)
        W = 6 + 2 * len(ENV_LEVELS)
        assert cmpc.envelope_len(ctx.dims, N_OUT, len(ENV_LEVELS)) == (N_OUT + nu) * W
        m = 3 * (N_OUT + nu) * W
        buf, p = guarded(m, np.zeros(m))
        ctx.envelope_bind(p)
        for k in range(4):
            ctx.envelope_step(d_y[k].data_ptr(), d_u[k].data_ptr() if k != 1 else 0)
        torch.cuda.synchronize()
        rows, n = ctx.envelope_download()
        assert n == 3 and rows.shape == (3, N_OUT + nu, W)
        assert np.array_equal(QR.bits(middle(buf, m)), QR.bits(rows.reshape(-1)))
        assert (rows[1, N_OUT:] == 0).all()                                      # step 1 had no u_control
        for k in range(3):
            for X, sl, th in ((ys[k], slice(0, N_OUT), thr[:N_OUT]), (us[k], slice(N_OUT, None), thr[N_OUT:])):
                if k == 1 and sl.start == N_OUT:
                    continue
                a = rows[k, sl]
                e = {s: a[None, :, i] for i, s in enumerate(cmpc._abi.ENSEMBLE_STATS)}
                pairs = a[:, 6:].reshape(a.shape[0], len(ENV_LEVELS), 2)
                e["lo"], e["hi"] = pairs[None, :, :, 0].transpose(0, 2, 1), pairs[None, :, :, 1].transpose(0, 2, 1)
                g = np.array([cmpc.quantile_rank(B, q)[2] for q in ENV_LEVELS]).reshape(1, -1, 1)
                e["value"] = cmpc.quantile_value(e["lo"], e["hi"], g)
                assert_envelope_row(e, 0, X, th, ENV_LEVELS)
        ctx.envelope_bind(0)
        # (b) no levels, no thresholds: the statistics only, in the context's own rows
        ctx.envelope_enable(N_OUT, 2)
        ctx.envelope_step(d_y[0].data_ptr(), d_u[0].data_ptr())
        rows, n = ctx.envelope_download()
        assert n == 1 and rows.shape == (2, N_OUT + nu, 6) and (rows[1] == 0).all()
        e = {s: rows[:1, :, i] for i, s in enumerate(cmpc._abi.ENSEMBLE_STATS)}
        assert_envelope_row(e, 0, np.concatenate([ys[0], us[0]], axis=1), None, ())
        ctx.envelope_reset()
        rows, n = ctx.envelope_download()
        assert n == 0 and (rows == 0).all()
        ctx.envelope_disable()
        with pytest.raises(RuntimeError, match="no envelope is enabled"):
            ctx.envelope_step(d_y[0].data_ptr())


# ---- 6. refusals ------------------------------------------------------------------------

def test_gpu_quantile_and_envelope_refusals():
    cfg = GC.case("coop-par", p=50)[0]
    with cmpc.Context(cfg, 2) as ctx:
        with pytest.raises(RuntimeError, match="scoring is not enabled"):
            ctx.score_quantiles((0.5,))
        with pytest.raises(RuntimeError, match="no envelope is enabled"):
            ctx.envelope_step(dev(np.zeros((2, N_OUT))).data_ptr())
        with pytest.raises(RuntimeError, match="no envelope is enabled"):
            ctx.envelope_download()
        with pytest.raises(RuntimeError, match="t_cap must be"):
            ctx.envelope_enable(N_OUT, 0)
        ctx.envelope_enable(N_OUT, 4, (0.5,))
        with pytest.raises(RuntimeError, match="null y"):
            ctx.envelope_step(0)
        with pytest.raises(RuntimeError, match="not a device allocation"):
            ctx.envelope_bind(np.zeros(4096).ctypes.data)          # host memory
        ctx.score_enable(N_OUT, Ts=0.05)
        with pytest.raises(RuntimeError, match="must be inside"):
            ctx.score_quantiles((0.5, -0.1))
        with pytest.raises(RuntimeError, match="n_levels must be inside"):
            ctx.score_quantiles(np.full(9, 0.5))
        q = ctx.score_quantiles((0.5,))                            # the record after a reset
        assert (q["ise"]["value"] == 0).all() and (q["last_out"]["lo"] == -1).all()
