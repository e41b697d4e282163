"""Per-scenario setpoints and input limits on the device (include/cmpc.h,
cmpc_set_scenario_reference / cmpc_set_scenario_constraints and their bind
forms).  Marked gpu; runs on an MI355X.

Setpoints: a build with per-slot offsets dy equals, bit for bit, a build
without them from records whose y_prev is y_prev - dy (the identity the
kernels use), and agrees with the oracle run on y_ref + dy within the build
tolerances of test_gpu_parity.py.  Limits: scenarios are independent, so a
batch whose scenarios carry three classes of limits equals, class by class,
three batches that each have one class as their shared cmpc_set_constraints
(that path is pinned to the oracle by test_gpu_parity.py)."""
import dataclasses
import functools

import numpy as np
import pytest

import _oracle as O
import cmpc
import golden_cases as GC
from cmpc._abi import CmpcDims, dptr
from cmpc.configs import reference_setup
from cmpc.synthetic import synthetic_batch

pytestmark = pytest.mark.gpu
CUS = 256  # MI355X


@pytest.fixture(autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()
    yield


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def make_ctx(cfg, arr, B, lin, u_old, du_old, ws):
    ctx = cmpc.Context(cfg, B)
    ctx.configure(arr)
    ctx.set_state(u_old, du_old, ws)
    ctx.upload_lin(lin)
    return ctx


def offsets(rng, y_ref, y_prev):
    """dy uniform in +-0.2 max(|y_ref|, |y_prev|), per slot and output"""
    return rng.uniform(-1.0, 1.0, y_prev.shape) * 0.2 * np.maximum(np.abs(y_ref), np.abs(y_prev))


# ---- 1. build: the shifted-record identity ------------------------------------

BUILD_CASES = [("coop-par", 50),    # ny = 3
               ("ncoop-par", 50),   # ny = 2: the row kernel's unroll of 10
               ("cent-ser", 50),    # ny = 4: the one-QP-per-wave kernel's pre-pass
               ("cent-par", 200)]   # the row kernel's ring lines
B_BUILD = 47                        # 47 or 94 QPs: the row kernel's last group is partial


@functools.lru_cache(maxsize=None)
def build_problem(name, p):
    """batch, offsets, shifted records and the oracle's QPs for y_ref + dy"""
    cfg, setup, arr, _ = GC.case(name, p=p)
    lin, u_old, du_old, ws = synthetic_batch(cfg, B_BUILD, seed=11 + p)
    dims = CmpcDims.from_config(cfg, 1)
    L = cmpc.layout_of(dims)
    nq = B_BUILD * cfg.S
    y_prev = lin[:, L.off_y:L.off_y + cfg.ny]
    y_ref0 = np.stack([arr.y_ref[q % cfg.S].reshape(cfg.p, cfg.ny)[0] for q in range(nq)])
    dy = np.ascontiguousarray(offsets(np.random.default_rng(77 + p), y_ref0, y_prev))
    shifted = lin.copy()
    shifted[:, L.off_y:L.off_y + cfg.ny] = y_prev - dy   # one FP64 subtraction per entry
    Ho, fo, Go = [], [], []
    for q in range(nq):
        s = q % cfg.S
        yr = arr.y_ref[s].reshape(cfg.p, cfg.ny) + dy[q]
        H, f, _, _, G = O.build_qp(dims, lin[q], u_old[q], yr, arr.ywt[s], arr.uwt[s])
        Ho.append(H); fo.append(f); Go.append(G)
    for a in (lin, u_old, du_old, ws, dy, shifted):
        a.setflags(write=False)
    return cfg, arr, (lin, u_old, du_old, ws), dy, shifted, (np.stack(Ho), np.stack(fo), np.stack(Go))


@pytest.mark.parametrize("variant", [cmpc.CMPC_BUILD_WAVE, cmpc.CMPC_BUILD_ROWS, cmpc.CMPC_BUILD_SPLIT])
@pytest.mark.parametrize("name,p", BUILD_CASES)
def test_gpu_build_offsets_equal_shifted_records(name, p, variant):
    cfg, arr, (lin, u_old, du_old, ws), dy, shifted, (Ho, fo, Go) = build_problem(name, p)
    nq = B_BUILD * cfg.S
    with make_ctx(cfg, arr, B_BUILD, lin, u_old, du_old, ws) as ctx:   # never sets offsets
        ctx.set_build_variant(variant)
        ctx.build()
        assert ctx.last_build_kernel() == variant
        H0, f0, G0 = ctx.download_qp()
        ctx.upload_lin(shifted)
        ctx.build()
        Hs, fs, Gs = ctx.download_qp()
    with make_ctx(cfg, arr, B_BUILD, lin, u_old, du_old, ws) as ctx:
        ctx.set_build_variant(variant)
        ctx.set_scenario_reference(dy)
        assert np.array_equal(ctx.get_scenario_reference(), dy)
        ctx.build()
        assert ctx.last_build_kernel() == variant
        H, f, G = ctx.download_qp()
        ctx.set_scenario_reference(None)
        ctx.build()
        Hc, fc, Gc = ctx.download_qp()
    assert np.array_equal(H, Hs) and np.array_equal(f, fs) and np.array_equal(G, Gs)
    assert np.array_equal(Hc, H0) and np.array_equal(fc, f0) and np.array_equal(Gc, G0)
    assert np.array_equal(H, H0) and np.array_equal(G, G0)   # the offset moves f only
    assert all(not np.array_equal(f[q], f0[q]) for q in range(nq))
    # the oracle on y_ref + dy, tolerances of test_gpu_build_matches_oracle
    for q in range(nq):
        sH = np.abs(Ho[q]).max()
        np.testing.assert_allclose(H[q], Ho[q], rtol=0, atol=1e-11 * sH)
        sf = max(np.abs(fo[q]).max(), 1e-300)
        np.testing.assert_allclose(f[q], fo[q], rtol=0, atol=1e-10 * max(sf, 1e-6 * sH))
        if cfg.nVo:
            sG = max(np.abs(Go[q]).max(), 1e-300)
            np.testing.assert_allclose(G[q], Go[q], rtol=0, atol=1e-11 * max(sG, 1e-6 * sH))


# ---- 2. step: three classes of limits in one batch ----------------------------

def class_arrays(arr, k):
    """class 0: the setup's limits; 1: rate limits x 0.25 and the position
    range halved about its middle; 2: rate limits x 4"""
    if k == 0:
        return arr
    if k == 2:
        return dataclasses.replace(arr, rate_lower=arr.rate_lower * 4.0, rate_upper=arr.rate_upper * 4.0)
    mid, half = (arr.lower + arr.upper) / 2.0, (arr.upper - arr.lower) / 4.0
    return dataclasses.replace(arr, lower=mid - half, upper=mid + half, rate_lower=arr.rate_lower * 0.25,
                               rate_upper=arr.rate_upper * 0.25)


def slot_limits(cfg, arr, nq, cls):
    """(lower, upper, rate_lower, rate_upper), each (nq, nu): slot q's class is cls[q]"""
    ca = [class_arrays(arr, k) for k in range(3)]
    pick = lambda name: np.ascontiguousarray(
        np.stack([getattr(ca[cls[q]], name)[q % cfg.S] for q in range(nq)]))
    return pick("lower"), pick("upper"), pick("rate_lower"), pick("rate_upper")


@functools.lru_cache(maxsize=None)
def step_problem(name, B, seed, p=50):
    cfg, setup, arr, _ = GC.case(name, p=p)
    batch = synthetic_batch(cfg, B, seed=seed)
    for a in batch:
        a.setflags(write=False)
    return cfg, arr, batch


def fused_exists(name, B, solve):
    cfg = cmpc.reference_config(name.split("-")[1], name.split("-")[0], p=50)
    pl = cmpc.plan(CmpcDims.from_config(cfg, B), CUS, solve=solve, step=cmpc.CMPC_STEP_FUSED, K=9)
    return bool(pl.step_fused) and not pl.step_error


STEP_PARAMS = [(name, solve, step, init)
               for name in ("coop-par", "cent-ser")
               for solve in (cmpc.CMPC_SOLVE_LANE, cmpc.CMPC_SOLVE_ROWS)
               for step in (cmpc.CMPC_STEP_SPLIT, cmpc.CMPC_STEP_FUSED)
               for init in (True, False)
               if step == cmpc.CMPC_STEP_SPLIT or fused_exists(name, 48, solve)]


def run_steps(cfg, arr, batch, limits, solve, step, init, K=9, steps=3):
    lin, u, du, ws = batch
    out = []
    with make_ctx(cfg, arr, lin.shape[0] // cfg.S, lin, u, du, ws) as ctx:
        if limits is not None:
            ctx.set_scenario_constraints(*limits)
        ctx.set_solve_variant(solve)
        ctx.set_step_variant(step)
        if init:
            ctx.build()
            ctx.init_warmstart()
        for _ in range(steps):
            ctx.step(K, cmpc.CMPC_APPLY_MOVE)
            assert ctx.last_step_fused() == (step == cmpc.CMPC_STEP_FUSED)
            out.append((*ctx.download(), *ctx.get_state()))
    return out


STEP_NAMES = ("du", "status", "nwsr", "u_old", "du_old", "ws")


def assert_classes_equal(mixed, shared, cls, what=STEP_NAMES):
    for k in range(3):
        rows = np.flatnonzero(cls == k)
        for t, (a, b) in enumerate(zip(mixed, shared[k])):
            for name, x, y in zip(what, a, b):
                assert np.array_equal(x[rows], y[rows]), (k, t, name)


@pytest.mark.parametrize("name,solve,step,init", STEP_PARAMS)
def test_gpu_step_with_per_slot_limits(name, solve, step, init):
    """B = 48 scenarios, scenario b in class b % 3, three steps with the first
    move applied, against three contexts with one class each as their shared
    limits.  The limits are active: at least a quarter of class 1's slots end
    with a non-empty working set (the oracle on the CPU: 100 % with the halved
    range, 61 % / 83 % with the rate limits alone), and every status is OK
    (the halved range leaves every QP feasible under the oracle, so class 1
    keeps it)."""
    B = 48
    cfg, arr, batch = step_problem(name, B, 7)
    nq = B * cfg.S
    cls = (np.arange(nq) // cfg.S) % 3
    mixed = run_steps(cfg, arr, batch, slot_limits(cfg, arr, nq, cls), solve, step, init)
    shared = [run_steps(cfg, class_arrays(arr, k), batch, None, solve, step, init) for k in range(3)]
    assert_classes_equal(mixed, shared, cls)
    du, status, nwsr, u_old, du_old, ws = mixed[-1]
    assert all((o[1] == cmpc.CMPC_QP_OK).all() for o in mixed)
    assert (ws[cls == 1] != 0).mean() >= 0.25
    # the classes do differ: class 1's plans are not the setup's
    assert not np.array_equal(du[cls == 1], shared[0][-1][0][cls == 1])


# ---- 3. both features through the one-launch control step ---------------------

CTRL = [0, 3, 4, 7]  # ControlInputIndex of both plants


def observer_setup(plant, ctype, p, B, seed, xs=1e-4, us=1e-3, ms=0.01):
    """operating points near the equilibrium and a small observer gain (as
    test_observer.py's control-step test: the estimate stays where the
    linearisation is finite)"""
    cfg = cmpc.reference_config(plant, ctype, p=p)
    arr = cmpc.controller_arrays(cfg, reference_setup(plant, ctype))
    L = cmpc.layout_of(CmpcDims.from_config(cfg, B))
    rng = np.random.default_rng(seed)
    x0, u0 = O.plant_default(cfg.plant)
    x = x0[None, :] * (1 + xs * rng.normal(size=(B, len(x0))))
    u = np.tile(u0, (B, 1))
    u[:, CTRL] += rng.uniform(-us, us, (B, 4))
    y = np.stack([O.plant_output(cfg.plant, xb) for xb in x])
    M = [ms * rng.normal(size=(L.nobs, y.shape[1])) for _ in range(cfg.S)]
    return cfg, arr, rng, x, u, y, M


@pytest.mark.parametrize("plant,ctype,B", [("par", "coop", 2), ("ser", "cent", 1)])
def test_gpu_control_step_one_launch_equals_three_calls_with_both(plant, ctype, B):
    """cmpc_control_step with offsets and limits set: the one launch (default
    variants) against the three calls (CMPC_STEP_SPLIT), three steps, bit for
    bit; and both do read them (a context without them plans differently)."""
    K, p = 9, 50
    cfg, arr, rng, x, u, y, M = observer_setup(plant, ctype, p, B, 17)
    nq = B * cfg.S
    ys = [y * (1 + 3e-4 * rng.normal(size=y.shape)) for _ in range(3)]
    dy = cmpc.scenario_reference_offsets(cfg, rng.uniform(-0.02, 0.02, (B, 4)))
    # rate limits x 0.25 (the position range stays: the loop starts at u = 0)
    tight = dataclasses.replace(arr, rate_lower=arr.rate_lower * 0.25, rate_upper=arr.rate_upper * 0.25)
    limits = tuple(np.ascontiguousarray(np.tile(getattr(tight, k), (B, 1)))
                   for k in ("lower", "upper", "rate_lower", "rate_upper"))
    assert cmpc.plan(CmpcDims.from_config(cfg, B), CUS, K=K).control_fused
    assert not cmpc.plan(CmpcDims.from_config(cfg, B), CUS, K=K, step=cmpc.CMPC_STEP_SPLIT).control_fused
    out = {}
    for kind in ("one", "three", "unset"):
        with cmpc.Context(cfg, B, device=0) as ctx:
            ctx.configure(arr)
            ctx.set_state(np.zeros((nq, cfg.nu_tot)), np.zeros((nq, cfg.nV)), np.zeros(nq, np.uint32))
            for s in range(cfg.S):
                ctx.set_observer(s, M[s])
            if kind != "unset":
                ctx.set_scenario_reference(dy)
                ctx.set_scenario_constraints(*limits)
            if kind == "three":
                ctx.set_step_variant(cmpc.CMPC_STEP_SPLIT)
            tx, tu, tys = dev(x), dev(u), [dev(a) for a in ys]
            ctx.observer_init(tx.data_ptr(), tu.data_ptr(), dev(y).data_ptr())
            ctx.build()
            ctx.init_warmstart()
            res = []
            for t in range(3):
                ctx.control_step(tu.data_ptr(), tys[t].data_ptr(), K)
                assert ctx.last_step_fused() == (kind != "three")
                res.append((*ctx.download(), *ctx.get_state(), ctx.observer_state()))
            out[kind] = res
    for t, (a, b) in enumerate(zip(out["one"], out["three"])):
        for i, (va, vb) in enumerate(zip(a, b)):
            assert np.array_equal(va, vb, equal_nan=True), (t, i)
    assert np.isfinite(out["one"][-1][0]).all()
    assert not np.array_equal(out["one"][-1][0], out["unset"][-1][0])


# ---- 4. cmpc_get_input and cmpc_coupled_iterate read the per-slot limits ------

def run_get_input(cfg, arr, batch, limits, du_last):
    lin, u, du, ws = batch
    with make_ctx(cfg, arr, lin.shape[0] // cfg.S, lin, u, du, ws) as ctx:
        if limits is not None:
            ctx.set_scenario_constraints(*limits)
        ctx.build()
        ctx.init_warmstart()
        out = []
        for d in du_last:
            cmpc._abi.check(ctx.lib.cmpc_get_input_host(ctx._h, dptr(d), cmpc.CMPC_APPLY_MOVE), "cmpc_get_input_host")
            out.append((*ctx.download(), *ctx.get_state()))
    return out


def test_gpu_get_input_reads_per_slot_limits():
    B = 6
    cfg, arr, batch = step_problem("coop-par", B, 7)
    nq = B * cfg.S
    cls = (np.arange(nq) // cfg.S) % 3
    rng = np.random.default_rng(3)
    du_last = [np.ascontiguousarray(rng.normal(0, 0.05, (nq, cfg.nVo))) for _ in range(2)]
    mixed = run_get_input(cfg, arr, batch, slot_limits(cfg, arr, nq, cls), du_last)
    shared = [run_get_input(cfg, class_arrays(arr, k), batch, None, du_last) for k in range(3)]
    assert_classes_equal(mixed, shared, cls)
    assert not np.array_equal(mixed[-1][0][cls == 1], shared[0][-1][0][cls == 1])


S_TOTAL, B_COUPLED, K_COUPLED = 8, 6, 9   # test_coupled.py's smallest shape


def run_coupled(cfg, arr, batch, limits):
    import torch
    from cmpc.coupled import CoupledRank, synthetic_g_ext
    lin, u_old, _, _ = batch
    n = lin.shape[0]
    with cmpc.Context(cfg, n // cfg.S, device=0) as ctx:
        ctx.configure(arr)
        ctx.set_build_variant(cmpc.CMPC_BUILD_ROWS)
        ctx.set_state(u_old, np.zeros((n, cfg.nV)), np.zeros(n, np.uint32))
        ctx.upload_lin(lin)
        if limits is not None:
            ctx.set_scenario_constraints(*limits)
        ctx.build()
        _, _, Gd = ctx.download_qp()
        Gx = torch.from_numpy(synthetic_g_ext(Gd, S_TOTAL, S_TOTAL, 0)).cuda()
        cr = CoupledRank(ctx, S_TOTAL, S_TOTAL, 0, 1, Gx)
        cr.step(K_COUPLED)
        torch.cuda.synchronize()
        return [(cr.du_local.cpu().numpy(), *ctx.download()[1:], *ctx.get_state())]


def test_gpu_coupled_iterate_reads_per_slot_limits():
    cfg = cmpc.reference_config("par", "coop", p=20)
    arr = cmpc.controller_arrays(cfg, reference_setup("par", "coop"))
    n = B_COUPLED * S_TOTAL
    batch = synthetic_batch(cfg, n // cfg.S, seed=12)
    cls = (np.arange(n) // S_TOTAL) % 3     # a coupled scenario is S_TOTAL adjacent slots
    mixed = run_coupled(cfg, arr, batch, slot_limits(cfg, arr, n, cls))
    shared = [run_coupled(cfg, class_arrays(arr, k), batch, None) for k in range(3)]
    assert_classes_equal(mixed, shared, cls)
    assert not np.array_equal(mixed[-1][0][cls == 1], shared[0][-1][0][cls == 1])


# ---- 5. bind variants, getters and refusals -----------------------------------

def test_gpu_bound_arrays_equal_host_setters():
    import torch
    B = 48
    cfg, arr, batch = step_problem("coop-par", B, 7)
    nq = B * cfg.S
    cls = (np.arange(nq) // cfg.S) % 3
    limits = slot_limits(cfg, arr, nq, cls)
    L = cmpc.layout_of(CmpcDims.from_config(cfg, 1))
    y_prev = batch[0][:, L.off_y:L.off_y + cfg.ny]
    dy = np.ascontiguousarray(0.05 * np.random.default_rng(9).uniform(-1, 1, y_prev.shape) * np.abs(y_prev))
    packed = np.ascontiguousarray(np.stack(limits, axis=1))      # (nq, 4, nu)
    t_dy, t_lim = dev(dy), dev(packed)

    def run(bound):
        lin, u, du, ws = batch
        with make_ctx(cfg, arr, B, lin, u, du, ws) as ctx:
            if bound:
                ctx.bind_scenario_reference(t_dy.data_ptr())
                ctx.bind_scenario_constraints(t_lim.data_ptr())
            else:
                ctx.set_scenario_reference(dy)
                ctx.set_scenario_constraints(*limits)
            assert np.array_equal(ctx.get_scenario_reference(), dy)
            assert all(np.array_equal(a, b) for a, b in zip(ctx.get_scenario_constraints(), limits))
            ctx.build()
            ctx.init_warmstart()
            ctx.step(9, cmpc.CMPC_APPLY_MOVE)
            res = (*ctx.download(), *ctx.get_state(), *ctx.download_qp())
            # unbinding / clearing restores the shared configuration
            if bound:
                ctx.bind_scenario_reference(0)
                ctx.bind_scenario_constraints(0)
            else:
                ctx.set_scenario_reference(None)
                ctx.set_scenario_constraints()
            with pytest.raises(RuntimeError, match="no per-slot"):
                ctx.get_scenario_reference()
            with pytest.raises(RuntimeError, match="no per-slot"):
                ctx.get_scenario_constraints()
        return res

    for a, b in zip(run(True), run(False)):
        assert np.array_equal(a, b)
    torch.cuda.synchronize()


def test_gpu_scenario_setters_refuse_bad_arguments():
    """Bad pointers and values are refused before anything is launched or
    changed: a host pointer, an address on no allocation, an allocation that
    ends before the array does, a misaligned pointer, partial limits, a
    non-finite value and lower > upper (the message names the slot)."""
    import torch
    B = 48
    cfg, arr, batch = step_problem("coop-par", B, 7)
    nq = B * cfg.S
    limits = slot_limits(cfg, arr, nq, np.zeros(nq, dtype=int))
    host = np.zeros(nq * 4 * cfg.nu)
    ok = torch.zeros(nq * 4 * cfg.nu, dtype=torch.float64, device="cuda:0")
    # 256 bytes before the end of the device allocation (a segment of torch's
    # caching allocator) that holds `ok`: either array would run past its end
    seg = [s for s in torch.cuda.memory_snapshot()
           if s["address"] <= ok.data_ptr() < s["address"] + s["total_size"]]
    assert len(seg) == 1
    tail = seg[0]["address"] + seg[0]["total_size"] - 256
    lin, u, du, ws = batch
    with make_ctx(cfg, arr, B, lin, u, du, ws) as ctx:
        ctx.build()
        H0, f0, G0 = ctx.download_qp()
        for bind in (ctx.bind_scenario_reference, ctx.bind_scenario_constraints):
            for bad in (host.ctypes.data, 4096, tail, ok.data_ptr() + 4):
                with pytest.raises(RuntimeError):
                    bind(bad)
        lo, up, rlo, rup = limits
        with pytest.raises(RuntimeError, match="all four"):
            ctx.set_scenario_constraints(lo, None, rlo, rup)
        bad_up = up.copy()
        bad_up[5, 1] = lo[5, 1] - 1.0
        with pytest.raises(RuntimeError, match="slot 5"):
            ctx.set_scenario_constraints(lo, bad_up, rlo, rup)
        bad_r = rlo.copy()
        bad_r[7, 0] = np.nan
        with pytest.raises(RuntimeError, match="slot 7"):
            ctx.set_scenario_constraints(lo, up, bad_r, rup)
        bad_dy = np.zeros((nq, cfg.ny))
        bad_dy[11, 2] = np.inf
        with pytest.raises(RuntimeError, match="slot 11"):
            ctx.set_scenario_reference(bad_dy)
        with pytest.raises(ValueError):
            ctx.set_scenario_reference(np.zeros((nq, cfg.ny + 1)))
        # nothing is in force after the refusals
        with pytest.raises(RuntimeError, match="no per-slot"):
            ctx.get_scenario_reference()
        with pytest.raises(RuntimeError, match="no per-slot"):
            ctx.get_scenario_constraints()
        ctx.build()
        H1, f1, G1 = ctx.download_qp()
        assert np.array_equal(f0, f1) and np.array_equal(H0, H1) and np.array_equal(G0, G1)


# ---- 6. closed loop --------------------------------------------------------------

@pytest.mark.parametrize("name", ["coop-par", "cent-ser"])
def test_gpu_closed_loop_setpoint_offsets_match_oracle(name):
    """B = 4 scenarios from one initial state, 200 instants, one segment; the
    setpoint of plant output 3 offset by [0, +0.02, -0.02, 0].  Scenarios 0
    and 3 are bit-identical; each agrees with an oracle closed loop that has
    y_ref + dy in its arrays within rtol 2e-6, atol 1e-10 (the tolerances of
    test_gpu_closed_loop_scenarios_match_oracle); the offset scenarios leave
    the base one by far more than that (1.6e-2 to 3.6e-2 in the tracked
    outputs under the oracle)."""
    import torch
    from cmpc.driver import ClosedLoop
    from oracle_loop import OracleClosedLoop
    cfg, setup, arr, g = GC.case(name)
    B, n, K = 4, 200, g["n_iterations"]
    x0, u_def = cmpc.plant_default(cfg.plant)
    yo = np.zeros((B, 4))
    yo[:, 3] = [0.0, 0.02, -0.02, 0.0]
    M = cmpc.reference_observer_gain(cfg)
    loop = ClosedLoop(cfg, arr, [M] * cfg.S, np.tile(x0, (B, 1)), np.tile(u_def, (B, 1)), K, y_offset=yo)
    ub = torch.zeros(n, B, 4, dtype=torch.float64, device="cuda")
    yb = torch.zeros(n, B, 4, dtype=torch.float64, device="cuda")
    try:
        loop.initialize()
        for k in range(n):
            _, y = loop.step()
            ub[k].copy_(loop.u_ctrl)
            yb[k].copy_(y)
        _, _, _, st = loop.sim.download()
    finally:
        loop.close()
    assert not st.any(), st
    u, y = ub.cpu().numpy(), yb.cpu().numpy()
    assert np.array_equal(u[:, 0], u[:, 3]) and np.array_equal(y[:, 0], y[:, 3])
    dy = cmpc.scenario_reference_offsets(cfg, yo)
    for b in range(3):
        y_ref = np.stack([arr.y_ref[s] + np.tile(dy[b * cfg.S + s], cfg.p) for s in range(cfg.S)])
        ora = OracleClosedLoop(cfg, dataclasses.replace(arr, y_ref=y_ref), [M] * cfg.S, K)
        for k in range(n):
            yk = ora.step()
            np.testing.assert_allclose(u[k, b], ora.u_ctrl, rtol=2e-6, atol=1e-10, err_msg=f"u {b} {k}")
            np.testing.assert_allclose(y[k, b], yk, rtol=2e-6, atol=1e-10, err_msg=f"y {b} {k}")
    for b in (1, 2):
        assert np.abs(y[-1, b] - y[-1, 0]).max() > 1e-3
