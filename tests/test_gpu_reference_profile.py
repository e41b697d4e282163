"""Per-scenario reference profiles on the device (include/cmpc.h,
cmpc_set_scenario_reference_profile; csrc/refshift.hip).  Marked gpu; runs on
an MI355X.

B = 3 gives 6 (distributed) or 3 (centralized) QP slots: the kernel's one
workgroup of four rows is partly filled, or a second one holds two.  The
bars: f within 1e-11 max|f| of the oracle run on y_ref + dy + dref (the build
tolerance), the shift f_unset - f_profile within 1e-11 max|g| of the oracle's
Su' w (the sweep in numpy sits at 3e-15, test_reference_profile.py; the
subtraction of two f's adds 1e-16 max|f|, about 1e-13 max|g| where the
offsets dy make max|f| a thousand times max|g|; 3.7e-14 measured), H and G
untouched bit for bit."""
import numpy as np
import pytest

import cmpc
import predict_ref as PR
import refprofile_ref as RP
from cmpc._abi import CmpcDims

pytestmark = pytest.mark.gpu
CUS = 256  # MI355X
B = 3
TOL = RP.TOL
SPLIT, FUSED = cmpc._abi.CMPC_STEP_SPLIT, cmpc._abi.CMPC_STEP_FUSED


@pytest.fixture(autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()
    yield


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")   # (a copy: the shared inputs are read-only)


def make_ctx(cfg, arr, nB, lin, u_old, du_old, ws):
    ctx = cmpc.Context(cfg, nB)
    ctx.configure(arr)
    ctx.set_state(u_old, du_old, ws)
    ctx.upload_lin(lin)
    return ctx


# ---- 1. build: every dimension set and build kernel --------------------------------

SETS = [("coop-par", 50, 2, None),     # (11, 3, 2, 2)
        ("coop-par", 17, 2, None),     # ... one partial chunk; the delayed inputs never arrive
        ("ncoop-par", 17, 2, None),    # (11, 2, 2, 2)
        ("cent-par", 50, 2, None),     # (11, 3, 4, 2): nu = 4
        ("ncoop-ser", 50, 2, None),    # (10, 2, 2, 2)
        ("coop-ser", 17, 2, None),     # (10, 4, 2, 2): ny = 4
        ("cent-ser", 50, 2, None),     # (10, 4, 4, 2)
        ("coop-par", 50, 1, None),     # (11, 3, 2, 1)
        ("coop-par", 17, 3, None),     # (11, 3, 2, 3)
        ("ncoop-par", 64, 2, (0, 2, 0, 63))]   # whole chunks; delays 2 and p - 1


def build_available(name, p, m, delays, variant):
    cfg, _, _ = RP.config(name, p, m, delays)
    return not cmpc.plan(CmpcDims.from_config(cfg, B), CUS, build=variant, K=0).build_error


BUILD_PARAMS = [(*c, v) for c in SETS
                for v in (cmpc.CMPC_BUILD_WAVE, cmpc.CMPC_BUILD_ROWS, cmpc.CMPC_BUILD_SPLIT)
                if build_available(*c, v)]


def test_every_wave_set_and_build_kernel_is_covered():
    from test_predict import wave_sets
    seen = {}
    for name, p, m, delays, v in BUILD_PARAMS:
        cfg, _, _ = RP.config(name, p, m, delays)
        seen.setdefault((cfg.ns, cfg.ny, cfg.nu, cfg.m), set()).add(v)
    assert set(seen) == set(wave_sets())
    assert all({cmpc.CMPC_BUILD_WAVE, cmpc.CMPC_BUILD_SPLIT} <= v for v in seen.values())
    assert sum(cmpc.CMPC_BUILD_ROWS in v for v in seen.values()) >= 6


@pytest.mark.parametrize("name,p,m,delays,variant", BUILD_PARAMS)
def test_gpu_build_with_profile_matches_oracle(name, p, m, delays, variant):
    cfg, arr, batch, dref, dy, ora = RP.problem(name, p, m, delays, B)
    nq = B * cfg.S
    assert cmpc.reference_profile_available(CmpcDims.from_config(cfg, B))
    with make_ctx(cfg, arr, B, *batch) as ctx:
        ctx.set_build_variant(variant)
        ctx.set_scenario_reference(dy)
        ctx.build()
        H0, f0, G0 = ctx.download_qp()
        ctx.set_scenario_reference_profile(dref)
        ctx.build()
        assert ctx.last_build_kernel() == variant
        H, f, G = ctx.download_qp()
    assert np.array_equal(H, H0) and np.array_equal(G, G0)
    worst_f = worst_g = 0.0
    for q in range(nq):
        sf, sg = np.abs(ora["f"][q]).max(), np.abs(ora["g"][q]).max()
        worst_f = max(worst_f, np.abs(f[q] - ora["f"][q]).max() / sf)
        worst_g = max(worst_g, np.abs(f0[q] - f[q] - ora["g"][q]).max() / sg)
    print(f"{name} p={p} m={m} delays={delays} build {variant}: f {worst_f:.2e} of max|f|, "
          f"shift {worst_g:.2e} of max|g|")
    for q in range(nq):
        sf, sg = np.abs(ora["f"][q]).max(), np.abs(ora["g"][q]).max()
        assert sg >= 1e5 * TOL * sf   # a missing correction is 1e5 times the bar on f (dy makes f larger here)
        np.testing.assert_allclose(f[q], ora["f"][q], rtol=0, atol=TOL * sf, err_msg=f"slot {q}")
        np.testing.assert_allclose(f0[q] - f[q], ora["g"][q], rtol=0, atol=TOL * sg, err_msg=f"slot {q}")
    late = [c for c in range(cfg.nu) if cfg.delays[c] >= cfg.p]
    if p == 17 and delays is None:
        assert late   # the inputs delayed by 40
    for c in late:
        assert np.array_equal(f[:, c::cfg.nu], f0[:, c::cfg.nu])
    for c in set(range(cfg.nu)) - set(late):
        assert not np.array_equal(f[:, c::cfg.nu], f0[:, c::cfg.nu])


# ---- 2. set, bind, get, clear and refusals ----------------------------------------

def test_gpu_profile_set_bind_get_clear():
    import torch
    cfg, arr, batch, dref, dy, ora = RP.problem("coop-par", 50, 2, None, B)
    nq = B * cfg.S
    const = np.random.default_rng(1).uniform(-0.1, 0.1, (nq, cfg.ny))
    with make_ctx(cfg, arr, B, *batch) as ctx:
        ctx.set_scenario_reference(dy)
        ctx.build()
        H0, f0, G0 = ctx.download_qp()
        with pytest.raises(RuntimeError, match="no reference profile"):
            ctx.get_scenario_reference_profile()
        # all zero: the unset QPs as values
        ctx.set_scenario_reference_profile(np.zeros_like(dref))
        ctx.build()
        Hz, fz, Gz = ctx.download_qp()
        assert np.array_equal(Hz, H0) and np.array_equal(fz, f0) and np.array_equal(Gz, G0)
        # constant over the horizon: the f of dy_ref + c
        ctx.set_scenario_reference_profile(np.ascontiguousarray(np.broadcast_to(const[:, None, :], dref.shape)))
        ctx.build()
        fc = ctx.download_qp()[1]
        ctx.set_scenario_reference_profile(None)
        ctx.set_scenario_reference(dy + const)
        ctx.build()
        fd = ctx.download_qp()[1]
        ctx.set_scenario_reference(dy)
        for q in range(nq):
            np.testing.assert_allclose(fc[q], fd[q], rtol=0, atol=TOL * np.abs(fd[q]).max(), err_msg=f"slot {q}")
            assert np.abs(fc[q] - f0[q]).max() > 1e-6 * np.abs(f0[q]).max()
        # set / get, bind, clear
        ctx.set_scenario_reference_profile(dref)
        assert np.array_equal(ctx.get_scenario_reference_profile(), dref)
        ctx.build()
        fs = ctx.download_qp()[1]
        ctx.set_scenario_reference_profile(None)
        t = dev(dref)
        ctx.bind_scenario_reference_profile(t.data_ptr())
        assert np.array_equal(ctx.get_scenario_reference_profile(), dref)
        ctx.build()
        fb = ctx.download_qp()[1]
        assert np.array_equal(fs, fb) and not np.array_equal(fs, f0)
        ctx.bind_scenario_reference_profile(0)
        with pytest.raises(RuntimeError, match="no reference profile"):
            ctx.get_scenario_reference_profile()
        ctx.build()
        Hc, fcl, Gc = ctx.download_qp()
        assert np.array_equal(Hc, H0) and np.array_equal(fcl, f0) and np.array_equal(Gc, G0)
        # refusals: a NaN (the slot is named), a wrong size, a host pointer,
        # an allocation that ends before the array does, a misaligned pointer
        bad = dref.copy()
        bad[4, 7, 1] = np.nan
        with pytest.raises(RuntimeError, match="slot 4"):
            ctx.set_scenario_reference_profile(bad)
        with pytest.raises(ValueError):
            ctx.set_scenario_reference_profile(dref[:, :-1])
        seg = [s for s in torch.cuda.memory_snapshot()
               if s["address"] <= t.data_ptr() < s["address"] + s["total_size"]]
        assert len(seg) == 1
        tail = seg[0]["address"] + seg[0]["total_size"] - 256   # 256 bytes < nq * p * ny doubles
        for ptr in (bad.ctypes.data, tail, t.data_ptr() + 4):
            with pytest.raises(RuntimeError):
                ctx.bind_scenario_reference_profile(ptr)
        with pytest.raises(RuntimeError, match="no reference profile"):
            ctx.get_scenario_reference_profile()
        ctx.build()
        assert np.array_equal(ctx.download_qp()[1], f0)
        torch.cuda.synchronize()


# ---- 3. step paths -----------------------------------------------------------------

def solve_state(ctx):
    return (*ctx.download(), ctx.get_state()[2])   # du, status, nwsr, ws


@pytest.mark.parametrize("name,nB,flags", [("coop-par", B, 0), ("coop-par", B, cmpc.CMPC_APPLY_MOVE),
                                           ("cent-ser", 300, 0)])   # 300 QPs: the unset AUTO step is fused
def test_gpu_step_with_profile_is_build_plus_iterate(name, nB, flags):
    K = 9
    cfg, arr, batch, dref, dy, _ = RP.problem(name, 50, 2, None, nB)
    fused_unset = bool(cmpc.plan(CmpcDims.from_config(cfg, nB), CUS, K=K).step_fused)
    assert fused_unset == (name == "cent-ser")
    out = []
    for one_call in (True, False):
        with make_ctx(cfg, arr, nB, *batch) as ctx:
            if fused_unset and one_call:
                ctx.step(K, 0)
                assert ctx.last_step_fused() == 1
                ctx.set_state(batch[1], batch[2], batch[3])
            ctx.set_scenario_reference_profile(dref)
            for _ in range(2):
                if one_call:
                    ctx.step(K, flags)
                    assert ctx.last_step_fused() == 0
                else:
                    ctx.build()
                    ctx.iterate(K, flags)
            out.append(solve_state(ctx))
            if one_call:
                ctx.set_step_variant(FUSED)
                with pytest.raises(RuntimeError, match="reference profile is in force"):
                    ctx.step(K, flags)
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert np.abs(out[0][0]).max() > 0


def test_gpu_control_step_with_profile_is_the_three_calls():
    from test_gpu_scenario_config import observer_setup
    K, p, nB = 9, 50, 2
    cfg, arr, rng, x, u, y, M = observer_setup("par", "coop", p, nB, 17)
    nq = nB * cfg.S
    ys = [y * (1 + 3e-4 * rng.normal(size=y.shape)) for _ in range(3)]
    dref = np.ascontiguousarray(rng.uniform(-0.02, 0.02, (nq, p, cfg.ny)))
    assert cmpc.plan(CmpcDims.from_config(cfg, nB), CUS, K=K).control_fused
    out = {}
    for kind in ("one", "three", "unset"):
        with cmpc.Context(cfg, nB, device=0) as ctx:
            ctx.configure(arr)
            ctx.set_state(np.zeros((nq, cfg.nu_tot)), np.zeros((nq, cfg.nV)), np.zeros(nq, np.uint32))
            for s in range(cfg.S):
                ctx.set_observer(s, M[s])
            if kind != "unset":
                ctx.set_scenario_reference_profile(dref)
            tx, tu, tys = dev(x), dev(u), [dev(a) for a in ys]
            ctx.observer_init(tx.data_ptr(), tu.data_ptr(), dev(y).data_ptr())
            ctx.build()
            ctx.init_warmstart()
            res = []
            for t in range(3):
                if kind == "three":
                    ctx.observe_step(tu.data_ptr(), tys[t].data_ptr())
                    ctx.step(K, 0)
                    ctx.observe_apply()
                else:
                    ctx.control_step(tu.data_ptr(), tys[t].data_ptr(), K)
                assert ctx.last_step_fused() == (kind == "unset")
                res.append((*ctx.download(), *ctx.get_state(), ctx.observer_state()))
            out[kind] = res
    for t, (a, b) in enumerate(zip(out["one"], out["three"])):
        for i, (va, vb) in enumerate(zip(a, b)):
            assert np.array_equal(va, vb, equal_nan=True), (t, i)
    assert np.isfinite(out["one"][-1][0]).all()
    assert not np.array_equal(out["one"][-1][0], out["unset"][-1][0])


def test_gpu_solves_with_profile_are_the_documented_ones():
    """cmpc_iterate(1, 0) after a build with a profile: the map-form solve of
    the downloaded H, f, G with the other controllers' last plans, bit for bit."""
    cfg, arr, batch, dref, dy, _ = RP.problem("coop-par", 50, 2, None, B)
    nq, n, nu = B * cfg.S, cfg.nV, cfg.nu
    with make_ctx(cfg, arr, B, *batch) as ctx:
        ctx.set_scenario_reference_profile(dref)
        ctx.build()
        ctx.init_warmstart()
        ctx.iterate(3, 0)
        H, f, G = ctx.download_qp()
        u_old, du_old, ws = ctx.get_state()
        ctx.iterate(1, 0)
        du, status, nwsr = ctx.download()
        ws1 = ctx.get_state()[2]
    lb = np.zeros((nq, n)); ub = np.zeros((nq, n)); lbA = np.zeros((nq, n)); ubA = np.zeros((nq, n))
    for q in range(nq):
        s = q % cfg.S
        for mv in range(cfg.m):
            lb[q, mv * nu:(mv + 1) * nu] = arr.lower[s] - u_old[q, :nu]
            ub[q, mv * nu:(mv + 1) * nu] = arr.upper[s] - u_old[q, :nu]
            lbA[q, mv * nu:(mv + 1) * nu] = arr.rate_lower[s]
            ubA[q, mv * nu:(mv + 1) * nu] = arr.rate_upper[s]
    x, st, nchg, wso, _, _ = cmpc.qp_solve_batch_map(H, f, G, PR.gather_other(cfg, du_old), lb, ub, lbA, ubA, nu, ws)
    assert np.array_equal(x, du) and np.array_equal(st, status) and np.array_equal(nchg, nwsr)
    assert np.array_equal(wso, ws1)
    assert np.abs(du).max() > 0


# ---- 4. predict ---------------------------------------------------------------------

@pytest.mark.parametrize("name", ["coop-par", "cent-ser"])
def test_gpu_predict_honours_the_profile(name):
    cfg, arr, batch, dref, dy, _ = RP.problem(name, 50, 2, None, B)
    lin, u_old = batch[0], batch[1]
    dims = CmpcDims.from_config(cfg, 1)
    L = cmpc.layout_of(dims)
    with make_ctx(cfg, arr, B, *batch) as ctx:
        ctx.set_scenario_reference(dy)
        ctx.set_scenario_reference_profile(dref)
        ctx.build()
        ctx.init_warmstart()
        ctx.step(9, 0)
        H, f, G = ctx.download_qp()
        du = ctx.download()[0]
        d = PR.gather_other(cfg, du)
        ctx.predict()
        Y, J = ctx.download_prediction()
        t0, td = dev(np.zeros_like(du)), dev(d) if d.size else None
        ctx.predict(t0.data_ptr(), td.data_ptr() if td is not None else 0)
        _, J0 = ctx.download_prediction()
        ctx.set_scenario_reference_profile(dref)
        with pytest.raises(RuntimeError, match="reference profile"):
            ctx.predict()
        ctx.build()
        ctx.predict()
    assert np.abs(du).max() > 0 and (J0[:, 1] == 0).all()
    worst = 0.0
    for q in range(du.shape[0]):
        quad = 0.5 * du[q] @ H[q] @ du[q]
        lin_term = (f[q] + (G[q] @ d[q] if cfg.nVo else 0.0)) @ du[q]
        mag = abs(J[q, 0]) + abs(J[q, 1]) + abs(J0[q, 0]) + abs(quad) + abs(lin_term)
        worst = max(worst, abs(J[q, 0] + J[q, 1] - J0[q, 0] - quad - lin_term) / mag)
    print(f"{name}: worst identity error {worst:.2e} of the summed magnitudes")
    assert worst <= TOL   # the bar of test_gpu_predict.py
    Yo, Jo = PR.oracle_batch(cfg, dims, L, arr, lin, u_old, du, d, dy=dy[:, None, :] + dref)
    _, Jn = PR.oracle_batch(cfg, dims, L, arr, lin, u_old, du, d, dy=dy)
    for q in range(du.shape[0]):
        np.testing.assert_allclose(Y[q], Yo[q], rtol=0, atol=TOL * np.abs(Yo[q]).max(), err_msg=f"slot {q}")
        np.testing.assert_allclose(J[q], Jo[q], rtol=TOL, atol=0, err_msg=f"slot {q}")
        assert abs(Jo[q, 0] - Jn[q, 0]) > 1e-6 * Jn[q, 0]   # the profile does move J_track


# ---- 5. slots are independent -------------------------------------------------------

def test_gpu_profile_of_one_scenario_leaves_the_other():
    nB, K = 2, 9
    cfg, arr, batch, dref, _, _ = RP.problem("coop-par", 50, 2, None, nB)
    S = cfg.S
    one = dref.copy()
    one[:S] = 0.0
    out = []
    for prof in (one, None):
        with make_ctx(cfg, arr, nB, *batch) as ctx:
            ctx.set_step_variant(SPLIT)
            if prof is not None:
                ctx.set_scenario_reference_profile(prof)
            ctx.build()
            ctx.init_warmstart()
            ctx.step(K, cmpc.CMPC_APPLY_MOVE)
            ctx.step(K, cmpc.CMPC_APPLY_MOVE)
            out.append((ctx.download_qp()[1], *solve_state(ctx)))
    for a, b in zip(*out):
        assert np.array_equal(a[:S], b[:S])
    assert not np.array_equal(out[0][0][S:], out[1][0][S:]) and not np.array_equal(out[0][1][S:], out[1][1][S:])


# ---- 6. the driver's setpoint schedule ----------------------------------------------

def test_gpu_closed_loop_setpoint_schedule_previews_the_step():
    """B = 2, p = 50, a setpoint step of 0.02 in plant output 3 at schedule
    index t0 = 53 in scenario 1 only.  The window of control step t is
    [t + 1, t + p]: up to t = t0 - p - 1 = 2 the moves are those of the run
    without a schedule, at t = 3 the last horizon row sees the step."""
    import golden_cases as GC
    from cmpc.driver import ClosedLoop
    cfg, setup, arr, g = GC.case("coop-par", p=50)
    nB, n, K, t0, T = 2, 6, g["n_iterations"], 53, 60
    x0, u_def = cmpc.plant_default(cfg.plant)
    M = cmpc.reference_observer_gain(cfg)
    step = np.zeros((nB, T, 4))
    step[1, t0:, 3] = 0.02
    runs = {}
    for kind, sched in (("none", None), ("zero", np.zeros((nB, T, 4))), ("step", step)):
        loop = ClosedLoop(cfg, arr, [M] * cfg.S, np.tile(x0, (nB, 1)), np.tile(u_def, (nB, 1)), K)
        try:
            if sched is not None:
                loop.set_setpoint_schedule(sched)
            loop.initialize()
            res = []
            for k in range(n):
                _, y = loop.step()
                res.append((loop.u_ctrl.cpu().numpy().copy(), y.cpu().numpy().copy()))
                if sched is not None:
                    want = cmpc.scenario_reference_profiles(cfg, RP.schedule_window(sched, k, cfg.p))
                    assert np.array_equal(loop.ctx.get_scenario_reference_profile(), want), k
            runs[kind] = res
            if kind == "step":
                loop.set_setpoint_schedule(None)
                with pytest.raises(RuntimeError, match="no reference profile"):
                    loop.ctx.get_scenario_reference_profile()
        finally:
            loop.close()
    last_before = t0 - cfg.p - 1
    assert 0 <= last_before < n - 1
    for k in range(n):
        for i in range(2):
            assert np.array_equal(runs["zero"][k][i], runs["none"][k][i]), (k, i)
            assert np.array_equal(runs["step"][k][i][0], runs["none"][k][i][0]), (k, i)   # scenario 0
        if k <= last_before:
            assert np.array_equal(runs["step"][k][0][1], runs["none"][k][0][1]), k
    assert not np.array_equal(runs["step"][last_before + 1][0][1], runs["none"][last_before + 1][0][1])
    assert np.isfinite(runs["step"][-1][0]).all()
