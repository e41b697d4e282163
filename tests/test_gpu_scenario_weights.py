"""Per-scenario weights on the device (include/cmpc.h,
cmpc_set_scenario_weights; the SCW instances of build_wave_body in
csrc/cmpc_kernels.hip, predict.hip, refshift.hip).  Marked gpu; runs on an
MI355X.

The bars: H, f and G within 1e-11 max|.| of the oracle run with the slot's own
weights (the project's build tolerance); against the shared path bit for bit,
because a slot whose block [L_W' | uwt] equals the sub-controller's shared one
goes through the same arithmetic in the same order; the predict identity at
test_gpu_predict.py's 1e-11 of the summed magnitudes."""
import dataclasses

import numpy as np
import pytest

import cmpc
import predict_ref as PR
import refprofile_ref as RP
import weights_ref as WR
from cmpc._abi import CmpcDims
from test_gpu_reference_profile import SETS

pytestmark = pytest.mark.gpu
CUS = 256  # MI355X
B = 3
TOL = WR.TOL
WAVE, ROWS, SPLITB = cmpc.CMPC_BUILD_WAVE, cmpc.CMPC_BUILD_ROWS, cmpc.CMPC_BUILD_SPLIT
FUSED = cmpc._abi.CMPC_STEP_FUSED


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


def with_weights(arr, uwt, ywt):
    """arr with the shared weights replaced (uwt (S, nu, nu), ywt (S, ny, ny))"""
    return dataclasses.replace(arr, uwt=np.ascontiguousarray(uwt), ywt=np.ascontiguousarray(ywt))


# ---- 1. oracle parity: every dimension set --------------------------------------------

def test_every_wave_set_is_covered():
    from test_predict import wave_sets
    seen = {(c.ns, c.ny, c.nu, c.m) for c in (RP.config(n, p, m, d)[0] for n, p, m, d in SETS)}
    assert seen == set(wave_sets())


@pytest.mark.parametrize("name,p,m,delays", SETS)
def test_gpu_build_with_weights_matches_oracle(name, p, m, delays):
    cfg, arr, batch, uwt, ywt, dy, ora = WR.problem(name, p, m, delays, B)
    nq = B * cfg.S
    assert cmpc.scenario_weights_available(CmpcDims.from_config(cfg, B))
    with make_ctx(cfg, arr, B, *batch) as ctx:
        ctx.set_scenario_reference(dy)
        ctx.set_scenario_weights(uwt, ywt)
        ctx.build()
        assert ctx.last_build_kernel() == WAVE
        got = dict(zip("HfG", ctx.download_qp()))
    worst = {k: 0.0 for k in "HfG"}
    for q in range(nq):
        for k in ("HfG" if cfg.nVo else "Hf"):
            worst[k] = max(worst[k], np.abs(got[k][q] - ora[k][q]).max() / np.abs(ora[k][q]).max())
    print(f"{name} p={p} m={m} delays={delays}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for q in range(nq):
        sH = np.abs(ora["H"][q]).max()
        # a build that ignored the slot's weights is 1e5 times the bar away
        assert np.abs(ora["H"][q] - ora["H0"][q]).max() >= 1e5 * TOL * sH, q
        for k in ("HfG" if cfg.nVo else "Hf"):
            np.testing.assert_allclose(got[k][q], ora[k][q], rtol=0, atol=TOL * np.abs(ora[k][q]).max(),
                                       err_msg=f"{k} of slot {q}")


# ---- 2. and 3. bit for bit against the shared path --------------------------------------

def three_weight_sets(cfg, arr, seed):
    rng = np.random.default_rng(seed)
    return [WR.draw_weights(rng, cfg, arr, cfg.S) for _ in range(3)]   # [(uwt (S, ..), ywt (S, ..))]


def per_slot_of(sets, cfg, nq):
    q = np.arange(nq)
    uwt = np.stack([sets[k][0][s] for k, s in zip(q % 3, q % cfg.S)])
    ywt = np.stack([sets[k][1][s] for k, s in zip(q % 3, q % cfg.S)])
    return np.ascontiguousarray(uwt), np.ascontiguousarray(ywt)


def check_bitwise_against_shared(cfg, arr, nB, batch, on_device):
    import torch
    nq = nB * cfg.S
    sets = three_weight_sets(cfg, arr, 5)
    same = dev if on_device else (lambda a: a)
    equal = torch.equal if on_device else np.array_equal
    shared = []
    for uw, yw in sets:
        with make_ctx(cfg, with_weights(arr, uw, yw), nB, *batch) as ctx:
            ctx.set_build_variant(WAVE)
            ctx.build()
            assert ctx.last_build_kernel() == WAVE
            shared.append([same(a) for a in ctx.download_qp()])
    with make_ctx(cfg, arr, nB, *batch) as ctx:
        ctx.set_build_variant(WAVE)
        ctx.build()
        unset = [same(a) for a in ctx.download_qp()]
        ctx.set_build_variant(cmpc.CMPC_BUILD_AUTO)
        ctx.set_scenario_weights(*per_slot_of(sets, cfg, nq))
        ctx.build()
        assert ctx.last_build_kernel() == WAVE
        mixed = [same(a) for a in ctx.download_qp()]
        ctx.set_scenario_weights(*WR.shared_weights(cfg, arr, nq))
        ctx.build()
        alls = [same(a) for a in ctx.download_qp()]
    for k in range(3):
        for i, what in enumerate("HfG"):
            assert equal(mixed[i][k::3], shared[k][i][k::3]), (k, what)
            other = shared[(k + 1) % 3][i][k::3]
            assert not equal(mixed[i][k::3], other), (k, what)   # the classes do differ
    for i, what in enumerate("HfG"):
        assert equal(alls[i], unset[i]), what


def test_gpu_weights_are_bitwise_the_shared_build():
    cfg, arr, batch, *_ = WR.problem("coop-par", 50, 2, None, B)
    check_bitwise_against_shared(cfg, arr, B, batch, on_device=False)


def test_gpu_weights_bitwise_ny4():
    """ny = 4: the free-response pre-pass reads the private yhat table too"""
    cfg, arr, batch, *_ = WR.problem("coop-ser", 17, 2, None, B)
    check_bitwise_against_shared(cfg, arr, B, batch, on_device=False)


def test_gpu_weights_bitwise_in_the_persistent_loop():
    """32 768 QPs, twice the 256 x 8 x 4 waves that can be resident: every wave
    builds several QPs of different weight classes (q mod 3 with q += a
    multiple of 4 waves) and rewrites its private tables in between."""
    from cmpc.synthetic import synthetic_batch
    cfg, arr, _ = RP.config("coop-par", 17)
    nB = 16384
    lin, u_old, du_old, ws = synthetic_batch(cfg, 32, seed=91)   # 64 distinct records
    rep = nB // 32
    batch = (np.tile(lin, (rep, 1)), np.tile(u_old, (rep, 1)), np.tile(du_old, (rep, 1)), np.tile(ws, rep))
    assert batch[0].shape[0] == nB * cfg.S == 32768 >= 2 * CUS * 8 * 4
    check_bitwise_against_shared(cfg, arr, nB, batch, on_device=True)


# ---- 4. predict -------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["coop-par", "cent-ser"])
def test_gpu_predict_identity_with_weights(name):
    cfg, arr, batch, uwt, ywt, dy, _ = WR.problem(name, 50, 2, None, B)
    nq = B * cfg.S
    rng = np.random.default_rng(77)
    du = np.ascontiguousarray(rng.uniform(-0.05, 0.05, (nq, cfg.nV)))
    d = PR.gather_other(cfg, du)
    with make_ctx(cfg, arr, B, *batch) as ctx:
        ctx.set_scenario_reference(dy)
        ctx.set_scenario_weights(uwt, ywt)
        ctx.build()
        H, f, G = ctx.download_qp()
        tdu, t0, td = dev(du), dev(np.zeros_like(du)), dev(d) if d.size else None
        ctx.predict(tdu.data_ptr())
        _, J = ctx.download_prediction()
        ctx.predict(t0.data_ptr(), td.data_ptr() if td is not None else 0)
        _, J0 = ctx.download_prediction()
        ctx.set_scenario_weights(None, None)
        ctx.build()
        ctx.predict(tdu.data_ptr())
        _, Js = ctx.download_prediction()
    assert (J0[:, 1] == 0).all()
    worst = worst_m = 0.0
    for q in range(nq):
        quad = 0.5 * du[q] @ H[q] @ du[q]
        lin_term = (f[q] + (G[q] @ d[q] if cfg.nVo else 0.0)) @ du[q]
        mag = abs(J[q, 0]) + abs(J[q, 1]) + abs(J0[q, 0]) + abs(quad) + abs(lin_term)
        worst = max(worst, abs(J[q, 0] + J[q, 1] - J0[q, 0] - quad - lin_term) / mag)
        dm = du[q].reshape(cfg.m, cfg.nu)
        jm = 0.5 * float(np.einsum("ki,ij,kj->", dm, uwt[q], dm))
        worst_m = max(worst_m, abs(J[q, 1] - jm) / jm)
        assert abs(J[q, 1] - Js[q, 1]) > 1e-6 * Js[q, 1]   # the slot's uwt does move J_move
    print(f"{name}: worst identity error {worst:.2e} of the summed magnitudes, J_move {worst_m:.2e} relative")
    assert worst <= TOL   # the bar of test_gpu_predict.py
    assert worst_m <= TOL


# ---- 5. a reference profile with weights -----------------------------------------------

@pytest.mark.parametrize("name,p", [("coop-par", 50), ("coop-ser", 17)])
def test_gpu_profile_with_weights(name, p):
    cfg, arr, batch, uwt, ywt, dy, _ = WR.problem(name, p, 2, None, B)
    dref = RP.problem(name, p, 2, None, B)[3]
    nq = B * cfg.S
    Ho, fo, Go = WR.oracle_qps(cfg, arr, batch[0], batch[1], uwt, ywt, dy, dref)
    with make_ctx(cfg, arr, B, *batch) as ctx:
        ctx.set_scenario_reference(dy)
        ctx.set_scenario_weights(uwt, ywt)
        ctx.build()
        H0, f0, G0 = ctx.download_qp()
        ctx.set_scenario_reference_profile(dref)
        ctx.build()
        H, f, G = ctx.download_qp()
        ctx.set_scenario_weights(None, None)
        ctx.build()
        fs = ctx.download_qp()[1]
    assert np.array_equal(H, H0) and np.array_equal(G, G0)
    worst = max(np.abs(f[q] - fo[q]).max() / np.abs(fo[q]).max() for q in range(nq))
    print(f"{name} p={p}: f {worst:.2e} of max|f|")
    for q in range(nq):
        sf = np.abs(fo[q]).max()
        np.testing.assert_allclose(f[q], fo[q], rtol=0, atol=TOL * sf, err_msg=f"slot {q}")
        assert np.abs(f[q] - f0[q]).max() > 1e5 * TOL * sf   # the profile moves f,
        assert np.abs(f[q] - fs[q]).max() > 1e5 * TOL * sf   # and so do the slot's weights under it


# ---- 6. set, bind, get, clear and refusals ----------------------------------------------

def test_gpu_weights_set_bind_get_clear():
    import torch
    cfg, arr, batch, uwt, ywt, dy, _ = WR.problem("coop-par", 50, 2, None, B)
    nq = B * cfg.S
    pk = WR.packed(uwt, ywt)
    with make_ctx(cfg, arr, B, *batch) as ctx:
        ctx.build()
        kernel0 = ctx.last_build_kernel()
        qp0 = ctx.download_qp()
        with pytest.raises(RuntimeError, match="no per-slot weights"):
            ctx.get_scenario_weights()
        ctx.set_scenario_weights(uwt, ywt)
        gu, glw = ctx.get_scenario_weights()
        assert np.array_equal(gu, uwt) and np.array_equal(glw.reshape(nq, -1), pk[:, :cfg.ny ** 2])
        ctx.build()
        qps = ctx.download_qp()
        assert ctx.last_build_kernel() == WAVE
        ctx.set_scenario_weights(None, None)
        t = dev(pk)
        ctx.bind_scenario_weights(t.data_ptr())
        gu, glw = ctx.get_scenario_weights()
        assert np.array_equal(gu, uwt) and np.array_equal(glw.reshape(nq, -1), pk[:, :cfg.ny ** 2])
        ctx.build()
        qpb = ctx.download_qp()
        for a, b, c in zip(qps, qpb, qp0):
            assert np.array_equal(a, b) and not np.array_equal(a, c)
        ctx.bind_scenario_weights(0)
        with pytest.raises(RuntimeError, match="no per-slot weights"):
            ctx.get_scenario_weights()
        ctx.build()
        assert ctx.last_build_kernel() == kernel0
        for a, c in zip(ctx.download_qp(), qp0):
            assert np.array_equal(a, c)
        # refusals: the slot is named; one array only; wrong sizes; bad pointers
        bad = ywt.copy()
        bad[4] = np.diag([1.0, -1.0, 1.0])
        with pytest.raises(RuntimeError, match="slot 4.*positive semi-definite"):
            ctx.set_scenario_weights(uwt, bad)
        bad = ywt.copy()
        bad[3, 0, 1] += 1.0
        with pytest.raises(RuntimeError, match="slot 3.*ywt must be symmetric"):
            ctx.set_scenario_weights(uwt, bad)
        bad = uwt.copy()
        bad[5, 0, 1] += 1.0
        with pytest.raises(RuntimeError, match="slot 5.*uwt must be symmetric"):
            ctx.set_scenario_weights(bad, ywt)
        bad = uwt.copy()
        bad[2, 1, 1] = np.nan
        with pytest.raises(RuntimeError, match="slot 2.*finite"):
            ctx.set_scenario_weights(bad, ywt)
        with pytest.raises(ValueError):
            ctx.set_scenario_weights(uwt, None)
        with pytest.raises(ValueError):
            ctx.set_scenario_weights(uwt[:-1], ywt)
        lib = ctx.lib
        assert lib.cmpc_set_scenario_weights(ctx._h, cmpc._abi.dptr(np.ascontiguousarray(uwt)), None) == -1
        assert b"both" in lib.cmpc_last_error()
        seg = [s for s in torch.cuda.memory_snapshot()
               if s["address"] <= t.data_ptr() < s["address"] + s["total_size"]]
        assert len(seg) == 1
        tail = seg[0]["address"] + seg[0]["total_size"] - 64   # 64 bytes < nq * 13 doubles
        for ptr in (pk.ctypes.data, tail, t.data_ptr() + 4):
            with pytest.raises(RuntimeError):
                ctx.bind_scenario_weights(ptr)
        with pytest.raises(RuntimeError, match="no per-slot weights"):
            ctx.get_scenario_weights()
        ctx.build()
        for a, c in zip(ctx.download_qp(), qp0):
            assert np.array_equal(a, c)
        torch.cuda.synchronize()


def test_gpu_predict_is_stale_after_new_weights():
    cfg, arr, batch, uwt, ywt, _, _ = WR.problem("coop-par", 50, 2, None, B)
    with make_ctx(cfg, arr, B, *batch) as ctx:
        ctx.build()
        ctx.init_warmstart()
        ctx.iterate(3, 0)
        ctx.predict()
        ctx.set_scenario_weights(uwt, ywt)
        with pytest.raises(RuntimeError, match="per-scenario weights have changed"):
            ctx.predict()
        ctx.build()
        ctx.predict()
        t = dev(WR.packed(uwt, ywt))
        ctx.bind_scenario_weights(t.data_ptr())
        with pytest.raises(RuntimeError, match="per-scenario weights have changed"):
            ctx.predict()
        ctx.build()
        ctx.predict()
        ctx.set_scenario_weights(None, None)
        with pytest.raises(RuntimeError, match="per-scenario weights have changed"):
            ctx.predict()
        ctx.synchronize()


@pytest.mark.parametrize("nB", [B, 2048])   # 6 QPs: the unset build is the role split; 4 096: the row build
def test_gpu_forced_variants_fail_with_the_plans_text(nB):
    from cmpc.synthetic import synthetic_batch
    cfg, arr, _ = RP.config("coop-par", 50)
    batch = synthetic_batch(cfg, nB, seed=3)
    nq = nB * cfg.S
    unset = cmpc.plan(CmpcDims.from_config(cfg, nB), CUS, K=0).build_kernel
    assert unset == (SPLITB if nB == B else ROWS)
    with make_ctx(cfg, arr, nB, *batch) as ctx:
        ctx.build()
        assert ctx.last_build_kernel() == unset
        ctx.set_scenario_weights(*WR.shared_weights(cfg, arr, nq))
        ctx.build()
        assert ctx.last_build_kernel() == WAVE
        for variant in (ROWS, SPLITB):
            ctx.set_build_variant(variant)
            with pytest.raises(RuntimeError) as e:
                ctx.build()
            assert cmpc.plan_error_string(cmpc._abi.CMPC_PLAN_WEIGHTS_NEED_WAVE) in str(e.value)
        ctx.set_build_variant(cmpc.CMPC_BUILD_AUTO)
        ctx.set_step_variant(FUSED)
        with pytest.raises(RuntimeError) as e:
            ctx.step(9, 0)
        assert cmpc.plan_error_string(cmpc._abi.CMPC_PLAN_WEIGHTS_NEED_SPLIT) in str(e.value)
        ctx.synchronize()


def solve_state(ctx):
    return (*ctx.download(), ctx.get_state()[2])   # du, status, nwsr, ws


@pytest.mark.parametrize("name,nB", [("coop-par", B), ("cent-ser", 300)])   # 300 QPs: the unset AUTO step is fused
def test_gpu_step_with_weights_is_build_plus_iterate(name, nB):
    K = 9
    cfg, arr, batch, uwt, ywt, _, _ = WR.problem(name, 50, 2, None, nB)
    fused_unset = bool(cmpc.plan(CmpcDims.from_config(cfg, nB), CUS, K=K).step_fused)
    assert fused_unset == (name == "cent-ser")
    out = []
    for one_call in (True, False):
        with make_ctx(cfg, arr, nB, *batch) as ctx:
            if fused_unset and one_call:
                ctx.step(K, 0)
                assert ctx.last_step_fused() == 1
                ctx.set_state(batch[1], batch[2], batch[3])
            ctx.set_scenario_weights(uwt, ywt)
            for _ in range(2):
                if one_call:
                    ctx.step(K, cmpc.CMPC_APPLY_MOVE)
                    assert ctx.last_step_fused() == 0 and ctx.last_build_kernel() == WAVE
                else:
                    ctx.build()
                    ctx.iterate(K, cmpc.CMPC_APPLY_MOVE)
            out.append((*ctx.download_qp(), *solve_state(ctx)))
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert np.abs(out[0][3]).max() > 0


def test_gpu_closed_loop_weights_per_scenario():
    """B = 2 with per-scenario weights against, for each scenario, a B = 1 loop
    whose shared weights are that scenario's: the same inputs, bit for bit."""
    import golden_cases as GC
    from cmpc.driver import ClosedLoop
    cfg, setup, arr, g = GC.case("coop-par", p=50)
    nB, n, K = 2, 3, g["n_iterations"]
    x0, u_def = cmpc.plant_default(cfg.plant)
    M = cmpc.reference_observer_gain(cfg)
    rng = np.random.default_rng(12)
    uw, yw = WR.draw_weights(rng, cfg, arr, nB * cfg.S)
    uw, yw = uw.reshape(nB, cfg.S, cfg.nu, cfg.nu), yw.reshape(nB, cfg.S, cfg.ny, cfg.ny)

    def run(loop):
        try:
            loop.initialize()
            res = []
            for _ in range(n):
                loop.step()
                res.append(loop.u_ctrl.cpu().numpy().copy())
            return np.stack(res)   # (n, B, nu_tot)
        finally:
            loop.close()

    loop = ClosedLoop(cfg, arr, [M] * cfg.S, np.tile(x0, (nB, 1)), np.tile(u_def, (nB, 1)), K)
    loop.set_weights_per_scenario(uw, yw)
    assert loop.ctx.get_scenario_weights()[0].shape == (nB * cfg.S, cfg.nu, cfg.nu)
    both = run(loop)
    plain = run(ClosedLoop(cfg, arr, [M] * cfg.S, np.tile(x0, (nB, 1)), np.tile(u_def, (nB, 1)), K))
    assert np.isfinite(both).all() and np.abs(both).max() > 0
    for b in range(nB):
        one = run(ClosedLoop(cfg, with_weights(arr, uw[b], yw[b]), [M] * cfg.S, x0[None], u_def[None], K))
        assert np.array_equal(both[:, b], one[:, 0]), b
        assert not np.array_equal(both[:, b], plain[:, b]), b
