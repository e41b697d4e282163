"""Prediction on the device (include/cmpc.h, cmpc_predict; csrc/predict.hip)
against the oracle's prediction matrices.  Marked gpu; runs on an MI355X.

Tolerances: per slot max|y_pred - oracle| <= 1e-11 max|oracle y_pred| (the
build tolerance of test_gpu_parity.py: the kernel steps the model forward and
never forms Su, so it sums in another order; the same recursion in numpy sits
at 5e-15), J_track and J_move each within 1e-11 relative (sums of
non-negative terms for the positive semi-definite weights: nothing cancels).
B = 47 gives 47 or 94 slots, so the last wave's rows are partly empty."""
import dataclasses
import functools

import numpy as np
import pytest

import cmpc
import golden_cases as GC
import predict_ref as PR
from cmpc._abi import CmpcDims
from cmpc.synthetic import synthetic_batch

pytestmark = pytest.mark.gpu
B_PAR = 47
TOL = 1e-11


@pytest.fixture(autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()
    yield


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")   # (a copy: the shared inputs are read-only)


def make_ctx(cfg, arr, B, lin, u_old, du_old, ws):
    ctx = cmpc.Context(cfg, B)
    ctx.configure(arr)
    ctx.set_state(u_old, du_old, ws)
    ctx.upload_lin(lin)
    return ctx


@functools.lru_cache(maxsize=None)
def problem(name, p, m=2, delays=None, B=B_PAR):
    """batch, random plans in +-0.1 and the oracle's evaluation of them"""
    ctype, plant = name.split("-")
    _, setup, _, _ = GC.case(name)
    cfg = cmpc.reference_config(plant, ctype, p=p, m=m)
    if delays is not None:
        cfg = dataclasses.replace(cfg, delays=tuple(delays))
    arr = cmpc.controller_arrays(cfg, setup)
    batch = synthetic_batch(cfg, B, seed=11 + p)
    lin, u_old = batch[0], batch[1]
    dims = CmpcDims.from_config(cfg, 1)
    L = cmpc.layout_of(dims)
    nq = B * cfg.S
    rng = np.random.default_rng(101 + p + m)
    du = np.ascontiguousarray(rng.uniform(-0.1, 0.1, (nq, L.nV)))
    d = np.ascontiguousarray(rng.uniform(-0.1, 0.1, (nq, L.nVo)))
    Yo, Jo = PR.oracle_batch(cfg, dims, L, arr, lin, u_old, du, d)
    for a in (*batch, du, d, Yo, Jo):
        a.setflags(write=False)
    return cfg, arr, batch, du, d, Yo, Jo


def run_predict(ctx, du=None, d=None):
    t_du = dev(du) if du is not None else None
    t_d = dev(d) if d is not None and d.size else None
    ctx.predict(t_du.data_ptr() if t_du is not None else 0, t_d.data_ptr() if t_d is not None else 0)
    return ctx.download_prediction()


def assert_matches_oracle(Y, J, Yo, Jo, what=""):
    worst_y = worst_j = 0.0
    for q in range(Yo.shape[0]):
        sy = np.abs(Yo[q]).max()
        worst_y = max(worst_y, np.abs(Y[q] - Yo[q]).max() / sy)
        worst_j = max(worst_j, np.abs(J[q] - Jo[q]).max() / np.abs(Jo[q]).min())
    print(f"{what}: worst y_pred error {worst_y:.2e} of max|y_pred|, worst cost error {worst_j:.2e} relative")
    for q in range(Yo.shape[0]):
        np.testing.assert_allclose(Y[q], Yo[q], rtol=0, atol=TOL * np.abs(Yo[q]).max(), err_msg=f"slot {q}")
        np.testing.assert_allclose(J[q], Jo[q], rtol=TOL, atol=0, err_msg=f"slot {q}")


# ---- 1. parity with the oracle matrices ----------------------------------------

PARITY = [("coop-par", 50, 2, None),            # ny = 3
          ("ncoop-par", 50, 2, None),           # ny = 2
          ("cent-ser", 50, 2, None),            # ns = 10, ny = 4, nVo = 0
          ("coop-ser", 50, 2, None),            # ns = 10, ny = 4, distributed
          ("cent-par", 200, 2, None),           # the horizon several times the delay
          ("coop-par", 30, 2, None),            # delay 40 > p: the delayed inputs' plans never arrive
          ("coop-par", 50, 1, None),            # the (11, 3, 2, 1) set
          ("coop-par", 50, 3, None),            # the (11, 3, 2, 3) set
          # delay sets of test_gpu_parity.py's build parity: the shortest delay a
          # context accepts with two delayed inputs (2: a one-entry shift block;
          # a delay of 1 is refused at cmpc_create, test_abi.py) beside one of
          # p - 1, and two different delays inside the horizon
          ("ncoop-par", 64, 2, (0, 2, 0, 63)),
          ("coop-par", 50, 2, (0, 10, 0, 25))]


@pytest.mark.parametrize("name,p,m,delays", PARITY)
def test_gpu_predict_matches_oracle(name, p, m, delays):
    cfg, arr, batch, du, d, Yo, Jo = problem(name, p, m, delays)
    assert cmpc.predict_available(CmpcDims.from_config(cfg, B_PAR))
    with make_ctx(cfg, arr, B_PAR, *batch) as ctx:
        ctx.build()
        Y, J = run_predict(ctx, du, d)
    assert Y.shape == (B_PAR * cfg.S, cfg.p, cfg.ny) and J.shape == (B_PAR * cfg.S, 2)
    assert_matches_oracle(Y, J, Yo, Jo, f"{name} p={p} m={m} delays={delays}")


# ---- 2. default arguments --------------------------------------------------------

@pytest.mark.parametrize("name,B", [("coop-par", B_PAR),   # plans in device memory
                                    ("coop-par", 8),       # 16 slots: plans in page-locked host memory
                                    ("cent-ser", 8)])      # nVo = 0
def test_gpu_predict_default_arguments(name, B):
    cfg, arr, batch, *_ = problem(name, 50, B=B)
    with make_ctx(cfg, arr, B, *batch) as ctx:
        ctx.build()
        ctx.iterate(3, 0)
        Y0, J0 = run_predict(ctx)
        du, status, _ = ctx.download()
        Y1, J1 = run_predict(ctx, du, PR.gather_other(cfg, du))
        Y2, J2 = run_predict(ctx, du, None)   # the plans given, the others' gathered from them
    assert np.isfinite(Y0).all() and np.abs(du).max() > 0
    assert np.array_equal(Y0, Y1) and np.array_equal(J0, J1)
    assert np.array_equal(Y0, Y2) and np.array_equal(J0, J2)


def test_gpu_predict_host_arrays_equal_device_arrays():
    cfg, arr, batch, du, d, Yo, Jo = problem("coop-par", 50)
    from cmpc._abi import check, dptr
    with make_ctx(cfg, arr, B_PAR, *batch) as ctx:
        ctx.build()
        Y, J = run_predict(ctx, du, d)
        check(ctx.lib.cmpc_predict_host(ctx._h, dptr(du), dptr(d), 0), "cmpc_predict_host")
        Yh, Jh = ctx.download_prediction()
        assert ctx.lib.cmpc_predict_host(ctx._h, dptr(du), dptr(d), 4) == -1   # flags are reserved
    assert np.array_equal(Y, Yh) and np.array_equal(J, Jh)


# ---- 3. the QP identity on the device --------------------------------------------

@pytest.mark.parametrize("name", ["coop-par", "cent-ser"])
def test_gpu_predicted_cost_is_the_qp_objective(name):
    """J(du) - J(0) = 1/2 du' H du + (f + G d)' du with the device's own H, f,
    G, within 1e-11 of the summed magnitudes of the five terms."""
    cfg, arr, batch, du, d, _, _ = problem(name, 50)
    with make_ctx(cfg, arr, B_PAR, *batch) as ctx:
        ctx.build()
        H, f, G = ctx.download_qp()
        _, J = run_predict(ctx, du, d)
        _, J0 = run_predict(ctx, np.zeros_like(du), d)
    assert (J0[:, 1] == 0).all()
    worst = 0.0
    for q in range(du.shape[0]):
        quad = 0.5 * du[q] @ H[q] @ du[q]
        lin_term = (f[q] + (G[q] @ d[q] if cfg.nVo else 0.0)) @ du[q]
        mag = abs(J[q, 0]) + abs(J[q, 1]) + abs(J0[q, 0]) + abs(quad) + abs(lin_term)
        err = abs(J[q, 0] + J[q, 1] - J0[q, 0] - quad - lin_term)
        worst = max(worst, err / mag)
    print(f"{name}: worst identity error {worst:.2e} of the summed magnitudes")
    assert worst <= TOL


# ---- 4. per-scenario setpoints ---------------------------------------------------

def test_gpu_predict_with_setpoint_offsets():
    """The offset moves the target, not the prediction: y_pred bit for bit as
    without offsets, J_track the oracle's with y_ref + dy."""
    cfg, arr, batch, du, d, Yo, Jo = problem("coop-par", 50)
    lin, u_old = batch[0], batch[1]
    dims = CmpcDims.from_config(cfg, 1)
    L = cmpc.layout_of(dims)
    nq = B_PAR * cfg.S
    y_prev = lin[:, L.off_y:L.off_y + cfg.ny]
    dy = np.ascontiguousarray(0.2 * np.random.default_rng(7).uniform(-1, 1, y_prev.shape) * np.abs(y_prev))
    Jd = np.zeros((nq, 2))
    for q in range(nq):
        s = q % cfg.S
        yr = np.asarray(arr.y_ref[s]).reshape(cfg.p, cfg.ny) + dy[q]
        Jd[q] = PR.costs(cfg, Yo[q], du[q], yr, arr.ywt[s], arr.uwt[s])
    with make_ctx(cfg, arr, B_PAR, *batch) as ctx:
        ctx.build()
        Y0, J0 = run_predict(ctx, du, d)
        ctx.set_scenario_reference(dy)
        with pytest.raises(RuntimeError, match="offsets"):
            ctx.predict()
        ctx.build()
        Y1, J1 = run_predict(ctx, du, d)
    assert np.array_equal(Y0, Y1)
    assert np.array_equal(J0[:, 1], J1[:, 1])
    assert_matches_oracle(Y1, J1, Yo, Jd, "coop-par with offsets")
    assert all(abs(J1[q, 0] - J0[q, 0]) > 1e-6 * J0[q, 0] for q in range(nq))


# ---- 5. staleness ----------------------------------------------------------------

def test_gpu_predict_refuses_a_stale_build():
    cfg, arr, batch, du, d, Yo, Jo = problem("coop-par", 50)
    with make_ctx(cfg, arr, B_PAR, *batch) as ctx:
        with pytest.raises(RuntimeError, match="no build has run"):
            ctx.predict()
        with pytest.raises(RuntimeError, match="nothing has been predicted"):
            ctx.download_prediction()
        ctx.build()
        ctx.init_warmstart()
        ctx.iterate(3, 0)
        ctx.predict()                       # plans without the move applied: fine
        ctx.upload_lin(batch[0])
        with pytest.raises(RuntimeError, match="cmpc_upload_lin"):
            ctx.predict()
        ctx.build()
        Y, J = run_predict(ctx, du, d)
        ctx.iterate(3, cmpc.CMPC_APPLY_MOVE)
        with pytest.raises(RuntimeError, match="CMPC_APPLY_MOVE applied the first move"):
            ctx.predict()
        ctx.build()                         # from the moved u_old
        u_moved = ctx.get_state()[0]
        Ym, Jm = run_predict(ctx, du, d)
        ctx.set_state(u_old=batch[1])
        with pytest.raises(RuntimeError, match="cmpc_set_state"):
            ctx.predict()
        ctx.step(3, 0)                      # the build inside cmpc_step
        ctx.predict()
        ctx.step(3, cmpc.CMPC_APPLY_MOVE)
        with pytest.raises(RuntimeError, match="CMPC_APPLY_MOVE"):
            ctx.predict()
    assert_matches_oracle(Y, J, Yo, Jo, "after a rebuild")
    assert not np.array_equal(u_moved, batch[1])
    dims = CmpcDims.from_config(cfg, 1)
    Yo2, Jo2 = PR.oracle_batch(cfg, dims, cmpc.layout_of(dims), arr, batch[0], u_moved, du, d)
    assert_matches_oracle(Ym, Jm, Yo2, Jo2, "after the move and a rebuild")


def test_gpu_no_prediction_buffers_unless_used():
    cfg, arr, batch, *_ = problem("coop-par", 50)
    with make_ctx(cfg, arr, B_PAR, *batch) as ctx:
        ctx.build()
        ctx.iterate(3, 0)
        ctx.synchronize()
        assert ctx.prediction_ptrs() == (0, 0)
        ctx.predict()
        y_ptr, c_ptr = ctx.prediction_ptrs()
        assert y_ptr and c_ptr
        ctx.synchronize()


# ---- 6. closed loop --------------------------------------------------------------

def test_gpu_closed_loop_with_prediction_is_the_same_loop():
    """ClosedLoop.step(predict=True) against the plain step, five instants,
    B = 3: plant outputs and u_ctrl bit for bit; the last instant's prediction
    (row 0 of slot 0) against the oracle on the records, state and plans the
    context held before the move was applied."""
    from cmpc.driver import ClosedLoop
    cfg, setup, arr, g = GC.case("coop-par", p=50)
    B, n, K = 3, 5, g["n_iterations"]
    x0, u_def = cmpc.plant_default(cfg.plant)
    M = cmpc.reference_observer_gain(cfg)
    out, held = {}, {}
    for predict in (True, False):
        loop = ClosedLoop(cfg, arr, [M] * cfg.S, np.tile(x0, (B, 1)), np.tile(u_def, (B, 1)), K)
        try:
            if predict:
                apply_ = loop.ctx.observe_apply

                def capture():
                    held["lin"], held["u_old"] = loop.ctx.download_lin(), loop.ctx.get_state()[0]
                    held["du"] = loop.ctx.download()[0]
                    apply_()
                loop.ctx.observe_apply = capture
            loop.initialize()
            res = []
            for _ in range(n):
                _, y = loop.step(predict=predict) if predict else loop.step()
                res.append((y.cpu().numpy().copy(), loop.u_ctrl.cpu().numpy().copy()))
            out[predict] = res
            if predict:
                Yp, Jp = loop.last_prediction, loop.last_cost
            else:
                assert not hasattr(loop, "last_prediction")
        finally:
            loop.close()
    for k in range(n):
        assert np.array_equal(out[True][k][0], out[False][k][0]), k
        assert np.array_equal(out[True][k][1], out[False][k][1]), k
    assert Yp.shape == (B * cfg.S, 50, 3) and Jp.shape == (B * cfg.S, 2)
    assert np.isfinite(Yp).all() and np.isfinite(Jp).all()
    dims = CmpcDims.from_config(cfg, 1)
    L = cmpc.layout_of(dims)
    d = PR.gather_other(cfg, held["du"])
    Yo = PR.oracle_prediction(dims, L, held["lin"][0], held["u_old"][0], held["du"][0], d[0])
    np.testing.assert_allclose(Yp[0, 0], Yo[0], rtol=0, atol=TOL * np.abs(Yo).max())
    np.testing.assert_allclose(Yp[0], Yo, rtol=0, atol=TOL * np.abs(Yo).max())
