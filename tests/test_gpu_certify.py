"""Multipliers and KKT certificate on the device (include/cmpc.h,
cmpc_certify*; csrc/certify.hip) against the long-double model (kkt_ref.py).
Marked gpu; runs on an MI355X.  The batches are certify_cases.py's: p = 17,
70 slots (two 64-lane workgroups, the last one partial); test_certify.py
checks on the CPU that they cover the working sets named there.

Tolerance of the parity: a plain float64 evaluation of the model's formulas
sits F64_DEV = 1.2 (measured 1.12) eps units from the long-double model on
these inputs (test_certify.py, kkt_ref.units: eps times the slot's summed
magnitudes); the device sums in another order and with FMAs, no less
accurately, and gets 8 x that: BAR = 9.6 eps units.  n_active, status and
rank_def are exact.  The certificate's bar is test_solver_kkt.py's 1e-9 of
the problem scale; the objective identity's is test_gpu_predict.py's 1e-11 of
the summed magnitudes."""
import dataclasses

import numpy as np
import pytest

import certify_cases as CC
import cmpc
import golden_cases as GC
import kkt_ref as KR
import predict_ref as PR
from cmpc._abi import check, dptr
from test_certify import F64_DEV

pytestmark = pytest.mark.gpu
BAR = 8 * F64_DEV
KKT_TOL = 1e-9
TOL_ID = 1e-11
OK = cmpc.CMPC_QP_OK


@pytest.fixture(autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()
    yield


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")   # (a copy: the shared inputs are read-only)


def make_ctx(key, per_slot=True, du_old=None):
    cfg, arr, B, batch, lim, d = CC.case(key)
    ctx = cmpc.Context(cfg, B)
    ctx.configure(arr)
    ctx.set_state(batch[1], batch[2] if du_old is None else du_old, batch[3])
    ctx.upload_lin(batch[0])
    if per_slot:
        ctx.set_scenario_constraints(*[np.ascontiguousarray(lim[:, i]) for i in range(4)])
    return ctx


def limits_of(key, per_slot):
    cfg, arr, B, batch, lim, d = CC.case(key)
    return lim if per_slot else CC.shared_limits(cfg, arr, B * cfg.S)


def solve_with(ctx, cfg, d):
    """one solve of every slot with the other controllers' plans d"""
    ctx.build()
    if cfg.nVo:
        check(ctx.lib.cmpc_get_input_host(ctx._h, dptr(d), 0), "cmpc_get_input_host")
    else:
        ctx.iterate(1, 0)


def held(ctx):
    """what the context holds for the certificate: H, f, G, du, status, u_old, ws"""
    H, f, G = ctx.download_qp()
    du, status, _ = ctx.download()
    u_old, _, ws = ctx.get_state()
    return H, f, G, du, status, u_old, ws


def certify(ctx, d=None):
    t = dev(d) if d is not None and d.size else None
    ctx.certify(t.data_ptr() if t is not None else 0)
    return ctx.certify_download()


def model_of(cfg, h, d, lim):
    H, f, G, du, status, u_old, ws = h
    args = (H, f, G, d, du, ws, status, lim, u_old, cfg.nu)
    return KR.certify_batch(*args), KR.units(H, f, G, d, du, lim, u_old, cfg.nu)


def assert_parity(rec, model, unit, what):
    for k in KR.EXACT:
        assert np.array_equal(rec[k], np.asarray(model[k], float)), (what, k)
    worst, where = KR.deviation(rec, model, unit)
    print(f"{what}: the device is {worst:.3f} eps units from the model ({where}); bar {BAR}")
    assert worst <= BAR, (what, where, worst)


def assert_certified(rec, what):
    """every OK slot inside test_solver_kkt.py's 1e-9 bar; no dependent normals"""
    ok = rec["status"] == OK
    assert ok.any() and (rec["rank_def"] == 0).all(), what
    sc = rec["scale"][ok]
    worst = {k: float((rec[k][ok] / (1.0 if k == "r_prim" else sc)).max()) for k in ("r_stat", "r_prim", "r_dual", "r_comp")}
    print(f"{what}: worst residuals over {int(ok.sum())} OK slots {worst}")
    for k, v in worst.items():
        assert v <= KKT_TOL, (what, k, v)
    return worst


# ---- 1. parity with the model ------------------------------------------------------

@pytest.mark.parametrize("key", list(CC.CASES))
@pytest.mark.parametrize("per_slot", [True, False], ids=["slot-limits", "shared-limits"])
def test_gpu_certify_matches_model(key, per_slot):
    cfg, arr, B, batch, _, d = CC.case(key)
    lim = limits_of(key, per_slot)
    with make_ctx(key, per_slot) as ctx:
        assert cmpc.certify_available(ctx.dims)
        solve_with(ctx, cfg, d)
        h = held(ctx)
        rec_d = certify(ctx, d)
        rec_0 = certify(ctx)                      # d gathered from the scenario's other slots
        dg = PR.gather_other(cfg, h[3])
        rec_g = certify(ctx, dg)                  # the same plans given explicitly
        ctx.certify_host(dg)
        rec_h = ctx.certify_download()
    n = cfg.nV
    assert rec_d["lam"].shape == (B * cfg.S, 2 * n) and rec_d["r_stat"].shape == (B * cfg.S,)
    for k in KR.FIELDS:
        assert np.array_equal(rec_0[k], rec_g[k]), k
        assert np.array_equal(rec_h[k], rec_g[k]), k
    what = f"{key} {'slot' if per_slot else 'shared'} limits"
    m_d, u_d = model_of(cfg, h, d, lim)
    assert_parity(rec_d, m_d, u_d, what + ", d given")
    m_g, u_g = model_of(cfg, h, dg, lim)
    assert_parity(rec_0, m_g, u_g, what + ", d gathered")
    if per_slot:   # (the working sets test_certify.py found on the oracle's solutions of this batch)
        assert (rec_d["status"] != OK).any() and (rec_d["n_active"] >= (3 if cfg.m >= 2 else 1)).any()
        assert not rec_d["lam"][rec_d["status"] != OK].any()


@pytest.mark.parametrize("key", ["coop-par", "cent-par", "coop-par-m3"])
def test_gpu_certify_foreign_working_sets(key):
    """Working-set words the solve did not leave (cmpc_set_state after it):
    random subsets of the rows on random sides, and for every fourth slot both
    rows of variable 0 (bound 0 and rate row 0 are both e_0: dependent).  The
    wrong-signed multipliers, the slack of rows that are not tight and the
    rank_def path, all against the model."""
    cfg, arr, B, batch, lim, d = CC.case(key)
    n, nq = cfg.nV, B * cfg.S
    rng = np.random.default_rng(11)
    ws = np.zeros(nq, np.uint32)
    for q in range(nq):
        w = 0
        for j in rng.choice(2 * n, size=int(rng.integers(0, n + 1)), replace=False):
            w |= (1 << int(j)) | (int(rng.integers(0, 2)) << (16 + int(j)))
        ws[q] = w | ((1 | (1 << n)) if q % 4 == 0 else 0)
    with make_ctx(key) as ctx:
        solve_with(ctx, cfg, d)
        ctx.set_state(ws=ws)
        h = held(ctx)
        rec = certify(ctx, d)
    assert np.array_equal(h[6], ws)
    model, unit = model_of(cfg, h, d, lim)
    assert_parity(rec, model, unit, f"{key}, foreign working sets")
    ok = rec["status"] == OK
    assert (rec["rank_def"][~ok] == 0).all() and (rec["n_active"][~ok] == 0).all()
    assert (rec["rank_def"][(np.arange(nq) % 4 == 0) & ok] == 1).all()
    assert not rec["lam"][rec["rank_def"] == 1].any()
    assert (rec["r_dual"] > 0).any() and (rec["r_comp"] > 0).any() and (0 < rec["rank_def"].sum() < nq)


# ---- 2. certificate of the solver ----------------------------------------------------

def test_gpu_certificate_centralized():
    cfg, arr, B, batch, lim, d = CC.case("cent-par")
    with make_ctx("cent-par") as ctx:
        ctx.build()
        ctx.iterate(1, 0)
        rec = certify(ctx)
    assert_certified(rec, "centralized, iterate(1)")
    assert (rec["n_active"] > 0).any() and rec["lam"].any()


@pytest.mark.parametrize("key", ["coop-par", "coop-par-m1", "coop-par-m3", "coop-ser"])
def test_gpu_certificate_after_get_input(key):
    cfg, arr, B, batch, lim, d = CC.case(key)
    with make_ctx(key) as ctx:
        solve_with(ctx, cfg, d)
        rec = certify(ctx, d)
    assert_certified(rec, f"{key}, get_input")


def test_gpu_certificate_after_one_iteration():
    """cmpc_iterate(1): d is the du_old in force before the call."""
    cfg, arr, B, batch, lim, _ = CC.case("coop-par")
    plans = np.ascontiguousarray(np.random.default_rng(5).uniform(-0.05, 0.05, (B * cfg.S, cfg.nV)))
    with make_ctx("coop-par", du_old=plans) as ctx:
        ctx.build()
        ctx.iterate(1, 0)
        rec = certify(ctx, PR.gather_other(cfg, plans))
    assert_certified(rec, "coop-par, iterate(1) from du_old")


@pytest.mark.parametrize("key", ["coop-par", "coop-ser"])
def test_gpu_certificate_and_jacobi_gap_after_nine_iterations(key):
    """K = 9 as nine cmpc_iterate(1): the same bits as one cmpc_iterate(9); with
    the plans the last iteration saw the record certifies the solver, with the
    final plans (d NULL) r_stat is the scenario's Jacobi gap, the model's value.
    On the serial plant's batch the ninth iteration still moves the plans (by
    1e-12 in the oracle's emulation of these nine iterations) and the gap is
    larger than the certificate's r_stat on some slot.  On the parallel plant's
    batch at p = 17 the coupling is weak (max|G| 56 against max|H| 1.9e5) and
    the oracle's plans stop changing exactly before the ninth iteration: where
    the device's do too, d is the same array either way and the gap record is
    the certificate bit for bit, the gap of a fixed point."""
    cfg, arr, B, batch, lim, _ = CC.case(key)
    with make_ctx(key) as ctx:
        ctx.build()
        ctx.iterate(9, 0)
        once = (*ctx.download(), *ctx.get_state())
        rec_gap9 = certify(ctx)
    with make_ctx(key) as ctx:
        ctx.build()
        for _ in range(8):
            ctx.iterate(1, 0)
        seen = PR.gather_other(cfg, ctx.get_state()[1])
        ctx.iterate(1, 0)
        nine = (*ctx.download(), *ctx.get_state())
        h = held(ctx)
        rec_cert = certify(ctx, seen)
        rec_gap = certify(ctx)
    for a, b in zip(once, nine):
        assert np.array_equal(a, b)
    for k in KR.FIELDS:
        assert np.array_equal(rec_gap[k], rec_gap9[k]), k
    assert_certified(rec_cert, f"{key}, K = 9")
    m_g, u_g = model_of(cfg, h, PR.gather_other(cfg, h[3]), lim)
    assert_parity(rec_gap, m_g, u_g, f"{key}, Jacobi gap")
    ok = rec_gap["status"] == OK
    gap, cert = rec_gap["r_stat"][ok] / rec_gap["scale"][ok], rec_cert["r_stat"][ok] / rec_cert["scale"][ok]
    print(f"{key}: Jacobi gap r_stat/scale max {gap.max():.3e}, median {np.median(gap):.3e}; certificate max {cert.max():.3e}")
    fixed = np.array_equal(seen, PR.gather_other(cfg, h[3]))
    assert not (fixed and key == "coop-ser")
    if fixed:
        for k in KR.FIELDS:
            assert np.array_equal(rec_gap[k], rec_cert[k]), k
    else:
        assert (rec_gap["r_stat"][ok] > rec_cert["r_stat"][ok]).any()   # the two readings differ


# ---- 3. objective ----------------------------------------------------------------------

@pytest.mark.parametrize("key", ["coop-par", "cent-par"])
def test_gpu_certify_obj_is_the_predicted_cost(key):
    cfg, arr, B, batch, lim, d = CC.case(key)
    with make_ctx(key) as ctx:
        solve_with(ctx, cfg, d)
        H, f, G, du, *_ = held(ctx)
        rec = certify(ctx, d)
        td = dev(d) if d.size else None
        ctx.predict(0, td.data_ptr() if td is not None else 0)
        _, J = ctx.download_prediction()
        tz = dev(np.zeros_like(du))
        ctx.predict(tz.data_ptr(), td.data_ptr() if td is not None else 0)
        _, J0 = ctx.download_prediction()
    worst = 0.0
    for q in range(du.shape[0]):
        quad = 0.5 * du[q] @ H[q] @ du[q]
        lin_term = (f[q] + (G[q] @ d[q] if cfg.nVo else 0.0)) @ du[q]
        mag = abs(J[q, 0]) + abs(J[q, 1]) + abs(J0[q, 0]) + abs(quad) + abs(lin_term)
        worst = max(worst, abs(J[q, 0] + J[q, 1] - J0[q, 0] - rec["obj"][q]) / mag)
    print(f"{key}: worst |J - J(0) - obj| {worst:.2e} of the summed magnitudes")
    assert np.abs(du).max() > 0 and worst <= TOL_ID


# ---- 4. summary ------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["coop-par", "cent-par"])
def test_gpu_certify_summary_is_the_host_reduction(key):
    cfg, arr, B, batch, lim, d = CC.case(key)
    with make_ctx(key) as ctx:
        ctx.build()
        if cfg.nVo:
            ctx.iterate(9, 0)
        else:
            ctx.iterate(1, 0)
        with pytest.raises(RuntimeError, match="nothing has been certified"):
            ctx.certify_summary(1e-9)
        ctx.certify()
        raw = ctx.certify_record()
        F = cmpc.certify_fields(ctx.dims)
        ok = raw[F["status"].start] == OK
        ratio = (raw[F["r_stat"].start] / raw[F["scale"].start])[ok]
        tol = float(np.median(ratio[ratio > 0]))   # (a fully determined working set leaves r_stat = 0 exactly)
        got = [ctx.certify_summary(t) for t in (tol, 0.0, 1e300)]
    want = [KR.host_summary(raw, F, t) for t in (tol, 0.0, 1e300)]
    print(f"{key}: tol {tol:.3e} -> {got[0]}")
    for g, w in zip(got, want):
        assert g == w
    assert 0 < want[0]["n_above"] < int(ok.sum())          # the tolerance splits the OK slots
    assert want[0]["n_not_ok"] == int((~ok).sum()) > 0 and want[2]["n_above"] == 0


# ---- 5. refusals -----------------------------------------------------------------------

def test_gpu_certify_refusals():
    cfg, arr, B, batch, lim, d = CC.case("coop-par")
    with make_ctx("coop-par") as ctx:
        assert ctx.certify_ptr() == 0
        with pytest.raises(RuntimeError, match="no build has run"):
            ctx.certify()
        with pytest.raises(RuntimeError, match="nothing has been certified"):
            ctx.certify_download()
        ctx.build()
        with pytest.raises(RuntimeError, match="no solve has written plans for the last build"):
            ctx.certify()
        ctx.iterate(0, 0)
        with pytest.raises(RuntimeError, match="no solve has written plans"):
            ctx.certify()
        ctx.init_warmstart()
        with pytest.raises(RuntimeError, match="no solve has written plans"):
            ctx.certify()
        ctx.synchronize()
        assert ctx.certify_ptr() == 0                       # nothing allocated, nothing launched so far
        ctx.iterate(2, 0)
        ctx.certify()
        assert ctx.certify_ptr() != 0
        assert ctx.lib.cmpc_certify(ctx._h, None, 4) == -1   # flags are reserved
        assert b"flags must be 0" in ctx.lib.cmpc_last_error()
        ctx.build()                                         # new QPs: the plans are the old ones'
        with pytest.raises(RuntimeError, match="no solve has written plans"):
            ctx.certify()
        ctx.iterate(2, cmpc.CMPC_APPLY_MOVE)
        with pytest.raises(RuntimeError, match="cmpc_certify: u_old has moved since the build .CMPC_APPLY_MOVE"):
            ctx.certify()
        ctx.step(2, 0)                                      # the build and the solve inside cmpc_step
        ctx.certify()
        ctx.step(0, 0)
        with pytest.raises(RuntimeError, match="no solve has written plans"):
            ctx.certify()
        ctx.step(2, cmpc.CMPC_APPLY_MOVE)
        with pytest.raises(RuntimeError, match="CMPC_APPLY_MOVE"):
            ctx.certify()
        ctx.step(2, 0)
        ctx.set_state(u_old=batch[1])
        with pytest.raises(RuntimeError, match="cmpc_set_state"):
            ctx.certify()
        ctx.step(2, 0)
        ctx.upload_lin(batch[0])
        with pytest.raises(RuntimeError, match="cmpc_upload_lin"):
            ctx.certify()
        ctx.step(2, 0)
        check(ctx.lib.cmpc_get_input_host(ctx._h, dptr(d), 0), "cmpc_get_input_host")
        ctx.certify()
        ctx.synchronize()


def test_gpu_certify_needs_the_other_plans_of_a_lone_sub_controller():
    """S = 1 with nu < nu_tot: the other controllers' plans are not in the
    context, so a NULL d is refused; given, the slot is certified."""
    cfg2, arr, B, batch, lim, d = CC.case("coop-par")
    cfg = dataclasses.replace(cfg2, input_order=[cfg2.input_order[0]], out_idx=[cfg2.out_idx[0]])
    sel = slice(0, None, 2)                                  # sub-controller 0 of every scenario
    with cmpc.Context(cfg, B) as ctx:
        ctx.configure(arr)
        ctx.set_state(batch[1][sel], batch[2][sel], batch[3][sel])
        ctx.upload_lin(batch[0][sel])
        ctx.build()
        d1 = np.ascontiguousarray(d[sel])
        check(ctx.lib.cmpc_get_input_host(ctx._h, dptr(d1), 0), "cmpc_get_input_host")
        with pytest.raises(RuntimeError, match="other controllers' plans are not in this context .nu_tot != S . nu."):
            ctx.certify()
        rec = certify(ctx, d1)
    assert_certified(rec, "lone sub-controller")


# ---- 6. nothing moves ------------------------------------------------------------------

def test_gpu_certify_changes_nothing():
    cfg, arr, B, batch, lim, d = CC.case("coop-par")
    with make_ctx("coop-par") as ctx:
        ctx.build()
        ctx.iterate(3, 0)
        before = (*ctx.download(), *ctx.get_state(), *ctx.download_qp())
        ctx.certify()
        td = dev(d)
        ctx.certify(td.data_ptr())
        ctx.certify_summary(1e-9)
        after = (*ctx.download(), *ctx.get_state(), *ctx.download_qp())
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


def test_gpu_closed_loop_with_certify_is_the_same_loop():
    """ClosedLoop.step(certify=True) against the plain step, 20 instants, B = 3:
    plant outputs and u_ctrl bit for bit; the summary is there and sane."""
    from cmpc.driver import ClosedLoop
    cfg, setup, arr, g = GC.case("coop-par", p=50)
    B, n, K = 3, 20, g["n_iterations"]
    x0, u_def = cmpc.plant_default(cfg.plant)
    M = cmpc.reference_observer_gain(cfg)
    out, summ = {}, []
    for cert in (True, False):
        loop = ClosedLoop(cfg, arr, [M] * cfg.S, np.tile(x0, (B, 1)), np.tile(u_def, (B, 1)), K)
        try:
            loop.initialize()
            res = []
            for _ in range(n):
                _, y = loop.step(certify=True) if cert else loop.step()
                res.append((y.cpu().numpy().copy(), loop.u_ctrl.cpu().numpy().copy()))
                if cert:
                    summ.append(loop.last_certificate)
            out[cert] = res
            if not cert:
                assert not hasattr(loop, "last_certificate") and loop.ctx.certify_ptr() == 0
        finally:
            loop.close()
    for k in range(n):
        assert np.array_equal(out[True][k][0], out[False][k][0]), k
        assert np.array_equal(out[True][k][1], out[False][k][1]), k
    print(f"closed loop: Jacobi gap r_stat/scale per step, first {summ[0]['r_stat']:.3e}, last {summ[-1]['r_stat']:.3e}")
    for s in summ:   # (d is the final plans: r_stat and r_dual carry the Jacobi gap, r_prim does not)
        assert -1 <= s["slot_stat"] < B * cfg.S and 0 <= s["n_not_ok"] <= B * cfg.S
        assert np.isfinite(s["r_stat"]) and s["r_prim"] <= KKT_TOL
