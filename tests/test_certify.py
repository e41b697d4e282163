"""Multipliers and KKT certificate (include/cmpc.h, cmpc_certify*): the host
side, the long-double model (kkt_ref.py) and the coverage of the GPU tests'
inputs, all on the CPU through the oracle.  Not marked gpu.

The model is checked against test_solver_kkt.kkt_certificate (numpy lstsq, an
independent formulation: signed normals, mu >= 0) on the oracle's solutions of
the batches test_gpu_certify.py runs: multipliers and stationarity residual
agree within that file's 1e-9 of the problem scale, and every OK slot is
inside the bar on all four residuals.

F64_DEV is the measured distance of a plain float64 evaluation of the model's
formulas from the long-double one on these inputs, in units of eps times the
slot's summed magnitudes (kkt_ref.units): 1.12 at most (coop-par, lam), taken
as 1.2.  test_gpu_certify.py gives the device 8 x that."""
import ctypes

import numpy as np
import pytest

import certify_cases as CC
import cmpc
import golden_cases as GC
import kkt_ref as KR
import test_solver_kkt as TK
from cmpc._abi import CERTIFY_FIELDS, CmpcDims

F64_DEV = 1.2
SOLVE_DIMS = {(4, 2, 4), (8, 4, 0), (2, 2, 2), (6, 2, 6)}   # CMPC_FOR_SOLVE (csrc/kernel_dims.h)


def configs():
    out = [(name, cmpc.reference_config(name.split("-")[1], name.split("-")[0], p=50)) for name in GC.NAMES]
    for key, (name, m, _) in CC.CASES.items():
        ctype, plant = name.split("-")
        out.append((key, cmpc.reference_config(plant, ctype, p=CC.P, m=m)))
    out.append(("coop-par-m4", cmpc.reference_config("par", "coop", p=50, m=4)))   # (8, 2, 8): no solve instance
    return out


@pytest.mark.parametrize("name,cfg", configs(), ids=[c[0] for c in configs()])
def test_certify_len_fields_available(name, cfg):
    dims = CmpcDims.from_config(cfg, 5)
    n = cfg.nV
    assert cmpc.certify_len(dims) == 2 * n + 9
    F = cmpc.certify_fields(dims)
    assert tuple(F) == CERTIFY_FIELDS == KR.FIELDS
    assert F["lam"] == slice(0, 2 * n)
    for i, k in enumerate(CERTIFY_FIELDS[1:]):
        assert F[k] == slice(2 * n + i, 2 * n + i + 1), k
    assert cmpc.certify_available(dims) == ((n, cfg.nu, cfg.nVo) in SOLVE_DIMS)
    lib = cmpc.load_library()
    off = ctypes.c_int()
    assert lib.cmpc_certify_field(ctypes.byref(dims), b"mu", ctypes.byref(off), None) == -1
    assert b"no field named 'mu'" in lib.cmpc_last_error()


def test_solve_instances_are_all_covered():
    have = {(cfg.nV, cfg.nu, cfg.nVo) for _, cfg in configs() if cmpc.certify_available(CmpcDims.from_config(cfg, 1))}
    assert have == SOLVE_DIMS


def _active(ws, n):
    w = int(ws)
    return [(j, bool((w >> (16 + j)) & 1)) for j in range(2 * n) if (w >> j) & 1]


@pytest.mark.parametrize("key", list(CC.CASES))
def test_input_coverage(key):
    """What the GPU parity tests need among the slots of each batch, checked on
    the oracle's solutions before anything reaches a GPU.  m = 1 (n = nu = 2)
    cannot have three active rows: the two rows of a variable are both e_0, so
    at most one per variable is in an independent working set; and it has no
    variable j >= nu."""
    cfg, arr, B, batch, lim, d = CC.case(key)
    H, f, G, x, ws, st, _ = CC.oracle_solution(key)
    n, nu, nq = cfg.nV, cfg.nu, B * cfg.S
    assert nq == 70                                   # two 64-lane workgroups, the last one partial
    ok = st == cmpc.CMPC_QP_OK
    acts = [_active(ws[q], n) if ok[q] else [] for q in range(nq)]
    empty = sum(1 for q in range(nq) if ok[q] and not acts[q])
    nonempty = sum(1 for a in acts if a)
    assert 4 * empty >= nq and 4 * nonempty >= nq, (empty, nonempty)
    assert any(j < n and not up for a in acts for j, up in a), "no bound active on its lower side"
    assert any(j < n and up for a in acts for j, up in a), "no bound active on its upper side"
    assert any(j >= n and not up for a in acts for j, up in a), "no rate row active on its lower side"
    assert any(j >= n and up for a in acts for j, up in a), "no rate row active on its upper side"
    if cfg.m >= 2:
        assert any(len(a) >= 3 for a in acts), "no slot with three active rows"
        assert any({j, n + j} <= {r for r, _ in a} for a in acts for j in range(nu, n)), \
            "no slot with the bound and the rate row of a later move both active"
    assert (st == cmpc.CMPC_QP_INFEASIBLE).any() and not ok.all()
    assert (x[~ok] == 0).all()                        # such slots hold the zero move


@pytest.mark.parametrize("key", list(CC.CASES))
@pytest.mark.parametrize("per_slot", [True, False], ids=["slot-limits", "shared-limits"])
def test_model_agrees_with_lstsq_certificate(key, per_slot):
    cfg, arr, B, batch, _, d = CC.case(key)
    H, f, G, x, ws, st, lim = CC.oracle_solution(key, per_slot)
    n, nu, m, nq = cfg.nV, cfg.nu, cfg.m, B * cfg.S
    u_old = batch[1]
    M = KR.certify_batch(H, f, G, d, x, ws, st, lim, u_old, nu)
    C = TK.rows(n, nu)
    worst = dict.fromkeys(("r_stat", "r_prim", "r_dual", "r_comp"), 0.0)
    for q in range(nq):
        g = f[q] + (G[q] @ d[q] if cfg.nVo else 0.0)
        lo, hi = KR.slot_limits(lim[q], u_old[q], nu, m, np.float64)
        scale = np.abs(H[q]).max() * max(1.0, np.abs(x[q]).max()) + np.abs(g).max() + 1.0
        assert abs(float(M["scale"][q]) - scale) <= 4 * KR.EPS * scale
        assert M["status"][q] == st[q] and M["rank_def"][q] == 0
        if st[q] != cmpc.CMPC_QP_OK:
            assert M["n_active"][q] == 0 and not M["lam"][q].any()
            assert abs(float(M["r_stat"][q]) - np.abs(H[q] @ x[q] + g).max()) <= 1e-9 * scale
            continue
        TK.kkt_certificate(H[q], g, lo, hi, C, x[q], int(ws[q]))   # (raises outside its 1e-9 bars)
        act = _active(ws[q], n)
        assert M["n_active"][q] == len(act)
        grad = H[q] @ x[q] + g
        lam = np.zeros(2 * n)
        if act:
            N = np.stack([C[j] * (-1.0 if up else 1.0) for j, up in act], axis=1)
            mu, *_ = np.linalg.lstsq(N, grad, rcond=None)
            for (j, up), v in zip(act, mu):
                lam[j] = -v if up else v
            resid = np.abs(grad - N @ mu).max()
        else:
            resid = np.abs(grad).max()
        assert np.abs(np.asarray(M["lam"][q], float) - lam).max() <= 1e-9 * scale
        assert abs(float(M["r_stat"][q]) - resid) <= 1e-9 * scale
        assert M["r_stat"][q] <= 1e-9 * scale and M["r_dual"][q] <= 1e-9 * scale
        assert M["r_comp"][q] <= 1e-9 * scale and M["r_prim"][q] <= 1e-9
        obj = 0.5 * x[q] @ H[q] @ x[q] + g @ x[q]
        assert abs(float(M["obj"][q]) - obj) <= 1e-12 * (abs(obj) + scale * np.abs(x[q]).max())
        for k in worst:
            worst[k] = max(worst[k], float(M[k][q]) / (1.0 if k == "r_prim" else scale))
    print(f"{key} {'slot' if per_slot else 'shared'} limits: worst residuals over the OK slots {worst}")


def test_model_flags_dependent_normals_and_wrong_signs():
    """A working set with both rows of variable 0 (both e_0): rank_def, lam = 0.
    A multiplier of the wrong sign and an inactive-looking active row show in
    r_dual and r_comp."""
    n, nu = 4, 2
    H = np.diag([2.0, 3.0, 4.0, 5.0])
    f = np.array([1.0, -2.0, 0.5, 0.25])
    x = np.array([0.1, 0.2, -0.1, 0.05])
    lo, hi = -np.ones(2 * n), np.ones(2 * n)
    r = KR.certify_slot(H, f, None, None, x, (1 << 0) | (1 << n), 0, lo, hi, nu)
    assert r["rank_def"] == 1 and not r["lam"].any() and r["n_active"] == 2
    g = H @ x + f
    assert abs(float(r["r_stat"]) - np.abs(g).max()) < 1e-15
    # row 1 active on its upper side: lam_1 = g_1 = -1.4 <= 0 is the right sign; on its lower side it is wrong
    up = KR.certify_slot(H, f, None, None, x, (1 << 1) | (1 << 17), 0, lo, hi, nu)
    dn = KR.certify_slot(H, f, None, None, x, (1 << 1), 0, lo, hi, nu)
    assert up["r_dual"] == 0 and abs(float(dn["r_dual"]) - 1.4) < 1e-15
    assert abs(float(up["r_comp"]) - 1.4 * 0.8) < 1e-15 and abs(float(dn["r_comp"]) - 1.4 * 1.2) < 1e-15
    # a slot that is not OK: W is taken as empty
    bad = KR.certify_slot(H, f, None, None, x, (1 << 1), 2, lo, hi, nu)
    assert bad["n_active"] == 0 and not bad["lam"].any() and bad["status"] == 2


@pytest.mark.parametrize("key", list(CC.CASES))
def test_float64_distance_from_the_model(key):
    """The tolerance of the device parity test: a plain float64 evaluation of
    the same formulas against the long-double model, in kkt_ref.units."""
    cfg, arr, B, batch, _, d = CC.case(key)
    worst = 0.0
    for per_slot in (True, False):
        H, f, G, x, ws, st, lim = CC.oracle_solution(key, per_slot)
        args = (H, f, G, d, x, ws, st, lim, batch[1], cfg.nu)
        ld, f64 = KR.certify_batch(*args), KR.certify_batch(*args, dtype=np.float64)
        for k in KR.EXACT:
            assert np.array_equal(np.asarray(ld[k], float), f64[k]), k
        dev, where = KR.deviation(f64, ld, KR.units(H, f, G, d, x, lim, batch[1], cfg.nu))
        print(f"{key} {'slot' if per_slot else 'shared'} limits: float64 is {dev:.3f} eps units from the model ({where})")
        worst = max(worst, dev)
    assert worst <= F64_DEV


def test_host_summary_reduction():
    """kkt_ref.host_summary on a hand-made record: ties go to the lowest slot,
    only OK slots count, r_prim is not scaled."""
    cfg = cmpc.reference_config("par", "coop", p=CC.P)
    F = cmpc.certify_fields(CmpcDims.from_config(cfg, 3))
    rec = np.zeros((cmpc.certify_len(CmpcDims.from_config(cfg, 3)), 6))
    rec[F["scale"].start] = [2.0, 4.0, 2.0, 1.0, 2.0, 2.0]
    rec[F["status"].start] = [0, 0, 0, 2, 0, 0]
    rec[F["r_stat"].start] = [1.0, 2.0, 1.0, 100.0, 0.5, 0.0]     # / scale: .5 .5 .5 - .25 0
    rec[F["r_prim"].start] = [0.0, 0.0, 3.0, 9.0, 3.0, 0.0]
    s = KR.host_summary(rec, F, 0.3)
    assert (s["r_stat"], s["slot_stat"]) == (0.5, 0) and (s["r_prim"], s["slot_prim"]) == (3.0, 2)
    assert (s["r_dual"], s["slot_dual"]) == (0.0, 0) and s["n_not_ok"] == 1 and s["n_above"] == 4
    rec[F["status"].start] = 2
    s = KR.host_summary(rec, F, 0.3)
    assert s["slot_stat"] == -1 and s["r_stat"] == 0.0 and s["n_not_ok"] == 6 and s["n_above"] == 0
