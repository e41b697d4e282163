"""The dense solver cases (tests/solver_cases.py) on the oracle alone: what
test_gpu_dense_solver.py relies on when it holds the solve kernels to the
oracle bit for bit.  No GPU.

  coverage     per case and regime the oracle's traces show at least half the
               working-set activity measured when the seeds were chosen
               (solver_cases.MEASURED): changes, drops after an add within one
               solve, solves with >= 5 changes, slots whose working set fills,
               cold starts from a dependent warm start
  statuses     natural and adversarial: every solve OK, but for MAX_NWSR in the
               adversarial regime; failure: INFEASIBLE, NOT_PD, NONFINITE and
               (where solver_cases.CAN_MAX_NWSR) MAX_NWSR all occur, half or
               more of the slots stay OK, and some sub-controller fails while
               its partner solves on with the exchanged zero move
  difficulty   median cond(H) >= 100, median largest off-diagonal >= 1e-2 of
               the largest diagonal entry
  optimum      every OK solve of a step's last iteration carries the KKT
               certificate of test_solver_kkt.py at its 1e-9 (measured: all
               pass at CERT_TIGHTEST), with the gradient f + G d, d the other
               sub-controllers' plans of iteration K - 1; for nV <= 4 the
               enumeration of every working set gives the same point within
               1e-9 (1 + max|x|)
  sensitivity  with H's entry pair (0, nV - 1) set to zero the oracle's plans
               move by more than 1e-6 relative in half or more of the slots; on
               the par-coop plant batch of test_gpu_small_batch.JCASES the same
               edit moves (printed, for the record) next to nothing: the error
               the plant data hides
"""
import dataclasses

import numpy as np
import pytest

import cmpc
import jacobi_ref as JR
import solver_cases as SC
from test_solver_kkt import enumerate_optimum, kkt_certificate_batch

OK = cmpc.CMPC_QP_OK
CERT_TOL = 1e-9         # test_solver_kkt.py's
CERT_TIGHTEST = 1e-12   # the tightest decade at which every certificate below passed when measured

case_regimes = [(c, r) for c in SC.CASES for r in SC.REGIMES]
cr_id = lambda cr: SC.case_id(cr[0]) + "-" + cr[1]


@pytest.mark.parametrize("cr", [cr for cr in case_regimes if cr[1] != "failure"], ids=cr_id)
def test_coverage_floors(cr):
    case, regime = cr
    cfg = SC.problem(case)["cfg"]
    cov = SC.coverage(cfg, SC.oracle_run(case, regime))
    got = tuple(cov[k] for k in SC.COVERAGE_KEYS)
    measured = SC.MEASURED[SC.case_id(case)][regime]
    floors = SC.floors(case, regime)
    print(f"{cr_id(cr)}: {dict(zip(SC.COVERAGE_KEYS, got))}, largest working set {cov['max_active']}, "
          f"MAX_NWSR solves {cov['max_nwsr']}; measured {measured}, floors {floors}")
    for k, g, fl in zip(SC.COVERAGE_KEYS, got, floors):
        assert g >= fl, (k, g, fl)
        if fl == 0:   # only where the regime or the dimension set cannot produce it (solver_cases.floors)
            assert (k == "cold_starts" and regime == "natural") or (k == "full_slots" and cfg.nV == 8) \
                or (k in SC.NV2_CANNOT and cfg.nV == 2), k
    if cfg.nV == 8:
        assert cov["max_active"] >= 4
        if regime == "adversarial" and case[1] == max(SC.SCALES):
            assert cov["max_nwsr"] >= 1


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_statuses(case):
    c = SC.problem(case)
    cfg, S = c["cfg"], c["cfg"].S
    for st in SC.oracle_run(case, "natural"):
        assert (st["log"]["status"] == OK).all()
    for st in SC.oracle_run(case, "adversarial"):
        s = st["log"]["status"]
        assert ((s == OK) | (s == cmpc.CMPC_QP_MAX_NWSR)).all()
    run = SC.oracle_run(case, "failure")
    every = np.concatenate([st["log"]["status"].ravel() for st in run])
    counts = np.bincount(every, minlength=5)
    print(f"{SC.case_id(case)} failure: solves per status {counts.tolist()}, final "
          f"{np.bincount(run[-1]['out'][1], minlength=5).tolist()}")
    for code in (cmpc.CMPC_QP_INFEASIBLE, cmpc.CMPC_QP_NOT_PD, cmpc.CMPC_QP_NONFINITE):
        assert all((st["out"][1] == code).any() for st in run), code
    if cfg.nV in SC.CAN_MAX_NWSR:
        assert counts[cmpc.CMPC_QP_MAX_NWSR] >= 1
    for q, field, _ in SC.POISON:
        want = cmpc.CMPC_QP_NOT_PD if field == "A" else cmpc.CMPC_QP_NONFINITE
        assert all(st["out"][1][q] == want for st in run), (q, field)
    for st in run:
        fin, plans = st["out"][1], st["out"][0]
        assert (fin == OK).mean() >= 0.5
        assert (plans[fin != OK] == 0.0).all()
        if S == 2:   # one sub-controller fails, its partner goes on with the exchanged zero move
            pair = fin.reshape(-1, 2)
            assert (((pair[:, 0] != OK) & (pair[:, 1] == OK)) | ((pair[:, 0] == OK) & (pair[:, 1] != OK))).any()
    # the failing slots sit among healthy ones: inside the first wave and inside one 16-slot group
    fin = run[-1]["out"][1]
    assert (fin[:16] != OK).any() and (fin[:16] == OK).any() and (fin[16:32] != OK).any() and (fin[16:32] == OK).any()


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_difficulty(case):
    cond, off = SC.difficulty(SC.natural(case)[0]["H"])
    print(f"{SC.case_id(case)}: median cond(H) {cond:.3g}, median largest off-diagonal / diagonal {off:.3g}")
    assert cond >= 100 and off >= 1e-2


def _ok_qps(cfg, c, st, limits):
    ok = st["out"][1] == OK
    lb, ub, lbA, ubA = JR.slot_bounds(cfg, c["arr"], st["u0"], limits)
    lo, hi = np.concatenate([lb, lbA], 1), np.concatenate([ub, ubA], 1)
    g = SC.last_gradient(cfg, st)
    return ok, st["H"][ok], g[ok], lo[ok], hi[ok], st["out"][0][ok], st["out"][3][ok]


@pytest.mark.parametrize("cr", case_regimes, ids=cr_id)
def test_oracle_reaches_the_optimum(cr):
    case, regime = cr
    c = SC.problem(case)
    cfg = c["cfg"]
    n, nu = cfg.nV, cfg.nu
    C = SC.rows_of(n, nu)
    _, _, limits = SC.regime_inputs(case, regime)
    tightest = 0.0
    for i, st in enumerate(SC.oracle_run(case, regime)):
        ok, H, g, lo, hi, x, ws = _ok_qps(cfg, c, st, limits)
        assert ok.sum() >= 0.5 * len(ok)
        assert kkt_certificate_batch(H, g, lo, hi, C, x, ws, tol=CERT_TOL).all(), i
        tol = CERT_TOL
        while tol > 1e-16 and kkt_certificate_batch(H, g, lo, hi, C, x, ws, tol=tol / 10).all():
            tol /= 10
        tightest = max(tightest, tol)
        if n <= 4:
            for q in range(len(x)):
                pts = SC.enumerate_optimum(H[q], g[q], lo[q], hi[q], nu)
                assert len(pts), (i, q)
                xscale = 1e-9 * (1.0 + np.abs(pts[0]).max())
                # the failure regime's boxes are 1e-4 wide and the enumeration accepts multipliers down to
                # -1e-9 (max|H| + max|g| + 1), which there is a multiplier's own size: it finds neighbouring
                # vertices as well, and the oracle's point has to be one of its points
                if regime != "failure":
                    assert np.abs(pts - pts[0]).max() <= xscale, (i, q)
                assert np.abs(pts - x[q]).max(axis=1).min() <= xscale, (i, q)
            if regime == "failure":   # a slot the oracle calls infeasible has no KKT point
                bad = np.flatnonzero(st["out"][1] == cmpc.CMPC_QP_INFEASIBLE)[:4]
                lb, ub, lbA, ubA = JR.slot_bounds(cfg, c["arr"], st["u0"], limits)
                gg = SC.last_gradient(cfg, st)
                for q in bad:
                    assert not len(SC.enumerate_optimum(st["H"][q], gg[q], np.concatenate([lb[q], lbA[q]]),
                                                        np.concatenate([ub[q], ubA[q]]), nu))
    print(f"{cr_id(cr)}: every certificate passes at {tightest:g}")
    assert tightest <= CERT_TOL


def test_batched_enumeration_is_the_enumeration():
    """solver_cases.enumerate_optimum finds the points of
    test_solver_kkt.enumerate_optimum (a few slots, nV = 4 and nV = 2)"""
    for case in (SC.CASES[1], ((11, 3, 2, 1), 0.3)):
        c = SC.problem(case)
        cfg = c["cfg"]
        st = SC.oracle_run(case, "adversarial")[-1]
        ok, H, g, lo, hi, x, ws = _ok_qps(cfg, c, st, None)
        C = SC.rows_of(cfg.nV, cfg.nu)
        for q in (0, 7, 30):
            _, ref = enumerate_optimum(H[q], g[q], lo[q], hi[q], C)
            got = SC.enumerate_optimum(H[q], g[q], lo[q], hi[q], cfg.nu)
            assert len(ref) == len(got) and np.abs(np.array(ref) - got).max() <= 1e-12 * (1 + np.abs(got).max())


def _edit_sensitivity(cfg, arr, H, f, G, u, K):
    """fraction of the slots whose plans move by more than 1e-6 relative when
    H's entry pair (0, nV - 1) is set to zero, and the median relative change"""
    nq, n = H.shape[0], cfg.nV
    H2 = H.copy()
    H2[:, 0, n - 1] = H2[:, n - 1, 0] = 0.0
    zero = np.zeros((nq, n)), np.zeros(nq, np.uint32)
    x = JR.oracle_jacobi(cfg, arr, H, f, G, u, zero[0], zero[1], K)[0]
    x2 = JR.oracle_jacobi(cfg, arr, H2, f, G, u, zero[0], zero[1], K)[0]
    rel = np.abs(x - x2).max(axis=1) / np.maximum(np.abs(x).max(axis=1), 1e-300)
    return float((rel > 1e-6).mean()), float(np.median(rel))


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_a_wrong_hessian_entry_shows(case):
    c = SC.problem(case)
    st = SC.natural(case)[0]
    frac, med = _edit_sensitivity(c["cfg"], c["arr"], st["H"], st["f"], st["G"], st["u0"], c["K"])
    print(f"{SC.case_id(case)}: H[0, nV-1] = 0 moves the plans of {frac:.2f} of the slots by > 1e-6, median {med:.3g}")
    assert frac >= 0.5


def test_plant_data_hides_a_wrong_hessian_entry():
    """For the record (printed, no bar): the same edit on the par-coop plant
    batch of test_gpu_small_batch.JCASES (p = 20, tight 0.3)."""
    from cmpc.configs import reference_setup
    from cmpc.synthetic import synthetic_batch
    cfg = cmpc.reference_config("par", "coop", p=20, m=2)
    arr = cmpc.controller_arrays(cfg, reference_setup("par", "coop"))
    arr = dataclasses.replace(arr, lower=arr.lower * 0.3, upper=arr.upper * 0.3, rate_lower=arr.rate_lower * 0.3,
                              rate_upper=arr.rate_upper * 0.3)
    lin, u, _, _ = synthetic_batch(cfg, 96, seed=70 + 20 + 2, n_distinct=96)
    H, f, G = SC.oracle_qps(cfg, arr, lin, u)
    frac, med = _edit_sensitivity(cfg, arr, H, f, G, u, 9)
    cond, off = SC.difficulty(H)
    print(f"par-coop plant batch: H[0, nV-1] = 0 moves the plans of {frac:.2f} of the slots by > 1e-6, median "
          f"{med:.3g}; median cond(H) {cond:.3g}, largest off-diagonal / diagonal {off:.3g}")
