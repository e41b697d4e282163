"""Every solve kernel on dense, active-set-heavy QPs (tests/solver_cases.py),
bit for bit against the oracle on identical inputs.  Marked gpu; runs on an
MI355X.

The oracle (jacobi_ref.oracle_jacobi, or_qp.c's map form) is run on the QPs
the device itself built (download_qp) and on the device's state before the
step, so nothing is excused: no near-tie allowance, no slot left out.
Compared per step: the plans, statuses, change counts and working sets of the
last iteration, u_old and du_old after the step, and the working-set change
sequence of every Jacobi iteration.

  a  the lane and the row iterate kernels, every case x regime, and
     init_warmstart against the oracle's cold solve
  b  the four fused step instances of kernel_dims.h (SWL, SWR, SRL, SRR), each
     at the smallest B at which cmpc.plan reports it under CMPC_STEP_FUSED
     (the large batches repeat the case's 37 scenarios): fused == build +
     iterate bit for bit, and the fused run against the oracle
  c  the stand-alone batch solvers, all five instances
  d  the device's final plans against an optimum that owes nothing to the
     algorithm: the KKT certificate of test_solver_kkt.py at 1e-9 on the
     device's own H, f, G with the gradient f + G d, d downloaded after
     iterate(K - 1); the enumeration of every working set for nV <= 4; and
     iterate(K - 1) + iterate(1) == iterate(K)

What the cases are worth (coverage, statuses, difficulty, the oracle against
the optimum) is checked without a GPU in test_solver_cases.py.
"""
import numpy as np
import pytest

import _oracle as O
import cmpc
import jacobi_ref as JR
import solver_cases as SC
from cmpc._abi import CmpcDims
from test_solver_kkt import kkt_certificate_batch

pytestmark = pytest.mark.gpu

LANE, ROWS = cmpc.CMPC_SOLVE_LANE, cmpc.CMPC_SOLVE_ROWS
SOLVERS = {"lane": LANE, "rows": ROWS}
NAMES = ("plans", "status", "nchg", "ws", "u_old", "du_old")
CERT_TOL = 1e-9   # test_solver_kkt.py's; measured on an MI355X: every certificate below passes at 1e-13

case_regimes = [(c, r) for c in SC.CASES for r in SC.REGIMES]
cr_id = lambda cr: SC.case_id(cr[0]) + "-" + cr[1]


def device_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def tiled(a, reps, n):
    return None if a is None else np.ascontiguousarray(np.concatenate([a] * reps)[:n])


def inputs(case, regime, B=SC.B):
    """(lin, u_old, ws, limits) of a case and regime for B scenarios: the
    case's 37 scenarios, repeated in order where B is larger"""
    c = SC.problem(case)
    S = c["cfg"].S
    lin, ws, limits = SC.regime_inputs(case, regime)
    reps = -(-B // SC.B)
    t = lambda a: tiled(a, reps, B * S)
    return t(lin), t(c["u_old"]), t(ws), None if limits is None else tuple(t(a) for a in limits)


def open_ctx(cfg, arr, lin, u_old, ws, limits):
    nq = lin.shape[0]
    ctx = cmpc.Context(cfg, nq // cfg.S)
    ctx.configure(arr)
    ctx.set_state(u_old, np.zeros((nq, cfg.nV)), ws)
    ctx.upload_lin(lin)
    if limits is not None:
        ctx.set_scenario_constraints(*limits)
    return ctx


def results(ctx, K):
    d, st, nw = ctx.download()
    tr, ntr = ctx.download_trace(K)
    u, du, ws = ctx.get_state()
    return dict(plans=d.reshape(du.shape), status=st, nchg=nw, ws=ws, u_old=u, du_old=du, trace=tr, ntrace=ntr)


def assert_same(a, b, what, names=NAMES):
    """two results dicts bit for bit, the traces up to their lengths"""
    for name in names:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        assert x.shape == y.shape, (what, name, x.shape, y.shape)
        assert np.array_equal(x, y), (what, name, np.flatnonzero((x != y).reshape(len(x), -1).any(1))[:8])
    assert np.array_equal(a["ntrace"], b["ntrace"]), (what, "ntrace", np.flatnonzero((a["ntrace"] != b["ntrace"]).any(1))[:8])
    live = np.arange(16)[None, None, :] < a["ntrace"][:, :, None]
    differ = live & (a["trace"] != b["trace"])
    assert not differ.any(), (what, "trace", np.flatnonzero(differ.any(axis=(1, 2)))[:8])


def oracle_step(cfg, arr, qp, state, K, limits, log=None):
    """The oracle's step on the device's QPs and the device's state before the
    step: the results dict the device must return"""
    H, f, G = qp
    u0, du0, ws0 = state
    with np.errstate(all="ignore"):
        x, st, nw, ws, tr, ntr = JR.oracle_jacobi(cfg, arr, H, f, G, u0, du0, ws0, K, limits=limits, log=log)
    u = u0.copy()
    u[:, :cfg.nu] += x[:, :cfg.nu]
    return dict(plans=x, status=st, nchg=nw, ws=ws.astype(np.uint32), u_old=u, du_old=x, trace=tr, ntrace=ntr)


def first_scenarios(res, nq):
    return {k: v[:nq] for k, v in res.items()}


def assert_repeats(res, nq, what):
    """a batch that repeats its first nq slots returns their results repeated"""
    for k, v in res.items():
        if v is None:
            continue
        n = v.shape[0]
        want = tiled(v[:nq], -(-n // nq), n)
        assert np.array_equal(v, want, equal_nan=v.dtype.kind == "f"), (what, k)


# ---- a. the iterate kernels -------------------------------------------------------

@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("cr", case_regimes, ids=cr_id)
def test_gpu_iterate_kernels_on_dense_qps(cr, solver):
    case, regime = cr
    c = SC.problem(case)
    cfg, arr, K = c["cfg"], c["arr"], c["K"]
    lin, u_old, ws, limits = inputs(case, regime)
    changes = 0
    with open_ctx(cfg, arr, lin, u_old, ws, limits) as ctx:
        ctx.set_solve_variant(SOLVERS[solver])
        for step in range(SC.STEPS):
            ctx.build()
            qp = ctx.download_qp()
            state = ctx.get_state()
            ctx.iterate(K, SC.FLAGS)
            assert ctx.last_solve_kernel() == SOLVERS[solver]
            dev = results(ctx, K)
            assert_same(dev, oracle_step(cfg, arr, qp, state, K, limits), (cr_id(cr), solver, step))
            changes += int(dev["ntrace"].sum())
    print(f"{cr_id(cr)} {solver}: {changes} traced working-set changes, final statuses "
          f"{np.bincount(dev['status'], minlength=5).tolist()}")
    if regime == "failure":
        assert len(np.unique(dev["status"])) >= 4 and (dev["status"] == 0).mean() >= 0.5


@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_gpu_init_warmstart_on_dense_qps(case, solver):
    """init_warmstart: the working sets of the cold solve of (H, f), the
    oracle's O.qp_solve, with the shared and with per-slot limits"""
    c = SC.problem(case)
    cfg, arr = c["cfg"], c["arr"]
    for regime in ("natural", "failure"):
        lin, u_old, _, limits = inputs(case, regime)
        nq = lin.shape[0]
        with open_ctx(cfg, arr, lin, u_old, np.zeros(nq, np.uint32), limits) as ctx:
            ctx.set_solve_variant(SOLVERS[solver])
            ctx.build()
            H, f, _ = ctx.download_qp()
            ctx.init_warmstart()
            assert ctx.last_solve_kernel() == SOLVERS[solver]
            _, _, ws = ctx.get_state()
        lb, ub, lbA, ubA = JR.slot_bounds(cfg, arr, u_old, limits)
        want = np.zeros(nq, np.uint32)
        with np.errstate(all="ignore"):
            for q in range(nq):
                want[q] = O.qp_solve(H[q], f[q], lb[q], ub[q], lbA[q], ubA[q], cfg.nu, 0)[1].ws
        assert np.array_equal(ws, want), (regime, np.flatnonzero(ws != want)[:8])
        assert (want != 0).any()


# ---- b. the fused steps ------------------------------------------------------------

WAVE, RBUILD = cmpc.CMPC_BUILD_WAVE, cmpc.CMPC_BUILD_ROWS
FUSED = {  # instance: (build dimension set, build kernel, solver); kernel_dims.h
    "SWL": ((11, 3, 2, 2), WAVE, LANE), "SWR": ((11, 3, 4, 2), WAVE, ROWS),
    "SRL": ((11, 3, 2, 2), RBUILD, LANE), "SRR": ((10, 4, 4, 2), RBUILD, ROWS)}
# B: None = the smallest the library's plan reports the instance at; the wave
# instances (smallest B: 1) also at the cases' own 37 scenarios
FUSED_RUNS = [("SWL", None, "natural"), ("SWL", None, "adversarial"), ("SWL", SC.B, "natural"),
              ("SWL", SC.B, "adversarial"), ("SWL", SC.B, "failure"),
              ("SWR", None, "natural"), ("SWR", None, "adversarial"), ("SWR", SC.B, "natural"),
              ("SWR", SC.B, "adversarial"), ("SWR", SC.B, "failure"),
              ("SRL", None, "natural"), ("SRL", None, "adversarial"),
              ("SRR", None, "natural"), ("SRR", None, "adversarial"), ("SRR", None, "failure")]


def fused_plan(cfg, B, cus, K):
    pl = cmpc.plan(CmpcDims.from_config(cfg, B), cus, step=cmpc.CMPC_STEP_FUSED, K=K, flags=cmpc.CMPC_TRACE)
    return (pl.step_build_kernel, pl.step_solve_kernel) if pl.step_fused and not pl.step_error else None


def smallest_batch(cfg, kind, cus, K, limit=1 << 14):
    for B in range(1, limit):
        if fused_plan(cfg, B, cus, K) == kind:
            return B
    raise AssertionError(f"no batch below {limit} scenarios gets the fused instance {kind}")


def run_steps(cfg, arr, K, ins, variant, build=None, solve=None):
    """three cmpc_step calls; per step the state before, the results and the QPs"""
    out = []
    with open_ctx(cfg, arr, *ins) as ctx:
        ctx.set_step_variant(variant)
        if build is not None:
            ctx.set_build_variant(build)
        if solve is not None:
            ctx.set_solve_variant(solve)
        for _ in range(SC.STEPS):
            state = ctx.get_state()
            ctx.step(K, SC.FLAGS)
            kernels = (ctx.last_step_fused(), ctx.last_build_kernel(), ctx.last_solve_kernel())
            out.append((state, results(ctx, K), ctx.download_qp(), kernels))
    return out


@pytest.mark.parametrize("inst,B,regime", FUSED_RUNS, ids=lambda v: "min" if v is None else str(v))
def test_gpu_fused_steps_on_dense_qps(inst, B, regime):
    ds, build, solver = FUSED[inst]
    case = (ds, max(SC.SCALES))
    c = SC.problem(case)
    cfg, arr, K = c["cfg"], c["arr"], c["K"]
    cus = device_cus()
    if B is None:
        B = smallest_batch(cfg, (build, solver), cus, K)
    assert fused_plan(cfg, B, cus, K) == (build, solver)
    ins = inputs(case, regime, B)
    limits = ins[3]
    fused = run_steps(cfg, arr, K, ins, cmpc.CMPC_STEP_FUSED)
    split = run_steps(cfg, arr, K, ins, cmpc.CMPC_STEP_SPLIT, build=build, solve=solver)
    nq = min(B, SC.B) * cfg.S
    lim0 = None if limits is None else tuple(a[:nq] for a in limits)
    for step, ((state, dev, qp, kernels), (_, sdev, sqp, skernels)) in enumerate(zip(fused, split)):
        assert kernels == (True, build, solver), (step, kernels)
        assert skernels == (False, build, solver), (step, skernels)
        assert_same(sdev, dev, (inst, "fused against build + iterate", step))
        for name, a, b in zip("HfG", sqp, qp):
            assert np.array_equal(a, b, equal_nan=True), (inst, step, name)
        # a batch of repeated scenarios: every copy equals the first, which the oracle checks
        assert_repeats(dev, nq, (inst, step))
        assert_repeats(dict(zip("HfG", qp)), nq, (inst, step))
        want = oracle_step(cfg, arr, tuple(a[:nq] for a in qp), tuple(a[:nq] for a in state), K, lim0)
        assert_same(first_scenarios(dev, nq), want, (inst, "fused against the oracle", step))
    st = fused[-1][1]["status"]
    print(f"{inst} ({SC.case_id(case)}, {regime}) at B = {B} on {cus} CUs: "
          f"{sum(int(s[1]['ntrace'][:nq].sum()) for s in fused)} traced changes in the distinct scenarios, final "
          f"statuses {np.bincount(st[:nq], minlength=5).tolist()}")


# ---- c. the stand-alone batch solvers ---------------------------------------------------

def _batch_inputs(case):
    c = SC.problem(case)
    cfg = c["cfg"]
    st = SC.natural(case)[0]           # the oracle's QPs at the first step: identical inputs for both solvers
    ws, _ = SC.adversarial_ws(case)
    bounds = JR.slot_bounds(cfg, c["arr"], st["u0"])
    return cfg, st["H"], st["f"], st["G"], bounds, ws


def _assert_solutions(got, want_of, nq, what):
    x, st, nchg, wso, tr, ntr = got
    counts = np.zeros(5, int)
    for q in range(nq):
        xo, info = want_of(q)
        assert st[q] == info.status and nchg[q] == info.nchg and wso[q] == info.ws, (what, q)
        assert ntr[q] == info.ntrace and bytes(tr[q][:ntr[q]]) == bytes(info.trace[:info.ntrace]), (what, q)
        assert np.array_equal(x[q], xo), (what, q, x[q], xo)
        counts[info.status] += 1
    return counts, int(nchg.sum())


@pytest.mark.parametrize("ds", [(11, 3, 2, 2), (10, 4, 2, 2), (11, 3, 4, 2), (10, 4, 4, 2)], ids=str)
def test_gpu_batch_solver_on_dense_qps(ds):
    """cmpc_qp_solve_batch, (n, nu) = (4, 2) and (8, 4): the plain form with
    g = f + G d for Gaussian d, and with g scaled by U(1, 40) per QP"""
    total = np.zeros(5, int)
    for sc in SC.SCALES:
        cfg, H, f, G, (lb, ub, lbA, ubA), ws = _batch_inputs((ds, sc))
        nq, nu = H.shape[0], cfg.nu
        rng = np.random.default_rng(41 + cfg.nV)
        g = f + np.einsum("qac,qc->qa", G, rng.normal(0, 0.05, (nq, cfg.nVo))) if cfg.nVo else f.copy()
        for gg in (g, g * rng.uniform(1, 40, (nq, 1))):
            got = cmpc.qp_solve_batch(H, gg, lb, ub, lbA, ubA, nu, ws)
            counts, chg = _assert_solutions(
                got, lambda q: O.qp_solve(H[q], gg[q], lb[q], ub[q], lbA[q], ubA[q], nu, int(ws[q])), nq, (ds, sc))
            total += counts
            print(f"qp_solve_batch {ds} scale {sc}: statuses {counts.tolist()}, {chg} changes")
    assert total[0] >= 0.5 * total.sum()
    if cfg.nV == 8:
        assert total[cmpc.CMPC_QP_MAX_NWSR] >= 1


@pytest.mark.parametrize("ds", [(11, 3, 2, 2), (10, 4, 2, 2), (11, 3, 2, 3), (11, 3, 2, 1)], ids=str)
def test_gpu_batch_map_solver_on_dense_qps(ds):
    """cmpc_qp_solve_batch_map, (n, nu, nvo) = (4, 2, 4), (6, 2, 6) and
    (2, 2, 2): plans d of three sizes, and f scaled by U(1, 40) per QP"""
    total = np.zeros(5, int)
    for sc in SC.SCALES:
        cfg, H, f, G, (lb, ub, lbA, ubA), ws = _batch_inputs((ds, sc))
        nq, nu = H.shape[0], cfg.nu
        rng = np.random.default_rng(43 + cfg.nV)
        f2 = f * rng.uniform(1, 40, (nq, 1))
        for ff, dscale in ((f, 0.01), (f, 0.2), (f, 2.0), (f2, 0.2)):
            d = rng.normal(0, dscale, (nq, cfg.nVo))
            got = cmpc.qp_solve_batch_map(H, ff, G, d, lb, ub, lbA, ubA, nu, ws)
            counts, chg = _assert_solutions(
                got, lambda q: O.qp_solve_map(H[q], ff[q], G[q], d[q], lb[q], ub[q], lbA[q], ubA[q], nu, int(ws[q])),
                nq, (ds, sc, dscale))
            total += counts
            print(f"qp_solve_batch_map {ds} scale {sc} d ~ {dscale}: statuses {counts.tolist()}, {chg} changes")
    assert total[0] >= 0.5 * total.sum()


# ---- d. the device's plans against an independent optimum -------------------------------

@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("cr", [cr for cr in case_regimes if cr[1] != "failure"], ids=cr_id)
def test_gpu_dense_plans_are_optimal(cr, solver):
    case, regime = cr
    c = SC.problem(case)
    cfg, arr, K = c["cfg"], c["arr"], c["K"]
    n, nu = cfg.nV, cfg.nu
    ins = inputs(case, regime)
    runs = {}
    for split_last in (True, False):
        with open_ctx(cfg, arr, *ins) as ctx:
            ctx.set_solve_variant(SOLVERS[solver])
            for step in range(SC.STEPS):
                ctx.build()
                if split_last and step == SC.STEPS - 1:
                    qp = ctx.download_qp()
                    u0, du0, _ = ctx.get_state()
                    prev = du0
                    if K > 1:
                        ctx.iterate(K - 1, cmpc.CMPC_TRACE)
                        prev = ctx.download()[0].reshape(du0.shape)
                    ctx.iterate(1, SC.FLAGS)
                else:
                    ctx.iterate(K, SC.FLAGS)
                assert ctx.last_solve_kernel() == SOLVERS[solver]
            runs[split_last] = results(ctx, 1 if split_last else K)
    whole, parts = runs[False], runs[True]
    assert_same(dict(whole, trace=whole["trace"][:, K - 1:], ntrace=whole["ntrace"][:, K - 1:]), parts,
                "iterate(K - 1) + iterate(1) against iterate(K)")
    H, f, G = qp
    g = f.copy()
    if cfg.nVo:
        for q in range(len(f)):
            g[q] = f[q] + G[q] @ JR.gather_other(cfg, prev, q)
    ok = parts["status"] == 0
    assert ok.sum() >= 0.5 * len(ok)
    lb, ub, lbA, ubA = JR.slot_bounds(cfg, arr, u0)
    lo, hi = np.concatenate([lb, lbA], 1)[ok], np.concatenate([ub, ubA], 1)[ok]
    x, ws = parts["plans"][ok], parts["ws"][ok]
    C = SC.rows_of(n, nu)
    passed = kkt_certificate_batch(H[ok], g[ok], lo, hi, C, x, ws, tol=CERT_TOL)
    tol = CERT_TOL
    while passed.all() and tol > 1e-16 and kkt_certificate_batch(H[ok], g[ok], lo, hi, C, x, ws, tol=tol / 10).all():
        tol /= 10
    print(f"{cr_id(cr)} {solver}: {ok.sum()} OK solves, every certificate passes at {tol:g}")
    assert passed.all(), np.flatnonzero(ok)[~passed][:8]
    if n <= 4:
        for q in range(len(x)):
            pts = SC.enumerate_optimum(H[ok][q], g[ok][q], lo[q], hi[q], nu)
            assert len(pts), q
            xscale = 1e-9 * (1.0 + np.abs(pts[0]).max())
            assert np.abs(pts - pts[0]).max() <= xscale and np.abs(x[q] - pts[0]).max() <= xscale, q
