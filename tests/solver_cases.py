"""Dense, active-set-heavy QPs for every solve kernel.  TEST INFRASTRUCTURE ONLY.

The plant-derived QPs of the other solver tests have cond(H) ~ 10 and
off-diagonals of 3e-4 of the diagonal (R = 2e5 dominates H), and their working
sets almost never change.  These cases are dense_ref.dense_problem draws
(dense A, Bin, C, dense SPD weights, O(1) data): cond(H) 1e2 to 1e3, off-diagonals
0.01 to 0.4 of the diagonal and tens to hundreds of working-set changes per
step.  Built on the CPU, cached per process, read-only.  What
test_gpu_dense_solver.py relies on is checked on the oracle alone in
test_solver_cases.py.

Shapes: p = 17 (the solver does not see p), B = 37 scenarios = 74 or 37 slots
(the lane kernel's 64-lane wave, the row kernel's four QPs per wave and the
16-QP groups all end partly filled), K = 9 (distributed) or 3 (centralized),
three closed-loop steps with the first move applied.

Regimes:
  natural      empty working sets before step 0, then each step's own
  adversarial  before step 0 the working-set words of adversarial_ws
  failure      adversarial words, per-slot limits (certify_cases.deal_limits:
               class 6 infeasible, classes 5 and 7 bound and rate both tight,
               wide or mildly tight otherwise) and three poisoned records
               (POISON); with S = 2 the infeasible class falls on
               sub-controller 0 only, whose partner goes on solving with the
               exchanged zero move

The working-set word holds one side bit per row, so "both sides of one row"
cannot be written into it; the dependent class is the bound of input j with
rate row j (both normals e_j, j < nu) and, for m >= 2, the bounds j and j + nu
with rate row j + nu (e_{j+nu} - e_j).
"""
import numpy as np

import _oracle as O
import certify_cases as CC
import cmpc
import dense_ref as DR
import jacobi_ref as JR

P, B, STEPS = 17, 37, 3
RHO = {2: 0.95, 4: 1.05, 6: 1.05, 8: 0.95}   # spectral radius of A, by nV


def delays_of(ds):
    """The delayed inputs' last move acts in the horizon's last step only
    (D = p - m).  With the reference's delays of 40 the delayed inputs never
    act: their diagonal entries of H are uwt's alone, cond(H) is 1e3 but the
    entry pair (0, nV - 1) of H is exactly zero and the 2 x 2 Hessians of m = 1
    have off-diagonals of 3e-4 of the diagonal.  With short delays
    (0, 8, 0, 12) cond(H) falls to 6 .. 35.  With D = p - m every entry of H
    holds a Gram term and, at the spectral radius RHO = 1.05 of A (over 17
    steps a growth of 2.3; the solver sees H alone), the median cond(H) is 110
    to 1 700.  D >= 14 also keeps the row build free of ring lines
    (p <= 2 D + 1), which its fused step with the lane solver needs."""
    return (0, P - ds[3], 0, P - ds[3])


SCALES = (0.03, 0.3)
REGIMES = ("natural", "adversarial", "failure")
FLAGS = cmpc.CMPC_APPLY_MOVE | cmpc.CMPC_TRACE

# build set -> solve set (kernel_dims.h).  The seed of a case (_SEEDS, per
# scale) is the first from 777 on with which the natural regime has no status
# but OK, the median cond(H) is >= 100 and the median largest off-diagonal
# >= 1e-2 of the diagonal, H's entry pair (0, nV - 1) matters to half the slots
# and no coverage figure that the set can produce is zero (what
# test_solver_cases.py asserts).
DIMSETS = {(11, 3, 2, 2): (4, 2, 4), (10, 4, 2, 2): (4, 2, 4), (11, 3, 4, 2): (8, 4, 0), (10, 4, 4, 2): (8, 4, 0),
           (11, 3, 2, 1): (2, 2, 2), (11, 3, 2, 3): (6, 2, 6)}
CASES = [(ds, sc) for ds in DIMSETS for sc in SCALES]
_SEEDS = {(11, 3, 2, 2): (780, 778), (10, 4, 2, 2): (777, 777), (11, 3, 4, 2): (777, 782), (10, 4, 4, 2): (777, 787),
          (11, 3, 2, 1): (804, 804), (11, 3, 2, 3): (782, 778)}
SEEDS = {(ds, sc): _SEEDS[ds][i] for ds in DIMSETS for i, sc in enumerate(SCALES)}

# Coverage measured on the oracle with these seeds (coverage() below), per case
# and regime: (working-set changes, drops that follow an add within one solve,
# solves with >= 5 changes, slots whose working set reaches nV rows, cold
# starts from a dependent warm start), over the three steps; the floor that
# test_solver_cases.py asserts is half of each, rounded up (floors()).  What a
# set or a regime cannot produce has no floor: cold starts in the natural
# regime (its warm starts are the solver's own working sets), a solve of five
# changes for nV = 2 (at most two active rows; none in 36 seeds), a full working
# set for nV = 8 in the natural regime (0 to 2 slots; required instead: at
# least 4 active rows, and at scale 0.3 a MAX_NWSR solve in the adversarial
# regime).  MAX_NWSR: nV = 8 and 6 produce it in the failure regime of every
# case (CAN_MAX_NWSR, asserted); nV = 4 in one or two cases only and nV = 2,
# with at most two active rows, in none, so neither is asserted.
COVERAGE_KEYS = ("changes", "late_drops", "long_solves", "full_slots", "cold_starts")
MEASURED = {   # measured; then: floors natural / adversarial; largest working set natural / adversarial
    "11-3-2-2-s0.03": {"natural": (626, 13, 17, 26, 0), "adversarial": (784, 13, 35, 41, 28)},     # 313 7 9 13 0 / 392 7 18 21 14; 4 / 4
    "11-3-2-2-s0.3": {"natural": (673, 49, 27, 61, 0), "adversarial": (811, 52, 59, 62, 31)},      # 337 25 14 31 0 / 406 26 30 31 16; 4 / 4
    "10-4-2-2-s0.03": {"natural": (747, 9, 25, 22, 0), "adversarial": (905, 9, 38, 41, 31)},       # 374 5 13 11 0 / 453 5 19 21 16; 4 / 4
    "10-4-2-2-s0.3": {"natural": (620, 31, 20, 53, 0), "adversarial": (766, 33, 55, 59, 31)},      # 310 16 10 27 0 / 383 17 28 30 16; 4 / 4
    "11-3-4-2-s0.03": {"natural": (100, 3, 1, 1, 0), "adversarial": (243, 3, 17, 13, 15)},         # 50 2 1 - 0 / 122 2 9 7 8; 8 / 8
    "11-3-4-2-s0.3": {"natural": (450, 47, 43, 11, 0), "adversarial": (574, 49, 53, 19, 17)},      # 225 24 22 - 0 / 287 25 27 10 9; 8 / 8
    "10-4-4-2-s0.03": {"natural": (98, 5, 3, 0, 0), "adversarial": (243, 5, 19, 12, 15)},          # 49 3 2 - 0 / 122 3 10 6 8; 6 / 8
    "10-4-4-2-s0.3": {"natural": (390, 35, 43, 2, 0), "adversarial": (524, 43, 53, 13, 19)},       # 195 18 22 - 0 / 262 22 27 7 10; 8 / 8
    "11-3-2-1-s0.03": {"natural": (272, 3, 0, 29, 0), "adversarial": (369, 3, 0, 47, 22)},         # 136 2 0 15 0 / 185 2 0 24 11; 2 / 2
    "11-3-2-1-s0.3": {"natural": (293, 7, 0, 65, 0), "adversarial": (386, 9, 0, 68, 22)},          # 147 4 0 33 0 / 193 5 0 34 11; 2 / 2
    "11-3-2-3-s0.03": {"natural": (1104, 35, 53, 13, 0), "adversarial": (1322, 35, 86, 34, 33)},   # 552 18 27 7 0 / 661 18 43 17 17; 6 / 6
    "11-3-2-3-s0.3": {"natural": (976, 61, 69, 39, 0), "adversarial": (1155, 66, 82, 49, 35)},     # 488 31 35 20 0 / 578 33 41 25 18; 6 / 6
}
# MAX_NWSR solves, adversarial / failure regime, in the table's order: 0/0 2/3 0/0 1/0 2/9 13/13 0/10 13/12 0/0 0/0
# 0/16 16/14.  Median cond(H): 225 168 157 157 644 471 619 932 138 138 189 236; median largest off-diagonal over the
# largest diagonal entry: 0.11 0.12 0.11 0.11 0.36 0.32 0.35 0.29 0.014 0.014 0.18 0.15.
NV2_CANNOT = ("long_solves",)
CAN_MAX_NWSR = (6, 8)


def floors(case, regime):
    """half of MEASURED, rounded up; none for a full working set at nV = 8 in
    the natural regime"""
    out = [(v + 1) // 2 for v in MEASURED[case_id(case)][regime]]
    if DIMSETS[case[0]][0] == 8 and regime == "natural":
        out[COVERAGE_KEYS.index("full_slots")] = 0
    return tuple(out)


# slot, record field, value: a NaN in y_prev (f only: NONFINITE), a NaN in A
# (H and f: NOT_PD), an Inf in a delay state (f only: NONFINITE); slots of the
# wide limit classes 0, 2 and 4, inside the first wave and, 16 and 20, inside
# one 16-slot group with the infeasible slot 22 and healthy ones
POISON = ((16, "y", np.nan), (10, "A", np.nan), (20, "x", np.inf))


def case_id(case):
    ds, sc = case
    return "-".join(map(str, ds)) + f"-s{sc:g}"


def K_of(cfg):
    return 9 if cfg.S > 1 else 3


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


_cache = {}


def problem(case):
    """dict(cfg, arr, lin, u_old, K): the dense draw of one case"""
    key = ("problem", case)
    if key not in _cache:
        ds, sc = case
        cfg = DR.config_for(ds, P, delays_of(ds))
        assert (cfg.nV, cfg.nu, cfg.nVo) == DIMSETS[ds]
        lin, u_old, arr = DR.dense_problem(cfg, B, SEEDS[case], rho=RHO[cfg.nV], scale=sc)
        _freeze(lin, u_old)
        _cache[key] = dict(cfg=cfg, arr=arr, lin=lin, u_old=u_old, K=K_of(cfg))
    return _cache[key]


def oracle_qps(cfg, arr, lin, u_old):
    dims = DR.dims_of(cfg, 1)
    out = [O.build_qp(dims, lin[q], u_old[q], arr.y_ref[q % cfg.S], arr.ywt[q % cfg.S], arr.uwt[q % cfg.S])
           for q in range(lin.shape[0])]
    nq = lin.shape[0]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]),
            np.stack([o[4] for o in out]).reshape(nq, cfg.nV, -1))


def oracle_loop(cfg, arr, lin, u_old, ws, K, limits=None, steps=STEPS):
    """The closed loop on the oracle alone: per step the oracle's QPs at the
    current u_old, the Jacobi loop (jacobi_ref), du_old = the plans and the
    first move added to the own inputs.  Returns per step dict(H, f, G, u0,
    du0, ws0, out=(plans, status, nchg, ws, trace, ntrace), log)."""
    nq = lin.shape[0]
    u, du, ws = u_old.copy(), np.zeros((nq, cfg.nV)), np.array(ws, np.uint32)
    res = []
    with np.errstate(all="ignore"):
        for _ in range(steps):
            H, f, G = oracle_qps(cfg, arr, lin, u)
            log = {}
            out = JR.oracle_jacobi(cfg, arr, H, f, G, u, du, ws, K, limits=limits, log=log)
            res.append(dict(H=H, f=f, G=G, u0=u.copy(), du0=du.copy(), ws0=ws.copy(), out=out, log=log))
            du, ws = out[0].copy(), out[3].astype(np.uint32)
            u = u.copy()
            u[:, :cfg.nu] += du[:, :cfg.nu]
    return res


def rows_of(n, nu):
    """the 2n constraint rows: bounds, then the rate rows (test_solver_kkt.rows)"""
    A = np.eye(n)
    for i in range(nu, n):
        A[i, i - nu] = -1.0
    return np.vstack([np.eye(n), A])


def random_ws(rng, n):
    """test_solver_kkt.random_ws: up to n random rows, random sides"""
    ws = 0
    for j in rng.choice(2 * n, size=rng.integers(0, n + 1), replace=False):
        ws |= (1 << int(j)) | ((int(rng.integers(0, 2)) << (16 + int(j))))
    return ws


def adversarial_ws(case):
    """(nq,) uint32 and the class of every slot, a third each (dealt by a
    seeded permutation): 0 random rows and sides; 1 a dependent set (module
    docstring) beside up to one random row; 2 every row active, on the side
    opposite to where the natural run ended: the other side of a row that ended
    active, the side farther from the final plan otherwise (the solver takes
    the first nV of them, the bounds)."""
    key = ("adv", case)
    if key not in _cache:
        c = problem(case)
        cfg = c["cfg"]
        n, nu, m = cfg.nV, cfg.nu, cfg.m
        nq = c["lin"].shape[0]
        nat = natural(case)[-1]
        x, wsn = nat["out"][0], nat["out"][3].astype(np.uint32)
        u_end = nat["u0"]
        lb, ub, lbA, ubA = JR.slot_bounds(cfg, c["arr"], u_end)
        lo, hi = np.concatenate([lb, lbA], 1), np.concatenate([ub, ubA], 1)
        cx = x @ rows_of(n, nu).T
        rng = np.random.default_rng(SEEDS[case] + 31)
        cls = rng.permutation(nq) % 3
        ws = np.zeros(nq, np.uint32)
        for q in range(nq):
            w = 0
            if cls[q] == 0:
                w = random_ws(rng, n)
            elif cls[q] == 1:
                j = int(rng.integers(0, nu))
                dep = [j, n + j] if m == 1 or rng.random() < 0.5 else [j, j + nu, n + j + nu]
                if rng.random() < 0.5:
                    dep.append(int(rng.integers(0, 2 * n)))
                for r in set(dep):
                    w |= (1 << r) | (int(rng.integers(0, 2)) << (16 + r))
            else:
                for r in range(2 * n):
                    if (wsn[q] >> r) & 1:
                        side = 1 - ((int(wsn[q]) >> (16 + r)) & 1)
                    else:
                        side = int(cx[q, r] - lo[q, r] < hi[q, r] - cx[q, r])   # nearer the lower side: take the upper
                    w |= (1 << r) | (side << (16 + r))
            ws[q] = w
        _freeze(ws, cls)
        _cache[key] = (ws, cls)
    return _cache[key]


def failure_inputs(case):
    """(lin with POISON applied, limits = four (nq, nu) arrays): the failure
    regime's records and per-slot limits (deal_limits around the first u_old)"""
    key = ("fail-in", case)
    if key not in _cache:
        c = problem(case)
        cfg = c["cfg"]
        L = DR.Layout(cfg)
        lin = c["lin"].copy()
        dslot = next(s for s in L.dslot if s >= 0)
        off = {"y": L.off_y, "A": L.off_A + 5, "x": L.off_x + dslot}
        for q, field, v in POISON:
            lin[q, off[field]] = v
        lim = CC.deal_limits(c["u_old"], cfg.nu, cfg.m)
        limits = tuple(np.ascontiguousarray(lim[:, i, :]) for i in range(4))
        _freeze(lin, *limits)
        _cache[key] = (lin, limits)
    return _cache[key]


def limit_class(nq):
    return np.arange(nq) % 8


def natural(case):
    key = ("natural", case)
    if key not in _cache:
        c = problem(case)
        nq = c["lin"].shape[0]
        _cache[key] = oracle_loop(c["cfg"], c["arr"], c["lin"], c["u_old"], np.zeros(nq, np.uint32), c["K"])
    return _cache[key]


def regime_inputs(case, regime):
    """(lin, ws before step 0, limits or None) of one regime"""
    c = problem(case)
    nq = c["lin"].shape[0]
    if regime == "natural":
        return c["lin"], np.zeros(nq, np.uint32), None
    ws, _ = adversarial_ws(case)
    if regime == "adversarial":
        return c["lin"], ws, None
    lin, limits = failure_inputs(case)
    return lin, ws, limits


def oracle_run(case, regime):
    """The oracle's closed loop of one case and regime (oracle_loop's result)"""
    if regime == "natural":
        return natural(case)
    key = ("run", case, regime)
    if key not in _cache:
        c = problem(case)
        lin, ws, limits = regime_inputs(case, regime)
        _cache[key] = oracle_loop(c["cfg"], c["arr"], lin, c["u_old"], ws, c["K"], limits=limits)
    return _cache[key]


# ---------------------------------------------------------------------------
# coverage, from the traces
# ---------------------------------------------------------------------------

def popcount16(ws):
    w = np.asarray(ws, np.uint32) & np.uint32(0xFFFF)
    return sum(((w >> np.uint32(j)) & np.uint32(1)).astype(np.int64) for j in range(16))


def solve_stats(n, ws_in, nchg, trace, ntrace):
    """Per solve (arrays over the slots): drops that follow an add, the largest
    working set on the way (the warm start's, cut to n rows and emptied by a
    cold start, then the trace's adds and drops), whether it began with a cold
    start (a change without a trace entry)."""
    ws_in, nchg, ntrace = np.asarray(ws_in), np.asarray(nchg), np.asarray(ntrace)
    cold = nchg > ntrace
    size = np.where(cold, 0, np.minimum(popcount16(ws_in), n))
    peak = size.copy()
    added = np.zeros(len(nchg), bool)
    late_drops = np.zeros(len(nchg), np.int64)
    for c in range(16):
        live = c < ntrace
        add = live & (trace[:, c] >= 0x80)
        drop = live & (trace[:, c] < 0x80)
        late_drops += drop & added
        added |= add
        size = size + add - drop
        peak = np.maximum(peak, size)
    return late_drops, peak, cold


def coverage(cfg, run):
    """dict(changes, late_drops, long_solves, full_slots, cold_starts,
    max_active, max_nwsr): totals over the run's steps, iterations and slots;
    full_slots counts the slots whose working set reached nV rows at some
    point, max_active is the largest working set seen, max_nwsr the number of
    solves that ended in CMPC_QP_MAX_NWSR."""
    n = cfg.nV
    nq = run[0]["H"].shape[0]
    tot = dict(changes=0, late_drops=0, long_solves=0, cold_starts=0, max_active=0, max_nwsr=0)
    full = np.zeros(nq, bool)
    for st in run:
        log, tr, ntr = st["log"], st["out"][4], st["out"][5]
        for k in range(tr.shape[1]):
            late, peak, cold = solve_stats(n, log["ws_in"][k], log["nchg"][k], tr[:, k], ntr[:, k])
            tot["changes"] += int(log["nchg"][k].sum())
            tot["late_drops"] += int(late.sum())
            tot["long_solves"] += int((log["nchg"][k] >= 5).sum())
            tot["cold_starts"] += int(cold.sum())
            tot["max_active"] = max(tot["max_active"], int(peak.max()))
            tot["max_nwsr"] += int((log["status"][k] == cmpc.CMPC_QP_MAX_NWSR).sum())
            full |= peak >= n
    tot["full_slots"] = int(full.sum())
    return tot


def difficulty(H):
    """(median cond(H), median of the largest |off-diagonal| over the largest diagonal)"""
    n = H.shape[1]
    off = np.abs(H * (1 - np.eye(n))).max(axis=(1, 2)) / np.abs(np.einsum("qii->qi", H)).max(axis=1)
    return float(np.median(np.linalg.cond(H))), float(np.median(off))


def last_gradient(cfg, st):
    """g = f + G d of the step's last iteration, d the other sub-controllers'
    plans of iteration K - 1 (the step's du_old for K = 1)"""
    K = st["log"]["plans"].shape[0]
    prev = st["log"]["plans"][K - 2] if K > 1 else st["du0"]
    g = st["f"].copy()
    if cfg.nVo:
        for q in range(g.shape[0]):
            g[q] = st["f"][q] + st["G"][q] @ JR.gather_other(cfg, prev, q)
    return g


# ---------------------------------------------------------------------------
# the enumeration of test_solver_kkt.enumerate_optimum, batched over the
# candidate working sets (the same candidates, rank test, KKT system and 1e-9
# acceptance; one numpy solve per working-set size)
# ---------------------------------------------------------------------------

def _candidates(n, nu):
    import itertools
    key = ("cand", n, nu)
    if key not in _cache:
        C = rows_of(n, nu)
        out = []
        for k in range(n + 1):
            Ns, js, ss = [], [], []
            for act in itertools.combinations(range(2 * n), k):
                for sides in itertools.product((0, 1), repeat=k):
                    N = np.array([C[j] * (-1.0 if s else 1.0) for j, s in zip(act, sides)]).reshape(k, n)
                    if k and np.linalg.matrix_rank(N) < k:
                        continue
                    Ns.append(N); js.append(act); ss.append(sides)
            out.append((np.array(Ns).reshape(len(Ns), k, n), np.array(js, np.int64).reshape(len(Ns), k),
                        np.array(ss, np.int64).reshape(len(Ns), k)))
        _cache[key] = (C, out)
    return _cache[key]


def enumerate_optimum(H, g, lo, hi, nu):
    """Every KKT point of one QP (n <= 4) by enumeration of the working sets:
    (T, n); empty for an infeasible QP"""
    n = len(g)
    C, cand = _candidates(n, nu)
    scale = np.abs(H).max() + np.abs(g).max() + 1.0
    bscale = 1.0 + np.maximum(np.abs(lo), np.abs(hi))
    found = []
    for k, (N, js, ss) in enumerate(cand):
        T = N.shape[0]
        Kmat = np.zeros((T, n + k, n + k))
        Kmat[:, :n, :n] = H
        Kmat[:, :n, n:] = -np.transpose(N, (0, 2, 1))
        Kmat[:, n:, :n] = N
        b = np.where(ss == 1, -hi[js], lo[js])
        rhs = np.concatenate([np.tile(-g, (T, 1)), b], axis=1)
        sol = np.linalg.solve(Kmat, rhs[:, :, None])[:, :, 0]
        x, mu = sol[:, :n], sol[:, n:]
        cx = x @ C.T
        ok = np.all(mu >= -1e-9 * scale, axis=1) & np.all(cx >= lo - 1e-9 * bscale, axis=1) \
            & np.all(cx <= hi + 1e-9 * bscale, axis=1)
        found.append(x[ok])
    return np.concatenate(found)
