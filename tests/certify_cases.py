"""The batches of test_certify.py (CPU) and test_gpu_certify.py (GPU): p = 17,
synthetic operating points, two 64-lane workgroups with a partial last one.
TEST INFRASTRUCTURE ONLY.

Per-slot limits are dealt round-robin over the slots in eight classes around
each slot's u_old (DELTA = 1e-3, far inside the plans' unconstrained size):
  0, 2, 4     wide: bounds u_old -+ 1, rates -+ 1 (nothing binds)
  1           tight rates: -+ DELTA / 10
  3           a bound just above u_old on input 0 (lower = u_old + DELTA) and
              just below it on input 1 (upper = u_old - DELTA)
  5, 7        bound and rate both tight, on every input: upper = u_old + DELTA5
              with rate_lower = 0.8 DELTA5 / m (every move at least that much
              above the one before, the last one held by its bound; DELTA5 =
              1e-4), class 7 the mirror image (lower, rate_upper)
  6           infeasible: lower = u_old + 1 against rate_upper = 0.1
and from one round of the eight classes to the next the sides of classes 3, 5
and 7 are mirrored, so that lower and upper sides both occur.
"""
import functools

import numpy as np

import cmpc
import golden_cases as GC
from cmpc._abi import CmpcDims
from cmpc.synthetic import synthetic_batch

P = 17
DELTA = 1e-3
DELTA5 = 1e-4
# key: (golden case, m, B)
CASES = {"coop-par": ("coop-par", 2, 35),      # (nV, nu, nVo) = (4, 2, 4), 70 slots
         "cent-par": ("cent-par", 2, 70),      # (8, 4, 0)
         "coop-par-m1": ("coop-par", 1, 35),   # (2, 2, 2)
         "coop-par-m3": ("coop-par", 3, 35),   # (6, 2, 6)
         "coop-ser": ("coop-ser", 2, 35)}      # serial plant, ny = 4, (4, 2, 4)


def deal_limits(u_old, nu, m):
    """(nq, 4, nu): per slot [lower | upper | rate_lower | rate_upper]"""
    nq = u_old.shape[0]
    lim = np.zeros((nq, 4, nu))
    for q in range(nq):
        uo = u_old[q, :nu]
        lower, upper = uo - 1.0, uo + 1.0
        rlo, rhi = -np.ones(nu), np.ones(nu)
        cls = q % 8
        sgn = 1.0 if (q // 8) % 2 == 0 else -1.0   # (one sign per round of the eight classes)
        if cls == 1:
            rlo, rhi = -np.full(nu, DELTA / 10), np.full(nu, DELTA / 10)
        elif cls == 3:
            lower, upper = lower.copy(), upper.copy()
            a, b = (0, 1) if sgn > 0 else (1, 0)
            lower[a] = uo[a] + DELTA
            upper[b] = uo[b] - DELTA
        elif cls in (5, 7):
            rho = 0.8 * DELTA5 / m
            if (sgn > 0) == (cls == 5):
                upper, rlo = uo + DELTA5, np.full(nu, rho)
            else:
                lower, rhi = uo - DELTA5, np.full(nu, -rho)
        elif cls == 6:
            lower, rhi = uo + 1.0, np.full(nu, 0.1)
        lim[q] = [lower, upper, rlo, rhi]
    return lim


def shared_limits(cfg, arr, nq):
    """(nq, 4, nu): every slot its sub-controller's limits"""
    per_s = np.array([[arr.lower[s], arr.upper[s], arr.rate_lower[s], arr.rate_upper[s]] for s in range(cfg.S)])
    return np.ascontiguousarray(per_s[np.arange(nq) % cfg.S])


@functools.lru_cache(maxsize=None)
def case(key):
    """cfg, arr, B, batch (lin, u_old, du_old, ws), per-slot limits (nq, 4, nu)
    and the other controllers' plans d (nq, nVo) in +-0.05; all read-only."""
    name, m, B = CASES[key]
    ctype, plant = name.split("-")
    _, setup, _, _ = GC.case(name)
    cfg = cmpc.reference_config(plant, ctype, p=P, m=m)
    arr = cmpc.controller_arrays(cfg, setup)
    batch = synthetic_batch(cfg, B, seed=200 + 10 * m + len(name))
    nq = B * cfg.S
    lim = deal_limits(batch[1], cfg.nu, cfg.m)
    L = cmpc.layout_of(CmpcDims.from_config(cfg, 1))
    d = np.ascontiguousarray(np.random.default_rng(300 + m).uniform(-0.05, 0.05, (nq, L.nVo)))
    for a in (*batch, lim, d):
        a.setflags(write=False)
    return cfg, arr, B, batch, lim, d


@functools.lru_cache(maxsize=None)
def oracle_solution(key, per_slot=True):
    """The oracle's QPs and its cold solve of every slot with the plans d:
    H, f, G, x, ws (uint32), status (int32), limits (nq, 4, nu)."""
    import _oracle as O
    cfg, arr, B, batch, lim, d = case(key)
    lin, u_old = batch[0], batch[1]
    dims = CmpcDims.from_config(cfg, 1)
    nq, nu, m = B * cfg.S, cfg.nu, cfg.m
    if not per_slot:
        lim = shared_limits(cfg, arr, nq)
    Hs, fs, Gs, xs = [], [], [], []
    ws, st = np.zeros(nq, np.uint32), np.zeros(nq, np.int32)
    for q in range(nq):
        s = q % cfg.S
        H, f, _, _, G = O.build_qp(dims, lin[q], u_old[q], arr.y_ref[s], arr.ywt[s], arr.uwt[s])
        uo = u_old[q][:nu]
        x, info = O.qp_solve_map(H, f, G, d[q], np.tile(lim[q, 0] - uo, m), np.tile(lim[q, 1] - uo, m),
                                 np.tile(lim[q, 2], m), np.tile(lim[q, 3], m), nu, 0)
        Hs.append(H); fs.append(f); Gs.append(G); xs.append(x)
        ws[q], st[q] = info.ws, info.status
    out = (np.array(Hs), np.array(fs), np.array(Gs).reshape(nq, cfg.nV, -1), np.array(xs), ws, st, lim)
    for a in out:
        a.setflags(write=False)
    return out
