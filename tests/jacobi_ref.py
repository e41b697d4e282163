"""The Jacobi loop of one control step on given QPs, with the oracle's
map-form solve.  TEST INFRASTRUCTURE ONLY.

Shared by test_gpu_small_batch.py, solver_cases.py, test_solver_cases.py and
test_gpu_dense_solver.py: the device's iterate and fused step kernels are held
to it bit for bit on the QPs the device itself built (download_qp)."""
import numpy as np

import _oracle as O


def slot_bounds(cfg, arr, u_old, limits=None):
    """(lb, ub, lbA, ubA), each (nq, nV): the solver's bounds of every slot,
    lower - u_old and upper - u_old of the own inputs per move and the rate
    limits per move.  limits = (lower, upper, rate_lower, rate_upper), each
    (nq, nu): the slot's own (Context.set_scenario_constraints); None: the
    sub-controller's of arr."""
    nq, nu, m, S = u_old.shape[0], cfg.nu, cfg.m, cfg.S
    out = [np.zeros((nq, nu * m)) for _ in range(4)]
    for q in range(nq):
        s = q % S
        lower, upper, rlo, rhi = ((arr.lower[s], arr.upper[s], arr.rate_lower[s], arr.rate_upper[s])
                                  if limits is None else (a[q] for a in limits))
        out[0][q] = np.tile(lower - u_old[q, :nu], m)
        out[1][q] = np.tile(upper - u_old[q, :nu], m)
        out[2][q] = np.tile(rlo, m)
        out[3][q] = np.tile(rhi, m)
    return tuple(out)


def gather_other(cfg, plans, q):
    """d of slot q: the other sub-controllers' plans (nq, nV) in G's column
    order (controller-major inside each move, include/nerve_center.h:283-285)"""
    S, nu, m = cfg.S, cfg.nu, cfg.m
    nV = nu * m
    b, s = divmod(q, S)
    d = np.zeros((S - 1) * nV)
    for rk in range(S - 1):
        s2 = rk + (rk >= s)
        for mv in range(m):
            d[mv * (S - 1) * nu + rk * nu: mv * (S - 1) * nu + rk * nu + nu] = plans[b * S + s2, mv * nu:(mv + 1) * nu]
    return d


def oracle_jacobi(cfg, arr, H, f, G, u_old, du_old, ws, K, limits=None, log=None):
    """The Jacobi loop of one step on the device's own (H, f, G) with the
    oracle's map-form solve (or_qp.c step A, version 3): per iteration each
    sub-controller solves with d = the other sub-controllers' previous plans
    (gather_other), bounds from slot_bounds (per-slot limits where given).
    Returns (plans, status, nchg, ws, trace (nq, K, 16), ntrace (nq, K)) of the
    last iteration (trace, ntrace: of every iteration).  log: a dict that
    receives every iteration's plans (K, nq, nV), status, nchg, ws_in (K, nq)
    and the smallest decision margin per slot."""
    nV = cfg.nu * cfg.m
    nqp = H.shape[0]
    dprev = du_old.reshape(nqp, nV).copy()
    ws = ws.copy()
    lb, ub, lbA, ubA = slot_bounds(cfg, arr, u_old, limits)
    st = np.zeros(nqp, np.int32); nw = np.zeros(nqp, np.int32)
    tr = np.full((nqp, K, 16), 0xFF, np.uint8); ntr = np.zeros((nqp, K), np.int32)
    if log is not None:
        log.update(plans=np.zeros((K, nqp, nV)), status=np.zeros((K, nqp), np.int32), nchg=np.zeros((K, nqp), np.int32),
                   ws_in=np.zeros((K, nqp), np.uint32), margin=np.full(nqp, np.inf))
    for k in range(K):
        dnew = np.zeros_like(dprev)
        for q in range(nqp):
            d = gather_other(cfg, dprev, q)
            x, info = O.qp_solve_map(H[q], f[q], G[q], d, lb[q], ub[q], lbA[q], ubA[q], cfg.nu, int(ws[q]))
            if log is not None:
                log["ws_in"][k, q] = ws[q]
                log["status"][k, q], log["nchg"][k, q] = info.status, info.nchg
                log["margin"][q] = min(log["margin"][q], info.margin)
            dnew[q] = x
            ws[q] = info.ws
            st[q] = info.status; nw[q] = info.nchg
            tr[q, k] = np.frombuffer(bytes(info.trace), np.uint8); ntr[q, k] = info.ntrace
        dprev = dnew
        if log is not None:
            log["plans"][k] = dnew
    return dprev, st, nw, ws, tr, ntr
