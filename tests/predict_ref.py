"""The oracle's evaluation of a plan, shared by test_predict.py and
test_gpu_predict.py: predicted outputs from the matrices of
or_generate_prediction and the two parts of the objective (include/cmpc.h,
cmpc_predict).  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import _oracle as O


def adjusted_xa(dims, L, rec, u_old):
    """dx_aug after AdjustAllDelayedStates with u_old (or_build_qp, oracle/or_condense.c:225-238)"""
    xa = np.array(rec[L.off_x:L.off_x + L.naug], dtype=np.float64)
    idi, ids = dims.ndist, dims.ndist + L.nd
    for i in range(dims.nu_tot):
        D = dims.delay[i]
        if D:
            xa[idi] -= u_old[i]
            xa[ids:ids + D - 1] -= u_old[i]
            ids += D - 1
            idi += 1
    return xa


def gather_other(cfg, du):
    """The other controllers' plans per slot as the Jacobi iteration lays them
    out (oracle/or_nerve.c:95-101): d[mv*nuo + rank*nu + c], from (nq, nV) plans."""
    nq, S, nu, m, nuo = du.shape[0], cfg.S, cfg.nu, cfg.m, cfg.nu_tot - cfg.nu
    d = np.zeros((nq, m * nuo))
    if nuo == 0:
        return d
    for q in range(nq):
        b, s = divmod(q, S)
        rank = 0
        for s2 in range(S):
            if s2 == s:
                continue
            for mv in range(m):
                d[q, mv * nuo + rank * nu:mv * nuo + (rank + 1) * nu] = du[b * S + s2, mv * nu:(mv + 1) * nu]
            rank += 1
    return d


def costs(cfg, y_pred, du, y_ref, ywt, uwt):
    """(J_track, J_move) of one slot: y_pred, y_ref (p, ny)"""
    e = y_pred - y_ref
    jt = 0.5 * float(np.einsum("ri,ij,rj->", e, np.asarray(ywt).reshape(cfg.ny, cfg.ny), e))
    dm = np.asarray(du).reshape(cfg.m, cfg.nu)
    jm = 0.5 * float(np.einsum("ki,ij,kj->", dm, np.asarray(uwt).reshape(cfg.nu, cfg.nu), dm))
    return jt, jm


def oracle_prediction(dims, L, rec, u_old, du, d):
    """y_pred (p, ny) = y_prev + Su du + Su_other d + Sf fd + Sx xa"""
    Su, Sx, Sf, Suo = O.generate_prediction(dims, rec)
    y = Su @ du + Sf @ rec[L.off_f:L.off_f + dims.ns] + Sx @ adjusted_xa(dims, L, rec, u_old)
    if L.nVo:
        y = y + Suo @ d
    return y.reshape(dims.p, dims.ny) + rec[L.off_y:L.off_y + dims.ny]


def oracle_batch(cfg, dims, L, arr, lin, u_old, du, d, dy=None):
    """per slot: y_pred (nq, p, ny) and cost (nq, 2) against y_ref[s] (+ dy[q])"""
    nq = lin.shape[0]
    Y = np.zeros((nq, cfg.p, cfg.ny))
    J = np.zeros((nq, 2))
    for q in range(nq):
        s = q % cfg.S
        Y[q] = oracle_prediction(dims, L, lin[q], u_old[q], du[q], d[q])
        yr = np.asarray(arr.y_ref[s]).reshape(cfg.p, cfg.ny)
        if dy is not None:
            yr = yr + dy[q]
        J[q] = costs(cfg, Y[q], du[q], yr, arr.ywt[s], arr.uwt[s])
    return Y, J
