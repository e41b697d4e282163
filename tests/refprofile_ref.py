"""Reference profiles (include/cmpc.h, cmpc_set_scenario_reference_profile),
shared by test_reference_profile.py and test_gpu_reference_profile.py: the
numpy model of the backward sweep csrc/refshift.hip runs, the oracle's
g = Su' w from the matrices of or_generate_prediction, and the problems the
tests build on.  TEST INFRASTRUCTURE ONLY."""
import dataclasses
import functools

import numpy as np

import _oracle as O
import cmpc
import golden_cases as GC
from cmpc._abi import CmpcDims
from cmpc.synthetic import synthetic_batch

TOL = 1e-11   # the project's build tolerance (test_gpu_parity.py)


def weighted(cfg, ywt, dref):
    """w[r] = ywt dref[r], (p, ny)"""
    return np.asarray(dref).reshape(cfg.p, cfg.ny) @ np.asarray(ywt, dtype=np.float64).reshape(cfg.ny, cfg.ny).T


def sweep_g(cfg, dims, L, rec, ywt, dref):
    """g = Su' w by the adjoint of the forward model, never forming Su:
    lam = A' lam + Cx' w[k] for k = p-1 .. 0, and for each own input c with
    k >= delay[c]: g[min(k - delay[c], m-1)*nu + c] += Bin[:, c] . lam"""
    ns, ny, nu, m, p = cfg.ns, cfg.ny, cfg.nu, cfg.m, cfg.p
    A = rec[L.off_A:L.off_A + ns * ns].reshape(ns, ns)
    Bin = rec[L.off_B:L.off_B + ns * cfg.nu_tot].reshape(ns, cfg.nu_tot)
    Cx = rec[L.off_C:L.off_C + ny * L.nobs].reshape(ny, L.nobs)[:, :ns]
    w = weighted(cfg, ywt, dref)
    lam = np.zeros(ns)
    g = np.zeros(m * nu)
    for k in range(p - 1, -1, -1):
        lam = A.T @ lam + Cx.T @ w[k]
        for c in range(nu):
            D = dims.delay[c]
            if k >= D:
                g[min(k - D, m - 1) * nu + c] += Bin[:, c] @ lam
    return g


def oracle_g(cfg, dims, rec, ywt, dref):
    """Su' w from the oracle's Su"""
    Su = O.generate_prediction(dims, rec)[0]
    return Su.T @ weighted(cfg, ywt, dref).reshape(-1)


def config(name, p, m=2, delays=None):
    ctype, plant = name.split("-")
    _, setup, _, g = GC.case(name)
    cfg = cmpc.reference_config(plant, ctype, p=p, m=m)
    if delays is not None:
        cfg = dataclasses.replace(cfg, delays=tuple(delays))
    return cfg, cmpc.controller_arrays(cfg, setup), g


@functools.lru_cache(maxsize=None)
def problem(name, p, m=2, delays=None, B=3):
    """A batch, profiles uniform in +-0.2, offsets, and the oracle's QPs
    without the profile and with y_ref + dy + dref; everything read-only."""
    cfg, arr, _ = config(name, p, m, delays)
    batch = synthetic_batch(cfg, B, seed=23 + p)
    lin, u_old = batch[0], batch[1]
    dims = CmpcDims.from_config(cfg, 1)
    L = cmpc.layout_of(dims)
    nq = B * cfg.S
    rng = np.random.default_rng(311 + p + m)
    dref = np.ascontiguousarray(rng.uniform(-0.2, 0.2, (nq, cfg.p, cfg.ny)))
    dy = np.ascontiguousarray(rng.uniform(-0.05, 0.05, (nq, cfg.ny)))
    out = {"H0": [], "f0": [], "G0": [], "H": [], "f": [], "G": [], "g": [], "f_dy": []}
    for q in range(nq):
        s = q % cfg.S
        yr = np.asarray(arr.y_ref[s]).reshape(cfg.p, cfg.ny)
        H0, f0, _, _, G0 = O.build_qp(dims, lin[q], u_old[q], yr, arr.ywt[s], arr.uwt[s])
        H, f, _, _, G = O.build_qp(dims, lin[q], u_old[q], yr + dy[q] + dref[q], arr.ywt[s], arr.uwt[s])
        f_dy = O.build_qp(dims, lin[q], u_old[q], yr + dy[q], arr.ywt[s], arr.uwt[s])[1]
        for k, v in zip(out, (H0, f0, G0, H, f, G, oracle_g(cfg, dims, lin[q], arr.ywt[s], dref[q]), f_dy)):
            out[k].append(v)
    ora = {k: np.stack(v) for k, v in out.items()}
    for a in (*batch, dref, dy, *ora.values()):
        a.setflags(write=False)
    return cfg, arr, batch, dref, dy, ora


def schedule_window(schedule, t, p):
    """rows min(t + 1 + r, T - 1), r = 0..p-1, of a (B, T, n_outputs) schedule: (B, p, n_outputs)"""
    schedule = np.asarray(schedule)
    idx = np.minimum(t + 1 + np.arange(p), schedule.shape[1] - 1)
    return schedule[:, idx, :]
