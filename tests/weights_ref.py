"""Per-scenario weights (include/cmpc.h, cmpc_set_scenario_weights), shared by
test_scenario_weights.py and test_gpu_scenario_weights.py: per-slot weight
draws, the oracle's QPs slot by slot with each slot's own weights
(_oracle.build_qp takes ywt and uwt per call), and the problems the tests
build on, made the way refprofile_ref.problem makes its own.
TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import _oracle as O
import cmpc
import refprofile_ref as RP
from cmpc._abi import CmpcDims
from cmpc.synthetic import synthetic_batch

TOL = RP.TOL   # the project's build tolerance (test_gpu_parity.py)


def draw_weights(rng, cfg, arr, nq):
    """Per slot a dense SPD ywt (every off-diagonal non-zero) and a dense
    symmetric uwt with every entry positive (diagonally dominant, so SPD),
    on the scale of the sub-controller's shared weights."""
    ny, nu = cfg.ny, cfg.nu
    ywt = np.zeros((nq, ny, ny))
    uwt = np.zeros((nq, nu, nu))
    for q in range(nq):
        s = q % cfg.S
        ys, us = np.abs(arr.ywt[s]).max(), np.abs(arr.uwt[s]).max()
        R = rng.uniform(0.3, 1.0, (ny, ny)) * rng.choice([-1.0, 1.0], (ny, ny))
        ywt[q] = ys * (R @ R.T / ny + 0.5 * np.eye(ny))
        Q = rng.uniform(0.1, 0.4, (nu, nu))
        uwt[q] = us * (0.5 * (Q + Q.T) + nu * np.eye(nu))
        assert (ywt[q][~np.eye(ny, dtype=bool)] != 0).all() and (uwt[q] > 0).all()
    return np.ascontiguousarray(uwt), np.ascontiguousarray(ywt)


def oracle_qps(cfg, arr, lin, u_old, uwt, ywt, dy=None, dref=None):
    """H, f, G of every slot from the oracle run with that slot's weights (and
    reference y_ref[s] + dy[q] + dref[q])."""
    dims = CmpcDims.from_config(cfg, 1)
    H, f, G = [], [], []
    for q in range(lin.shape[0]):
        s = q % cfg.S
        yr = np.asarray(arr.y_ref[s]).reshape(cfg.p, cfg.ny).copy()
        if dy is not None:
            yr = yr + dy[q]
        if dref is not None:
            yr = yr + dref[q]
        h, ff, _, _, g = O.build_qp(dims, lin[q], u_old[q], yr, ywt[q], uwt[q])
        H.append(h); f.append(ff); G.append(g)
    return np.stack(H), np.stack(f), np.stack(G)


def shared_weights(cfg, arr, nq):
    """The sub-controllers' shared weights repeated per slot."""
    s = np.arange(nq) % cfg.S
    return np.ascontiguousarray(arr.uwt[s]), np.ascontiguousarray(arr.ywt[s])


def packed(uwt, ywt):
    """The blocks Context.bind_scenario_weights takes: per slot [L_W' | uwt]."""
    nq = uwt.shape[0]
    lw = np.stack([cmpc.weight_factor(ywt[q]) for q in range(nq)])
    return np.ascontiguousarray(np.concatenate([lw.reshape(nq, -1), uwt.reshape(nq, -1)], axis=1))


@functools.lru_cache(maxsize=None)
def problem(name, p, m=2, delays=None, B=3):
    """A batch, per-slot weights, offsets, and the oracle's QPs with the slots'
    own weights (H, f, G) and with the shared ones (H0, f0, G0), both on
    y_ref + dy; everything read-only."""
    cfg, arr, _ = RP.config(name, p, m, delays)
    batch = synthetic_batch(cfg, B, seed=23 + p)
    lin, u_old = batch[0], batch[1]
    nq = B * cfg.S
    rng = np.random.default_rng(977 + p + m)
    uwt, ywt = draw_weights(rng, cfg, arr, nq)
    dy = np.ascontiguousarray(rng.uniform(-0.05, 0.05, (nq, cfg.ny)))
    H, f, G = oracle_qps(cfg, arr, lin, u_old, uwt, ywt, dy)
    H0, f0, G0 = oracle_qps(cfg, arr, lin, u_old, *shared_weights(cfg, arr, nq), dy)
    ora = {"H": H, "f": f, "G": G, "H0": H0, "f0": f0, "G0": G0}
    for a in (*batch, uwt, ywt, dy, *ora.values()):
        a.setflags(write=False)
    return cfg, arr, batch, uwt, ywt, dy, ora
