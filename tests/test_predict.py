"""Prediction (include/cmpc.h, cmpc_predict) without a GPU: the entry points
exist and refuse a null context, cmpc_predict_available follows kernel_dims.h,
and the definition of the objective the GPU tests use is the QP's:
J_track + J_move - J_track(du = 0) = 1/2 du' H du + (f + G d)' du on the
oracle alone.  CPU only."""
import os
import re

import numpy as np
import pytest

import _oracle as O
import cmpc
import golden_cases as GC
import predict_ref as PR
from cmpc._abi import CmpcDims, load_library
from cmpc.configs import reference_config
from cmpc.synthetic import synthetic_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_predict_symbols_refuse_null_context():
    lib = load_library()
    for name in ("cmpc_predict", "cmpc_predict_host", "cmpc_prediction_device", "cmpc_prediction_cost_device",
                 "cmpc_download_prediction", "cmpc_predict_available"):
        assert hasattr(lib, name), name
    assert lib.cmpc_predict(None, None, None, 0) == -1
    assert b"null" in lib.cmpc_last_error()
    assert lib.cmpc_predict_host(None, None, None, 0) == -1
    assert lib.cmpc_download_prediction(None, None, None) == -1
    assert not lib.cmpc_prediction_device(None)
    assert not lib.cmpc_prediction_cost_device(None)
    assert lib.cmpc_predict_available(None) == 0


def wave_sets():
    """(ns, ny, nu, m) of every CMPC_BUILD_DIMS row whose WAVE column is 1"""
    text = open(os.path.join(ROOT, "compressor-mpc_amd", "csrc", "kernel_dims.h")).read()
    rows = re.findall(r"^\s*X\(F,\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),", text, re.M)
    sets = [tuple(int(v) for v in r[:4]) for r in rows if r[4] == "1"]
    assert len(sets) >= 8
    return sets


def dims_of(ns, ny, nu, m, nu_tot=4, delays=(0, 40, 0, 40), p=50, B=3):
    d = CmpcDims()
    d.ns, d.ndist, d.nu_tot, d.nu, d.ny, d.p, d.m = ns, 4, nu_tot, nu, ny, p, m
    d.S, d.B = nu_tot // nu, B
    for i, v in enumerate(delays):
        d.delay[i] = v
    return d


def test_predict_available_follows_the_wave_column():
    for ns, ny, nu, m in wave_sets():
        assert cmpc.predict_available(dims_of(ns, ny, nu, m)), (ns, ny, nu, m)
        assert cmpc.predict_available(dims_of(ns, ny, nu, m, delays=(0, 2, 0, 63), p=64))
        assert not cmpc.predict_available(dims_of(ns, ny, nu, m, delays=(0, 40, 0, 0)))  # one delayed input
    assert not cmpc.predict_available(dims_of(12, 3, 2, 2))
    assert not cmpc.predict_available(dims_of(9, 3, 2, 2))
    assert not cmpc.predict_available(dims_of(10, 3, 1, 2, nu_tot=5, delays=(0, 40, 0, 40, 0)))
    # every reference configuration has one
    for plant in ("par", "ser"):
        for ctype in ("cent", "coop", "ncoop"):
            assert cmpc.predict_available(CmpcDims.from_config(reference_config(plant, ctype, p=50), 1))


IDENTITY_CASES = [("coop-par", 50), ("ncoop-par", 50), ("cent-ser", 50), ("cent-par", 200), ("coop-ser", 200)]


@pytest.mark.parametrize("name,p", IDENTITY_CASES)
def test_cost_identity_on_the_oracle(name, p):
    """J(du) - J(0) = 1/2 du' H du + (f + G d)' du with the oracle's H, f, G,
    within 1e-13 of the summed magnitudes of the five terms (5.9e-16 measured
    for these cases when the definition was written down)."""
    cfg, setup, arr, _ = GC.case(name, p=p)
    B = 2
    lin, u_old, _, _ = synthetic_batch(cfg, B, seed=5 + p)
    dims = CmpcDims.from_config(cfg, 1)
    L = cmpc.layout_of(dims)
    rng = np.random.default_rng(31 + p)
    worst = 0.0
    for q in range(B * cfg.S):
        s = q % cfg.S
        du = rng.uniform(-0.1, 0.1, L.nV)
        d = rng.uniform(-0.1, 0.1, L.nVo)
        yr = np.asarray(arr.y_ref[s]).reshape(cfg.p, cfg.ny)
        H, f, _, _, G = O.build_qp(dims, lin[q], u_old[q], arr.y_ref[s], arr.ywt[s], arr.uwt[s])
        jt, jm = PR.costs(cfg, PR.oracle_prediction(dims, L, lin[q], u_old[q], du, d), du, yr, arr.ywt[s],
                          arr.uwt[s])
        jt0, _ = PR.costs(cfg, PR.oracle_prediction(dims, L, lin[q], u_old[q], 0 * du, d), 0 * du, yr,
                          arr.ywt[s], arr.uwt[s])
        quad = 0.5 * du @ H @ du
        lin_term = (f + (G @ d if L.nVo else 0.0)) @ du
        mag = abs(jt) + abs(jm) + abs(jt0) + abs(quad) + abs(lin_term)
        err = abs(jt + jm - jt0 - quad - lin_term)
        worst = max(worst, err / mag)
        assert err <= 1e-13 * mag, (q, err / mag)
    print(f"{name} p={p}: worst identity error {worst:.2e} of the summed magnitudes")


def test_gather_other_is_the_jacobi_order():
    """predict_ref.gather_other against the documented order d[mv*nuo + rank*nu + c]"""
    cfg = reference_config("par", "coop", p=50)
    du = np.arange(4 * cfg.nV, dtype=np.float64).reshape(4, cfg.nV)
    d = PR.gather_other(cfg, du)
    assert np.array_equal(d[0], du[1]) and np.array_equal(d[1], du[0]) and np.array_equal(d[3], du[2])
    cent = reference_config("par", "cent", p=50)
    assert PR.gather_other(cent, np.zeros((2, cent.nV))).shape == (2, 0)
