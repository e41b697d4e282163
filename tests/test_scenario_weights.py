"""Per-scenario weights (include/cmpc.h, cmpc_set_scenario_weights) without a
GPU: the entry points exist and refuse a null context, cmpc_weight_factor is
the Cholesky factorisation the shared weights go through (L_W L_W' = ywt, zero
pivots allowed, non-symmetric and indefinite inputs refused),
cmpc_scenario_weights_available follows kernel_dims.h, and cmpc_plan under
CMPC_PLAN_SCENARIO_WEIGHTS builds on the one-QP-per-wave kernel and fuses
nothing.  CPU only."""
import ctypes

import numpy as np
import pytest

import cmpc
import weights_ref as WR
from cmpc._abi import (CMPC_PLAN_NO_WEIGHTS_BUILD, CMPC_PLAN_WEIGHTS_NEED_SPLIT, CMPC_PLAN_WEIGHTS_NEED_WAVE,
                       CmpcDims, CmpcPlan, load_library)
from cmpc.configs import reference_config
from test_predict import dims_of, wave_sets

CUS = 256  # MI355X


def test_weights_symbols_refuse_null_context():
    lib = load_library()
    for name in ("cmpc_set_scenario_weights", "cmpc_bind_scenario_weights", "cmpc_get_scenario_weights",
                 "cmpc_scenario_weights_available", "cmpc_weight_factor"):
        assert hasattr(lib, name), name
    assert lib.cmpc_set_scenario_weights(None, None, None) == -1
    assert b"null" in lib.cmpc_last_error()
    assert lib.cmpc_bind_scenario_weights(None, None) == -1
    assert lib.cmpc_get_scenario_weights(None, None, None) == -1
    assert lib.cmpc_scenario_weights_available(None) == 0
    assert lib.cmpc_weight_factor(3, None, None) == -1
    assert cmpc.CMPC_PLAN_SCENARIO_WEIGHTS == 0x400


# ---- cmpc_weight_factor ---------------------------------------------------------------

@pytest.mark.parametrize("ny", [2, 3, 4])
def test_weight_factor_reproduces_a_dense_spd_weight(ny):
    """L_W L_W' = ywt within a few ulps of max|ywt| (ny <= 4: at most three
    products and a square root per entry), L_W' upper triangular."""
    rng = np.random.default_rng(40 + ny)
    for _ in range(20):
        R = rng.uniform(-1, 1, (ny, ny))
        W = 3.7 * (R @ R.T + 0.1 * np.eye(ny))
        lwt = cmpc.weight_factor(W)
        assert np.array_equal(lwt, np.triu(lwt)) and (np.diag(lwt) > 0).all()
        assert (lwt[np.triu_indices(ny, 1)] != 0).all()
        np.testing.assert_allclose(lwt.T @ lwt, W, rtol=0, atol=16 * np.finfo(float).eps * np.abs(W).max())


def test_weight_factor_allows_a_zero_pivot():
    """PSD with a zero pivot in the middle: v v' + e_2 e_2' on (0, 2), rank 2."""
    v = np.array([2.0, 0.0, 1.0])
    W = np.outer(v, v)
    W[1, 1] = 0.0
    W[2, 2] += 4.0
    lwt = cmpc.weight_factor(W)
    assert (lwt[1] == 0).all()
    np.testing.assert_allclose(lwt.T @ lwt, W, rtol=0, atol=16 * np.finfo(float).eps * np.abs(W).max())
    # the diagonal weights of the reference configurations, zeros included
    D = np.diag([1.0, 0.0, 0.25])
    assert np.array_equal(cmpc.weight_factor(D), np.diag([1.0, 0.0, 0.5]))
    assert np.array_equal(cmpc.weight_factor(np.zeros((2, 2))), np.zeros((2, 2)))


def test_weight_factor_refuses_bad_weights():
    W = np.array([[2.0, 0.5], [0.4, 1.0]])
    with pytest.raises(RuntimeError, match="symmetric"):
        cmpc.weight_factor(W)
    with pytest.raises(RuntimeError, match="positive semi-definite"):
        cmpc.weight_factor(np.array([[1.0, 2.0], [2.0, 1.0]]))   # eigenvalues 3, -1
    with pytest.raises(RuntimeError, match="positive semi-definite"):
        cmpc.weight_factor(np.diag([1.0, -1e-3, 1.0]))
    with pytest.raises(ValueError):
        cmpc.weight_factor(np.zeros((2, 3)))
    with pytest.raises(RuntimeError):
        cmpc.weight_factor(np.eye(5))


def test_weight_factor_is_the_shared_weights_factor():
    """weights_ref.packed of the shared weights: the reference configurations'
    diagonal ywt factor to their square roots exactly."""
    for name in ("coop-par", "cent-ser"):
        cfg, arr, _ = WR.RP.config(name, 50)
        u, y = WR.shared_weights(cfg, arr, 2 * cfg.S)
        pk = WR.packed(u, y)
        assert pk.shape == (2 * cfg.S, cfg.ny ** 2 + cfg.nu ** 2)
        for q in range(2 * cfg.S):
            W = arr.ywt[q % cfg.S]
            if np.array_equal(W, np.diag(np.diag(W))):
                assert np.array_equal(pk[q, :cfg.ny ** 2].reshape(cfg.ny, cfg.ny), np.diag(np.sqrt(np.diag(W))))
            assert np.array_equal(pk[q, cfg.ny ** 2:].reshape(cfg.nu, cfg.nu), arr.uwt[q % cfg.S])


# ---- availability ----------------------------------------------------------------------

def test_weights_available_follows_the_wave_column():
    avail = cmpc.scenario_weights_available
    for ns, ny, nu, m in wave_sets():
        assert avail(dims_of(ns, ny, nu, m)), (ns, ny, nu, m)                      # p = 50
        assert avail(dims_of(ns, ny, nu, m, delays=(0, 2, 0, 63), p=64))
        assert not avail(dims_of(ns, ny, nu, m, delays=(0, 40, 0, 0)))   # one delayed input: no instance
    assert not avail(dims_of(12, 3, 2, 2))
    assert not avail(dims_of(9, 3, 2, 2))
    for plant in ("par", "ser"):
        for ctype in ("cent", "coop", "ncoop"):
            assert avail(CmpcDims.from_config(reference_config(plant, ctype, p=50), 1))


def _plain_wave_build_runs(dims):
    try:
        return not cmpc.plan(dims, CUS, build=cmpc.CMPC_BUILD_WAVE, K=0).build_error
    except RuntimeError:   # cmpc_plan itself refuses: the horizon is too long for the build's LDS
        return False


def test_weights_available_stops_where_the_lds_no_longer_fits():
    """The wave region grows by yl_stride + up(ny*ny + nu*nu, 2) doubles: there
    is a horizon the plain one-QP-per-wave build still takes (cmpc_plan, WAVE
    forced) and the per-slot-weights instances do not."""
    ns, ny, nu, m = 10, 4, 2, 2
    fits = [p for p in range(100, 300, 10)
            if _plain_wave_build_runs(dims_of(ns, ny, nu, m, p=p))]
    assert fits
    both = [p for p in fits if cmpc.scenario_weights_available(dims_of(ns, ny, nu, m, p=p))]
    assert both and max(both) < max(fits)
    p = max(fits)
    pl = cmpc.plan(dims_of(ns, ny, nu, m, p=p), CUS, K=0, scenario_weights=True)
    assert pl.build_error == CMPC_PLAN_NO_WEIGHTS_BUILD and pl.build_kernel == 0
    assert cmpc.plan_error_string(pl.build_error)


# ---- the plan ---------------------------------------------------------------------------

PLAN_FIELDS = [n for n, _ in CmpcPlan._fields_]


@pytest.mark.parametrize("nB", [65536, 3])   # coop-par: 131 072 QPs and 6 QPs
def test_plan_with_scenario_weights(nB):
    cfg = reference_config("par", "coop", p=50)
    dims = CmpcDims.from_config(cfg, nB)
    unset = cmpc.plan(dims, CUS, K=9)
    assert unset.build_kernel == (cmpc.CMPC_BUILD_ROWS if nB > 3 else cmpc.CMPC_BUILD_SPLIT)
    if nB == 3:
        assert unset.control_fused
    pl = cmpc.plan(dims, CUS, K=9, scenario_weights=True)
    assert pl.as_dict() == cmpc.plan(dims, CUS, K=9, flags=cmpc.CMPC_PLAN_SCENARIO_WEIGHTS).as_dict()
    assert pl.build_kernel == cmpc.CMPC_BUILD_WAVE and not pl.build_error
    assert not pl.step_fused and not pl.step_error
    assert not pl.control_fused and pl.control_grid == 0 and pl.control_polled == 0
    split = cmpc.plan(dims, CUS, build=cmpc.CMPC_BUILD_WAVE, step=cmpc.CMPC_STEP_SPLIT, K=9)
    assert (pl.step_build_kernel, pl.step_solve_kernel) == (split.step_build_kernel, split.step_solve_kernel)
    assert pl.step_build_kernel == cmpc.CMPC_BUILD_WAVE
    assert (pl.control_build_kernel, pl.control_solve_kernel) == (pl.step_build_kernel, pl.step_solve_kernel)
    assert (pl.solve_kernel, pl.solve_error) == (unset.solve_kernel, unset.solve_error)
    # WAVE forced is what AUTO gives; ROWS, SPLIT and FUSED forced are the new errors
    forced = cmpc.plan(dims, CUS, build=cmpc.CMPC_BUILD_WAVE, K=9, scenario_weights=True)
    assert forced.build_kernel == cmpc.CMPC_BUILD_WAVE and not forced.build_error
    for variant in (cmpc.CMPC_BUILD_ROWS, cmpc.CMPC_BUILD_SPLIT):
        bad = cmpc.plan(dims, CUS, build=variant, K=9, scenario_weights=True)
        assert bad.build_error == CMPC_PLAN_WEIGHTS_NEED_WAVE and bad.build_kernel == 0
        assert not cmpc.plan(dims, CUS, build=variant, K=9).build_error
    fused = cmpc.plan(dims, CUS, step=cmpc.CMPC_STEP_FUSED, K=9, scenario_weights=True)
    assert fused.step_error == CMPC_PLAN_WEIGHTS_NEED_SPLIT and not fused.step_fused
    texts = {cmpc.plan_error_string(e) for e in (CMPC_PLAN_WEIGHTS_NEED_WAVE, CMPC_PLAN_WEIGHTS_NEED_SPLIT,
                                                 CMPC_PLAN_NO_WEIGHTS_BUILD)}
    assert len(texts) == 3 and all("weights" in t for t in texts)
    assert "unknown" not in " ".join(texts)


def test_plan_without_the_flag_is_unchanged():
    """Without CMPC_PLAN_SCENARIO_WEIGHTS the plans of the two sizes are the
    ones recorded from the library before the flag existed (coop-par, p = 50,
    K = 9, 256 CUs, every variant AUTO), field by field."""
    cfg = reference_config("par", "coop", p=50)
    ROWS, SPLIT, LANE, SROWS = cmpc.CMPC_BUILD_ROWS, cmpc.CMPC_BUILD_SPLIT, cmpc.CMPC_SOLVE_LANE, cmpc.CMPC_SOLVE_ROWS
    recorded = {65536: (ROWS, 0, LANE, 0, 0, ROWS, LANE, 0, 0, ROWS, LANE, 0, 0),
                3: (SPLIT, 0, SROWS, 0, 0, SPLIT, SROWS, 0, 1, SPLIT, SROWS, 3, 0)}
    for nB, values in recorded.items():
        dims = CmpcDims.from_config(cfg, nB)
        pl = cmpc.plan(dims, CUS, K=9).as_dict()
        assert pl == dict(zip(PLAN_FIELDS, values)), nB
        assert pl == cmpc.plan(dims, CUS, K=9, scenario_weights=False).as_dict()
        assert pl != cmpc.plan(dims, CUS, K=9, scenario_weights=True).as_dict()
