"""Reference profiles (include/cmpc.h, cmpc_set_scenario_reference_profile)
without a GPU: the entry points exist and refuse a null context,
cmpc_reference_profile_available follows kernel_dims.h, the backward sweep the
kernel runs (refprofile_ref.sweep_g) is the oracle's f shift, cmpc_plan under
CMPC_PLAN_REF_PROFILE fuses nothing, and scenario_reference_profiles is
scenario_reference_offsets row by row.  CPU only."""
import numpy as np
import pytest

import cmpc
import refprofile_ref as RP
from cmpc._abi import CmpcDims, CmpcPlan, load_library
from cmpc.configs import reference_config
from test_predict import dims_of, wave_sets


def test_profile_symbols_refuse_null_context():
    lib = load_library()
    for name in ("cmpc_set_scenario_reference_profile", "cmpc_bind_scenario_reference_profile",
                 "cmpc_get_scenario_reference_profile", "cmpc_reference_profile_available"):
        assert hasattr(lib, name), name
    assert lib.cmpc_set_scenario_reference_profile(None, None) == -1
    assert b"null" in lib.cmpc_last_error()
    assert lib.cmpc_bind_scenario_reference_profile(None, None) == -1
    assert lib.cmpc_get_scenario_reference_profile(None, None) == -1
    assert lib.cmpc_reference_profile_available(None) == 0
    assert cmpc.CMPC_PLAN_REF_PROFILE == 0x200


def test_profile_available_follows_the_wave_column():
    avail = cmpc.reference_profile_available
    for ns, ny, nu, m in wave_sets():
        assert avail(dims_of(ns, ny, nu, m)), (ns, ny, nu, m)
        assert avail(dims_of(ns, ny, nu, m, delays=(0, 2, 0, 63), p=64))
        assert not avail(dims_of(ns, ny, nu, m, delays=(0, 40, 0, 0)))  # one delayed input
    assert not avail(dims_of(12, 3, 2, 2))
    assert not avail(dims_of(9, 3, 2, 2))
    assert not avail(dims_of(10, 3, 1, 2, nu_tot=5, delays=(0, 40, 0, 40, 0)))
    for plant in ("par", "ser"):
        for ctype in ("cent", "coop", "ncoop"):
            assert avail(CmpcDims.from_config(reference_config(plant, ctype, p=50), 1))


MODEL_CASES = [("coop-par", 50, None), ("ncoop-par", 50, None), ("cent-ser", 50, None), ("cent-par", 200, None),
               ("coop-ser", 200, None), ("coop-par", 17, None), ("ncoop-par", 64, (0, 2, 0, 63))]


@pytest.mark.parametrize("name,p,delays", MODEL_CASES)
def test_sweep_is_the_oracles_shift_of_f(name, p, delays):
    """The numpy sweep against the oracle: g within 1e-11 max|g| of Su' w,
    f - g within 1e-11 max|f| of the oracle's f for y_ref + dref, H and G
    bit-identical; max|g| >= 1e-3 max|f|, so doing nothing does not pass
    (1.3e-15, 2.8e-15 and >= 5e-3 measured when the route was chosen)."""
    cfg, arr, _ = RP.config(name, p, delays=delays)
    lin, u_old, _, _ = RP.synthetic_batch(cfg, 2, seed=23 + p)
    dims = CmpcDims.from_config(cfg, 1)
    L = cmpc.layout_of(dims)
    rng = np.random.default_rng(5 + p)
    worst_g = worst_f = 0.0
    least = np.inf
    for q in range(2 * cfg.S):
        s = q % cfg.S
        dref = rng.uniform(-0.2, 0.2, (cfg.p, cfg.ny))
        yr = np.asarray(arr.y_ref[s]).reshape(cfg.p, cfg.ny)
        H0, f0, _, _, G0 = RP.O.build_qp(dims, lin[q], u_old[q], yr, arr.ywt[s], arr.uwt[s])
        H1, f1, _, _, G1 = RP.O.build_qp(dims, lin[q], u_old[q], yr + dref, arr.ywt[s], arr.uwt[s])
        g = RP.sweep_g(cfg, dims, L, lin[q], arr.ywt[s], dref)
        go = RP.oracle_g(cfg, dims, lin[q], arr.ywt[s], dref)
        sg, sf = np.abs(go).max(), np.abs(f1).max()
        worst_g = max(worst_g, np.abs(g - go).max() / sg)
        worst_f = max(worst_f, np.abs(f0 - g - f1).max() / sf)
        least = min(least, sg / sf)
        assert np.array_equal(H0, H1) and np.array_equal(G0, G1)
        np.testing.assert_allclose(g, go, rtol=0, atol=RP.TOL * sg, err_msg=f"slot {q}")
        np.testing.assert_allclose(f0 - g, f1, rtol=0, atol=RP.TOL * sf, err_msg=f"slot {q}")
        assert sg >= 1e-3 * sf, (q, sg / sf)
        if p <= 40:   # the inputs delayed by 40 never arrive inside the horizon
            for c in range(cfg.nu):
                if dims.delay[c] >= p:
                    assert (g[c::cfg.nu] == 0).all()
    print(f"{name} p={p}: g {worst_g:.2e} of max|g|, f - g {worst_f:.2e} of max|f|, max|g|/max|f| >= {least:.2e}")


PLAN_FIELDS = [f[0] for f in CmpcPlan._fields_]
# cmpc_plan for coop-par, p = 50, K = 9 on 256 CUs without the flag, per B and
# step variant (AUTO, SPLIT, FUSED): the plans before reference profiles existed
PLANS_BEFORE = {
    (1, 0): [3, 0, 2, 0, 0, 3, 2, 0, 1, 3, 2, 1, 1],
    (1, 1): [3, 0, 2, 0, 0, 3, 2, 0, 0, 3, 2, 0, 0],
    (1, 2): [3, 0, 2, 0, 1, 1, 1, 0, 1, 3, 2, 1, 1],
    (64, 0): [3, 0, 2, 0, 0, 3, 2, 0, 1, 3, 2, 64, 0],
    (64, 1): [3, 0, 2, 0, 0, 3, 2, 0, 0, 3, 2, 0, 0],
    (64, 2): [3, 0, 2, 0, 1, 1, 1, 0, 1, 3, 2, 64, 0],
    (65536, 0): [2, 0, 1, 0, 0, 2, 1, 0, 0, 2, 1, 0, 0],
    (65536, 1): [2, 0, 1, 0, 0, 2, 1, 0, 0, 2, 1, 0, 0],
    (65536, 2): [2, 0, 1, 0, 1, 2, 1, 0, 0, 2, 1, 0, 0],
}


@pytest.mark.parametrize("B", [1, 64, 65536])
def test_plan_under_the_profile_flag(B):
    cfg = reference_config("par", "coop", p=50)
    dims = CmpcDims.from_config(cfg, B)
    fields = lambda pl: [getattr(pl, k) for k in PLAN_FIELDS]
    split = cmpc.plan(dims, 256, step=cmpc._abi.CMPC_STEP_SPLIT, K=9)
    for step in (cmpc._abi.CMPC_STEP_AUTO, cmpc._abi.CMPC_STEP_SPLIT, cmpc._abi.CMPC_STEP_FUSED):
        assert fields(cmpc.plan(dims, 256, step=step, K=9)) == PLANS_BEFORE[(B, step)], (B, step)
        pl = cmpc.plan(dims, 256, step=step, K=9, flags=cmpc.CMPC_PLAN_REF_PROFILE)
        assert pl.step_fused == 0 and pl.control_fused == 0 and pl.control_grid == 0 and pl.control_polled == 0
        assert (pl.build_kernel, pl.solve_kernel) == (split.build_kernel, split.solve_kernel)
        assert (pl.step_build_kernel, pl.step_solve_kernel) == (split.step_build_kernel, split.step_solve_kernel)
        assert (pl.control_build_kernel, pl.control_solve_kernel) == (split.control_build_kernel,
                                                                      split.control_solve_kernel)
        if step == cmpc._abi.CMPC_STEP_FUSED:
            assert pl.step_error == 6   # CMPC_PLAN_PROFILE_NEEDS_SPLIT
            assert "reference profile" in cmpc.plan_error_string(pl.step_error)
        else:
            assert pl.step_error == 0
    assert cmpc.plan_error_string(5) != cmpc.plan_error_string(6) != "unknown plan error"


def test_profiles_helper_is_offsets_row_by_row():
    rng = np.random.default_rng(2)
    for plant, ctype in (("par", "coop"), ("ser", "coop"), ("par", "ncoop"), ("ser", "cent")):
        cfg = reference_config(plant, ctype, p=7)
        B = 3
        y_dev = rng.normal(size=(B, cfg.p, 4))
        out = cmpc.scenario_reference_profiles(cfg, y_dev)
        assert out.shape == (B * cfg.S, cfg.p, cfg.ny) and out.flags.c_contiguous
        for r in range(cfg.p):
            assert np.array_equal(out[:, r, :], cmpc.scenario_reference_offsets(cfg, y_dev[:, r, :]))
    with pytest.raises(ValueError):
        cmpc.scenario_reference_profiles(cfg, np.zeros((3, 4)))
    with pytest.raises(ValueError):
        cmpc.scenario_reference_profiles(cfg, np.zeros((3, 7, 1)))


def test_schedule_window_rows():
    sch = np.arange(2 * 5 * 1, dtype=np.float64).reshape(2, 5, 1)
    w = RP.schedule_window(sch, 1, 6)
    assert np.array_equal(w[0, :, 0], [2, 3, 4, 4, 4, 4]) and np.array_equal(w[1, :, 0], [7, 8, 9, 9, 9, 9])
