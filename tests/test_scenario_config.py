"""Per-scenario setpoints and input limits (include/cmpc.h,
cmpc_set_scenario_reference / cmpc_set_scenario_constraints): what needs no
GPU.  The entry points exist and refuse a null context; the plant-to-slot
helpers; the identity the build kernels rely on (a constant setpoint offset
dy on y_ref is y_prev - dy in the record), shown with the oracle; and the
kernel selection does not depend on the feature."""
import numpy as np
import pytest

import _oracle as O
import cmpc
import golden_cases as GC
from cmpc._abi import CmpcDims, load_library
from cmpc.synthetic import synthetic_batch

ENTRY_POINTS = ("cmpc_set_scenario_reference", "cmpc_bind_scenario_reference", "cmpc_set_scenario_constraints",
                "cmpc_bind_scenario_constraints", "cmpc_get_scenario_reference", "cmpc_get_scenario_constraints")


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_entry_points_exist_and_refuse_a_null_context(name):
    lib = load_library()
    fn = getattr(lib, name, None)
    assert fn is not None, name
    buf = np.zeros(8)
    p = buf.ctypes.data_as(fn.argtypes[1]) if name.startswith(("cmpc_set", "cmpc_get")) else buf.ctypes.data
    nargs = len(fn.argtypes) - 1
    assert fn(None, *([p] * nargs)) == -1
    assert b"null" in lib.cmpc_last_error()


def test_reference_offsets_follow_out_idx():
    coop = cmpc.reference_config("par", "coop")
    assert [list(o) for o in coop.out_idx] == [[0, 1, 3], [0, 1, 3]]  # both track outputs <0,1,3>
    B = 5
    yo = np.arange(B * 4, dtype=float).reshape(B, 4) + 0.5
    dy = cmpc.scenario_reference_offsets(coop, yo)
    assert dy.shape == (B * coop.S, coop.ny) and dy.flags["C_CONTIGUOUS"]
    for b in range(B):
        for s in range(coop.S):
            assert np.array_equal(dy[b * coop.S + s], yo[b, [0, 1, 3]])
    cent = cmpc.reference_config("ser", "cent")
    dy = cmpc.scenario_reference_offsets(cent, yo)
    assert dy.shape == (B, cent.ny)
    for b in range(B):
        assert np.array_equal(dy[b], yo[b, list(cent.out_idx[0])])
    for bad in (np.zeros(4), np.zeros((B, 2)), np.zeros((B, 4, 1))):
        with pytest.raises(ValueError):
            cmpc.scenario_reference_offsets(coop, bad)


def test_limits_follow_input_order():
    B = 4
    rng = np.random.default_rng(0)
    for plant, ctype in (("par", "coop"), ("ser", "cent")):
        cfg = cmpc.reference_config(plant, ctype)
        plant_arrays = [rng.normal(size=(B, cfg.nu_tot)) for _ in range(4)]
        out = cmpc.scenario_limits(cfg, *plant_arrays)
        assert len(out) == 4
        for a, o in zip(plant_arrays, out):
            assert o.shape == (B * cfg.S, cfg.nu) and o.flags["C_CONTIGUOUS"]
            for b in range(B):
                for s in range(cfg.S):
                    assert np.array_equal(o[b * cfg.S + s], a[b, list(cfg.input_order[s][:cfg.nu])])
        # the shared limits, tiled to the plant and mapped back, are the shared limits
        arr = cmpc.controller_arrays(cfg, cmpc.reference_setup(plant, ctype))
        full = np.zeros((B, cfg.nu_tot))
        for s in range(cfg.S):
            full[:, list(cfg.input_order[s][:cfg.nu])] = arr.lower[s]
        lo = cmpc.scenario_limits(cfg, full, full, full, full)[0]
        for q in range(B * cfg.S):
            assert np.array_equal(lo[q], arr.lower[q % cfg.S])
        with pytest.raises(ValueError):
            cmpc.scenario_limits(cfg, full[:, :-1], full, full, full)
        with pytest.raises(ValueError):
            cmpc.scenario_limits(cfg, full, full[:-1], full, full)
        with pytest.raises(ValueError):
            cmpc.scenario_limits(cfg, full[0], full[0], full[0], full[0])


def offsets(rng, y_ref, y_prev, n):
    """dy uniform in +-0.2 max(|y_ref|, |y_prev|), per slot and output"""
    scale = 0.2 * np.maximum(np.abs(y_ref), np.abs(y_prev))
    return rng.uniform(-1.0, 1.0, (n, y_prev.shape[1])) * scale


@pytest.mark.parametrize("name", ["coop-par", "ncoop-par", "cent-ser"])
def test_oracle_offset_reference_is_shifted_record(name):
    """or_build_qp with y_ref + dy against or_build_qp with y_prev - dy: H and
    G equal, f within the suite's build tolerance 1e-10 max(|f|, 1e-6 |H|)
    (measured: 3.2e-15 relative at worst), and f moves in every slot."""
    cfg, setup, arr, _ = GC.case(name, p=50)
    B = 12
    lin, u_old, _, _ = synthetic_batch(cfg, B, seed=5)
    dims = CmpcDims.from_config(cfg, 1)
    L = cmpc.layout_of(dims)
    nq = B * cfg.S
    y_prev = lin[:, L.off_y:L.off_y + cfg.ny]
    y_ref0 = np.stack([np.asarray(arr.y_ref[q % cfg.S]).reshape(cfg.p, cfg.ny)[0] for q in range(nq)])
    dy = offsets(np.random.default_rng(55), y_ref0, y_prev, nq)
    worst = 0.0
    for q in range(nq):
        s = q % cfg.S
        yr = np.asarray(arr.y_ref[s], dtype=np.float64).reshape(cfg.p, cfg.ny)
        H0, f0, _, _, G0 = O.build_qp(dims, lin[q], u_old[q], yr, arr.ywt[s], arr.uwt[s])
        Ha, fa, _, _, Ga = O.build_qp(dims, lin[q], u_old[q], yr + dy[q], arr.ywt[s], arr.uwt[s])
        rec = lin[q].copy()
        rec[L.off_y:L.off_y + cfg.ny] -= dy[q]
        Hb, fb, _, _, Gb = O.build_qp(dims, rec, u_old[q], yr, arr.ywt[s], arr.uwt[s])
        assert np.array_equal(Ha, Hb) and np.array_equal(Ga, Gb)
        assert np.array_equal(Ha, H0) and np.array_equal(Ga, G0)  # the offset moves f only
        tol = 1e-10 * max(np.abs(fa).max(), 1e-6 * np.abs(Ha).max())
        assert np.abs(fa - fb).max() <= tol, (q, np.abs(fa - fb).max(), tol)
        worst = max(worst, np.abs(fa - fb).max() / np.abs(fa).max())
        assert not np.array_equal(fa, f0), q
    print(f"{name}: worst relative f difference {worst:.2e}")


def test_plan_does_not_depend_on_the_feature():
    """cmpc_plan takes dimensions, batch, CU count and variants only; the
    recorded selections (tests/test_dispatch.py) are the answers with the
    feature in the library.  A few rows of them, spelled out."""
    WAVE, ROWS_B, SPLIT = cmpc.CMPC_BUILD_WAVE, cmpc.CMPC_BUILD_ROWS, cmpc.CMPC_BUILD_SPLIT
    LANE, ROWS_S = cmpc.CMPC_SOLVE_LANE, cmpc.CMPC_SOLVE_ROWS

    def plan(plant, ctype, p, B, **kw):
        return cmpc.plan(CmpcDims.from_config(cmpc.reference_config(plant, ctype, p=p), B), 256, **kw)

    pl = plan("par", "coop", 50, 65536, K=9)  # the headline shape
    assert (pl.build_kernel, pl.solve_kernel, pl.step_fused) == (ROWS_B, LANE, 0)
    pl = plan("par", "coop", 50, 1, K=9)
    assert (pl.control_fused, pl.control_build_kernel, pl.control_solve_kernel, pl.control_polled) == \
        (1, SPLIT, ROWS_S, 1)
    pl = plan("par", "cent", 50, 512, K=2)
    assert (pl.step_fused, pl.step_build_kernel, pl.step_solve_kernel) == (1, WAVE, ROWS_S)
    assert plan("par", "cent", 20, 1025).build_kernel == WAVE
    a, b = plan("ser", "cent", 50, 48, K=9), plan("ser", "cent", 50, 48, K=9)
    assert a.as_dict() == b.as_dict()
