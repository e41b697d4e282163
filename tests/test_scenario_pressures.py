"""Per-scenario boundary pressures (include/cmpc.h) without a
GPU: the entry points exist and refuse a null handle, the host setters' check
refuses non-finite and non-positive values, cmpc_plan is what it was before
the feature, the host producer at non-default pressures equals the oracle's,
and the pressure-aware restatement of the oracle loop (pressure_loop.py) is
OracleClosedLoop itself at (1, 1).  CPU only."""
import ctypes

import numpy as np
import pytest

import _oracle as O
import cmpc
import golden_cases as GC
from cmpc._abi import CmpcDims, dptr, load_library
from cmpc.configs import reference_config

CUS = 256  # MI355X


def scenario_pressures(B, seed=0):
    """(B, 2) pressures in 1 +- 0.05, all 2 B values distinct and p_in != p_out
    in every scenario, so an index, stride or swap error shows."""
    rng = np.random.default_rng(100 + seed)
    v = 0.95 + 0.1 * (rng.permutation(2 * B) + 0.5) / (2 * B)
    p = v.reshape(B, 2)
    assert len(set(p.ravel())) == 2 * B and (np.abs(p - 1) <= 0.05).all()
    return p


def test_pressure_symbols_refuse_null_handle():
    lib = load_library()
    for name in ("cmpc_set_scenario_pressures", "cmpc_bind_scenario_pressures", "cmpc_get_scenario_pressures",
                 "cmpc_sim_set_pressures", "cmpc_sim_set_pressures_host", "cmpc_sim_bind_pressures",
                 "cmpc_sim_get_pressures", "cmpc_check_pressures"):
        assert hasattr(lib, name), name
    p = np.ones((3, 2))
    for call in (lambda: lib.cmpc_set_scenario_pressures(None, dptr(p)),
                 lambda: lib.cmpc_set_scenario_pressures(None, None),
                 lambda: lib.cmpc_bind_scenario_pressures(None, None),
                 lambda: lib.cmpc_get_scenario_pressures(None, dptr(p)),
                 lambda: lib.cmpc_sim_set_pressures(None, None),
                 lambda: lib.cmpc_sim_set_pressures_host(None, dptr(p)),
                 lambda: lib.cmpc_sim_bind_pressures(None, None),
                 lambda: lib.cmpc_sim_get_pressures(None, dptr(p)),
                 lambda: lib.cmpc_check_pressures(3, None),
                 lambda: lib.cmpc_check_pressures(0, dptr(p))):
        assert call() == -1
        assert b"null" in lib.cmpc_last_error()


def test_pressure_check_refuses_bad_values():
    """cmpc_check_pressures is the check of cmpc_set_scenario_pressures and
    cmpc_sim_set_pressures_host (which need a device for their handles)."""
    lib = load_library()
    good = scenario_pressures(7)
    assert lib.cmpc_check_pressures(7, dptr(good)) == 0
    for bad_value in (np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0):
        for where in ((0, 0), (4, 1), (6, 1)):
            p = good.copy()
            p[where] = bad_value
            assert lib.cmpc_check_pressures(7, dptr(p)) == -1, (bad_value, where)
            msg = lib.cmpc_last_error().decode()
            assert f"scenario {where[0]}:" in msg and "finite and positive" in msg, msg
    # the smallest positive values pass: > 0 is the whole rule
    tiny = np.full((2, 2), 5e-324)
    assert lib.cmpc_check_pressures(2, dptr(tiny)) == 0


# recorded from the library before the feature existed (p = 50, K = 9, 256 CUs,
# every variant AUTO): cmpc_plan_t field by field
PLANS_BEFORE = {
    ("par", "coop", 1): (3, 0, 2, 0, 0, 3, 2, 0, 1, 3, 2, 1, 1),
    ("par", "coop", 5): (3, 0, 2, 0, 0, 3, 2, 0, 1, 3, 2, 5, 0),
    ("par", "coop", 150): (3, 0, 2, 0, 0, 3, 2, 0, 1, 1, 1, 75, 0),
    ("par", "coop", 1024): (1, 0, 2, 0, 0, 1, 2, 0, 0, 1, 2, 0, 0),
    ("par", "coop", 65536): (2, 0, 1, 0, 0, 2, 1, 0, 0, 2, 1, 0, 0),
    ("par", "ncoop", 1): (3, 0, 2, 0, 0, 3, 2, 0, 1, 3, 2, 1, 1),
    ("par", "ncoop", 5): (3, 0, 2, 0, 0, 3, 2, 0, 1, 3, 2, 5, 0),
    ("par", "ncoop", 150): (3, 0, 2, 0, 0, 3, 2, 0, 1, 1, 1, 75, 0),
    ("par", "ncoop", 1024): (1, 0, 2, 0, 0, 1, 2, 0, 0, 1, 2, 0, 0),
    ("par", "ncoop", 65536): (2, 0, 1, 0, 0, 2, 1, 0, 0, 2, 1, 0, 0),
    ("par", "cent", 1): (3, 0, 2, 0, 0, 3, 2, 0, 1, 3, 2, 1, 1),
    ("par", "cent", 5): (3, 0, 2, 0, 0, 3, 2, 0, 1, 3, 2, 3, 0),
    ("par", "cent", 150): (3, 0, 2, 0, 0, 3, 2, 0, 1, 3, 2, 75, 0),
    ("par", "cent", 1024): (3, 0, 2, 0, 1, 1, 2, 0, 1, 1, 2, 256, 0),
    ("par", "cent", 65536): (2, 0, 1, 0, 0, 2, 1, 0, 0, 2, 1, 0, 0),
    ("ser", "coop", 1): (3, 0, 2, 0, 0, 3, 2, 0, 1, 3, 2, 1, 1),
    ("ser", "coop", 5): (3, 0, 2, 0, 0, 3, 2, 0, 1, 3, 2, 5, 0),
    ("ser", "coop", 150): (3, 0, 2, 0, 0, 3, 2, 0, 1, 1, 1, 75, 0),
    ("ser", "coop", 1024): (1, 0, 2, 0, 0, 1, 2, 0, 0, 1, 2, 0, 0),
    ("ser", "coop", 65536): (2, 0, 1, 0, 0, 2, 1, 0, 0, 2, 1, 0, 0),
    ("ser", "ncoop", 1): (3, 0, 2, 0, 0, 3, 2, 0, 1, 3, 2, 1, 1),
    ("ser", "ncoop", 5): (3, 0, 2, 0, 0, 3, 2, 0, 1, 3, 2, 5, 0),
    ("ser", "ncoop", 150): (3, 0, 2, 0, 0, 3, 2, 0, 1, 1, 1, 75, 0),
    ("ser", "ncoop", 1024): (1, 0, 2, 0, 0, 1, 2, 0, 0, 1, 2, 0, 0),
    ("ser", "ncoop", 65536): (2, 0, 1, 0, 0, 2, 1, 0, 0, 2, 1, 0, 0),
    ("ser", "cent", 1): (3, 0, 2, 0, 0, 3, 2, 0, 1, 3, 2, 1, 1),
    ("ser", "cent", 5): (3, 0, 2, 0, 0, 3, 2, 0, 1, 3, 2, 3, 0),
    ("ser", "cent", 150): (3, 0, 2, 0, 0, 3, 2, 0, 1, 3, 2, 75, 0),
    ("ser", "cent", 1024): (3, 0, 2, 0, 1, 1, 2, 0, 1, 1, 2, 256, 0),
    ("ser", "cent", 65536): (2, 0, 1, 0, 0, 2, 1, 0, 0, 2, 1, 0, 0),
}


def test_plan_is_unchanged_by_the_feature():
    """Pressures reach the record producer alone: cmpc_plan has no flag for
    them, and every plan is the one recorded before the feature."""
    for (plant, ctype, B), values in PLANS_BEFORE.items():
        cfg = reference_config(plant, ctype, p=50)
        pl = cmpc.plan(CmpcDims.from_config(cfg, B), CUS, K=9)
        assert tuple(pl.as_dict().values()) == values, (plant, ctype, B)


@pytest.mark.parametrize("plant", [0, 1])
def test_plant_producer_matches_oracle_at_other_pressures(plant):
    """cmpc_plant_lin_record == or_lin_record at pressures of 1 +- 0.05, by
    test_abi.py's comparison at the default; and the pressures matter."""
    rng = np.random.default_rng(17)
    cfg = reference_config("par" if plant == 0 else "ser", "coop", p=20)
    dims = CmpcDims.from_config(cfg, 1)
    x0, u0 = cmpc.plant_default(plant)
    press = scenario_pressures(20, seed=plant)
    for trial in range(20):
        x = x0 * (1 + 0.02 * rng.normal(size=len(x0)))
        u = u0.copy()
        if trial % 2 == 0:
            u[3] = 0.0; u[7] = 0.0          # closed recycle valves (the reference's operating point)
        else:
            u[3] = rng.uniform(0.02, 0.3); u[7] = rng.uniform(0.02, 0.3)
        u[[0, 3, 4, 7]] += rng.uniform(-0.02, 0.02, 4)
        p_in, p_out = press[trial]
        for s in range(cfg.S):
            a = cmpc.plant_lin_record(cfg, dims, s, x, u, p_in=p_in, p_out=p_out)
            b = O.lin_record(cfg, dims, s, x, u, p_in=p_in, p_out=p_out)
            np.testing.assert_allclose(a, b, rtol=1e-11, atol=1e-14)
            assert not np.array_equal(a, cmpc.plant_lin_record(cfg, dims, s, x, u))
            assert not np.array_equal(a, cmpc.plant_lin_record(cfg, dims, s, x, u, p_in=p_out, p_out=p_in))


@pytest.mark.parametrize("name", ["coop-par", "cent-ser"])
def test_pressure_loop_at_default_is_the_oracle_loop(name):
    """pressure_loop.PressureClosedLoop with both pairs at (1, 1), through a
    plant-input step, reproduces OracleClosedLoop exactly; with a constant
    schedule of (1, 1) rows too."""
    from oracle_loop import OracleClosedLoop
    from pressure_loop import PressureClosedLoop
    cfg, setup, arr, g = GC.case(name)
    M = [cmpc.reference_observer_gain(cfg)] * cfg.S
    _, u_def = O.plant_default(cfg.plant)
    d = np.zeros(len(u_def))
    d[8 if cfg.plant == 0 else 6] = -0.05
    segs = [(np.zeros(len(u_def)), 1.0), (d, 1e9)]
    ref = OracleClosedLoop(cfg, arr, M, g["n_iterations"], segs)
    a = PressureClosedLoop(cfg, arr, M, g["n_iterations"], (1.0, 1.0), (1.0, 1.0), segments=segs)
    b = PressureClosedLoop(cfg, arr, M, g["n_iterations"], segments=segs, plant_schedule=np.ones((3, 2)),
                           model_schedule=np.ones((1, 2)))
    for k in range(50):
        y = ref.step()
        for loop in (a, b):
            assert np.array_equal(loop.step(), y), k
            assert np.array_equal(loop.u_ctrl, ref.u_ctrl), k
            assert np.array_equal(loop.sim.x, ref.sim.x), k


def test_pressure_loop_responds_to_each_pair():
    """The helper's two pairs are wired to different things: the plant's move
    y with the model untouched, the model's move u at once."""
    from pressure_loop import PressureClosedLoop
    cfg, setup, arr, g = GC.case("coop-par")
    M = [cmpc.reference_observer_gain(cfg)] * cfg.S
    mk = lambda pp, pm, **kw: PressureClosedLoop(cfg, arr, M, g["n_iterations"], pp, pm, **kw)
    base, plant, model = mk((1, 1), (1, 1)), mk((0.96, 1.03), (1, 1)), mk((1, 1), (0.96, 1.03))
    sched = mk((1, 1), (1, 1), plant_schedule=np.array([[1, 1]] * 3 + [[0.96, 1.03]]))
    ys = {n: [] for n in ("base", "plant", "model", "sched")}
    for k in range(6):
        for n, loop in (("base", base), ("plant", plant), ("model", model), ("sched", sched)):
            ys[n].append((loop.step().copy(), loop.u_ctrl.copy()))
    # instant 0: same measurement everywhere; only the model pair moves u(0)
    assert np.array_equal(ys["plant"][0][0], ys["base"][0][0])
    assert np.array_equal(ys["plant"][0][1], ys["base"][0][1])
    assert not np.array_equal(ys["model"][0][1], ys["base"][0][1])
    # the plant pair shows in y from instant 1 on
    assert not np.array_equal(ys["plant"][1][0], ys["base"][1][0])
    # the schedule's row 3 acts on the interval after instant 3: y(4) moves, y(3) does not
    assert np.array_equal(ys["sched"][3][0], ys["base"][3][0])
    assert not np.array_equal(ys["sched"][4][0], ys["base"][4][0])
