"""The steady-state target solve on the device (cmpc_sim_target, DESIGN.md
§3.21) against its host twin (cmpc_plant_target_host), bit for bit: batches
with full and partial waves, one to four held outputs, pressures as scalars,
set and bound, a short iteration budget, one wave with four different
statuses, nh = 0 against cmpc_sim_equilibrium, the simulator state the call
must leave alone, and ClosedLoop.trim_to_outputs."""
import numpy as np
import pytest

import cmpc
import equilibrium_cases as EC
import target_cases as TC

pytestmark = pytest.mark.gpu
TS = 0.05
NAMES = ("x", "u_full", "status", "iters", "resid")


@pytest.fixture(autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()
    yield


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda()   # (a copy: the cases are read-only)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def device_solve(plant, hold, free, t, u, x0, scalars=(1.0, 1.0), pressures=None, bind=False, on_device=False, **kw):
    """(x, u_full, status, iters, resid) of PlantSimulator.target from x0 at
    the plant input u: the scalars, or `pressures` set (copied) or bound; the
    targets from the host or as a device tensor.  The input offset must follow
    the plant input where the status is OK and stay elsewhere."""
    from cmpc.sim import PlantSimulator
    B = len(x0)
    with PlantSimulator(plant, B, p_in=scalars[0], p_out=scalars[1]) as sim:
        sim.reset(dev(x0), dev(u), TS)
        keep = None
        if pressures is not None and bind:
            keep = dev(pressures)
            sim.bind_pressures(keep.data_ptr())
        elif pressures is not None:
            sim.set_pressures(np.ascontiguousarray(pressures))
        tt = dev(np.broadcast_to(t, (B, len(hold)))) if on_device else t
        st, it, r = sim.target(hold, free, tt, **kw)
        x, uf, dt, sst = sim.download()
        off, ring = sim.download_inputs()
        assert (dt == TS).all() and (sst == 0).all() and (ring == 0).all()   # step sizes, status, delay lines stay
        assert np.array_equal(bits(off), bits(uf))      # after reset the offset is the plant input
    return x, uf, st, it, r


def assert_same(dev_res, host_res, rows=slice(None)):
    for a, b, what in zip(dev_res, host_res, NAMES):
        a, b = np.asarray(a)[rows], np.asarray(b)[rows]
        if a.dtype == np.float64:
            a, b = bits(a), bits(b)
        assert np.array_equal(a, b), (what, np.argwhere(a != b)[:4])


def rows_of(plant):
    """(held outputs, free inputs, recycle valves opened) for nh = 1, 2 and,
    for the serial plant, 4."""
    if plant == 0:
        return (((3,), (0,), False), ((0, 1), (0, 2), False))
    return (((3,), (2,), False), ((1, 3), (0, 2), False), TC.ALL_FOUR + (True,))


@pytest.mark.parametrize("B", [1, 5, 70])
@pytest.mark.parametrize("plant", [0, 1])
def test_device_equals_host_twin(plant, B):
    """Per-scenario pressures: x, u_full, status, iters and resid with no
    tolerance.  B = 70: seventeen full waves of four rows and a wave with two
    rows idle."""
    for hold, free, recycle in rows_of(plant):
        p, u, x, t = TC.cases(plant, hold, B=B, recycle=recycle)
        host = cmpc.plant_target(plant, p, hold, free, t, u, x)
        assert (host[2] == cmpc.CMPC_EQ_OK).all() and host[3].min() >= 2
        assert_same(device_solve(plant, hold, free, t, u, x, pressures=p), host)
        assert_same(device_solve(plant, hold, free, t, u, x, pressures=p, on_device=True), host)
        # an iteration budget that stops every scenario short
        budget = int(host[3].min()) - 1
        short = cmpc.plant_target(plant, p, hold, free, t, u, x, max_iter=budget)
        assert (short[2] == cmpc.CMPC_EQ_NO_CONVERGENCE).all()
        assert_same(device_solve(plant, hold, free, t, u, x, pressures=p, max_iter=budget), short)


@pytest.mark.parametrize("plant", [0, 1])
def test_parallel_all_four_and_the_dead_zone_crossings(plant):
    """All four inputs free, B = 64: for the parallel plant some scenarios
    cross into the dead zone during the iteration or lose their flow, and the
    device reports each as the host does."""
    p, u, x, t = TC.cases(plant, TC.ALL_FOUR[0], recycle=True)
    host = cmpc.plant_target(plant, p, *TC.ALL_FOUR, t, u, x)
    if plant == 0:
        assert (host[2] == cmpc.CMPC_EQ_DEADZONE).sum() >= 2 and (host[2] == cmpc.CMPC_EQ_OK).sum() >= 32
    assert_same(device_solve(plant, *TC.ALL_FOUR, t, u, x, pressures=p), host)


@pytest.mark.parametrize("plant", [0, 1])
def test_scalar_and_per_scenario_pressures_agree(plant):
    B = 70
    hold, free, _ = rows_of(plant)[1]
    pc = EC.class_pressures(B)
    # every scenario starts at the equilibrium of its class and moves a little from there
    _, u, x0, move = TC.cases(plant, hold, B=B)
    x, st, _, _ = cmpc.plant_equilibrium(plant, pc, u, x0)
    assert (st == cmpc.CMPC_EQ_OK).all()
    t = TC.outputs(plant, x)[:, list(hold)] + 0.2 * (move - TC.outputs(plant, x0)[:, list(hold)])
    cls = np.arange(B) % len(EC.CLASSES)
    scalar = [device_solve(plant, hold, free, t, u, x, scalars=tuple(c)) for c in EC.CLASSES]
    for bind in (False, True):
        got = device_solve(plant, hold, free, t, u, x, pressures=pc, bind=bind)
        assert (got[2] == cmpc.CMPC_EQ_OK).all()
        for k in range(len(EC.CLASSES)):
            assert_same(got, scalar[k], rows=cls == k)
    assert not np.array_equal(scalar[0][0], scalar[1][0])     # the classes do differ
    assert_same(scalar[1], cmpc.plant_target(plant, np.tile(EC.CLASSES[1], (B, 1)), hold, free, t, u, x))


def test_one_wave_with_four_statuses():
    """B = 4, the parallel plant with all four inputs free: a scenario that
    converges, one with a recycle valve in the dead zone, one without
    a flow (pressures (1.0, 1.2)) and one whose integration failed (skipped).
    The plant input carries a control input on top of the offset, so the
    offset written is v - (u_full - u_offset) of before."""
    from cmpc.sim import PlantSimulator
    plant = 0
    p, u, x, t = TC.cases(plant, TC.ALL_FOUR[0], recycle=True)
    st64 = cmpc.plant_target(plant, p, *TC.ALL_FOUR, t, u, x)[2]
    pick = [int(np.flatnonzero(st64 == cmpc.CMPC_EQ_OK)[0])] * 4
    p, u, x, t = (np.array(a[pick]) for a in (p, u, x, t))
    q = p.copy()
    q[2] = EC.NO_EQUILIBRIUM
    u[1, 3] = 0.015                                      # a free recycle valve below 2e-2
    x[3, 2] = np.nan
    uc = np.tile([1e-3, 0.0, -2e-3, 0.0], (4, 1))        # the torques are not delayed
    with PlantSimulator(plant, 4) as sim:
        sim.reset(dev(x), dev(u), TS)
        sim.set_pressures(p)
        sim.set_input(dev(uc))
        sim.integrate(0.0, TS)
        sim.set_pressures(q)
        x_in, u_in, dt_in, sst = sim.download()
        off_in, ring_in = sim.download_inputs()
        assert sst.tolist() == [0, 0, 0, 3], sst
        assert np.array_equal(u_in[:, [0, 4]], off_in[:, [0, 4]] + uc[:, [0, 2]])
        status, iters, resid = sim.target(*TC.ALL_FOUR, t)
        x_out, u_out, dt_out, sst2 = sim.download()
        off_out, ring_out = sim.download_inputs()
    host = cmpc.plant_target(plant, q[:3], *TC.ALL_FOUR, t[:3], u_in[:3], x_in[:3])
    assert host[2].tolist() == [cmpc.CMPC_EQ_OK, cmpc.CMPC_EQ_DEADZONE, cmpc.CMPC_EQ_NONFINITE], host[2]
    assert_same((x_out, u_out, status, iters, resid), host, rows=slice(0, 3))
    assert status[3] == cmpc.CMPC_EQ_SKIPPED and iters[3] == 0 and (resid[3] == 0).all()
    # untouched: step sizes, delay lines, simulator status; x, input and offset of every row but the OK one
    assert np.array_equal(bits(dt_out), bits(dt_in)) and np.array_equal(sst2, sst)
    assert np.array_equal(bits(ring_out), bits(ring_in))
    for a, b in ((x_out, x_in), (u_out, u_in), (off_out, off_in)):
        assert np.array_equal(bits(a[1:]), bits(b[1:]))
    cols = list(TC.PLANT_INPUT)
    fixed = np.setdiff1d(np.arange(u.shape[1]), cols)
    assert np.array_equal(bits(off_out[0, fixed]), bits(off_in[0, fixed]))
    assert np.array_equal(bits(off_out[0, cols]), bits(u_out[0, cols] - (u_in[0, cols] - off_in[0, cols])))
    assert (off_out[0, [0, 4]] != u_out[0, [0, 4]]).all() and (u_out[0, cols] != u_in[0, cols]).all()


@pytest.mark.parametrize("plant", [0, 1])
def test_no_held_output_is_the_equilibrium_launch(plant):
    """nh = 0 against cmpc_sim_equilibrium on the same simulator state; the
    equilibrium solve's results stay in buffers of their own."""
    from cmpc.sim import PlantSimulator
    B = 9
    p, u, x0 = EC.cases(plant, B=B)
    p = p.copy()
    p[3] = EC.NO_EQUILIBRIUM
    res = []
    for which in (0, 1):
        with PlantSimulator(plant, B) as sim:
            sim.reset(dev(x0), dev(u), TS)
            sim.set_pressures(p)
            if which == 0:
                st, it, r = sim.equilibrium()
                tg = sim.target((0,), (0,), TC.outputs(plant, x0)[:, :1])      # a later target solve
                again = [np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B)]
                cmpc.check(sim.lib.cmpc_sim_equilibrium_download(sim._h, cmpc.iptr(again[0]), cmpc.iptr(again[1]),
                                                                 cmpc.dptr(again[2])), "download")
                assert np.array_equal(again[0], st) and np.array_equal(again[1], it)
                assert np.array_equal(bits(again[2]), bits(r)) and tg[2].shape == (B, 2)
                res.append((None, st, it, r))
            else:
                st, it, r = sim.target([], [], np.zeros((B, 0)))
                assert (r[:, 1] == 0).all()
                res.append((sim.download()[0], st, it, r[:, 0]))
    host = cmpc.plant_equilibrium(plant, p, u, x0)
    assert host[1][3] == cmpc.CMPC_EQ_NONFINITE and (np.delete(host[1], 3) == cmpc.CMPC_EQ_OK).all()
    for a, b in zip(res[1], host):
        assert np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b)
    for a, b in zip(res[0][1:], host[1:]):
        assert np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b)


def test_device_argument_errors_are_refused():
    from cmpc.sim import PlantSimulator
    x0, u0 = cmpc.plant_default(0)
    with PlantSimulator(0, 1) as sim:
        sim.reset(dev([x0]), dev([u0]), TS)
        assert sim.lib.cmpc_sim_target_download(sim._h, None, None, None) < 0
        assert "cmpc_sim_target first" in sim.lib.cmpc_last_error().decode()
        assert sim.lib.cmpc_sim_target_status(sim._h) is None
        for args, kw, word in ((((0, 0), (0, 2), [4.5, 4.5]), {}, "hold_idx repeats"),
                               (((0, 1), (0, 4), [4.5, 4.5]), {}, "free_idx"),
                               (((0,), (0,), [4.5]), {"max_iter": 65}, "max_iter"),
                               (((0,), (0,), [4.5]), {"tol_y": 0.0}, "tol_y")):
            with pytest.raises(RuntimeError, match=word):
                sim.target(*args, **kw)
        with pytest.raises(ValueError):
            sim.target((0, 1), (0, 2), [4.5])
        assert np.array_equal(sim.download()[0][0], x0)
        st, it, r = sim.target((0, 1), (0, 2), [4.5, 4.5])
        assert st[0] == cmpc.CMPC_EQ_OK
        assert all(f(sim._h) for f in (sim.lib.cmpc_sim_target_status, sim.lib.cmpc_sim_target_iters,
                                       sim.lib.cmpc_sim_target_resid))
    assert sim.lib.cmpc_sim_target(None, 0, None, None, None, 20, 1e-12, 1e-10) < 0


# ---- the closed loop ------------------------------------------------------------

def _loop(cfg, arr, x0, u_def, pressures, how, n=20, K=9):
    """(the trim's result or None, x0 in force, y per step (n, B, 4), u_ctrl per
    step, the scores): how = None, "trim" or "outputs"."""
    import torch
    from cmpc.driver import ClosedLoop
    B = len(x0)
    M = cmpc.reference_observer_gain(cfg)
    loop = ClosedLoop(cfg, arr, [M] * cfg.S, x0, np.tile(u_def, (B, 1)), K, pressures=pressures)
    try:
        loop.enable_scores()
        res = None
        if how == "trim":
            res = loop.trim()
        elif how == "outputs":
            res = loop.trim_to_outputs(hold=[0, 1], targets=[4.5, 4.5])
        x_start = loop.x0.cpu().numpy()
        loop.initialize()
        ys, us = [], []
        for _ in range(n):
            _, y = loop.step()
            ys.append(y.cpu().numpy().copy())
            us.append(loop.u_ctrl.cpu().numpy().copy())
        assert loop.plant_failures()[0] == 0
        scores = loop.scores()
    finally:
        loop.close()
    torch.cuda.synchronize()
    return res, x_start, np.stack(ys), np.stack(us), scores


def _peak01(cfg, scores):
    """(B,): the peak error over the controlled outputs that are plant outputs 0 and 1."""
    oi = np.asarray(cfg.out_idx)[:, :cfg.ny]
    sel = (oi == 0) | (oi == 1)
    assert sel.any()
    return scores["peak"][:, sel].max(axis=1)


def test_closed_loop_starts_at_rest_at_the_setpoint():
    """coop-par, p = 20, K = 9, B = 6, the three pressure classes twice, 20
    steps.  After trim() the loop opens with the distance of the rest point
    from the setpoint in outputs 0 and 1 (about 1.7e-2 at nominal pressures);
    after trim_to_outputs(hold=[0, 1], targets=[4.5, 4.5]) it opens within
    tol_y = 1e-10 of it, and the peak error over the run must be at most 1e-3
    of the former: five of the eight orders are left for what the discretised
    model and the integrator leave at rest.  Measured on an MI355X: 1.746e-2
    against 1.31e-5 at (1, 1), ratio 7.5e-4, and 1.470 against 1.24e-3 at
    (1.03, 0.98), ratio 8.4e-4.  At (0.97, 1.02) no torque holds a surge
    distance of 4.5: those scenarios report NONFINITE, keep
    their x0 and offset, and are held to that instead of the ratio."""
    from cmpc.configs import reference_setup
    cfg = cmpc.reference_config("par", "coop", p=20)
    arr = cmpc.controller_arrays(cfg, reference_setup("par", "coop"))
    B = 6
    xd, u_def = cmpc.plant_default(cfg.plant)
    x0 = np.tile(xd, (B, 1))
    pc = EC.class_pressures(B)

    res_t, _, ys_t, us_t, sc_t = _loop(cfg, arr, x0, u_def, pc, "trim")
    res_o, x_o, ys_o, us_o, sc_o = _loop(cfg, arr, x0, u_def, pc, "outputs")
    host = cmpc.plant_target(cfg.plant, pc, (0, 1), (0, 2), [4.5, 4.5], np.tile(u_def, (B, 1)), x0)
    # at (0.97, 1.02) the rest point has a surge distance of 3.0 and no torque brings it to 4.5
    # (DESIGN.md §3.21): those two scenarios report NONFINITE and keep what they were given
    ok = np.arange(B) % 3 != 1
    assert (res_t[0] == cmpc.CMPC_EQ_OK).all()
    assert (res_o.status[ok] == cmpc.CMPC_EQ_OK).all() and (res_o.status[~ok] == cmpc.CMPC_EQ_NONFINITE).all()
    assert np.array_equal(res_o.status, host[2]) and np.array_equal(res_o.iters, host[3])
    assert np.array_equal(bits(x_o), bits(host[0])) and np.array_equal(bits(res_o.u_free), bits(host[1][:, [0, 4]]))
    assert np.array_equal(bits(res_o.resid), bits(host[4]))
    assert np.array_equal(bits(res_o.du_free), bits(host[1][:, [0, 4]] - np.tile(u_def, (B, 1))[:, [0, 4]]))
    assert np.array_equal(bits(x_o[~ok]), bits(x0[~ok])) and (res_o.du_free[~ok] == 0).all()
    assert np.abs(ys_o[0][ok, :2] - 4.5).max() <= 1e-10

    peak_t, peak_o = _peak01(cfg, sc_t), _peak01(cfg, sc_o)
    print("peak error of outputs 0 and 1 after trim()", peak_t, "after trim_to_outputs", peak_o, "ratio",
          peak_o / peak_t)
    assert 1e-2 < peak_t[0] < 3e-2                  # nominal pressures: the rest point's distance, about 1.7e-2
    assert (peak_o[ok] <= 1e-3 * peak_t[ok]).all()

    # a loop that never calls the new method is what it was: the same run again, after the
    # new method has run in this process, repeats itself bit for bit
    _, _, ys_v, us_v, _ = _loop(cfg, arr, x0, u_def, pc, "trim")
    assert np.array_equal(bits(ys_v), bits(ys_t)) and np.array_equal(bits(us_v), bits(us_t))
    assert not np.array_equal(bits(ys_o), bits(ys_t))


def test_trim_to_outputs_moves_pending_segments_and_keeps_failures():
    """The change of the free inputs is added to every pending set_segments
    offset; a scenario that is not OK keeps its x0 and offset."""
    from cmpc.configs import reference_setup
    from cmpc.driver import ClosedLoop
    cfg = cmpc.reference_config("par", "coop", p=20)
    arr = cmpc.controller_arrays(cfg, reference_setup("par", "coop"))
    B = 3
    xd, u_def = cmpc.plant_default(cfg.plant)
    x0 = np.tile(xd, (B, 1))
    pc = np.array([[1.0, 1.0], EC.NO_EQUILIBRIUM, [1.03, 0.98]])
    step = np.zeros(len(u_def))
    step[8] = -0.1
    loop = ClosedLoop(cfg, arr, [cmpc.reference_observer_gain(cfg)] * cfg.S, x0, np.tile(u_def, (B, 1)), 3,
                      pressures=pc)
    try:
        loop.set_segments([(np.zeros(len(u_def)), 1.0), (step, 2.0)], u_def)
        res = loop.trim_to_outputs([0, 1], [4.5, 4.5])
        assert res.status.tolist() == [cmpc.CMPC_EQ_OK, cmpc.CMPC_EQ_NONFINITE, cmpc.CMPC_EQ_OK]
        off = loop.u_offset.cpu().numpy()
        later = loop._sched[0][1].cpu().numpy()
        assert np.array_equal(bits(loop.x0.cpu().numpy()[1]), bits(xd)) and np.array_equal(bits(off[1]), bits(u_def))
        assert (res.du_free[1] == 0).all() and (res.du_free[[0, 2]] != 0).all()
        assert np.array_equal(bits(off[:, [0, 4]]), bits(res.u_free))
        want = np.tile(u_def + step, (B, 1))
        want[:, [0, 4]] += res.du_free
        assert np.array_equal(bits(later), bits(want))
        with pytest.raises(ValueError):
            loop.trim_to_outputs([0, 1, 2], [4.5, 4.5, 0.0])
    finally:
        loop.close()
