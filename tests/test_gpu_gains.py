"""The steady-state gains on the device (cmpc_sim_gains)
against their host twin (cmpc_plant_gains_host), bit for bit on the record and
the status: batches of one row, a partial wave and several workgroups with a
ragged tail, both plants, selections 1 x 1, 2 x 2, 4 x 4 and 4 x 2, pressures
as scalars, set and bound, one wave with four different statuses, a selection
whose G is rank-deficient, the simulator state the call must leave alone, and
ClosedLoop.gains."""
import numpy as np
import pytest

import cmpc
import equilibrium_cases as EC
import gains_cases as GC

pytestmark = pytest.mark.gpu
TS = 0.05
OK = cmpc.CMPC_EQ_OK
bits = GC.bits


@pytest.fixture(autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()
    yield


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda()   # (a copy: the cases are read-only)


def snapshot(sim):
    """Everything of the simulator that the call must leave alone."""
    return sim.download() + sim.download_inputs()


def assert_untouched(before, after):
    for a, b in zip(before, after):
        assert np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b)


def device_gains(plant, selections, u, x, scalars=(1.0, 1.0), pressures=None, bind=False):
    """PlantSimulator.gains for every selection on one simulator at the state x
    and the plant input u: the scalars, or `pressures` set (copied) or bound.
    x, u_full, step sizes, status, offset and delay line must stay bit for bit."""
    from cmpc.sim import PlantSimulator
    with PlantSimulator(plant, len(x), p_in=scalars[0], p_out=scalars[1]) as sim:
        sim.reset(dev(x), dev(u), TS)
        keep = None
        if pressures is not None and bind:
            keep = dev(pressures)
            sim.bind_pressures(keep.data_ptr())
        elif pressures is not None:
            sim.set_pressures(np.ascontiguousarray(pressures))
        before = snapshot(sim)
        out = [sim.gains(*sel) for sel in selections]
        assert_untouched(before, snapshot(sim))
        assert np.array_equal(bits(before[0]), bits(x)) and np.array_equal(bits(before[1]), bits(u))
    return out


def assert_same(got, want, rows=slice(None)):
    assert np.array_equal(got.status[rows], want.status[rows]), (got.status, want.status)
    a, b = bits(got.record[rows]), bits(want.record[rows])
    assert np.array_equal(a, b), np.argwhere(a != b)[:6]


@pytest.mark.parametrize("B", [1, 5, 70])
@pytest.mark.parametrize("plant", [0, 1])
def test_device_equals_host_twin(plant, B):
    """Per-scenario pressures, every selection shape: the record and the
    status with no tolerance.  B = 70: seventeen full waves of four rows and a
    wave with two rows idle."""
    p, u, x = GC.cases(plant, B=B)
    got = device_gains(plant, GC.SELECTIONS, u, x, pressures=p)
    for sel, g in zip(GC.SELECTIONS, got):
        host = cmpc.plant_gains(plant, p, u, x, *sel)
        assert (host.status == OK).all() and not np.isnan(host.G).any()
        assert_same(g, host)
        assert g.G.shape == (B, len(sel[0]), len(sel[1]))


@pytest.mark.parametrize("plant", [0, 1])
def test_scalar_set_and_bound_pressures_agree(plant):
    B = 7
    _, u, _ = GC.cases(plant, B=B)
    pc = EC.class_pressures(B)
    x, st, _, _ = cmpc.plant_equilibrium(plant, pc, u, GC.cases(plant, B=B)[2])
    assert (st == OK).all()
    sel = GC.SELECTIONS[1:3]
    cls = np.arange(B) % len(EC.CLASSES)
    scalar = [device_gains(plant, sel, u, x, scalars=tuple(c)) for c in EC.CLASSES]
    host = [cmpc.plant_gains(plant, pc, u, x, *s) for s in sel]
    for bind in (False, True):
        got = device_gains(plant, sel, u, x, pressures=pc, bind=bind)
        for j in range(len(sel)):
            assert_same(got[j], host[j])
            for k in range(len(EC.CLASSES)):
                assert_same(got[j], scalar[k][j], rows=cls == k)
    assert not np.array_equal(bits(scalar[0][0].G), bits(scalar[1][0].G))     # the classes do differ


def test_one_wave_with_four_statuses():
    """B = 4, the parallel plant: a scenario at rest, one with a selected
    recycle valve in the dead zone, one with a NaN in its plant input and one
    whose integration failed (skipped).  The same wave with the valve not
    selected: the second row is OK too."""
    from cmpc.sim import PlantSimulator
    plant = 0
    p, u, x = (np.array(a[[0, 0, 0, 0]]) for a in GC.cases(plant))
    u[1, 3] = 0.01
    x[3, 2] = np.nan
    off = u.copy()
    off[2, 0] = np.nan
    with PlantSimulator(plant, 4) as sim:
        sim.reset(dev(x), dev(u), TS)
        sim.set_pressures(p)
        sim.integrate(0.0, TS)                    # row 3 fails and keeps its status
        sim.set_offset(dev(off))
        sim.set_input(dev(np.zeros((4, 4))))      # the torques are not delayed: row 2's plant input has the NaN
        before = snapshot(sim)
        x_in, u_in, _, sst = before[:4]
        assert sst.tolist() == [0, 0, 0, 3], sst
        assert np.isnan(u_in[2, 0]) and np.isfinite(np.delete(u_in[:3].ravel(), 2 * u.shape[1])).all()
        sel, other = sim.gains(GC.ALL, GC.ALL), sim.gains((0, 1), (0, 2))
        assert_untouched(before, snapshot(sim))
    for got, (outs, ins), second in ((sel, (GC.ALL, GC.ALL), cmpc.CMPC_EQ_DEADZONE), (other, ((0, 1), (0, 2)), OK)):
        host = cmpc.plant_gains(plant, p[:3], u_in[:3], x_in[:3], outs, ins)
        assert host.status.tolist() == [OK, second, cmpc.CMPC_EQ_NONFINITE], host.status
        assert_same(got, host, rows=slice(0, 3))
        assert got.status[3] == cmpc.CMPC_EQ_SKIPPED
        assert (bits(got.record[[2, 3]]) == GC.NAN_BITS).all()


def test_a_rank_deficient_selection():
    """Parallel plant, outputs (0, 3) against both inputs of the second
    compressor: they reach those outputs through one flow, G has rank 1, and
    the elimination meets an exactly zero pivot in some scenarios
    (CMPC_GAIN_SINGULAR_G) and a rounding-sized one in the others."""
    p, u, x = GC.cases(0)
    sel = ((0, 3), (2, 3))
    host = cmpc.plant_gains(0, p, u, x, *sel)
    assert (host.status == cmpc.CMPC_GAIN_SINGULAR_G).sum() >= 4 and (host.status == OK).sum() >= 4
    assert_same(device_gains(0, [sel], u, x, pressures=p)[0], host)


def test_device_argument_errors_are_refused():
    from cmpc.sim import PlantSimulator
    x0, u0 = cmpc.plant_default(0)
    with PlantSimulator(0, 1) as sim:
        sim.reset(dev([x0]), dev([u0]), TS)
        assert sim.lib.cmpc_sim_gains_download(sim._h, None, None) < 0
        assert "cmpc_sim_gains first" in sim.lib.cmpc_last_error().decode()
        assert sim.lib.cmpc_sim_gains_record(sim._h) is None and sim.lib.cmpc_sim_gains_status(sim._h) is None
        for args, word in ((((0, 0), (0, 2)), "out_idx repeats"), (((0, 1), (0, 4)), "in_idx"), (((), (0,)), "ny"),
                           (((0,), (0, 1, 2, 3, 0)), "nu")):
            with pytest.raises(RuntimeError, match=word):
                sim.gains(*args)
        res = sim.gains((0, 1))                           # the default inputs: the torques
        assert res.status[0] == OK and res.G.shape == (1, 2, 2) and res.resid[0] > 0
        assert sim.lib.cmpc_sim_gains_record(sim._h) and sim.lib.cmpc_sim_gains_status(sim._h)
        assert sim.lib.cmpc_sim_gains_download(sim._h, None, None) == 0
    assert sim.lib.cmpc_sim_gains(None, 1, None, 1, None) < 0


def test_closed_loop_gains_after_trim_to_outputs():
    """coop-par, B = 6, the three pressure classes twice: ClosedLoop.gains
    after trim_to_outputs returns what PlantSimulator.gains returns at the
    trimmed states, and the host twin agrees bit for bit."""
    from cmpc.configs import reference_setup
    from cmpc.driver import ClosedLoop
    cfg = cmpc.reference_config("par", "coop", p=20)
    arr = cmpc.controller_arrays(cfg, reference_setup("par", "coop"))
    B = 6
    xd, u_def = cmpc.plant_default(cfg.plant)
    pc = EC.class_pressures(B)
    loop = ClosedLoop(cfg, arr, [cmpc.reference_observer_gain(cfg)] * cfg.S, np.tile(xd, (B, 1)),
                      np.tile(u_def, (B, 1)), 3, pressures=pc)
    try:
        loop.trim()
        trim = loop.trim_to_outputs(hold=[0, 1], targets=[4.5, 4.5])
        x0, off = loop.x0.cpu().numpy(), loop.u_offset.cpu().numpy()
        res = loop.gains((0, 1))
        direct = loop.sim.gains((0, 1), (0, 2))
        four = loop.gains(GC.ALL, (0, 2))
        assert np.array_equal(bits(loop.x0.cpu().numpy()), bits(x0))
        assert np.array_equal(bits(loop.u_offset.cpu().numpy()), bits(off))
    finally:
        loop.close()
    assert_same(res, direct)
    host = cmpc.plant_gains(cfg.plant, pc, off, x0, (0, 1), (0, 2))
    assert_same(res, host)
    assert_same(four, cmpc.plant_gains(cfg.plant, pc, off, x0, GC.ALL, (0, 2)))
    assert (res.status == OK).all()
    ok = trim.status == OK
    assert ok.sum() >= 4 and (res.resid[ok] <= 1e-12).all()
    assert res.rga.shape == (B, 2, 2) and res.k_ff.shape == (B, 2, 2) and np.isnan(four.rga).all()
    # the torques hold the two surge distances: the pairing on the diagonal dominates
    assert (res.rga[ok][:, [0, 1], [0, 1]] > 0.5).all()
