"""The plant frequency responses on the device (cmpc_sim_freq)
against their host twin (cmpc_plant_freq_host), bit for bit on the record, the
summary and the status: batches of one row, a partial wave and several
workgroups with a ragged tail, both plants, selections 1 x 1, 2 x 2, 4 x 4 and
4 x 2, one frequency and the 12-point grid, pressures as scalars, set and bound,
one wave with four different statuses, result buffers that grow between calls,
the simulator state the call must leave alone, and ClosedLoop.freq_response."""
import numpy as np
import pytest

import cmpc
import equilibrium_cases as EC
import freq_cases as FC
import gains_cases as GC

pytestmark = pytest.mark.gpu
TS = 0.05
OK = cmpc.CMPC_EQ_OK
bits = GC.bits
ONE = np.array([31.6])
LISTS = (ONE, FC.GRID)


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


def device_freq(plant, calls, u, x, scalars=(1.0, 1.0), pressures=None, bind=False):
    """PlantSimulator.freq_response for every (omega, outputs, inputs) of
    `calls` on one simulator at the state x and the plant input u: the scalars,
    or `pressures` set (copied) or bound.  x, u_full, step sizes, status, offset
    and delay line must stay bit for bit over every call."""
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
        out = []
        for call in calls:
            out.append(sim.freq_response(*call))
            assert_untouched(before, snapshot(sim))
        assert np.array_equal(bits(before[0]), bits(x)) and np.array_equal(bits(before[1]), bits(u))
    return out


def assert_same(got, want, rows=slice(None)):
    assert np.array_equal(got.status[rows], want.status[rows]), (got.status, want.status)
    for name in ("record", "summary"):
        a, b = bits(getattr(got, name)[rows]), bits(getattr(want, name)[rows])
        assert np.array_equal(a, b), (name, np.argwhere(a != b)[:6])


def every_call():
    return [(w, *sel) for sel in GC.SELECTIONS for w in LISTS]


@pytest.mark.parametrize("B", [1, 5, 70])
@pytest.mark.parametrize("plant", [0, 1])
def test_device_equals_host_twin(plant, B):
    """Per-scenario pressures, every selection shape, one frequency and the
    grid: record, summary and status with no tolerance.  B = 70: seventeen full
    waves of four rows and a wave with two rows idle."""
    p, u, x = GC.cases(plant, B=B)
    calls = every_call()
    got = device_freq(plant, calls, u, x, pressures=p)
    for (w, outs, ins), g in zip(calls, got):
        host = cmpc.plant_freq_response(plant, p, u, x, w, outs, ins)
        assert (host.status == OK).all() and not np.isnan(host.G.real).any()
        assert_same(g, host)
        assert g.G.shape == (B, len(w), len(outs), len(ins)) and g.Gp.shape == (B, len(w), len(outs), 2)


@pytest.mark.parametrize("plant", [0, 1])
def test_scalar_set_and_bound_pressures_agree(plant):
    B = 7
    _, u, _ = GC.cases(plant, B=B)
    pc = EC.class_pressures(B)
    x, st, _, _ = cmpc.plant_equilibrium(plant, pc, u, GC.cases(plant, B=B)[2])
    assert (st == OK).all()
    calls = every_call()
    cls = np.arange(B) % len(EC.CLASSES)
    scalar = [device_freq(plant, calls, u, x, scalars=tuple(c)) for c in EC.CLASSES]
    host = [cmpc.plant_freq_response(plant, pc, u, x, *c) for c in calls]
    for bind in (False, True):
        got = device_freq(plant, calls, u, x, pressures=pc, bind=bind)
        for j in range(len(calls)):
            assert_same(got[j], host[j])
            for k in range(len(EC.CLASSES)):
                assert_same(got[j], scalar[k][j], rows=cls == k)
    assert not np.array_equal(bits(scalar[0][0].record), bits(scalar[1][0].record))     # the classes do differ


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
        sel, other = sim.freq_response(FC.GRID, GC.ALL, GC.ALL), sim.freq_response(FC.GRID, (0, 1), (0, 2))
        assert_untouched(before, snapshot(sim))
    for got, (outs, ins), second in ((sel, (GC.ALL, GC.ALL), cmpc.CMPC_EQ_DEADZONE), (other, ((0, 1), (0, 2)), OK)):
        host = cmpc.plant_freq_response(plant, p[:3], u_in[:3], x_in[:3], FC.GRID, outs, ins)
        assert host.status.tolist() == [OK, second, cmpc.CMPC_EQ_NONFINITE], host.status
        assert_same(got, host, rows=slice(0, 3))
        assert got.status[3] == cmpc.CMPC_EQ_SKIPPED
        assert (bits(got.record[[2, 3]]) == GC.NAN_BITS).all() and (bits(got.summary[[2, 3]]) == GC.NAN_BITS).all()


def test_two_calls_on_one_simulator_grow_the_buffers():
    """nw = 3, then nw = 12, then nw = 3 again on one simulator: the record
    buffer grows for the second call, which equals the host twin, and the third
    call equals the first."""
    from cmpc.sim import PlantSimulator
    plant, B = 1, 6
    p, u, x = GC.cases(plant, B=B)
    three = FC.GRID[[4, 1, 8]]
    with PlantSimulator(plant, B) as sim:
        sim.reset(dev(x), dev(u), TS)
        sim.set_pressures(np.ascontiguousarray(p))
        before = snapshot(sim)
        first = sim.freq_response(three, GC.ALL, GC.ALL)
        small = sim.lib.cmpc_sim_freq_record(sim._h)
        second = sim.freq_response(FC.GRID, GC.ALL, GC.ALL)
        large = sim.lib.cmpc_sim_freq_record(sim._h)
        third = sim.freq_response(three, GC.ALL, GC.ALL)
        assert small and large and sim.lib.cmpc_sim_freq_record(sim._h) == large     # (not shrunk again)
        assert_untouched(before, snapshot(sim))
    assert first.record.shape == (B, 3, cmpc.CMPC_FREQ_LEN) and second.record.shape == (B, 12, cmpc.CMPC_FREQ_LEN)
    assert_same(first, cmpc.plant_freq_response(plant, p, u, x, three, GC.ALL, GC.ALL))
    assert_same(second, cmpc.plant_freq_response(plant, p, u, x, FC.GRID, GC.ALL, GC.ALL))
    assert_same(third, first)
    # the list's order is the record's: grid points 4, 1 and 8
    assert np.array_equal(bits(first.record), bits(second.record[:, [4, 1, 8]]))


def test_device_argument_errors_are_refused():
    from cmpc.sim import PlantSimulator
    x0, u0 = cmpc.plant_default(0)
    with PlantSimulator(0, 1) as sim:
        sim.reset(dev([x0]), dev([u0]), TS)
        assert sim.lib.cmpc_sim_freq_download(sim._h, None, None, None) < 0
        assert "cmpc_sim_freq first" in sim.lib.cmpc_last_error().decode()
        assert (sim.lib.cmpc_sim_freq_record(sim._h) is None and sim.lib.cmpc_sim_freq_summary(sim._h) is None
                and sim.lib.cmpc_sim_freq_status(sim._h) is None)
        for args, word in (((ONE, (0, 0), (0, 2)), "out_idx repeats"), ((ONE, (0, 1), (0, 4)), "in_idx"),
                           ((ONE, (), (0,)), "ny"), ((ONE, (0,), (0, 1, 2, 3, 0)), "nu"), (([], (0,), (0,)), "nw"),
                           ((np.zeros(65), (0,), (0,)), "nw"), (([1.0, -1.0], (0,), (0,)), r"omega\[1\]"),
                           (([np.nan], (0,), (0,)), r"omega\[0\]"), (([np.inf], (0,), (0,)), r"omega\[0\]")):
            with pytest.raises(RuntimeError, match=word):
                sim.freq_response(*args)
        assert sim.lib.cmpc_sim_freq_record(sim._h) is None                  # a refusal allocates nothing
        res = sim.freq_response(ONE, (0, 1))                                 # the default inputs: the torques
        assert res.status[0] == OK and res.G.shape == (1, 1, 2, 2) and res.resid[0] > 0
        assert (sim.lib.cmpc_sim_freq_record(sim._h) and sim.lib.cmpc_sim_freq_summary(sim._h)
                and sim.lib.cmpc_sim_freq_status(sim._h))
        assert sim.lib.cmpc_sim_freq_download(sim._h, None, None, None) == 0
    assert sim.lib.cmpc_sim_freq(None, 1, None, 1, None, 1, None) < 0


def test_closed_loop_freq_response_after_trim_to_outputs():
    """coop-par, B = 6, the three pressure classes twice:
    ClosedLoop.freq_response after trim_to_outputs returns what
    PlantSimulator.freq_response returns at the trimmed states, and the host
    twin agrees bit for bit."""
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
        res = loop.freq_response(FC.GRID, (0, 1))
        direct = loop.sim.freq_response(FC.GRID, (0, 1), (0, 2))
        four = loop.freq_response(ONE, GC.ALL, (0, 2))
        assert np.array_equal(bits(loop.x0.cpu().numpy()), bits(x0))
        assert np.array_equal(bits(loop.u_offset.cpu().numpy()), bits(off))
    finally:
        loop.close()
    assert_same(res, direct)
    assert_same(res, cmpc.plant_freq_response(cfg.plant, pc, off, x0, FC.GRID, (0, 1), (0, 2)))
    assert_same(four, cmpc.plant_freq_response(cfg.plant, pc, off, x0, ONE, GC.ALL, (0, 2)))
    assert (res.status == OK).all()
    ok = trim.status == OK
    assert ok.sum() >= 4 and (res.resid[ok] <= 1e-12).all()
    assert res.G.shape == (B, 12, 2, 2) and res.peak.shape == (B, 2, 2) and res.peak_p_omega.shape == (B, 2, 2)
    # every response rolls off: three decades past the poles nothing is left of the peak
    assert (np.abs(res.G[:, -1]) < 1e-2 * res.peak).all()
