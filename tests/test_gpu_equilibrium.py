"""Plant equilibrium on the device (cmpc_sim_equilibrium)
against its host twin (cmpc_plant_equilibrium_host), bit for bit: batches with
full and partial waves, per-scenario pressures set and bound, a scenario
without an equilibrium, a skipped scenario, and ClosedLoop.trim."""
import numpy as np
import pytest

import cmpc
import equilibrium_cases as EC

pytestmark = pytest.mark.gpu
TS = 0.05


@pytest.fixture(autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()
    yield


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def device_solve(plant, u, x0, scalars=(1.0, 1.0), pressures=None, bind=False, **kw):
    """(x, status, iters, resid) of PlantSimulator.equilibrium from x0 at the
    plant input u: the scalars, or `pressures` set (copied) or bound."""
    from cmpc.sim import PlantSimulator
    B = len(x0)
    with PlantSimulator(plant, B, p_in=scalars[0], p_out=scalars[1]) as sim:
        sim.reset(dev(x0), dev(u), TS)
        t = None
        if pressures is not None and bind:
            t = dev(pressures)
            sim.bind_pressures(t.data_ptr())
        elif pressures is not None:
            sim.set_pressures(np.ascontiguousarray(pressures))
        st, it, r = sim.equilibrium(**kw)
        x, _, dt, _ = sim.download()
        assert (dt == TS).all()            # the step sizes stay
    return x, st, it, r


def assert_same(dev_res, host_res, rows=slice(None)):
    for a, b, what in zip(dev_res, host_res, ("x", "status", "iters", "resid")):
        a, b = np.asarray(a)[rows], np.asarray(b)[rows]
        if a.dtype == np.float64:
            a, b = bits(a), bits(b)
        assert np.array_equal(a, b), (what, np.argwhere(a != b)[:4])


@pytest.mark.parametrize("B", [1, 5, 70])
@pytest.mark.parametrize("plant", [0, 1])
def test_device_equals_host_twin(plant, B):
    """The seeded cases of tests/test_equilibrium.py, per-scenario pressures:
    x, status, iters and resid with no tolerance.  B = 70: seventeen full
    waves of four rows and a wave with two rows idle."""
    p, u, x0 = EC.cases(plant, B=B)
    host = cmpc.plant_equilibrium(plant, p, u, x0)
    assert (host[1] == cmpc.CMPC_EQ_OK).all() and host[2].min() >= 3
    assert_same(device_solve(plant, u, x0, pressures=p), host)
    # an iteration budget that stops every scenario short: the statuses agree too
    host1 = cmpc.plant_equilibrium(plant, p, u, x0, max_iter=2)
    assert (host1[1] == cmpc.CMPC_EQ_NO_CONVERGENCE).all()
    assert_same(device_solve(plant, u, x0, pressures=p, max_iter=2), host1)


@pytest.mark.parametrize("plant", [0, 1])
def test_scalar_and_per_scenario_pressures_agree(plant):
    B = 70
    _, u, x0 = EC.cases(plant, B=B)
    pc = EC.class_pressures(B)
    cls = np.arange(B) % len(EC.CLASSES)
    scalar = [device_solve(plant, u, x0, scalars=tuple(c)) for c in EC.CLASSES]
    for bind in (False, True):
        got = device_solve(plant, u, x0, pressures=pc, bind=bind)
        assert (got[1] == cmpc.CMPC_EQ_OK).all()
        for k in range(len(EC.CLASSES)):
            assert_same(got, scalar[k], rows=cls == k)
    # the classes do differ
    assert not np.array_equal(scalar[0][0], scalar[1][0])
    assert_same(scalar[1], cmpc.plant_equilibrium(plant, np.tile(EC.CLASSES[1], (B, 1)), u, x0))


@pytest.mark.parametrize("plant", [0, 1])
def test_a_failing_scenario_is_contained(plant):
    B = 8
    p, u, x0 = EC.cases(plant, B=B)
    x0 = x0 * (1 + 1e-3 * np.random.default_rng(5).uniform(-1, 1, x0.shape))   # distinct starts
    q = p.copy()
    q[3] = EC.NO_EQUILIBRIUM
    p[3] = (1.0, 1.0)
    good = device_solve(plant, u, x0, pressures=p)
    bad = device_solve(plant, u, x0, pressures=q)
    keep = np.arange(B) != 3
    assert bad[1][3] == cmpc.CMPC_EQ_NONFINITE
    assert np.array_equal(bits(bad[0][3]), bits(x0[3]))
    assert (good[1] == cmpc.CMPC_EQ_OK).all()
    assert_same(bad, good, rows=keep)
    assert_same(bad, cmpc.plant_equilibrium(plant, q, u, x0))


def test_a_failed_integration_is_skipped():
    """A scenario whose integration failed (a non-finite state: the
    simulator's sticky status 3, as tests/test_sim.py reaches it) reports
    SKIPPED and keeps its state; its neighbour is solved."""
    from cmpc.sim import PlantSimulator
    plant = 1
    x0, u0 = cmpc.plant_default(plant)
    xn = np.stack([x0, x0])
    xn[1, 2] = np.nan
    with PlantSimulator(plant, 2) as sim:
        sim.reset(dev(xn), dev(np.stack([u0, u0])), TS)
        sim.set_input(dev(np.zeros((2, 4))))
        sim.integrate(0.0, TS)
        x_in, u_in, _, st = sim.download()
        assert st[0] == 0 and st[1] == 3, st
        status, iters, resid = sim.equilibrium()
        x, _, _, st2 = sim.download()
    assert np.array_equal(st2, st)
    assert status[1] == cmpc.CMPC_EQ_SKIPPED and iters[1] == 0 and resid[1] == 0.0
    assert np.array_equal(bits(x[1]), bits(x_in[1]))
    host = cmpc.plant_equilibrium(plant, [[1.0, 1.0]], u_in[:1], x_in[:1])
    assert status[0] == cmpc.CMPC_EQ_OK
    assert_same((x[:1], status[:1], iters[:1], resid[:1]), host)


def test_device_argument_errors_are_refused():
    from cmpc.sim import PlantSimulator
    x0, u0 = cmpc.plant_default(0)
    with PlantSimulator(0, 1) as sim:
        sim.reset(dev([x0]), dev([u0]), TS)
        assert sim.lib.cmpc_sim_equilibrium_download(sim._h, None, None, None) < 0
        assert "cmpc_sim_equilibrium first" in sim.lib.cmpc_last_error().decode()
        assert sim.lib.cmpc_sim_equilibrium_status(sim._h) is None
        for kw, word in (({"max_iter": 65}, "max_iter"), ({"max_iter": -1}, "max_iter"), ({"tol": 0.0}, "tol"),
                         ({"tol": float("nan")}, "tol")):
            with pytest.raises(RuntimeError, match=word):
                sim.equilibrium(**kw)
        assert np.array_equal(sim.download()[0][0], x0)
        st, it, r = sim.equilibrium()
        assert st[0] == cmpc.CMPC_EQ_OK
        assert all(f(sim._h) for f in (sim.lib.cmpc_sim_equilibrium_status, sim.lib.cmpc_sim_equilibrium_iters,
                                       sim.lib.cmpc_sim_equilibrium_resid))
    assert sim.lib.cmpc_sim_equilibrium(None, 20, 1e-12) < 0


# ---- the closed loop ------------------------------------------------------------

def _loop(cfg, arr, x0, u_def, pressures, trim, n=5):
    """(x0 after trim or None, trim's result or None, observer states after
    initialize, y per step (n, B, 4), u per step (n, B, 4), outputs at rest)."""
    import torch
    from cmpc.driver import ClosedLoop
    B = len(x0)
    M = cmpc.reference_observer_gain(cfg)
    loop = ClosedLoop(cfg, arr, [M] * cfg.S, x0, np.tile(u_def, (B, 1)), 3, pressures=pressures)
    try:
        res = x_eq = y_rest = None
        if trim:
            res = loop.trim()
            x_eq = loop.x0.cpu().numpy()
            y_rest = loop.sim.output().cpu().numpy()
        loop.initialize()
        obs = loop.ctx.observer_state()
        ys, us = [], []
        for _ in range(n):
            _, y = loop.step()
            ys.append(y.cpu().numpy().copy())
            us.append(loop.u_ctrl.cpu().numpy().copy())
        assert loop.plant_failures()[0] == 0
    finally:
        loop.close()
    torch.cuda.synchronize()
    return x_eq, res, obs, np.stack(ys), np.stack(us), y_rest


def test_closed_loop_starts_at_rest():
    """coop-par, p = 20, K = 3, B = 6: the three pressure classes twice."""
    from cmpc.configs import reference_setup
    cfg = cmpc.reference_config("par", "coop", p=20)
    arr = cmpc.controller_arrays(cfg, reference_setup("par", "coop"))
    B = 6
    xd, u_def = cmpc.plant_default(cfg.plant)
    x0 = np.tile(xd, (B, 1))
    pc = EC.class_pressures(B)
    host = cmpc.plant_equilibrium(cfg.plant, pc, np.tile(u_def, (B, 1)), x0)
    assert (host[1] == cmpc.CMPC_EQ_OK).all()

    x_eq, res, obs, ys, us, y_rest = _loop(cfg, arr, x0, u_def, pc, trim=True)
    assert_same((x_eq, *res), host)
    ns = cfg.ns
    for q in range(B * cfg.S):     # every observer starts at its scenario's equilibrium
        assert np.array_equal(bits(obs[q, :ns]), bits(x_eq[q // cfg.S]))
    y_host = np.stack([cmpc.plant_output(cfg.plant, x) for x in x_eq])
    assert np.array_equal(bits(ys[0]), bits(y_host))
    assert np.array_equal(bits(y_rest), bits(y_host))

    # scenario 0 of the batch is a B = 1 loop trimmed on its own
    x1, res1, _, ys1, us1, _ = _loop(cfg, arr, x0[:1], u_def, pc[:1], trim=True)
    assert np.array_equal(bits(x1[0]), bits(x_eq[0]))
    assert np.array_equal(bits(ys1[:, 0]), bits(ys[:, 0])) and np.array_equal(bits(us1[:, 0]), bits(us[:, 0]))

    # without trim the loop is what it was: it starts at the x0 given (y(x0)
    # in its first record), differs from the trimmed run, and repeats itself
    _, _, obs_u, ys_u, us_u, _ = _loop(cfg, arr, x0, u_def, pc, trim=False)
    _, _, _, ys_v, us_v, _ = _loop(cfg, arr, x0, u_def, pc, trim=False)
    assert np.array_equal(bits(obs_u[:, :ns]), bits(np.repeat(x0, cfg.S, axis=0)))
    assert np.array_equal(bits(ys_u[0]), bits(np.tile(cmpc.plant_output(cfg.plant, xd), (B, 1))))
    assert np.array_equal(bits(ys_v), bits(ys_u)) and np.array_equal(bits(us_v), bits(us_u))
    assert not np.array_equal(bits(ys_u), bits(ys))
