"""Eigenvalues and plant modes on the device (cmpc_eig_device, cmpc_sim_modes,
DESIGN.md §3.20) against their host twins (cmpc_eig_host,
cmpc_plant_modes_host), bit for bit: batches with full and partial waves,
pressures scalar, set and bound, rows of one wave that finish at different
iteration counts, a skipped scenario, and ClosedLoop.modes."""
import numpy as np
import pytest

import cmpc
import equilibrium_cases as EC
import modes_cases as MC

pytestmark = pytest.mark.gpu
TS = 0.05
bits = MC.bits


@pytest.fixture(autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()
    yield


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def device_modes(plant, u, x, scalars=(1.0, 1.0), pressures=None, bind=False, **kw):
    """(w, summary, status, iters) of PlantSimulator.modes at the states x and
    the plant input u: the scalars, or `pressures` set (copied) or bound."""
    from cmpc.sim import PlantSimulator
    B = len(x)
    with PlantSimulator(plant, B, p_in=scalars[0], p_out=scalars[1]) as sim:
        sim.reset(dev(x), dev(u), TS)
        t = None
        if pressures is not None and bind:
            t = dev(pressures)
            sim.bind_pressures(t.data_ptr())
        elif pressures is not None:
            sim.set_pressures(np.ascontiguousarray(pressures))
        out = sim.modes(**kw)
        x_after, _, dt, st = sim.download()
        assert np.array_equal(bits(x_after), bits(x)) and (dt == TS).all() and (st == 0).all()
    return out


def assert_same(a, b, rows=slice(None)):
    """(w, summary, status, iters) twice, with no tolerance."""
    for p, q, what in zip(a, b, ("w", "summary", "status", "iters")):
        p, q = np.asarray(p)[rows], np.asarray(q)[rows]
        if p.dtype == np.complex128:
            p, q = np.stack([bits(p.real), bits(p.imag)]), np.stack([bits(q.real), bits(q.imag)])
        elif p.dtype == np.float64:
            p, q = bits(p), bits(q)
        assert np.array_equal(p, q), (what, np.argwhere(p != q)[:4])


@pytest.mark.parametrize("B", [1, 5, 70])
@pytest.mark.parametrize("plant", [0, 1])
def test_device_equals_host_twin(plant, B):
    """The seeded cases at their equilibria and at cmpc_plant_default (no
    equilibrium, still a Jacobian), per-scenario pressures: w, summary, status
    and iters with no tolerance; x unchanged.  B = 70: seventeen full waves of
    four rows and a wave with two rows idle."""
    p, u, x0 = EC.cases(plant, B=B)
    x = cmpc.plant_equilibrium(plant, p, u, x0)[0]
    for states in (x, x0):
        host = cmpc.plant_modes(plant, p, u, states)
        assert (host[2] == cmpc.CMPC_EIG_OK).all() and host[3].min() >= 4
        assert_same(device_modes(plant, u, states, pressures=p), host)
    # a budget that stops the slowest scenarios short: the statuses agree too
    cap = int(host[3].max()) - 1
    host1 = cmpc.plant_modes(plant, p, u, x0, max_iter=cap)
    assert (host1[2] == cmpc.CMPC_EIG_NO_CONVERGENCE).any() and (host1[3] <= cap).all()
    assert_same(device_modes(plant, u, x0, pressures=p, max_iter=cap), host1)


@pytest.mark.parametrize("plant", [0, 1])
def test_scalar_set_and_bound_pressures_agree(plant):
    B = 70
    _, u, x0 = EC.cases(plant, B=B)
    pc = EC.class_pressures(B)
    cls = np.arange(B) % len(EC.CLASSES)
    scalar = [device_modes(plant, u, x0, scalars=tuple(c)) for c in EC.CLASSES]
    for bind in (False, True):
        got = device_modes(plant, u, x0, pressures=pc, bind=bind)
        assert (got[2] == cmpc.CMPC_EIG_OK).all()
        for k in range(len(EC.CLASSES)):
            assert_same(got, scalar[k], rows=cls == k)
    assert not np.array_equal(scalar[0][0], scalar[1][0])      # the classes do differ
    assert_same(scalar[1], cmpc.plant_modes(plant, np.tile(EC.CLASSES[1], (B, 1)), u, x0))


def eig_device(A, **kw):
    """(wr, wi, status, iters) of cmpc.eig_batch_device as host arrays."""
    import torch
    out = cmpc.eig_batch_device(dev(A), **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("n", [10, 11])
def test_eig_device_equals_host_twin(n):
    """Nine matrices: the rows of the first wave finish after 0 (all zero), 0
    (a NaN entry), many (the n-cycle) and some twenty (Gaussian) sweeps; the
    last wave has three rows idle."""
    H = MC.hard_matrices(n)
    bad = MC.gaussian(n).T.copy()
    bad[n - 1, 0] = np.nan
    A = np.stack([np.zeros((n, n)), bad, MC.cycle(n), H["gaussian"], H["scaled"], H["blocks"], H["perm4"],
                  H["jordan_rotated"], H["triangular"]])
    w, st, it = cmpc.eig_batch(A)
    print("host iters", it, "status", st)
    assert len(set(it[:4])) >= 3 and len(set(it[4:8])) >= 3 and it.max() > 20
    assert list(st) == [0, cmpc.CMPC_EIG_NONFINITE] + [0] * 7
    got = eig_device(A)
    for a, b in zip(got, (w.real, w.imag, st, it)):
        assert np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b)
    # a cap of three sweeps: OK and NO_CONVERGENCE side by side
    w3, st3, it3 = cmpc.eig_batch(A, max_iter=3)
    assert (st3 == cmpc.CMPC_EIG_OK).sum() >= 3 and (st3 == cmpc.CMPC_EIG_NO_CONVERGENCE).sum() >= 3
    assert (it3 <= 3).all()
    got = eig_device(A, max_iter=3)
    for a, b in zip(got, (w3.real, w3.imag, st3, it3)):
        assert np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b)
    import torch
    with pytest.raises(ValueError):
        cmpc.eig_batch_device(torch.zeros(2, 9, 9, dtype=torch.float64, device="cuda"))
    with pytest.raises(RuntimeError, match="max_iter"):
        cmpc.eig_batch_device(dev(A), max_iter=361)


def test_a_failed_integration_is_skipped():
    """A scenario whose integration failed (a non-finite state: the
    simulator's sticky status 3, as tests/test_gpu_equilibrium.py reaches it)
    reports SKIPPED with NaN results; its neighbours equal the run without it."""
    from cmpc.sim import PlantSimulator
    plant = 1
    x0, u0 = cmpc.plant_default(plant)
    xn = np.stack([x0, x0, x0 * 1.001])
    xn[1, 2] = np.nan
    with PlantSimulator(plant, 3) as sim:
        assert sim.lib.cmpc_sim_modes_download(sim._h, None, None, None, None, None) < 0
        assert "cmpc_sim_modes first" in sim.lib.cmpc_last_error().decode()
        assert sim.lib.cmpc_sim_modes_status(sim._h) is None
        sim.reset(dev(xn), dev(np.stack([u0] * 3)), TS)
        sim.set_input(dev(np.zeros((3, 4))))
        sim.integrate(0.0, TS)
        x_in, u_in, _, st = sim.download()
        assert list(st) == [0, 3, 0], st
        for kw in ({"max_iter": 0}, {"max_iter": 361}):
            with pytest.raises(RuntimeError, match="max_iter"):
                sim.modes(**kw)
        w, sm, status, iters = sim.modes()
        x_out, _, _, st2 = sim.download()
        assert all(f(sim._h) for f in (sim.lib.cmpc_sim_modes_wr, sim.lib.cmpc_sim_modes_wi,
                                       sim.lib.cmpc_sim_modes_summary, sim.lib.cmpc_sim_modes_status,
                                       sim.lib.cmpc_sim_modes_iters))
    assert np.array_equal(st2, st) and np.array_equal(bits(x_out), bits(x_in))
    assert status[1] == cmpc.CMPC_EIG_SKIPPED and iters[1] == 0
    assert (bits(w[1].real) == MC.NAN_BITS).all() and (bits(w[1].imag) == MC.NAN_BITS).all()
    assert (bits(sm[1]) == MC.NAN_BITS).all()
    keep = [0, 2]
    host = cmpc.plant_modes(plant, np.ones((2, 2)), u_in[keep], x_in[keep])
    assert (host[2] == cmpc.CMPC_EIG_OK).all()
    assert_same((w[keep], sm[keep], status[keep], iters[keep]), host)


def _loop(cfg, arr, x0, u_def, pressures, modes, n=4):
    """(the modes after trim or None, x0 after trim, y per step, u per step)."""
    import torch
    from cmpc.driver import ClosedLoop
    B = len(x0)
    M = cmpc.reference_observer_gain(cfg)
    loop = ClosedLoop(cfg, arr, [M] * cfg.S, x0, np.tile(u_def, (B, 1)), 3, pressures=pressures)
    try:
        res = loop.trim()
        assert (res[0] == cmpc.CMPC_EQ_OK).all()
        md = loop.modes() if modes else None
        x_eq = loop.x0.cpu().numpy()
        loop.initialize()
        md2 = loop.modes() if modes else None
        ys, us = [], []
        for _ in range(n):
            _, y = loop.step()
            ys.append(y.cpu().numpy().copy())
            us.append(loop.u_ctrl.cpu().numpy().copy())
        assert loop.plant_failures()[0] == 0
    finally:
        loop.close()
    torch.cuda.synchronize()
    return md, md2, x_eq, np.stack(ys), np.stack(us)


def test_closed_loop_modes():
    """coop-par, p = 20, K = 3, B = 6, the three pressure classes twice: the
    record after trim equals the host's analysis at the loop's x0, the same
    after initialize, and the loop's records are those of a loop that never
    asked."""
    from cmpc.configs import reference_setup
    cfg = cmpc.reference_config("par", "coop", p=20)
    arr = cmpc.controller_arrays(cfg, reference_setup("par", "coop"))
    B = 6
    xd, u_def = cmpc.plant_default(cfg.plant)
    x0 = np.tile(xd, (B, 1))
    pc = EC.class_pressures(B)
    md, md2, x_eq, ys, us = _loop(cfg, arr, x0, u_def, pc, modes=True)
    w, sm, st, _ = cmpc.plant_modes(cfg.plant, pc, np.tile(u_def, (B, 1)), x_eq)
    assert (st == cmpc.CMPC_EIG_OK).all()
    for rec in (md, md2):
        assert rec._fields == ("abscissa", "n_unstable", "zeta_min", "omega_d", "omega_n", "re_min", "w", "status")
        got = np.stack([rec.abscissa, rec.n_unstable, rec.zeta_min, rec.omega_d, rec.omega_n, rec.re_min], axis=1)
        assert np.array_equal(bits(got), bits(sm))
        assert np.array_equal(bits(rec.w.real), bits(w.real)) and np.array_equal(bits(rec.w.imag), bits(w.imag))
        assert np.array_equal(rec.status, st)
    assert (md.n_unstable == 0).all() and not np.array_equal(md.zeta_min[0], md.zeta_min[1])
    _, _, x_eq2, ys2, us2 = _loop(cfg, arr, x0, u_def, pc, modes=False)
    assert np.array_equal(bits(x_eq2), bits(x_eq))
    assert np.array_equal(bits(ys2), bits(ys)) and np.array_equal(bits(us2), bits(us))
