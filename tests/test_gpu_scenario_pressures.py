"""Per-scenario boundary pressures (include/cmpc.h) on the
GPU: the plant simulation, the record producer in both of its modes and
through every form of the control step, the shared build on such records, and
the closed loop with the plant's and the model's pressures apart.

References: the oracle per scenario (PlantSim, or_lin_record through
cmpc.plant_lin_record's own CPU check, pressure_loop.PressureClosedLoop) by
the tolerances of the tests that cover the default pressures, and the
scalar-argument launches that existed before the feature, bit for bit:
scenarios are dealt three pressure classes round-robin, and scenario b must
equal scenario b of a run with its class's scalars.  Marked gpu; runs on an
MI355X."""
import numpy as np
import pytest

import _oracle as O
import cmpc
import golden_cases as GC
from cmpc._abi import CmpcDims
from cmpc.configs import reference_setup
from test_gpu_producer import CASES, operating_points
from test_scenario_pressures import scenario_pressures

pytestmark = pytest.mark.gpu

TS = 0.05
# three classes within 1 +- 0.05, p_in != p_out, none at the default
CLASSES = np.array([[0.96, 1.03], [1.04, 0.97], [1.0125, 0.9875]])


@pytest.fixture(autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def class_pressures(B):
    return CLASSES[np.arange(B) % 3].copy()


# ---- 1. simulation --------------------------------------------------------------------

def _sim_inputs(plant, B, steps):
    rng = np.random.default_rng(3 + plant)
    x0, u0 = O.plant_default(plant)
    xs = x0[None, :] * (1 + 0.002 * rng.normal(size=(B, len(x0))))
    us = np.tile(u0, (B, 1))
    ucs = rng.uniform(-0.01, 0.01, (steps, B, 4))
    ucs[:, :, [1, 3]] = np.abs(ucs[:, :, [1, 3]])
    return xs, us, ucs


def _sim_run(sim, xs, us, ucs, between=None):
    """reset + one interval per row of ucs; (x, dt, status) after the last"""
    sim.reset(dev(xs), dev(us), TS)
    for k in range(len(ucs)):
        if between:
            between(k)
        sim.set_input(dev(ucs[k]))
        sim.integrate(k * TS, k * TS + TS)
    x, _, dt, st = sim.download()
    return x, dt, st


@pytest.mark.parametrize("plant", [0, 1])
def test_gpu_sim_per_scenario_pressures_match_oracle(plant):
    """B = 70 (a full wave and a partial one), 30 intervals, every scenario its
    own pair: states and carried step sizes against one PlantSim per scenario
    by test_gpu_sim_matches_oracle's tolerances; no failure."""
    from cmpc.sim import PlantSimulator
    B, steps = 70, 30
    xs, us, ucs = _sim_inputs(plant, B, steps)
    press = scenario_pressures(B, seed=plant)
    sims = [O.PlantSim(plant, xs[b], us[b], p_in=press[b, 0], p_out=press[b, 1]) for b in range(B)]
    for k in range(steps):
        for b in range(B):
            sims[b].set_input(ucs[k, b])
            sims[b].integrate(k * TS, k * TS + TS)
    with PlantSimulator(plant, B) as sim:
        assert np.array_equal(sim.get_pressures(), np.ones((B, 2)))
        sim.set_pressures(press)
        assert np.array_equal(sim.get_pressures(), press)
        x, dt, st = _sim_run(sim, xs, us, ucs)
        with pytest.raises(RuntimeError, match="scenario 69: pressures must be finite and positive"):
            bad = press.copy()
            bad[69, 1] = 0.0
            sim.set_pressures(bad)
        with pytest.raises(ValueError, match="pressures must be"):
            sim.set_pressures(press[:-1])
        assert np.array_equal(sim.get_pressures(), press)   # a refused call changes nothing
    assert not st.any(), st
    np.testing.assert_allclose(x, np.stack([s.x for s in sims]), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(dt, np.array([s.dt[0] for s in sims]), rtol=1e-10)
    # the pressures matter at these tolerances: the default run is elsewhere
    with PlantSimulator(plant, B) as sim:
        x1, _, _ = _sim_run(sim, xs, us, ucs)
    assert (np.abs(x - x1).max(axis=1) > 1e-6 * np.abs(x1).max(axis=1)).all()


@pytest.mark.parametrize("plant", [0, 1])
def test_gpu_sim_classes_equal_scalar_runs_bitwise(plant):
    """Three classes dealt round-robin: scenario b's x, dt and status equal, bit
    for bit, scenario b of a run with its class's scalars through
    cmpc_sim_create (the kernel that existed before); the device-tensor setter
    and the bound array give the same; after set_pressures(None) a reset run
    equals the scalar run of the simulator's own scalars."""
    from cmpc.sim import PlantSimulator
    B, steps = 70, 30
    xs, us, ucs = _sim_inputs(plant, B, steps)
    press = class_pressures(B)
    scalar = []
    for c in range(3):
        with PlantSimulator(plant, B, p_in=CLASSES[c, 0], p_out=CLASSES[c, 1]) as sim:
            scalar.append(_sim_run(sim, xs, us, ucs))
            if c == 0:
                own = scalar[0]
                t = dev(press)
                sim.set_pressures(press)
                runs = [_sim_run(sim, xs, us, ucs)]
                sim.set_pressures(None)
                sim.set_pressures(t)          # device tensor, copied
                t.fill_(7.0)                  # ... so this changes nothing
                runs.append(_sim_run(sim, xs, us, ucs))
                t.copy_(dev(press))
                sim.bind_pressures(t.data_ptr())
                runs.append(_sim_run(sim, xs, us, ucs))
                sim.set_pressures(None)
                assert np.array_equal(sim.get_pressures(), np.tile(CLASSES[0], (B, 1)))
                cleared = _sim_run(sim, xs, us, ucs)
    for a, b in zip(cleared, own):
        assert np.array_equal(a, b)
    cls = np.arange(B) % 3
    for x, dt, st in runs:
        assert not st.any()
        for c in range(3):
            sx, sdt, sst = scalar[c]
            assert np.array_equal(x[cls == c], sx[cls == c]), c
            assert np.array_equal(dt[cls == c], sdt[cls == c]), c
            assert np.array_equal(st[cls == c], sst[cls == c]), c
    # (and the classes differ from each other, so the equalities above select)
    assert not np.array_equal(scalar[0][0], scalar[1][0]) and not np.array_equal(scalar[1][0], scalar[2][0])


def test_gpu_sim_bound_pressures_rewritten_between_intervals():
    """A bound array is read by each integrate: rewritten after the first of
    two intervals, the second runs at the new pressures (the oracle with the
    same change, by the tolerances above), and differs from the run that was
    not rewritten."""
    from cmpc.sim import PlantSimulator
    plant, B = 0, 70
    xs, us, ucs = _sim_inputs(plant, B, 2)
    p0, p1 = scenario_pressures(B, seed=5), scenario_pressures(B, seed=6)
    sims = [O.PlantSim(plant, xs[b], us[b], p_in=p0[b, 0], p_out=p0[b, 1]) for b in range(B)]
    for k in range(2):
        for b in range(B):
            sims[b].p_in, sims[b].p_out = (p0 if k == 0 else p1)[b]
            sims[b].set_input(ucs[k, b])
            sims[b].integrate(k * TS, k * TS + TS)
    t = dev(p0)
    with PlantSimulator(plant, B) as sim:
        sim.bind_pressures(t.data_ptr())
        kept = _sim_run(sim, xs, us, ucs)
        t.copy_(dev(p0))
        x, dt, st = _sim_run(sim, xs, us, ucs, between=lambda k: t.copy_(dev(p1)) if k == 1 else None)
        assert np.array_equal(sim.get_pressures(), p1)
    assert not st.any()
    np.testing.assert_allclose(x, np.stack([s.x for s in sims]), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(dt, np.array([s.dt[0] for s in sims]), rtol=1e-10)
    assert (np.abs(x - kept[0]).max(axis=1) > 1e-9).all()


# ---- 2. producer ----------------------------------------------------------------------

@pytest.mark.parametrize("plant,ctype", CASES)
def test_gpu_producer_per_scenario_pressures(plant, ctype):
    """produce_lin at p = 50, B = 18 with every scenario its own pair against
    cmpc.plant_lin_record(p_in=, p_out=) per slot by
    test_gpu_producer_matches_host's rule; the scalar arguments are ignored
    while pressures are in force and used again after a clear; classes dealt
    round-robin equal the scalar-argument launches bit for bit, set or bound,
    and a bound array rewritten between two launches takes effect."""
    import torch
    cfg = cmpc.reference_config(plant, ctype, p=50)
    B = 18
    x, u, y = operating_points(cfg, B, seed=9)
    dims = CmpcDims.from_config(cfg, B)
    L = cmpc.layout_of(dims)
    dx = np.random.default_rng(4).normal(0, 1e-3, (B * cfg.S, L.naug))
    tx, tu, ty, tdx = dev(x), dev(u), dev(y), dev(dx)
    press, cpress = scenario_pressures(B, seed=1), class_pressures(B)
    with cmpc.Context(cfg, B, device=0) as ctx:
        produce = lambda **kw: (ctx.produce_lin(tx.data_ptr(), tu.data_ptr(), ty.data_ptr(), tdx.data_ptr(), **kw),
                                ctx.download_lin())[1]
        with pytest.raises(RuntimeError, match="no per-scenario pressures are set"):
            ctx.get_scenario_pressures()
        default = produce()
        scalar = [produce(p_in=c[0], p_out=c[1]) for c in CLASSES]
        ctx.set_scenario_pressures(press)
        assert np.array_equal(ctx.get_scenario_pressures(), press)
        got = produce()
        assert np.array_equal(got, produce(p_in=0.5, p_out=2.0))      # scalars ignored
        with pytest.raises(RuntimeError, match="scenario 3: pressures must be finite and positive"):
            bad = press.copy()
            bad[3, 0] = np.nan
            ctx.set_scenario_pressures(bad)
        with pytest.raises(ValueError, match="pressures must be"):
            ctx.set_scenario_pressures(press.T)
        ctx.set_scenario_pressures(cpress)
        by_class = [produce()]
        t = dev(cpress)
        ctx.bind_scenario_pressures(t.data_ptr())
        by_class.append(produce())
        t.copy_(dev(press))                                           # rewritten between launches
        torch.cuda.synchronize()                                      # (the context has its own stream)
        assert np.array_equal(produce(), got)
        assert np.array_equal(ctx.get_scenario_pressures(), press)
        ctx.bind_scenario_pressures(0)
        assert np.array_equal(produce(), default)                     # cleared: the scalars again
        assert np.array_equal(produce(p_in=CLASSES[1, 0], p_out=CLASSES[1, 1]), scalar[1])
    exact = 0
    for b in range(B):
        for s in range(cfg.S):
            q = b * cfg.S + s
            ref = np.zeros(L.rec_len)
            cmpc.plant_lin_record(cfg, dims, s, x[b], u[b], p_in=press[b, 0], p_out=press[b, 1], out=ref)
            ref[L.off_x:L.off_x + L.naug] = dx[q]
            ref[L.off_y:L.off_y + cfg.ny] = y[b][cfg.out_idx[s]]
            if np.array_equal(got[q], ref):
                exact += 1
            else:
                np.testing.assert_allclose(got[q], ref, rtol=1e-13, atol=1e-300)
            assert not np.array_equal(got[q], default[q])
    assert exact >= 0.5 * B * cfg.S, exact
    for run in by_class:
        for b in range(B):
            rows = slice(b * cfg.S, (b + 1) * cfg.S)
            assert np.array_equal(run[rows], scalar[b % 3][rows]), b
    assert not np.array_equal(scalar[0], scalar[1]) and not np.array_equal(scalar[1], scalar[2])


def _control_run(cfg, arr, B, form, x, u, ys, K, pressures=None, scalars=(1.0, 1.0)):
    """observer_init, then one call per row of ys in the given form; the
    records and observer rows after each call, and the plans of the control
    forms.  pressures: (B, 2) in force from before observer_init (bound for
    the control forms, set for the others), else the scalars."""
    nq = B * cfg.S
    tx, tu = dev(x), dev(u)
    tys = [dev(a) for a in ys]
    out = []
    with cmpc.Context(cfg, B, device=0) as ctx:
        ctx.configure(arr)
        ctx.set_state(np.zeros((nq, cfg.nu_tot)), np.zeros((nq, cfg.nV)), np.zeros(nq, np.uint32))
        for s in range(cfg.S):
            ctx.set_observer(s, cmpc.reference_observer_gain(cfg))
        if form == "three":
            ctx.set_step_variant(cmpc.CMPC_STEP_SPLIT)
        t = None
        if pressures is not None:
            if form == "observe":
                ctx.set_scenario_pressures(pressures)
            else:
                t = dev(pressures)
                ctx.bind_scenario_pressures(t.data_ptr())
        kw = dict(p_in=scalars[0], p_out=scalars[1])
        ctx.observer_init(tx.data_ptr(), tu.data_ptr(), tys[0].data_ptr(), **kw)
        out.append((ctx.download_lin(), ctx.observer_state()))
        if form != "observe":
            ctx.build()
            ctx.init_warmstart()
        for ty in tys[1:]:
            if form == "observe":
                ctx.observe_step(tu.data_ptr(), ty.data_ptr())
                out.append((ctx.download_lin(), ctx.observer_state()))
            else:
                ctx.control_step(tu.data_ptr(), ty.data_ptr(), K)
                assert ctx.last_step_fused() == (form != "three")
                out.append((ctx.download_lin(), ctx.observer_state(), *ctx.download(), *ctx.get_state()))
    return out


@pytest.mark.parametrize("plant,ctype", CASES)
def test_gpu_per_qp_producer_classes_equal_scalar_runs(plant, ctype):
    """The per-QP producer (one linearisation per slot at its observer state):
    observer_init then observe_step at B = 18; control_step at B = 5 (one
    launch, role-split pairs), at a batch between one and four QPs per CU
    (one launch, four slots per workgroup) and at B = 5 forced to the three
    calls.  With classes dealt round-robin every scenario's records, observer
    rows, plans, statuses and state equal, bit for bit, the same scenario's in
    the run with its class's scalars given to observer_init."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cfg = cmpc.reference_config(plant, ctype, p=50)
    arr = cmpc.controller_arrays(cfg, reference_setup(plant, ctype))
    K, S = 2, cfg.S
    B_mid = (300 * cus // 256) // S            # B = 150 for S = 2 at 256 CUs
    for form, B in (("observe", 18), ("control", 5), ("control", B_mid), ("three", 5)):
        if form == "control":                  # the plan says which one-launch form this batch gets
            pl = cmpc.plan(CmpcDims.from_config(cfg, B), cus, K=K)
            assert pl.control_fused
            if B == 5:
                assert pl.control_build_kernel == cmpc.CMPC_BUILD_SPLIT and pl.control_grid == (B * S + 1) // 2
            else:
                assert cus < B * S <= 4 * cus
                assert pl.control_build_kernel == cmpc.CMPC_BUILD_WAVE and pl.control_grid == (B * S + 3) // 4
        x, u, y = operating_points(cfg, B, seed=11)
        rng = np.random.default_rng(12)
        ys = [y] + [y * (1 + 1e-3 * rng.normal(size=y.shape)) for _ in range(2)]
        per = _control_run(cfg, arr, B, form, x, u, ys, K, pressures=class_pressures(B), scalars=(0.5, 2.0))
        scalar = [_control_run(cfg, arr, B, form, x, u, ys, K, scalars=tuple(c)) for c in CLASSES]
        for b in range(B):
            rows = slice(b * S, (b + 1) * S)
            for call, (got, want) in enumerate(zip(per, scalar[b % 3])):
                for i, (a, w) in enumerate(zip(got, want)):
                    assert np.array_equal(a[rows], w[rows], equal_nan=True), (form, B, b, call, i)
        # the classes give different records, so the equalities select
        assert not np.array_equal(scalar[0][1][0], scalar[1][1][0])
        assert not np.array_equal(scalar[1][1][0], scalar[2][1][0])


# ---- 3. shared build ------------------------------------------------------------------

def test_gpu_shared_build_on_per_scenario_pressure_records():
    """par-coop, B = 64, records from the producer with every scenario its own
    pair: both slots of a scenario still linearise one plant, so the shared
    form covers the whole batch and its QPs are the unpaired build's."""
    cfg = cmpc.reference_config("par", "coop", p=50)
    arr = cmpc.controller_arrays(cfg, reference_setup("par", "coop"))
    B = 64
    nq = B * cfg.S
    x, u, y = operating_points(cfg, B, seed=31)
    tx, tu, ty = dev(x), dev(u), dev(y)
    rng = np.random.default_rng(32)
    u_old = rng.uniform(-0.02, 0.02, (nq, cfg.nu_tot))
    qps = {}
    for mode in (cmpc.CMPC_PAIRING_ON, cmpc.CMPC_PAIRING_OFF):
        with cmpc.Context(cfg, B, device=0) as ctx:
            ctx.configure(arr)
            ctx.set_state(u_old, np.zeros((nq, cfg.nV)), np.zeros(nq, np.uint32))
            ctx.set_build_variant(cmpc.CMPC_BUILD_ROWS)
            ctx.set_build_pairing(mode)
            ctx.set_scenario_pressures(scenario_pressures(B, seed=2))
            ctx.produce_lin(tx.data_ptr(), tu.data_ptr(), ty.data_ptr())
            ctx.build()
            assert ctx.last_build_kernel() == cmpc.CMPC_BUILD_ROWS
            shared = ctx.last_build_shared_scenarios()
            assert shared == (B if mode == cmpc.CMPC_PAIRING_ON else -1)
            qps[mode] = [np.ascontiguousarray(a).view(np.uint64).copy() for a in ctx.download_qp()]
            lin = ctx.download_lin()
    for a, b in zip(qps[cmpc.CMPC_PAIRING_ON], qps[cmpc.CMPC_PAIRING_OFF]):
        assert np.array_equal(a, b)
    # the records do differ between scenarios in what the pressures reach
    assert not np.array_equal(lin[0, :cfg.ns * cfg.ns], lin[2, :cfg.ns * cfg.ns])


# ---- 4. closed loop -------------------------------------------------------------------

def _loop_inputs(cfg, B):
    rng = np.random.default_rng(21)
    x0, u_def = cmpc.plant_default(cfg.plant)
    xs = x0[None, :] * (1 + 0.002 * rng.uniform(-1, 1, (B, len(x0))))
    return xs, u_def


def _device_loop(cfg, arr, g, xs, u_def, n, **kw):
    import torch
    from cmpc.driver import ClosedLoop
    B = len(xs)
    M = cmpc.reference_observer_gain(cfg)
    sched = kw.pop("schedule", None)
    loop = ClosedLoop(cfg, arr, [M] * cfg.S, xs, np.tile(u_def, (B, 1)), g["n_iterations"], **kw)
    ub = torch.zeros(n, B, 4, dtype=torch.float64, device="cuda")
    yb = torch.zeros(n, B, 4, dtype=torch.float64, device="cuda")
    try:
        if sched is not None:
            loop.set_pressure_schedule(*sched)
        loop.initialize()
        for k in range(n):
            _, y = loop.step()
            ub[k].copy_(loop.u_ctrl)
            yb[k].copy_(y)
        nfail, st = loop.plant_failures()
    finally:
        loop.close()
    assert nfail == 0, st
    return ub.cpu().numpy(), yb.cpu().numpy()


@pytest.mark.parametrize("variant", ["follow", "mismatch", "schedule"])
@pytest.mark.parametrize("name", ["coop-par", "cent-ser"])
def test_gpu_closed_loop_pressures_match_oracle(name, variant):
    """B = 6 scenarios, each its own pressures, 60 instants (the 40-sample
    input delay has played out) against one pressure_loop.PressureClosedLoop
    per scenario within test_gpu_closed_loop_scenarios_match_oracle's bar
    (rtol 2e-6, atol 1e-10 on u and y per instant); no plant failure.
      follow    the model follows the plant's pressures
      mismatch  the model held at (1, 1)
      schedule  the plant's p_in steps by -0.04 at instant 20, unseen by the
                model, which keeps the pressures of before the step"""
    from pressure_loop import PressureClosedLoop
    cfg, setup, arr, g = GC.case(name)
    B, n = 6, 60
    xs, u_def = _loop_inputs(cfg, B)
    M = [cmpc.reference_observer_gain(cfg)] * cfg.S
    if variant == "schedule":
        # p_in from 0.992 so that the stepped value stays within 1 +- 0.05
        press = np.stack([0.992 + 0.01 * np.arange(B), 0.953 + 0.017 * np.arange(B)], axis=1)
        plant_sched = np.repeat(press[:, None, :], 21, axis=1)
        plant_sched[:, 20, 0] -= 0.04
        u, y = _device_loop(cfg, arr, g, xs, u_def, n, pressures=press, schedule=(plant_sched,))
        mk = lambda b: PressureClosedLoop(cfg, arr, M, g["n_iterations"], press[b], press[b], x0=xs[b],
                                          plant_schedule=plant_sched[b])
    else:
        press = scenario_pressures(B, seed=3)
        model = None if variant == "follow" else np.ones((B, 2))
        u, y = _device_loop(cfg, arr, g, xs, u_def, n, pressures=press, model_pressures=model)
        mk = lambda b: PressureClosedLoop(cfg, arr, M, g["n_iterations"], press[b],
                                          None if model is None else model[b], x0=xs[b])
    assert len(set(press.ravel())) == 2 * B and (np.abs(press - 1) <= 0.05).all()
    for b in range(B):
        ora = mk(b)
        for k in range(n):
            yo = ora.step()
            np.testing.assert_allclose(u[k, b], ora.u_ctrl, rtol=2e-6, atol=1e-10, err_msg=f"u {b} {k}")
            np.testing.assert_allclose(y[k, b], yo, rtol=2e-6, atol=1e-10, err_msg=f"y {b} {k}")


@pytest.mark.parametrize("name", ["coop-par", "cent-ser"])
def test_gpu_closed_loop_default_scenario_is_bit_identical(name):
    """A scenario at (1, 1) among scenarios at other pressures is, bit for
    bit, the same scenario of a ClosedLoop without the feature: plant and
    model, constant, set between steps and scheduled."""
    cfg, setup, arr, g = GC.case(name)
    B, n, at = 6, 60, 3
    xs, u_def = _loop_inputs(cfg, B)
    press = scenario_pressures(B, seed=3)
    press[at] = 1.0
    plain_u, plain_y = _device_loop(cfg, arr, g, xs, u_def, n)
    sched = np.repeat(press[:, None, :], 2, axis=1)
    shuffled = press[[1, 2, 0, at, 5, 4]]        # a mismatch for every scenario but `at`
    for kw in (dict(pressures=press), dict(pressures=press, model_pressures=shuffled),
               dict(schedule=(sched, sched))):
        u, y = _device_loop(cfg, arr, g, xs, u_def, n, **kw)
        assert np.array_equal(u[:, at], plain_u[:, at]) and np.array_equal(y[:, at], plain_y[:, at])
        others = [b for b in range(B) if b != at]
        assert not np.array_equal(y[:, others], plain_y[:, others])


def test_gpu_closed_loop_pressure_arguments():
    """Shape and value errors are ValueErrors; set_pressures between steps
    reaches plant and model; removing a schedule keeps the last rows."""
    from cmpc.driver import ClosedLoop
    cfg, setup, arr, g = GC.case("coop-par")
    B = 3
    xs, u_def = _loop_inputs(cfg, B)
    M = cmpc.reference_observer_gain(cfg)
    mk = lambda **kw: ClosedLoop(cfg, arr, [M] * cfg.S, xs, np.tile(u_def, (B, 1)), g["n_iterations"], **kw)
    for bad in (np.ones((B, 3)), np.ones((B + 1, 2)), np.ones(2 * B)):
        with pytest.raises(ValueError, match=r"must be \(B = 3, 2\)"):
            mk(pressures=bad)
    nan = np.ones((B, 2))
    nan[1, 1] = np.nan
    with pytest.raises(ValueError, match="finite and positive"):
        mk(model_pressures=nan)
    loop = mk()
    try:
        with pytest.raises(ValueError, match=r"must be \(B = 3, T >= 1, 2\)"):
            loop.set_pressure_schedule(np.ones((B, 2)))
        with pytest.raises(ValueError, match="finite and positive"):
            loop.set_pressure_schedule(np.zeros((B, 4, 2)))
        with pytest.raises(ValueError, match="needs a plant schedule"):
            loop.set_pressure_schedule(None, np.ones((B, 4, 2)))
        p = scenario_pressures(B, seed=8)
        loop.initialize()
        loop.step()
        loop.set_pressures(plant=p)
        assert np.array_equal(loop.sim.get_pressures(), p)
        with pytest.raises(RuntimeError, match="no per-scenario pressures"):
            loop.ctx.get_scenario_pressures()               # the model was left alone
        loop.set_pressures(model=p[::-1].copy())
        assert np.array_equal(loop.ctx.get_scenario_pressures(), p[::-1])
        sched = np.stack([p, 2 - p, p * p], axis=1)          # (B, T = 3, 2)
        loop.set_pressure_schedule(sched)
        for k in range(1, 5):
            assert loop.k == k
            loop.step()
            assert np.array_equal(loop.sim.get_pressures(), sched[:, min(k, 2)])
            assert np.array_equal(loop.ctx.get_scenario_pressures(), p[::-1])
        loop.set_pressure_schedule(None)
        loop.step()
        assert np.array_equal(loop.sim.get_pressures(), sched[:, 2])
        assert loop.plant_failures()[0] == 0
    finally:
        loop.close()
