"""Refusals of every entry point that takes a device array from the caller
(include/cmpc.h): cmpc_bind_lin, cmpc_bind_state, each cmpc_bind_scenario_*,
cmpc_score_bind, cmpc_envelope_bind, cmpc_sim_bind_pressures and the `out` of
cmpc_noise_step.  They share one pointer query (device_range_ok,
csrc/abi_common.cpp).  Marked gpu; runs on an MI355X.

Each entry point refuses, with its own message,
  a host pointer,
  device memory one element too short,
  a range that starts inside device memory and runs past its end,
  a pointer off its own alignment rule (4 bytes off where the rule is 8,
  8 bytes off where it is 16, 2 bytes off for the 4-byte working sets).
What the library can see is the allocation, and torch carves tensors out of
larger ones: the short ranges are therefore laid against the end of the
allocation that holds a tensor.

A refusal leaves nothing behind, and least of all a pending error of the
runtime that a later launch check would report: after the refusals on a
context, one build + iterate (K = 1) + download returns the du, status and
nWSR of a context that saw none, bit for bit; likewise one integrate +
download of a simulator, and one cmpc_noise_step.  No refused pointer is ever
bound, and nothing is launched before every refusal has been checked.

Shapes: par/coop, p = 20, B = 4 (8 QP slots); a simulator with B = 4."""
import functools
import re

import numpy as np
import pytest

import cmpc
import golden_cases as GC
from cmpc.sim import PlantSimulator
from cmpc.synthetic import synthetic_batch

pytestmark = pytest.mark.gpu
B, P, N_OUT = 4, 20, 4


@pytest.fixture(autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()
    yield


@functools.lru_cache(maxsize=None)
def problem():
    cfg, setup, arr, _ = GC.case("coop-par", p=P)
    batch = synthetic_batch(cfg, B, seed=7)
    for a in batch:
        a.setflags(write=False)
    return cfg, arr, batch


def make_ctx():
    cfg, arr, (lin, u_old, du_old, ws) = problem()
    ctx = cmpc.Context(cfg, B)
    ctx.configure(arr)
    ctx.set_state(u_old, du_old, ws)
    ctx.upload_lin(lin)
    return ctx


def one_step(ctx):
    ctx.build()
    ctx.iterate(1)
    return ctx.download()


@functools.lru_cache(maxsize=None)
def untouched_step():
    """du, status, nWSR of a context that saw no refusal"""
    with make_ctx() as ctx:
        out = one_step(ctx)
    for a in out:
        a.setflags(write=False)
    return out


class Pool:
    """A zeroed device tensor of 1 MiB, the end of the allocation that holds
    it, and the bad pointers for an array of `need` bytes."""

    def __init__(self):
        import torch
        self.t = torch.zeros(1 << 17, dtype=torch.float64, device="cuda:0")
        seg = [s for s in torch.cuda.memory_snapshot()
               if s["address"] <= self.t.data_ptr() < s["address"] + s["total_size"]]
        assert len(seg) == 1
        self.end = seg[0]["address"] + seg[0]["total_size"]
        self.host = np.zeros(1 << 17)
        assert self.t.data_ptr() % 16 == 0 and self.end % 16 == 0

    def good(self, k=0):
        """the k-th 256 KiB quarter of the tensor: a valid, aligned array"""
        return self.t.data_ptr() + k * (1 << 18)

    def out_of_range(self, need):
        assert 16 <= need <= 1 << 18 and need % 8 == 0
        return {"host": self.host.ctypes.data,
                "short": self.end - (need - 8),                  # one element is missing
                "overrun": (self.end - need // 2) & ~15}         # half the array is missing

    def misaligned(self, off):
        return self.t.data_ptr() + off


def refused(call, fragment):
    with pytest.raises(RuntimeError, match=re.escape(fragment)):
        call()


def assert_step_untouched(ctx):
    for got, want in zip(one_step(ctx), untouched_step()):
        assert np.array_equal(got, want)


# ---- the context's binds: (entry point, doubles, how the message spells them) -----

def scenario_binds(ctx):
    cfg, nq = ctx.cfg, ctx.nqp
    return [
        ("cmpc_bind_scenario_reference", ctx.bind_scenario_reference, nq * cfg.ny, "nqp * ny"),
        ("cmpc_bind_scenario_constraints", ctx.bind_scenario_constraints, nq * 4 * cfg.nu, "nqp * 4 nu"),
        ("cmpc_bind_scenario_reference_profile", ctx.bind_scenario_reference_profile, nq * cfg.p * cfg.ny,
         "nqp * p * ny"),
        ("cmpc_bind_scenario_weights", ctx.bind_scenario_weights, nq * (cfg.ny ** 2 + cfg.nu ** 2),
         "nqp * (ny*ny + nu*nu)"),
        ("cmpc_bind_scenario_pressures", ctx.bind_scenario_pressures, 2 * B, "B * 2"),
    ]


def test_gpu_bind_lin_refusals():
    pool = Pool()
    with make_ctx() as ctx:
        need = 8 * ctx.nqp * ctx.layout.rec_len
        for what, ptr in pool.out_of_range(need).items():
            refused(lambda: ctx.bind_lin(ptr),
                    "cmpc_bind_lin: not a device allocation of nqp * rec_len doubles on the context's device")
        refused(lambda: ctx.bind_lin(pool.misaligned(8)), "cmpc_bind_lin: records must be 16-byte aligned")
        assert_step_untouched(ctx)


def test_gpu_bind_state_refusals():
    pool = Pool()
    with make_ctx() as ctx:
        nq = ctx.nqp
        need = [8 * nq * ctx.cfg.nu_tot, 8 * nq * ctx.layout.nV, 4 * nq]
        good = [pool.good(0), pool.good(1), pool.good(2)]
        for k in range(3):
            for what, ptr in pool.out_of_range(need[k]).items():
                args = list(good)
                args[k] = ptr
                refused(lambda: ctx.bind_state(*args),
                        "cmpc_bind_state: not device allocations of the state's size on the context's device")
            args = list(good)
            args[k] = pool.misaligned(2 if k == 2 else 4) + k * (1 << 18)
            refused(lambda: ctx.bind_state(*args), "cmpc_bind_state: misaligned state array")
        refused(lambda: ctx.bind_state(good[0], 0, good[2]), "cmpc_bind_state: bind all three state arrays or none")
        assert_step_untouched(ctx)


@pytest.mark.parametrize("which", range(5))
def test_gpu_bind_scenario_refusals(which):
    pool = Pool()
    with make_ctx() as ctx:
        name, bind, n, words = scenario_binds(ctx)[which]
        for what, ptr in pool.out_of_range(8 * n).items():
            refused(lambda: bind(ptr), f"{name}: not a device allocation of {words} doubles on the context's device")
        refused(lambda: bind(pool.misaligned(4)), f"{name}: misaligned array")
        assert_step_untouched(ctx)


def test_gpu_score_and_envelope_bind_refusals():
    pool = Pool()
    with make_ctx() as ctx:
        ctx.score_enable(N_OUT, Ts=0.05)
        ctx.envelope_enable(N_OUT, 2, (0.5,))
        cases = [("cmpc_score_bind", ctx.score_bind, cmpc.score_len(ctx.dims) * ctx.nqp, "len * nqp"),
                 ("cmpc_envelope_bind", ctx.envelope_bind, 2 * cmpc.envelope_len(ctx.dims, N_OUT, 1),
                  "t_cap * cmpc_envelope_len")]
        for name, bind, n, words in cases:
            for what, ptr in pool.out_of_range(8 * n).items():
                refused(lambda: bind(ptr),
                        f"{name}: not a device allocation of {words} doubles on the context's device")
            refused(lambda: bind(pool.misaligned(4)), f"{name}: misaligned array")
        assert_step_untouched(ctx)


# ---- the simulator and the noise call ------------------------------------------------

def sim_interval(refuse):
    import torch
    cfg = problem()[0]
    x0, u_def = cmpc.plant_default(cfg.plant)
    x = torch.from_numpy(np.tile(x0, (B, 1))).to("cuda:0")
    u = torch.from_numpy(np.tile(u_def, (B, 1))).to("cuda:0")
    with PlantSimulator(cfg.plant, B) as sim:
        sim.reset(x, u)
        if refuse:
            refuse(sim)
        sim.integrate(0.0, 0.05)
        return sim.download()


def test_gpu_sim_bind_pressures_refusals():
    pool = Pool()

    def refuse(sim):
        for what, ptr in pool.out_of_range(8 * 2 * B).items():
            refused(lambda: sim.bind_pressures(ptr),
                    "cmpc_sim_bind_pressures: not a device allocation of B * 2 doubles on the simulator's device")
        refused(lambda: sim.bind_pressures(pool.misaligned(8)),
                "cmpc_sim_bind_pressures: the array must be 16-byte aligned")
        assert np.array_equal(sim.get_pressures(), np.ones((B, 2)))   # the scalars are still in force

    for got, want in zip(sim_interval(refuse), sim_interval(None)):
        assert np.array_equal(got, want)
    x, u, dt, st = sim_interval(None)
    assert not st.any() and np.isfinite(x).all()


def test_gpu_noise_step_out_refusals():
    import torch
    pool = Pool()
    n = 3
    key = cmpc.noise_key(2026, 1, 0)
    sigma = torch.full((B, n), 0.5, dtype=torch.float64, device="cuda:0")
    before = cmpc.noise_step(2026, 5, torch.zeros(B, n, dtype=torch.float64, device="cuda:0"), sigma=sigma, stream=1)
    torch.cuda.synchronize()
    msg = "cmpc_noise_step: out is not an 8-byte aligned device allocation of B * n doubles on the device"
    for ptr in list(pool.out_of_range(8 * B * n).values()) + [pool.misaligned(4)]:
        refused(lambda: cmpc.noise_step_ptr(0, 0, key, 5, B, n, sigma.data_ptr(), 0, 0, 0, ptr), msg)
    after = cmpc.noise_step(2026, 5, torch.zeros(B, n, dtype=torch.float64, device="cuda:0"), sigma=sigma, stream=1)
    torch.cuda.synchronize()
    assert torch.equal(before, after) and bool(before.abs().sum() > 0)
    with make_ctx() as ctx:   # nor does a context's next launch check see an error
        assert_step_untouched(ctx)
