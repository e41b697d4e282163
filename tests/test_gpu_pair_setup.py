"""The pair build's per-group set-up (csrc/build_pair_kernel.h, between the
staging wait and the first horizon step): the w tables, the guarded FMA chains
of the prologue and the zero restores, all of them branch-free batches of LDS
reads with clamped addresses and selects.  The tests that build are marked gpu
and run on an MI355X.

CMPC_PAIRING_ON against CMPC_PAIRING_OFF, the whole QP buffer (H, f, G of every
slot) bit for bit and the coverage counter, as in
test_gpu_build_pair_pipeline.py: the unpaired row build is the reference.
par-coop, the smallest shapes that reach every path the set-up touches:

  * with D the largest input delay (40): p = D - 1, D, D + 1, D + 3, 2 D + 1:
    lines that never drain and lines that do, w-table entries t < dlen and
    t >= dlen in the same pass of 16, passes of the table that are partly or
    wholly empty (WL = 40 .. 44);
  * p = 50 and p = 7: the 2-step and 1-step remainder blocks after the set-up
    (p = 7: a table shorter than the delay line, WL < dlen);
  * B = 1, 3, 5, 8: partial groups (a lone scenario among them) and whole ones;
  * B = 8 192 + 5: more groups than the launch has waves, so a set-up follows
    an epilogue in the same wave;
  * one scenario of every second group with one entry of slot 1's A changed in
    the last bit: the two-pass path, whose second set-up follows a restaging;
  * each with and without per-scenario output references (dy_ref), u_old
    distinct per slot throughout."""
import functools

import numpy as np
import pytest

import cmpc
import refprofile_ref as RP
from cmpc._abi import CmpcDims
from cmpc.synthetic import synthetic_batch

ON, OFF = cmpc.CMPC_PAIRING_ON, cmpc.CMPC_PAIRING_OFF
D = 40   # the parallel plant's largest input delay (asserted in problem())
HORIZONS = [D - 1, D, D + 1, D + 3, 2 * D + 1, 50, 7]
BATCHES = [1, 3, 5, 8]
B_LARGE = 8192 + 5


@pytest.fixture
def _torch_first():
    import torch
    torch.cuda.init()
    yield


def gpu(fn):
    return pytest.mark.gpu(pytest.mark.usefixtures("_torch_first")(fn))


@functools.lru_cache(maxsize=None)
def problem(p, B):
    """one linearisation per scenario (at most 64 distinct ones), distinct tails
    and u_old per slot, and one output-reference offset per QP slot; read-only"""
    cfg, arr, _ = RP.config("coop-par", p)
    assert max(cfg.delays) == D
    batch = synthetic_batch(cfg, B, seed=11 + p, n_distinct=min(B, 64))
    L = cmpc.layout_of(CmpcDims.from_config(cfg, B))
    lin, u_old = batch[0], batch[1]
    r0, r1 = lin[0::2], lin[1::2]
    assert np.array_equal(r0[:, :L.off_B].view(np.uint64), r1[:, :L.off_B].view(np.uint64))
    assert np.array_equal(r0[:, L.off_C:L.off_x].view(np.uint64), r1[:, L.off_C:L.off_x].view(np.uint64))
    B0 = r0[:, L.off_B:L.off_C].reshape(B, cfg.ns, cfg.nu_tot)
    B1 = r1[:, L.off_B:L.off_C].reshape(B, cfg.ns, cfg.nu_tot)
    assert np.array_equal(np.roll(B0, -cfg.nu, axis=2), B1)
    assert (r0[:, L.off_x:] != r1[:, L.off_x:]).any(axis=1).all()
    u2 = np.asarray(u_old).reshape(B, 2, -1)
    assert (u2[:, 0] != u2[:, 1]).any(axis=1).all()
    dy = np.ascontiguousarray(np.random.default_rng(300 + p).uniform(-0.05, 0.05, (2 * B, cfg.ny)))
    assert (dy[0::2] != dy[1::2]).any(axis=1).all()
    for a in (*batch, dy):
        a.setflags(write=False)
    return cfg, arr, batch, L, dy


def build_qp(cfg, arr, B, batch, mode, dy=None, lin=None):
    """(H, f, G) bit patterns and the coverage counter of one forced-rows build"""
    with cmpc.Context(cfg, B) as ctx:
        ctx.configure(arr)
        ctx.set_state(*batch[1:])
        ctx.upload_lin(batch[0] if lin is None else lin)
        ctx.set_build_variant(cmpc.CMPC_BUILD_ROWS)
        ctx.set_build_pairing(mode)
        if dy is not None:
            ctx.set_scenario_reference(dy)
        ctx.build()
        assert ctx.last_build_kernel() == cmpc.CMPC_BUILD_ROWS
        shared = ctx.last_build_shared_scenarios()
        qp = [np.ascontiguousarray(a).view(np.uint64).copy() for a in ctx.download_qp()]
    return qp, shared


def assert_same_bits(on, off):
    for name, a, b in zip("HfG", on, off):
        bad = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=1))
        assert bad.size == 0, f"{name} differs in {bad.size} QP slots, first {bad[:8].tolist()}"


def check(p, B, with_dy, lin=None, expect_shared=None):
    cfg, arr, batch, _, dy = problem(p, B)
    dy = dy if with_dy else None
    off, n_off = build_qp(cfg, arr, B, batch, OFF, dy, lin)
    on, n_on = build_qp(cfg, arr, B, batch, ON, dy, lin)
    assert n_off == -1 and n_on == (B if expect_shared is None else expect_shared)
    assert (off[0] != 0).any()
    assert_same_bits(on, off)
    return off


def test_setup_horizons_are_eligible():
    """host only: the shared form takes every horizon of the list (plain lines up to p = 2 D + 1)"""
    for p in HORIZONS:
        cfg, _, _ = RP.config("coop-par", p)
        for B in BATCHES + [B_LARGE]:
            assert cmpc.build_pairing_available(CmpcDims.from_config(cfg, B)), (p, B)


# ---- 1. every horizon, partial and whole groups ----------------------------------------

@gpu
@pytest.mark.parametrize("with_dy", [False, True], ids=["plain", "dy_ref"])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("p", HORIZONS)
def test_gpu_pair_setup_bit_identical(p, B, with_dy):
    check(p, B, with_dy)


@gpu
def test_gpu_pair_setup_dy_ref_reaches_the_qp():
    """the references are in force in the comparison above: they change f"""
    plain = check(50, 5, False)
    shifted = check(50, 5, True)
    assert (plain[1] != shifted[1]).any()


# ---- 2. a set-up after an epilogue -----------------------------------------------------

@gpu
@pytest.mark.parametrize("with_dy", [False, True], ids=["plain", "dy_ref"])
@pytest.mark.parametrize("p", [D + 3, 50])
def test_gpu_pair_setup_second_group(p, with_dy):
    import torch
    waves = torch.cuda.get_device_properties(0).multi_processor_count * 2 * 4   # pair_launch
    # a larger device must fail here, not pass with one group per wave
    assert -(-B_LARGE // 4) > waves and B_LARGE % 4 != 0
    check(p, B_LARGE, with_dy)


# ---- 3. the two-pass path: a set-up after a restaging -----------------------------------

def altered_a(cfg, L, lin, scenarios):
    """slot 1's record of each scenario with one non-zero entry of A moved by one ulp"""
    lin = lin.copy()
    for b in scenarios:
        r = lin[2 * b + 1]
        e = L.off_A + np.flatnonzero(r[L.off_A:L.off_B] != 0.0)[1 + b % 5]
        r[e] = np.nextafter(r[e], np.inf)
    return lin


@gpu
@pytest.mark.parametrize("with_dy", [False, True], ids=["plain", "dy_ref"])
@pytest.mark.parametrize("p,B", [(D + 3, 21), (50, 21), (7, 21), (D + 3, B_LARGE)])
def test_gpu_pair_setup_two_pass(p, B, with_dy):
    cfg, arr, batch, L, _ = problem(p, B)
    groups = range(0, -(-B // 4), 2)                      # every second group
    scenarios = [min(4 * g + (g // 2) % 4, B - 1) for g in groups]
    lin = altered_a(cfg, L, batch[0], scenarios)
    assert not np.array_equal(lin.view(np.uint64), batch[0].view(np.uint64))
    hit = {b // 4 for b in scenarios}
    assert len(hit) == len(scenarios)
    expect = sum(1 for b in range(B) if b // 4 not in hit)
    check(p, B, with_dy, lin=lin, expect_shared=expect)
