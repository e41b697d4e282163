"""The pair build's horizon loop (csrc/build_pair_kernel.h) where a deeper
software pipeline can go wrong: the 2-step and 1-step remainder blocks, the
segment switches next to them, and waves that build more than one group.
The tests that build are marked gpu and run on an MI355X.

CMPC_PAIRING_ON against CMPC_PAIRING_OFF, bit for bit, as in
test_gpu_build_pairing.py: the unpaired row build is the reference.  That
file's horizons (50, 20, 45 with the delays 0, 40, 0, 40) put every segment
boundary at a multiple of the 5-step block and its batches (B <= 9) give every
wave at most one group; here

  * p in {3, 7, 41, 43, 44, 48, 52, 84, 86}: p below the block length, every
    residue mod 5, segments such as 3 / 37 / 3 (p = 43), and the largest
    horizon whose LDS region fits (86);
  * B = 8 343 and 16 403: more groups of four scenarios than the launch has
    waves (2 workgroups per CU x 4 waves), so some waves build two and three
    groups, the last group partial;
  * the two-pass path (scenarios whose two records differ) at p = 43."""
import functools

import numpy as np
import pytest

import cmpc
import refprofile_ref as RP
from cmpc._abi import CmpcDims
from cmpc.synthetic import synthetic_batch

ON, OFF = cmpc.CMPC_PAIRING_ON, cmpc.CMPC_PAIRING_OFF
HORIZONS = [3, 7, 41, 43, 44, 48, 52, 84, 86]


@pytest.fixture
def _torch_first():
    import torch
    torch.cuda.init()
    yield


def gpu(fn):
    return pytest.mark.gpu(pytest.mark.usefixtures("_torch_first")(fn))


@functools.lru_cache(maxsize=None)
def problem(p, B):
    """one linearisation per scenario (at most 64 distinct ones), distinct
    tails and u_old per slot; read-only"""
    cfg, arr, _ = RP.config("coop-par", p)
    batch = synthetic_batch(cfg, B, seed=5 + p, n_distinct=min(B, 64))
    L = cmpc.layout_of(CmpcDims.from_config(cfg, B))
    lin = batch[0]
    # the premise: equal plants up to B's column rotation, distinct tails
    r0, r1 = lin[0::2], lin[1::2]
    assert np.array_equal(r0[:, :L.off_B].view(np.uint64), r1[:, :L.off_B].view(np.uint64))
    assert np.array_equal(r0[:, L.off_C:L.off_x].view(np.uint64), r1[:, L.off_C:L.off_x].view(np.uint64))
    B0 = r0[:, L.off_B:L.off_C].reshape(B, cfg.ns, cfg.nu_tot)
    B1 = r1[:, L.off_B:L.off_C].reshape(B, cfg.ns, cfg.nu_tot)
    assert np.array_equal(np.roll(B0, -cfg.nu, axis=2), B1)
    assert (r0[:, L.off_x:] != r1[:, L.off_x:]).any(axis=1).all()
    for a in batch:
        a.setflags(write=False)
    return cfg, arr, batch, L


def build_qp(cfg, arr, B, batch, mode, lin=None):
    """(H, f, G) bit patterns and the coverage counter of one forced-rows build"""
    with cmpc.Context(cfg, B) as ctx:
        ctx.configure(arr)
        ctx.set_state(*batch[1:])
        ctx.upload_lin(batch[0] if lin is None else lin)
        ctx.set_build_variant(cmpc.CMPC_BUILD_ROWS)
        ctx.set_build_pairing(mode)
        ctx.build()
        assert ctx.last_build_kernel() == cmpc.CMPC_BUILD_ROWS
        shared = ctx.last_build_shared_scenarios()
        qp = [np.ascontiguousarray(a).view(np.uint64).copy() for a in ctx.download_qp()]
    return qp, shared


def assert_same_bits(on, off):
    for name, a, b in zip("HfG", on, off):
        bad = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=1))
        assert bad.size == 0, f"{name} differs in {bad.size} QP slots, first {bad[:8].tolist()}"


def eligible(p, B=5):
    cfg, _, _ = RP.config("coop-par", p)
    return cmpc.build_pairing_available(CmpcDims.from_config(cfg, B))


def check(p, B):
    cfg, arr, batch, _ = problem(p, B)
    off, n_off = build_qp(cfg, arr, B, batch, OFF)
    on, n_on = build_qp(cfg, arr, B, batch, ON)
    assert n_off == -1 and n_on == B
    assert (off[0] != 0).any()
    assert_same_bits(on, off)


def launch_waves():
    """waves of a full pair-build launch: 2 workgroups per CU x 4 waves (pair_launch)"""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 2 * 4


# ---- 1. remainder blocks and segment switches ----------------------------------------

def test_horizon_list_is_eligible():
    """host only: the shared form takes p = 2 .. 84 and 86, not 85; at most one
    horizon of the list may ever be skipped below"""
    assert [p for p in range(2, 87) if not eligible(p)] == [85]
    assert sum(not eligible(p) for p in HORIZONS) <= 1


@gpu
@pytest.mark.parametrize("p", HORIZONS)
def test_gpu_pair_remainder_horizons(p):
    if not eligible(p):
        pytest.skip(f"cmpc.build_pairing_available says no at p = {p}")
    check(p, 5)


# ---- 2. several groups per wave --------------------------------------------------------

@gpu
@pytest.mark.parametrize("p,B,groups_per_wave", [(43, 8343, 2), (50, 16403, 3), (43, 16403, 3)])
def test_gpu_pair_several_groups_per_wave(p, B, groups_per_wave):
    waves = launch_waves()
    groups = -(-B // 4)
    # a larger device must fail here, not pass with one group per wave
    assert groups > (groups_per_wave - 1) * waves, (groups, waves)
    assert B % 4 != 0   # the last group is partial
    check(p, B)


# ---- 3. the two-pass path at a remainder horizon ---------------------------------------

def altered(cfg, L, lin, scenarios):
    """slot 1's record of scenarios[i] changed in the i % 4-th way: one ulp in
    an A, a B or a C entry, or the sign of a zero (test_gpu_build_pairing.py)"""
    lin = lin.copy()
    for i, b in enumerate(scenarios):
        r = lin[2 * b + 1]
        kind = i % 4
        if kind == 3:
            zeros = np.flatnonzero(r[:L.off_x] == 0.0)
            assert zeros.size
            r[zeros[0]] = -0.0 if not np.signbit(r[zeros[0]]) else 0.0
        else:
            lo, hi = [(L.off_A, L.off_B), (L.off_B, L.off_C), (L.off_C, L.off_f)][kind]
            e = lo + np.flatnonzero(r[lo:hi] != 0.0)[1]
            r[e] = np.nextafter(r[e], np.inf)
    return lin


@gpu
@pytest.mark.parametrize("scenarios", [(0,), (2, 8), (1, 3, 4, 6), tuple(range(9))], ids=str)
def test_gpu_pair_mixed_batch_remainder_horizon(scenarios):
    p, B = 43, 9
    cfg, arr, batch, L = problem(p, B)
    lin = altered(cfg, L, batch[0], scenarios)
    assert not np.array_equal(lin.view(np.uint64), batch[0].view(np.uint64))
    off, _ = build_qp(cfg, arr, B, batch, OFF, lin)
    on, shared = build_qp(cfg, arr, B, batch, ON, lin)
    assert_same_bits(on, off)
    groups = {b // 4 for b in scenarios}
    assert shared == sum(1 for b in range(B) if b // 4 not in groups)
