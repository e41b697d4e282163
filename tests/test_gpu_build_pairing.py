"""Build pairing (include/cmpc.h, cmpc_set_build_pairing; csrc/build_pair_kernel.h):
the shared form of the row build against the unpaired row build, bit for bit.
Marked gpu; runs on an MI355X.

Every case is the parallel plant's cooperative controller with the row build
forced.  No tolerance anywhere: with bitwise equal plants in a scenario's two
records the shared chain performs the same operations on the same bits, and
a scenario whose records differ is built the long way with each slot's own
plant, so CMPC_PAIRING_ON must reproduce CMPC_PAIRING_OFF exactly."""
import dataclasses
import functools

import numpy as np
import pytest

import cmpc
import refprofile_ref as RP
from cmpc._abi import CmpcDims
from cmpc.synthetic import synthetic_batch

pytestmark = pytest.mark.gpu
ON, OFF = cmpc.CMPC_PAIRING_ON, cmpc.CMPC_PAIRING_OFF


@pytest.fixture(autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()
    yield


@functools.lru_cache(maxsize=None)
def problem(p, B):
    """synthetic_batch records: one linearisation per scenario, distinct dx_aug,
    y_prev offsets and u_old per slot; read-only"""
    cfg, arr, _ = RP.config("coop-par", p)
    batch = synthetic_batch(cfg, B, seed=5 + p)
    L = cmpc.layout_of(CmpcDims.from_config(cfg, B))
    lin, u_old = batch[0], batch[1]
    for b in range(B):  # the premise of the test: equal plants up to B's column rotation, distinct tails
        r0, r1 = lin[2 * b], lin[2 * b + 1]
        B0 = r0[L.off_B:L.off_C].reshape(cfg.ns, cfg.nu_tot)
        B1 = r1[L.off_B:L.off_C].reshape(cfg.ns, cfg.nu_tot)
        assert np.array_equal(r0[:L.off_B].view(np.uint64), r1[:L.off_B].view(np.uint64))
        assert np.array_equal(r0[L.off_C:L.off_x].view(np.uint64), r1[L.off_C:L.off_x].view(np.uint64))
        assert np.array_equal(np.roll(B0, -cfg.nu, axis=1).view(np.uint64), B1.view(np.uint64))
        assert not np.array_equal(r0[L.off_x:], r1[L.off_x:])
        assert not np.array_equal(u_old[2 * b], u_old[2 * b + 1])
    for a in batch:
        a.setflags(write=False)
    return cfg, arr, batch, L


def context(cfg, arr, B, batch, lin=None):
    ctx = cmpc.Context(cfg, B)
    ctx.configure(arr)
    ctx.set_state(*batch[1:])
    ctx.upload_lin(batch[0] if lin is None else lin)
    ctx.set_build_variant(cmpc.CMPC_BUILD_ROWS)
    return ctx


def build_qp(cfg, arr, B, batch, mode, lin=None, prepare=None):
    """(H, f, G) bit patterns and the coverage counter of one forced-rows build"""
    with context(cfg, arr, B, batch, lin) as ctx:
        ctx.set_build_pairing(mode)
        if prepare:
            prepare(ctx)
        ctx.build()
        assert ctx.last_build_kernel() == cmpc.CMPC_BUILD_ROWS
        shared = ctx.last_build_shared_scenarios()
        qp = [np.ascontiguousarray(a).view(np.uint64).copy() for a in ctx.download_qp()]
    return qp, shared


def assert_same_bits(on, off):
    for name, a, b in zip("HfG", on, off):
        bad = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=1))
        assert bad.size == 0, f"{name} differs in QP slots {bad.tolist()}"


# ---- 1. the QP buffer and the coverage counter -------------------------------------
# p = 50: the delay inside the horizon; 20: delay >= p; 45: two loop segments (40, 5).
# B = 1, 3: partial groups; 4: one whole group; 5, 9: a second / third group, odd counts.

@pytest.mark.parametrize("p", [50, 20, 45])
@pytest.mark.parametrize("B", [1, 3, 4, 5, 9])
def test_gpu_pairing_qp_bit_identical(p, B):
    cfg, arr, batch, _ = problem(p, B)
    off, n_off = build_qp(cfg, arr, B, batch, OFF)
    on, n_on = build_qp(cfg, arr, B, batch, ON)
    assert n_off == -1
    assert_same_bits(on, off)
    assert n_on == B
    H = on[0].view(np.float64).reshape(2 * B, cfg.nV, cfg.nV)
    assert np.array_equal(H, H.transpose(0, 2, 1))   # exactly symmetric


# ---- 2. batches in which some scenarios' records differ ----------------------------

def altered(cfg, L, lin, scenarios, coarse=False):
    """slot 1's record of scenario scenarios[i] changed in the i % 4-th way: one
    ulp in an A, a B or a C entry, or the sign of a zero; coarse: its B scaled
    by 1.5 instead, which no rounding can hide from the QP"""
    lin = lin.copy()
    for i, b in enumerate(scenarios):
        r = lin[2 * b + 1]
        kind = i % 4
        if coarse:
            r[L.off_B:L.off_C] *= 1.5
        elif kind == 3:
            zeros = np.flatnonzero(r[:L.off_x] == 0.0)
            assert zeros.size
            r[zeros[0]] = -0.0 if not np.signbit(r[zeros[0]]) else 0.0
        else:
            lo, hi = [(L.off_A, L.off_B), (L.off_B, L.off_C), (L.off_C, L.off_f)][kind]
            e = lo + np.flatnonzero(r[lo:hi] != 0.0)[1]
            r[e] = np.nextafter(r[e], np.inf)
    return lin


@pytest.mark.parametrize("scenarios,coarse", [((0,), False), ((2, 8), False), ((1, 3, 4, 6), False),
                                              (tuple(range(9)), False), ((5,), True)], ids=str)
def test_gpu_pairing_mixed_batch(scenarios, coarse):
    B = 9
    cfg, arr, batch, L = problem(50, B)
    lin = altered(cfg, L, batch[0], scenarios, coarse)
    assert not np.array_equal(lin.view(np.uint64), batch[0].view(np.uint64))
    off, _ = build_qp(cfg, arr, B, batch, OFF, lin)
    on, shared = build_qp(cfg, arr, B, batch, ON, lin)
    assert_same_bits(on, off)
    U = len(scenarios)
    # a group of four falls back as a whole: at least the altered scenarios, at
    # most their groups, are built the long way
    assert B - 4 * U <= shared <= B - U
    if U == B:
        assert shared == 0
    # exactly: the scenarios outside the altered scenarios' groups (cmpc.h)
    groups = {b // 4 for b in scenarios}
    assert shared == sum(1 for b in range(B) if b // 4 not in groups)
    if coarse:   # the altered plant reaches slot 1's QP (and only it): the fallback used slot 1's own records
        base, _ = build_qp(cfg, arr, B, batch, OFF)
        rows = [np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=1)).tolist() for a, b in zip(off, base)]
        assert rows[0] == [2 * scenarios[0] + 1] and rows[1] == rows[0], rows


# ---- 3. settings that differ between the two slots ---------------------------------

def test_gpu_pairing_per_slot_settings():
    B = 5
    cfg, arr, batch, _ = problem(50, B)
    nq = 2 * B
    rng = np.random.default_rng(77)
    # the sub-controllers' own references and input weights (the output weights stay equal)
    y_ref = arr.y_ref.copy()
    y_ref[1] += rng.uniform(-0.1, 0.1, y_ref[1].shape)
    uwt = arr.uwt.copy()
    uwt[1] = uwt[1] * 1.75 + 0.125 * np.eye(cfg.nu)
    arr2 = dataclasses.replace(arr, y_ref=y_ref, uwt=uwt)
    dy = np.ascontiguousarray(rng.uniform(-0.05, 0.05, (nq, cfg.ny)))
    dref = np.ascontiguousarray(rng.uniform(-0.2, 0.2, (nq, cfg.p, cfg.ny)))
    scale = rng.uniform(0.3, 1.0, (nq, 1))
    limits = [np.ascontiguousarray(np.tile(getattr(arr, n), (B, 1)) * scale)
              for n in ("lower", "upper", "rate_lower", "rate_upper")]
    assert not np.array_equal(dy[0], dy[1]) and not np.array_equal(limits[1][0], limits[1][1])

    def prepare(ctx):
        ctx.set_scenario_reference(dy)
        ctx.set_scenario_constraints(*limits)
        ctx.set_scenario_reference_profile(dref)   # build + refshift

    off, _ = build_qp(cfg, arr2, B, batch, OFF, prepare=prepare)
    on, shared = build_qp(cfg, arr2, B, batch, ON, prepare=prepare)
    assert_same_bits(on, off)
    assert shared == B
    plain, _ = build_qp(cfg, arr, B, batch, OFF)
    assert (off[1] != plain[1]).any() and (off[0] != plain[0]).any()   # the settings reach f and H


# ---- 4. steps --------------------------------------------------------------------

def run_steps(cfg, arr, B, batch, mode, steps=3, K=9):
    out = []
    with context(cfg, arr, B, batch) as ctx:
        ctx.set_build_pairing(mode)
        ctx.set_step_variant(cmpc.CMPC_STEP_SPLIT)
        for _ in range(steps):
            ctx.step(K, cmpc.CMPC_APPLY_MOVE)
            assert ctx.last_build_kernel() == cmpc.CMPC_BUILD_ROWS
            assert ctx.last_build_shared_scenarios() == (B if mode == ON else -1)
            out.append((*ctx.download(), *ctx.get_state()))
    return out


def test_gpu_pairing_steps_bit_identical():
    B = 9
    cfg, arr, batch, _ = problem(50, B)
    on, off = run_steps(cfg, arr, B, batch, ON), run_steps(cfg, arr, B, batch, OFF)
    for t, (a, b) in enumerate(zip(on, off)):
        for name, x, y in zip(("du", "status", "nwsr", "u_old", "du_old", "ws"), a, b):
            x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
            assert x.tobytes() == y.tobytes(), (t, name)
    assert (on[0][1] == 0).all()
    assert not np.array_equal(on[0][3], on[2][3])   # the moves were applied


# ---- 5. refusal ---------------------------------------------------------------------

def test_gpu_pairing_on_refused_for_ncoop():
    cfg, arr, _ = RP.config("ncoop-par", 50)
    B = 3
    batch = synthetic_batch(cfg, B, seed=3)
    with context(cfg, arr, B, batch) as ctx:
        with pytest.raises(RuntimeError, match="cmpc_set_build_pairing: build pairing: no shared-form instance"):
            ctx.set_build_pairing(ON)
        # the mode is unchanged and nothing was launched: the build that follows is the unpaired one
        assert ctx.last_build_kernel() == 0
        ctx.build()
        assert ctx.last_build_kernel() == cmpc.CMPC_BUILD_ROWS
        assert ctx.last_build_shared_scenarios() == -1
