"""Closed-loop performance indices, host side (include/cmpc.h, cmpc_score_*):
the record's layout functions, the numpy model tests/score_ref.py against a
three-step example worked by hand, and every refusal that needs no device.
CPU only."""
import ctypes
import os
import re

import numpy as np
import pytest

import cmpc
from cmpc._abi import SCORE_FIELDS, CmpcDims, iptr, dptr, load_library
from score_ref import FIELDS, ScoreMirror

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def wave_dims():
    """(ns, ny, nu, m) of every set in kernel_dims.h's WAVE column"""
    text = open(os.path.join(ROOT, "compressor-mpc_amd", "csrc", "kernel_dims.h")).read()
    rows = re.findall(r"X\(F,\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),", text)
    out = [tuple(int(v) for v in r[:4]) for r in rows if r[4] == "1"]
    assert len(out) >= 8, out
    return out


def dims_of(ns, ny, nu, m, B=3):
    d = CmpcDims()
    d.ns, d.ndist, d.nu_tot, d.nu, d.ny, d.p, d.m = ns, 4, 4, nu, ny, 50, m
    for i, v in enumerate((0, 40, 0, 40)):
        d.delay[i] = v
    d.S, d.B = 4 // nu, B
    return d


@pytest.mark.parametrize("ns,ny,nu,m", wave_dims())
def test_score_fields_are_disjoint_and_cover_the_record(ns, ny, nu, m):
    d = dims_of(ns, ny, nu, m)
    n = cmpc.score_len(d)
    assert n == 4 * ny + 3 * nu + 6
    fields = cmpc.score_fields(d)
    assert tuple(fields) == SCORE_FIELDS == FIELDS
    seen = np.zeros(n, int)
    for name, sl in fields.items():
        assert 0 <= sl.start < sl.stop <= n, (name, sl)
        seen[sl] += 1
    assert (seen == 1).all(), seen                      # disjoint, and every row belongs to a field
    rows = {name: sl.stop - sl.start for name, sl in fields.items()}
    for name in ("ise", "iae", "peak", "last_out"):
        assert rows[name] == ny
    for name in ("tv", "sat_bound", "sat_rate"):
        assert rows[name] == nu
    for name in ("n", "j_track", "j_move", "n_fail", "nwsr_sum", "plant_fail_step"):
        assert rows[name] == 1
    lib = load_library()
    off, cnt = ctypes.c_int(-7), ctypes.c_int(-7)
    assert lib.cmpc_score_field(ctypes.byref(d), b"settling", ctypes.byref(off), ctypes.byref(cnt)) < 0
    assert b"settling" in lib.cmpc_last_error()
    assert off.value == -7 and cnt.value == -7
    # the mirror lays its record out through the same table
    mir = ScoreMirror(d.B, d.S, ny, nu, nu * m, [[0, 1, 2, 3][:ny]] * d.S, 0.05)
    rec = mir.record(fields)
    assert rec.shape == (n, d.B * d.S)
    assert (rec[fields["last_out"]] == -1).all() and (rec[fields["plant_fail_step"]] == -1).all()
    assert rec.sum() == -(ny + 1) * d.B * d.S


def test_score_len_refuses_bad_dims():
    d = dims_of(11, 3, 2, 2)
    d.m = 60   # m > p
    lib = load_library()
    assert lib.cmpc_score_len(ctypes.byref(d)) < 0
    assert b"invalid" in lib.cmpc_last_error()
    assert lib.cmpc_score_field(ctypes.byref(d), b"n", None, None) < 0


def test_mirror_three_steps_by_hand():
    """One slot, ny = nu = 2, nV = 4, Ts = 1/2, out_idx (1, 0), band (1/2, 1/4),
    ywt = diag(2, 4), uwt = diag(1, 2), target (2, 1); every value is a dyadic
    rational, so the sums below are exact.
      k  y           e            du            status nwsr ws     plant
      0  (1, 3)      (1, 0)       (1/2, -1/4)   0      2    0x21   0
      1  (1/2, 5/2)  (1/2, -1/2)  (0, 0)        2      10   0x03   0
      2  (1, 2)      (0, 0)       (-1, 1/2)     0      1    0x12   3
    k = 0: ise (1/2, 0), iae (1/2, 0), peak (1, 0), last_out (0, -1), j_track
    1/2 * 2 = 1, j_move 1/2 (1/4 + 2/16) = 3/16, tv (1/2, 1/4), ws bit 0: bound
    of input 0, bit 4 + 1: rate row of input 1.
    k = 1: ise + (1/8, 1/8), iae + (1/4, 1/4), peak (1, 1/2); |e0| = 1/2 is not
    above its band, |e1| = 1/2 is: last_out (0, 1); j_track + 1/2 (2/4 + 4/4) =
    7/4; the solve failed: n_fail 1, its working set is not counted.
    k = 2: e = 0 changes n only; j_move + 1/2 (1 + 2/4) = 15/16; tv (3/2, 3/4);
    ws bit 1: bound of input 1, bit 4: rate row of input 0; the plant fails."""
    m = ScoreMirror(1, 1, 2, 2, 4, [[1, 0]], 0.5, band=[[0.5, 0.25]])
    ywt, uwt = np.diag([2.0, 4.0])[None], np.diag([1.0, 2.0])[None]
    tgt = np.array([[2.0, 1.0]])
    steps = [([1.0, 3.0], [0.5, -0.25, 9.0, 9.0], 0, 2, 0x21, 0),
             ([0.5, 2.5], [0.0, 0.0, 9.0, 9.0], 2, 10, 0x03, 0),
             ([1.0, 2.0], [-1.0, 0.5, 9.0, 9.0], 0, 1, 0x12, 3)]
    for y, du, st, nw, ws, ps in steps:
        m.step(np.array([y]), tgt, np.array([du]), np.array([st]), np.array([nw]), np.array([ws], np.uint32),
               ywt, uwt, plant_status=np.array([ps]))
    want = {"n": 3.0, "ise": [0.625, 0.125], "iae": [0.75, 0.25], "peak": [1.0, 0.5], "last_out": [0.0, 1.0],
            "j_track": 1.75, "j_move": 0.9375, "tv": [1.5, 0.75], "sat_bound": [1.0, 1.0], "sat_rate": [1.0, 1.0],
            "n_fail": 1.0, "nwsr_sum": 13.0, "plant_fail_step": 2.0}
    for name in FIELDS:
        assert np.array_equal(m.f[name][0], np.asarray(want[name])), (name, m.f[name][0], want[name])
    # without a plant status the field keeps its start value
    m2 = ScoreMirror(1, 1, 2, 2, 4, [[1, 0]], 0.5)
    m2.step(np.array([[1.0, 3.0]]), tgt, np.zeros((1, 4)), np.array([0]), np.array([0]), np.zeros(1, np.uint32),
            ywt, uwt)
    assert m2.f["plant_fail_step"][0] == -1.0 and m2.f["last_out"][0].tolist() == [0.0, -1.0]


def _check(d, n_out, oi, Ts, band):
    oi = np.ascontiguousarray(oi, np.int32)
    bd = None if band is None else np.ascontiguousarray(band, np.float64)
    lib = load_library()
    rc = lib.cmpc_score_check(ctypes.byref(d), n_out, iptr(oi), Ts, dptr(bd) if bd is not None else None)
    return rc, lib.cmpc_last_error().decode()


def test_score_enable_argument_refusals():
    d = dims_of(11, 3, 2, 2)
    oi = [[0, 1, 3], [0, 1, 3]]
    assert _check(d, 4, oi, 0.05, None)[0] == 0
    assert _check(d, 4, oi, 0.05, np.full((2, 3), 0.01))[0] == 0
    for bad in ([[0, 1, 4], [0, 1, 3]], [[0, 1, 3], [0, -1, 3]]):
        rc, msg = _check(d, 4, bad, 0.05, None)
        assert rc < 0 and "out_idx" in msg, msg
    rc, msg = _check(d, 3, oi, 0.05, None)        # the same indices against three outputs
    assert rc < 0 and "out_idx" in msg
    for v in (-1e-9, float("nan"), float("inf")):
        band = np.full((2, 3), 0.01)
        band[1, 2] = v
        rc, msg = _check(d, 4, oi, 0.05, band)
        assert rc < 0 and "band" in msg and "sub-controller 1" in msg, msg
    for Ts in (-0.05, float("nan"), float("inf")):
        rc, msg = _check(d, 4, oi, Ts, None)
        assert rc < 0 and "Ts" in msg, msg
    with pytest.raises(ValueError):
        cmpc.score_check(d, 4, [[0, 1, 3]], 0.05)            # S*ny values
    with pytest.raises(ValueError):
        cmpc.score_check(d, 4, oi, 0.05, band=np.zeros(5))
    with pytest.raises(RuntimeError, match="band"):
        cmpc.score_check(d, 4, oi, 0.05, band=-np.ones((2, 3)))


def test_score_capture_argument_refusals():
    d = dims_of(11, 3, 2, 2, B=6)
    lib = load_library()

    def cap(sel, t_cap):
        sel = np.ascontiguousarray(sel, np.int32)
        rc = lib.cmpc_score_capture_check(ctypes.byref(d), len(sel), iptr(sel) if len(sel) else None, t_cap)
        return rc, lib.cmpc_last_error().decode()

    assert cap([0, 5, 3], 4)[0] == 0
    assert cap([], 0)[0] == 0                       # n_sel 0: off, whatever t_cap
    for t_cap in (0, -3):
        rc, msg = cap([0, 5, 3], t_cap)
        assert rc < 0 and "t_cap" in msg, msg
    for sel in ([0, 6], [-1, 2]):
        rc, msg = cap(sel, 4)
        assert rc < 0 and "outside" in msg, msg
    rc, msg = cap([0, 5, 0], 4)
    assert rc < 0 and "twice" in msg, msg
    with pytest.raises(RuntimeError, match="twice"):
        cmpc.score_capture_check(d, [2, 2], 3)


def test_score_calls_refuse_a_null_context():
    lib = load_library()
    z = ctypes.c_void_p(None)
    oi = np.zeros(6, np.int32)
    assert lib.cmpc_score_enable(z, 4, iptr(oi), 0.05, None) < 0
    assert lib.cmpc_score_bind(z, None) < 0
    assert lib.cmpc_score_capture(z, 0, None, 0) < 0
    assert lib.cmpc_score_bind_capture(z, None) < 0
    assert lib.cmpc_score_reset(z) < 0
    assert lib.cmpc_score_step(z, None, None, None, None, None) < 0
    assert lib.cmpc_score_download(z, None) < 0
    assert lib.cmpc_score_download_capture(z, None, None) < 0
    assert lib.cmpc_score_disable(z) < 0
    assert b"null" in lib.cmpc_last_error()
