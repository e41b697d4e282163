"""Exact ensemble quantiles on the host (cmpc_quantile_*, cmpc_quantiles_host,
cmpc_envelope_check; include/cmpc.h).  CPU only.

  1. cmpc_quantiles_host, the selection the kernels make, against the sort of
     tests/quantile_ref.py on every kind of tests/quantile_cases.py: lo and hi
     by value (NaN equal to NaN), arg exactly, and the value numpy.quantile's
     bit for bit on the finite kinds;
  2. the rank rule at its edges;
  3. every refusal;
  4. the shared text under AddressSanitizer and UndefinedBehaviorSanitizer.
"""
import ctypes

import numpy as np
import pytest

import cmpc
import golden_cases as GC
import quantile_cases as QC
import quantile_ref as QR
from cmpc._abi import CmpcDims, load_library


@pytest.mark.parametrize("B", [1, 2, 3, 63, 64, 65, 257, 1000])
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("n", [1, 3])
def test_host_selection_equals_the_sort(B, S, n):
    for kind, X in QC.cases(n, B, S).items():
        for levels in QC.LEVEL_CALLS:
            got, ref = cmpc.quantiles_host(X, levels), QR.model(X, levels)
            what = (kind, levels)
            assert QR.same(got["lo"], ref["lo"]), what
            assert QR.same(got["hi"], ref["hi"]), what
            assert np.array_equal(got["arg"], ref["arg"]), what
            assert QR.same(got["value"], ref["value"]), what
            if kind in QC.FINITE:
                # -0 is in no finite kind, so by bits is by value here; numpy's own result
                assert np.array_equal(QR.bits(got["lo"]), QR.bits(ref["lo"])), what
                assert np.array_equal(QR.bits(got["hi"]), QR.bits(ref["hi"])), what
                want = np.quantile(X, np.asarray(levels), axis=1)
                assert np.array_equal(QR.bits(got["value"]), QR.bits(want)), what
            else:
                # every NaN comes back as the one quiet NaN
                for k in ("lo", "hi"):
                    nan = np.isnan(got[k])
                    assert (QR.bits(got[k])[nan] == QR.QUIET_NAN).all(), what


def test_host_selection_on_a_two_dimensional_array():
    X = QC.cases(1, 65, 2)["normal"][0]                            # (B, C): len = 1, S = C
    got = cmpc.quantiles_host(X, (0.5,))
    assert got["lo"].shape == (1, 1, 2)
    assert np.array_equal(got["value"][0, 0], np.quantile(X, 0.5, axis=0))
    assert np.array_equal(X[got["arg"][0, 0], [0, 1]], got["lo"][0, 0])


def test_rank_rule():
    assert cmpc.quantile_rank(1, 0.0) == (0, 0, 0.0)
    assert cmpc.quantile_rank(1, 1.0) == (0, 0, 0.0)
    assert cmpc.quantile_rank(1, 0.37) == (0, 0, 0.0)
    for B in (2, 3, 64, 1000, 16389, 2 ** 31 - 1):
        assert cmpc.quantile_rank(B, 1.0) == (B - 1, B - 1, 0.0)
        assert cmpc.quantile_rank(B, 0.0) == (0, 0, 0.0)
        for q in QC.ALL8:
            assert cmpc.quantile_rank(B, q) == QR.rank(B, q), (B, q)
    assert cmpc.quantile_rank(3, 0.5) == (1, 1, 0.0)
    assert cmpc.quantile_rank(4, 0.5) == (1, 2, 0.5)


def test_value_rule():
    assert cmpc.quantile_value(1.0, 1.0, 0.3) == 1.0
    assert cmpc.quantile_value(1.0, 3.0, 0.25) == 1.5
    assert cmpc.quantile_value(1.0, 3.0, 0.75) == 2.5
    assert cmpc.quantile_value(1.0, np.inf, 0.25) == np.inf        # (numpy: NaN)
    assert cmpc.quantile_value(-np.inf, 1.0, 0.75) == -np.inf
    assert np.isnan(cmpc.quantile_value(1.0, np.nan, 0.5))
    rng = np.random.default_rng(3)
    a, d, g = rng.normal(size=500), rng.uniform(0, 1, 500), rng.uniform(0, 1, 500)
    got = cmpc.quantile_value(a, a + d, g)
    assert np.array_equal(QR.bits(got), QR.bits(QR.value(a, a + d, g)))


def test_quantile_refusals():
    lib = load_library()
    P = ctypes.POINTER(ctypes.c_double)
    one = np.array([0.5])
    ptr = lambda a: a.ctypes.data_as(P)
    x, out = np.zeros(4), np.zeros(3 * 9)

    def refused(rc, text):
        assert rc == -1
        assert text in lib.cmpc_last_error().decode(), lib.cmpc_last_error()

    refused(lib.cmpc_quantile_check(0, 1, ptr(one)), "B must be >= 1")
    refused(lib.cmpc_quantile_check(4, 0, ptr(one)), "n_levels must be inside [1, 8]")
    refused(lib.cmpc_quantile_check(4, 9, ptr(np.full(9, 0.5))), "n_levels must be inside [1, 8]")
    refused(lib.cmpc_quantile_check(4, 1, None), "null levels")
    for bad in (-1e-9, 1.0 + 1e-9, np.nan, np.inf):
        refused(lib.cmpc_quantile_check(4, 2, ptr(np.array([0.5, bad]))), "level 1 must be inside [0, 1]")
    assert lib.cmpc_quantile_check(4, 8, ptr(np.linspace(0, 1, 8))) == 0
    lo, hi, g = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
    refused(lib.cmpc_quantile_rank(0, 0.5, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(g)), "B must be >= 1")
    refused(lib.cmpc_quantile_rank(4, 1.5, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(g)), "must be inside")
    refused(lib.cmpc_quantile_rank(4, 0.5, None, ctypes.byref(hi), ctypes.byref(g)), "null argument")
    refused(lib.cmpc_quantiles_host(None, 1, 4, 1, 1, ptr(one), ptr(out)), "null argument")
    refused(lib.cmpc_quantiles_host(ptr(x), 1, 4, 1, 1, ptr(one), None), "null argument")
    refused(lib.cmpc_quantiles_host(ptr(x), 1, 4, 1, 1, None, ptr(out)), "null levels")
    refused(lib.cmpc_quantiles_host(ptr(x), 1, 0, 1, 1, ptr(one), ptr(out)), "B must be >= 1")
    refused(lib.cmpc_quantiles_host(ptr(x), 1, 4, 1, 9, ptr(np.full(9, 0.5)), ptr(out)), "n_levels must be inside")
    refused(lib.cmpc_quantiles_host(ptr(x), 0, 4, 1, 1, ptr(one), ptr(out)), "len and S must be >= 1")
    refused(lib.cmpc_score_quantiles(None, 1, ptr(one), ptr(out)), "null argument")
    with pytest.raises(RuntimeError, match="must be inside"):
        cmpc.quantiles_host(np.zeros((4, 1)), (2.0,))
    with pytest.raises(RuntimeError, match="n_levels must be inside"):
        cmpc.quantiles_host(np.zeros((4, 1)), ())


def test_envelope_check_refusals():
    cfg = GC.case("coop-par", p=50)[0]
    dims = CmpcDims.from_config(cfg, 6)
    chans = 4 + cfg.nu_tot
    lv, th = cmpc.envelope_check(dims, 4, 8, (0.05, 0.5, 0.95), np.zeros(chans))
    assert lv.size == 3 and th.size == chans
    assert cmpc.envelope_check(dims, 4, 1)[0].size == 0            # no levels: the statistics only
    assert cmpc.envelope_len(dims, 4, 3) == chans * 12 and cmpc.envelope_len(dims, 4, 0) == chans * 6
    for kw, text in ((dict(t_cap=0), "t_cap must be >= 1"),
                     (dict(n_outputs=0), "n_outputs must be >= 1"),
                     (dict(levels=(0.5, 1.5)), "level 1 must be inside"),
                     (dict(levels=(np.nan,)), "level 0 must be inside"),
                     (dict(levels=np.full(9, 0.5)), "n_levels must be inside \\[0, 8\\]"),
                     (dict(thresholds=np.array([0.0] * (chans - 1) + [np.nan])), "is not a number")):
        args = dict(n_outputs=4, t_cap=8, levels=(0.5,), thresholds=None)
        args.update(kw)
        with pytest.raises(RuntimeError, match=text):
            cmpc.envelope_check(dims, **args)
    with pytest.raises(ValueError, match="thresholds must hold"):
        cmpc.envelope_check(dims, 4, 8, (0.5,), np.zeros(chans + 1))
    lib = load_library()
    assert lib.cmpc_envelope_check(None, 4, 8, 0, None, None) == -1
    assert lib.cmpc_envelope_enable(None, 4, 8, 0, None, None) == -1
    assert lib.cmpc_envelope_step(None, None, None) == -1


def test_selection_body_under_sanitizers():
    """csrc/ensemble_select.h, the text the host entry points and the kernels
    share, in a stand-alone program under AddressSanitizer and
    UndefinedBehaviorSanitizer (tests/cpp/ensemble_select_asan.cpp): exact-size
    heap buffers over random dimensions, checked against std::sort."""
    import os
    import subprocess
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    subprocess.check_call(["make", "-s", "-C", here, "-f", "ensemble_select_asan.mk", "ensemble_select_asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(here, "ensemble_select_asan")], capture_output=True, text=True, timeout=120,
                       env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("ensemble_select_asan ok"), r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-2000:]
