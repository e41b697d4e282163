"""Build pairing's host predicate (include/cmpc.h, cmpc_build_pairing_available;
csrc/dispatch.cpp, cmpc_pairing_error), without a GPU: which configurations
the shared form of the row build takes, the reason it gives for the others,
and that it leaves cmpc.plan alone (the shared form is a mode of the row
family, not a plan entry)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cmpc
import test_dispatch as TD
from cmpc._abi import CmpcDims

CUS = 256
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dims_of(ctype, p=50, B=4096, m=2, plant="par"):
    return CmpcDims.from_config(cmpc.reference_config(plant, ctype, p=p, m=m), B)


def lwt_of(ywt):
    """L_W' of a weight matrix (cmpc_abi.cpp, rebuild_cfg): upper triangular"""
    return np.ascontiguousarray(np.linalg.cholesky(np.asarray(ywt, dtype=np.float64)).T)


REF_LWT = lwt_of(np.diag([1.0, 1.0, 4.2e2]))


@pytest.mark.parametrize("p", [50, 20, 45])
@pytest.mark.parametrize("B", [1, 9, 4096, 65536])
def test_reference_par_coop_is_eligible(p, B):
    d = dims_of("coop", p, B)
    assert (d.ns, d.ny, d.nu, d.m, d.S, d.nu_tot) == (11, 3, 2, 2, 2, 4)
    assert list(d.delay[:4]) == [0, 40, 0, 40]
    assert cmpc.build_pairing_reason(d, REF_LWT, REF_LWT.copy()) == ""
    assert cmpc.build_pairing_available(d, REF_LWT, REF_LWT.copy())
    assert cmpc.build_pairing_available(d)   # the weights left out


def one_bit_off(a):
    b = a.copy()
    b.reshape(-1).view(np.uint64)[b.size - 1] ^= 1
    return b


def rotated_delays(d, delays):
    for i, v in enumerate(delays):
        d.delay[i] = v
    return d


INELIGIBLE = [
    ("ncoop", lambda: (dims_of("ncoop"), None, None), "no shared-form instance"),
    ("cent", lambda: (dims_of("cent"), None, None), "S = 2"),
    ("delays not rotation-invariant", lambda: (rotated_delays(dims_of("coop"), (0, 40, 0, 30)), None, None),
     "not invariant under the rotation"),
    ("delays (40, 0, 0, 40)", lambda: (rotated_delays(dims_of("coop"), (40, 0, 0, 40)), None, None),
     "not invariant under the rotation"),
    ("lwt one bit apart", lambda: (dims_of("coop"), REF_LWT, one_bit_off(REF_LWT)), "not bitwise equal"),
    ("lwt -0.0 against +0.0", lambda: (dims_of("coop"), REF_LWT, REF_LWT * np.where(REF_LWT == 0, -1.0, 1.0)),
     "not bitwise equal"),
    ("m = 3", lambda: (dims_of("coop", p=20, m=3), None, None), "no shared-form instance"),
    ("m = 1", lambda: (dims_of("coop", m=1), None, None), "no shared-form instance"),
    ("serial plant", lambda: (dims_of("coop", plant="ser"), None, None), "no shared-form instance"),
]


@pytest.mark.parametrize("what,make,reason", INELIGIBLE, ids=[c[0] for c in INELIGIBLE])
def test_ineligible_configurations_say_why(what, make, reason):
    d, l0, l1 = make()
    assert not cmpc.build_pairing_available(d, l0, l1)
    text = cmpc.build_pairing_reason(d, l0, l1)
    assert text.startswith("build pairing") and reason in text, text


def test_a_horizon_that_needs_a_ring_is_ineligible():
    """Some horizon of the reference par-coop set gets ring hand-off lines from
    the layout search; the shared form has no ring instance.  Longer plain
    horizons fail on the LDS two workgroups per CU need."""
    reasons = {p: cmpc.build_pairing_reason(dims_of("coop", p)) for p in (100, 150, 200, 300)}
    assert all(reasons.values()), reasons
    assert all("ring" in r or "LDS" in r or "row build cannot run" in r for r in reasons.values()), reasons
    assert any("ring" in r for r in reasons.values()), reasons


def test_null_and_invalid_dimensions():
    lib = cmpc.load_library()
    assert lib.cmpc_build_pairing_available(None, None, None) == 0
    assert lib.cmpc_build_pairing_reason(None, None, None) == b"null argument"
    d = dims_of("coop")
    d.ns = 0
    assert not cmpc.build_pairing_available(d)
    assert cmpc.build_pairing_reason(d) == "invalid dimensions"
    with pytest.raises(ValueError):
        cmpc.build_pairing_available(dims_of("coop"), np.zeros(4), np.zeros(4))


def test_plan_struct_and_ids_unchanged():
    assert ctypes.sizeof(cmpc._abi.CmpcPlan) == 13 * 4
    assert (cmpc.CMPC_BUILD_AUTO, cmpc.CMPC_BUILD_WAVE, cmpc.CMPC_BUILD_ROWS, cmpc.CMPC_BUILD_SPLIT) == (0, 1, 2, 3)
    assert (cmpc.CMPC_PAIRING_AUTO, cmpc.CMPC_PAIRING_OFF, cmpc.CMPC_PAIRING_ON) == (0, 1, 2)


def _rows(test):
    mark = [m for m in test.pytestmark if m.name == "parametrize"][0]
    return mark.args[1]


def test_plans_of_the_dispatch_tests_are_unchanged():
    """Every case tests/test_dispatch.py enumerates, through its own checks: the
    pinned selection, every switch point, the forced variants and the recorded
    grid (tests/golden/dispatch_parent.json)."""
    for row in _rows(TD.test_plan_gives_the_pinned_gpu_selection):
        TD.test_plan_gives_the_pinned_gpu_selection(*row)
    for row in _rows(TD.test_fused_step_switch_points):
        TD.test_fused_step_switch_points(*row)
    for row in _rows(TD.test_build_switch_points):
        TD.test_build_switch_points(*row)
    for row in _rows(TD.test_solve_switch_points):
        TD.test_solve_switch_points(*row)
    for row in _rows(TD.test_control_step_switch_points):
        TD.test_control_step_switch_points(*row)
    TD.test_forced_variants_and_their_errors()
    TD.test_plan_reproduces_the_recorded_selection()
    # and where the shared form is eligible the plan still names the row family
    for B in (2048, 4096, 65536):
        pl = cmpc.plan(dims_of("coop", 50, B), CUS, K=9)
        assert (pl.build_kernel, pl.step_build_kernel, pl.step_fused) == (cmpc.CMPC_BUILD_ROWS, cmpc.CMPC_BUILD_ROWS, 0)


def test_pair_layout_under_sanitizers():
    """The shared form's LDS region (rows_layout.cpp, cmpc_pair_layout; host
    code) built with AddressSanitizer and UndefinedBehaviorSanitizer as a
    stand-alone program and run on 40 random dimension sets: no memory or UB
    error, and every region build_pair_kernel.h addresses lies inside the
    wave's LDS (tests/cpp/pair_layout_asan.cpp)."""
    here = os.path.join(ROOT, "tests", "cpp")
    csrc = os.path.join(ROOT, "compressor-mpc_amd", "csrc")
    libdir = os.path.join(ROOT, "compressor-mpc_amd", "cmpc")
    exe = os.path.join(here, "pair_layout_asan")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O1", "-g", "-std=c++17",
                           "-fno-omit-frame-pointer", "-Xarch_host", "-fsanitize=address", "-Xarch_host",
                           "-fsanitize=undefined", "-o", exe, os.path.join(here, "pair_layout_asan.cpp"),
                           os.path.join(csrc, "rows_layout.cpp"), "-L" + libdir, "-lcmpc",
                           "-Wl,-rpath," + libdir])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, "40"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("ok"), r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-2000:]
