"""The kernel selection (compressor-mpc_amd/csrc/dispatch.cpp) through
cmpc.plan, without a GPU: the rows test_gpu_auto_kernel_selection pins on the
device, every switch point from both sides, the forced variants with their
error texts, and every case of tests/golden/dispatch_parent.json, recorded
on an MI355X (tools/record_dispatch.py) from the library before the
selection became one function."""
import json
import os
import subprocess
import sys

import pytest

import cmpc
from cmpc._abi import (CMPC_PLAN_NO_BUILD, CMPC_PLAN_NO_FUSED_STEP, CMPC_PLAN_NO_ROWS_BUILD,
                       CMPC_PLAN_NO_ROWS_SOLVE, CmpcDims)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256  # MI355X
WAVE, ROWS_B, SPLIT = cmpc.CMPC_BUILD_WAVE, cmpc.CMPC_BUILD_ROWS, cmpc.CMPC_BUILD_SPLIT
LANE, ROWS_S = cmpc.CMPC_SOLVE_LANE, cmpc.CMPC_SOLVE_ROWS


def plan_of(plant, ctype, p, B, cus=CUS, **kw):
    """the plan for B scenarios (nqp = B * S QPs) of a reference configuration"""
    cfg = cmpc.reference_config(plant, ctype, p=p)
    return cmpc.plan(CmpcDims.from_config(cfg, B), cus, **kw)


# the parameter rows of test_gpu_auto_kernel_selection (tests/test_gpu_small_batch.py), verbatim
@pytest.mark.parametrize("ctype,B,solve,fused,p", [
    ("cent", 16, cmpc.CMPC_SOLVE_ROWS, False, 20), ("cent", 1024, cmpc.CMPC_SOLVE_ROWS, False, 20),
    ("cent", 1024, cmpc.CMPC_SOLVE_ROWS, True, 50), ("cent", 2048, cmpc.CMPC_SOLVE_ROWS, False, 50),
    ("cent", 65536, cmpc.CMPC_SOLVE_LANE, False, 20),
    ("coop", 1, cmpc.CMPC_SOLVE_ROWS, False, 20), ("coop", 512, cmpc.CMPC_SOLVE_ROWS, False, 20),
    ("coop", 2048, cmpc.CMPC_SOLVE_ROWS, False, 20),   # 4 096 QPs: four per SIMD
    ("coop", 4096, cmpc.CMPC_SOLVE_LANE, False, 20),
    ("coop", 65536, cmpc.CMPC_SOLVE_LANE, False, 20)])
def test_plan_gives_the_pinned_gpu_selection(ctype, B, solve, fused, p):
    """What test_gpu_auto_kernel_selection observes on the device: the solve
    kernel after iterate(1), whether step(2) fuses, and the fused kernel's
    solver."""
    pl = plan_of("par", ctype, p, B, K=2)
    assert pl.solve_kernel == solve
    assert bool(pl.step_fused) == fused
    if fused:
        assert pl.step_solve_kernel == solve


@pytest.mark.parametrize("nqp,fused", [(256, False), (257, True), (1024, True), (1025, False)])
def test_fused_step_switch_points(nqp, fused):
    """AUTO fuses nV = 8, p = 50 steps above one and up to four QPs per CU,
    on the one-QP-per-wave kernel with its row solver; at p = 20 nowhere."""
    pl = plan_of("par", "cent", 50, nqp)
    assert bool(pl.step_fused) == fused
    if fused:
        assert (pl.step_build_kernel, pl.step_solve_kernel) == (WAVE, ROWS_S)
    else:
        assert (pl.step_build_kernel, pl.step_solve_kernel) == (pl.build_kernel, pl.solve_kernel)
    assert not plan_of("par", "cent", 20, nqp).step_fused
    assert not plan_of("par", "cent", 50, nqp, K=0).step_fused


@pytest.mark.parametrize("nqp,build", [(1024, SPLIT), (1025, WAVE), (4092, WAVE), (4093, ROWS_B)])
def test_build_switch_points(nqp, build):
    """The role-split build up to one QP per SIMD (4 cus), the row build from
    a row group per SIMD (ceil(nqp / 4) >= 4 cus), the wave build between."""
    assert plan_of("par", "cent", 20, nqp).build_kernel == build
    if nqp % 2 == 0:
        assert plan_of("par", "coop", 20, nqp // 2).build_kernel == build


@pytest.mark.parametrize("ctype,nqp,solve", [("coop", 4096, ROWS_S), ("coop", 4098, LANE),
                                             ("cent", 16383, ROWS_S), ("cent", 16384, LANE)])
def test_solve_switch_points(ctype, nqp, solve):
    """nV = 4: the row solver up to 16 cus QPs; nV = 8: below 16 384 QPs."""
    cfg = cmpc.reference_config("par", ctype, p=20)
    assert plan_of("par", ctype, 20, nqp // cfg.S).solve_kernel == solve


@pytest.mark.parametrize("nqp,fused,build", [(256, True, SPLIT), (257, True, WAVE), (1024, True, WAVE),
                                             (1025, False, None)])
def test_control_step_switch_points(nqp, fused, build):
    """One launch up to four QPs per CU, its build as role-split pairs (two
    QP slots per workgroup) up to one QP per CU; polled completion for one
    workgroup only; the three calls with a forced variant or K = 0."""
    pl = plan_of("par", "cent", 50, nqp)
    assert bool(pl.control_fused) == fused
    if fused:
        assert pl.control_build_kernel == build and pl.control_solve_kernel == ROWS_S
        assert pl.control_grid == ((nqp + 1) // 2 if build == SPLIT else (nqp + 3) // 4)
        assert not pl.control_polled
    else:  # the three calls: what cmpc_step launches
        assert (pl.control_build_kernel, pl.control_solve_kernel, pl.control_grid) == \
            (pl.step_build_kernel, pl.step_solve_kernel, 0)
    for kw in (dict(K=0), dict(step=cmpc.CMPC_STEP_SPLIT), dict(build=WAVE), dict(solve=LANE)):
        assert not plan_of("par", "cent", 50, nqp, **kw).control_fused
    one = plan_of("par", "coop", 50, 1)  # B = 1: one pair workgroup, the coop row solver, polled
    assert (one.control_fused, one.control_build_kernel, one.control_solve_kernel, one.control_grid,
            one.control_polled) == (1, SPLIT, ROWS_S, 1, 1)
    assert plan_of("par", "coop", 50, 13).control_polled == 0


def test_forced_variants_and_their_errors():
    # ROWS build on (ns, ny, nu, m) = (11, 3, 2, 3): no row instance for m = 3
    cfg = cmpc.reference_config("par", "coop", p=20, m=3)
    d = CmpcDims.from_config(cfg, 64)
    assert (d.ns, d.ny, d.nu, d.m) == (11, 3, 2, 3)
    pl = cmpc.plan(d, CUS, build=ROWS_B)
    assert (pl.build_kernel, pl.build_error) == (0, CMPC_PLAN_NO_ROWS_BUILD)
    assert cmpc.plan_error_string(pl.build_error) == "row-layout build kernel not available for these dimensions"
    assert cmpc.plan(d, CUS).build_kernel == SPLIT and cmpc.plan(d, CUS, build=WAVE).build_kernel == WAVE
    # no build instance at all: a third delayed input
    d3 = CmpcDims.from_config(cmpc.reference_config("ser", "ncoop", p=20), 64)
    d3.delay[0] = 5
    pl = cmpc.plan(d3, CUS)
    assert pl.build_error == CMPC_PLAN_NO_BUILD and not pl.solve_error
    assert cmpc.plan_error_string(pl.build_error) == \
        "build kernel not instantiated for these dimensions (ns, ny, nu, m)"
    # ROWS solve with S = 8: the plan exchange stays inside a wave's four rows
    d8 = CmpcDims.from_config(cmpc.reference_config("par", "coop", p=20), 8)
    d8.S, d8.nu, d8.nu_tot, d8.m, d8.ns = 8, 1, 8, 1, 7
    pl = cmpc.plan(d8, CUS, solve=ROWS_S)
    assert (pl.solve_kernel, pl.solve_error) == (0, CMPC_PLAN_NO_ROWS_SOLVE)
    assert cmpc.plan_error_string(pl.solve_error) == \
        "row solve kernel not available for these dimensions (S must divide 4)"
    # FUSED with K = 0 falls to the two launches, without an error
    pl = plan_of("par", "cent", 50, 512, step=cmpc.CMPC_STEP_FUSED, K=0)
    assert (pl.step_fused, pl.step_error, pl.step_build_kernel, pl.step_solve_kernel) == (0, 0, SPLIT, ROWS_S)
    # FUSED with a trace: the same family (its trace instantiation)
    for ctype, B, fam in (("cent", 512, (WAVE, ROWS_S)), ("coop", 13, (WAVE, LANE)), ("coop", 4096, (ROWS_B, LANE)),
                          ("cent", 8192, (ROWS_B, ROWS_S))):
        for flags in (0, cmpc.CMPC_TRACE):
            pl = plan_of("par", ctype, 20, B, step=cmpc.CMPC_STEP_FUSED, K=3, flags=flags)
            assert (pl.step_fused, pl.step_build_kernel, pl.step_solve_kernel) == (1,) + fam, (ctype, B, flags)
    # FUSED where no fused kernel exists (m = 3)
    pl = cmpc.plan(d, CUS, step=cmpc.CMPC_STEP_FUSED, K=1)
    assert (pl.step_fused, pl.step_error) == (0, CMPC_PLAN_NO_FUSED_STEP)
    assert cmpc.plan_error_string(pl.step_error) == "cmpc_step: no fused step kernel for these dimensions"
    with pytest.raises(RuntimeError, match="unknown variant"):
        cmpc.plan(d, CUS, build=7)


def _expect(value_or_error, kernel, error, prefix=""):
    """a recorded outcome (a cmpc_last_* value or "error: <text>") against the plan's"""
    if isinstance(value_or_error, str):
        assert error and value_or_error == "error: " + prefix + cmpc.plan_error_string(error)
    else:
        assert not error and value_or_error == kernel


def test_plan_reproduces_the_recorded_selection():
    """Every case of the recorder's grid (tools/record_dispatch.py), as the
    library chose before the selection became one function."""
    with open(os.path.join(ROOT, "tests", "golden", "dispatch_parent.json")) as f:
        rec = json.load(f)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from record_dispatch import expanded  # one case per (K, B) of the file's segments
    cus = rec["cus"]
    rows, control_rows = list(expanded(rec["rows"])), list(expanded(rec["control_rows"]))
    assert len(rows) > 4000 and len(control_rows) > 500
    for plant, ctype, p, B, bv, sv, stv, K, after_build, after_iterate, after_step in rows:
        where = (plant, ctype, p, B, bv, sv, stv, K)
        try:
            pl = plan_of(plant, ctype, p, B, cus=cus, build=bv, solve=sv, step=stv, K=K)
        except RuntimeError as e:  # no build kernel takes the dimensions: every build call says so
            msg = "error: " + str(e).split("): ", 1)[1]
            assert (after_build, after_iterate, after_step) == (msg, None, msg), where
            continue
        try:
            _expect(after_build, pl.build_kernel, pl.build_error)
            _expect(after_iterate, pl.solve_kernel, pl.solve_error, "cmpc_iterate: ")
            if isinstance(after_step, str):  # the fused step's error, else the build's, else the iterate's
                err = pl.step_error or pl.build_error
                _expect(after_step, None, err or pl.solve_error, "" if err else "cmpc_iterate: ")
            else:
                assert after_step == [pl.step_build_kernel, pl.step_solve_kernel, pl.step_fused]
        except AssertionError as e:
            raise AssertionError(f"{where}: recorded {after_build, after_iterate, after_step}, "
                                 f"plan {pl.as_dict()}") from e
    for plant, ctype, p, B, bv, sv, stv, K, after in control_rows:
        where = (plant, ctype, p, B, bv, sv, stv, K)
        try:
            pl = plan_of(plant, ctype, p, B, cus=cus, build=bv, solve=sv, step=stv, K=K)
        except RuntimeError as e:
            assert after == "error: " + str(e).split("): ", 1)[1], where
            continue
        if isinstance(after, str):
            err = pl.step_error or pl.build_error
            _expect(after, None, err or pl.solve_error, "" if err else "cmpc_iterate: ")
        else:
            assert after == [pl.control_build_kernel, pl.control_solve_kernel,
                             int(pl.control_fused or pl.step_fused)], (where, after, pl.as_dict())


def test_dispatch_under_sanitizers():
    """The selection (dispatch.cpp, host code) built with AddressSanitizer and
    UndefinedBehaviorSanitizer as a stand-alone program and run over 4 000
    random batches, CU counts, variants and calls on 24 random dimension sets:
    no memory or UB error, no plan names an unavailable kernel, a forced
    variant is taken or an error, AUTO has no error where a wave build and a
    lane solve exist (tests/cpp/dispatch_asan.cpp)."""
    here = os.path.join(ROOT, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-C", here, "dispatch_asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(here, "dispatch_asan"), "4000", "24"], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("ok"), r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-2000:]
