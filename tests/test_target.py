"""The steady-state target solve on the host (cmpc_plant_target_host,
csrc/target_body.h): the solutions against the oracle's plant,
one bordered Newton step against numpy and a long-double elimination, nh = 0
against the equilibrium solve bit for bit, every status, every refusal of
cmpc_target_check, and the body under ASan + UBSan.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

import cmpc
import equilibrium_cases as EC
import target_cases as TC
from cmpc._abi import dptr, iptr, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_F, TOL_Y = 1e-12, 1e-10
STEP_FACTOR = 8.0    # the product's step against numpy's measured error (DESIGN.md §3.19's rule)
# the most Newton steps the host twin takes over the 64 seeded cases of each
# row (measured); the tests allow two more
MEASURED_ITERS = {TC.TORQUE_ROWS[0]: 4, TC.TORQUE_ROWS[1]: 5, TC.TORQUE_ROWS[2]: 4, TC.TORQUE_ROWS[3]: 4,
                  TC.TORQUE_ROWS[4]: 4, TC.TORQUE_ROWS[5]: 4, TC.TORQUE_ROWS[6]: 6,
                  (1,) + TC.ALL_FOUR: 4}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check_solutions(plant, hold, free, p, u, x, t, rows, budget):
    xs, us, st, it, rs = cmpc.plant_target(plant, p, hold, free, t, u, x)
    print("statuses", np.bincount(st).tolist(), "iters", it[rows].min(), "to", it[rows].max(), "resid", rs[rows].max(0))
    assert (st[rows] == cmpc.CMPC_EQ_OK).all(), st
    assert it[rows].max() <= budget + 2
    fixed = np.setdiff1d(np.arange(u.shape[1]), [TC.PLANT_INPUT[c] for c in free])
    assert np.array_equal(bits(us[:, fixed]), bits(u[:, fixed]))
    for b in np.flatnonzero(rows):
        assert np.abs(EC.or_derivative(plant, xs[b], us[b], *p[b])).max() <= 1e-11, b
    assert np.abs(TC.outputs(plant, xs[rows])[:, list(hold)] - t[rows]).max() <= TOL_Y
    assert (rs[rows, 0] <= TOL_F).all() and (rs[rows, 1] <= TOL_Y).all()
    return xs, us, st, it, rs


@pytest.mark.parametrize("row", TC.TORQUE_ROWS, ids=str)
def test_torque_rows_reach_their_targets(row):
    plant, hold, free = row
    p, u, x, t = TC.cases(plant, hold)
    _, us, *_ = _check_solutions(plant, hold, free, p, u, x, t, np.ones(len(x), bool), MEASURED_ITERS[row])
    cols = [TC.PLANT_INPUT[c] for c in free]
    assert (us[:, cols] != u[:, cols]).all()       # the free inputs did move


def test_serial_plant_with_all_four_inputs_free():
    p, u, x, t = TC.cases(1, TC.ALL_FOUR[0], recycle=True)
    _, us, *_ = _check_solutions(1, *TC.ALL_FOUR, p, u, x, t, np.ones(len(x), bool), MEASURED_ITERS[(1,) + TC.ALL_FOUR])
    assert (us[:, [3, 7]] >= 2e-2).all()


@pytest.mark.parametrize("row", TC.TORQUE_ROWS + ((1,) + TC.ALL_FOUR,), ids=str)
def test_one_newton_step_against_a_dense_model(row):
    """[x; u_free] after exactly one bordered step against the same step with
    the oracle's A, B, C, f solved by numpy.linalg.solve.  A call returns that
    state when tol_y lies between r_y(start) and r_y(after one step) and tol_f
    admits everything: tol_y = r_y(start) / 2 gives OK with iters = 1.
    Tolerance: STEP_FACTOR times the largest distance of numpy's float64 step
    from the long-double step over the same cases (measured here)."""
    plant, hold, free = row
    p, u, x, t = TC.cases(plant, hold, recycle=len(hold) == 4)
    cols = [TC.PLANT_INPUT[c] for c in free]
    measured = product = 0.0
    for b in range(len(x)):
        ry0 = np.abs(TC.outputs(plant, x[b])[0, list(hold)] - t[b]).max()
        xs, us, st, it, rs = cmpc.plant_target(plant, p[b:b + 1], hold, free, t[b:b + 1], u[b:b + 1], x[b:b + 1],
                                               max_iter=1, tol_f=1e300, tol_y=0.5 * ry0)
        assert st[0] == cmpc.CMPC_EQ_OK and it[0] == 1, (b, st, it, rs, ry0)
        z64, zld = TC.newton_step_models(plant, hold, free, t[b], x[b], u[b], *p[b])
        measured = max(measured, EC.rel_diff(z64, zld))
        product = max(product, EC.rel_diff(np.concatenate([xs[0], us[0, cols]]), zld))
    print("float64 numpy against long double", measured, "product against long double", product)
    assert measured > 0
    assert product <= STEP_FACTOR * measured


@pytest.mark.parametrize("plant", [0, 1])
@pytest.mark.parametrize("max_iter", [20, 2])
def test_no_held_output_is_the_equilibrium_solve(plant, max_iter):
    p, u, x0 = EC.cases(plant)
    p, x0 = p.copy(), x0.copy()
    p[3] = EC.NO_EQUILIBRIUM
    xe, st, it, rs = cmpc.plant_equilibrium(plant, p, u, x0, max_iter=max_iter)
    xt, ut, st2, it2, rs2 = cmpc.plant_target(plant, p, [], [], np.zeros((len(x0), 0)), u, x0, max_iter=max_iter)
    assert len(set(st.tolist())) >= 2
    assert np.array_equal(bits(xt), bits(xe)) and np.array_equal(bits(ut), bits(u))
    assert np.array_equal(st2, st) and np.array_equal(it2, it)
    assert np.array_equal(bits(rs2[:, 0]), bits(rs)) and (rs2[:, 1] == 0).all()


def _untouched(res, x, u, rows):
    return np.array_equal(bits(res[0][rows]), bits(x[rows])) and np.array_equal(bits(res[1][rows]), bits(u[rows]))


def test_a_free_recycle_valve_at_zero_is_the_dead_zone():
    p, u, x, t = TC.cases(0, (0, 1), B=8)
    assert (u[:, [3, 7]] == 0).all()
    res = cmpc.plant_target(0, p, (0, 1), (1, 3), t, u, x)
    assert (res[2] == cmpc.CMPC_EQ_DEADZONE).all() and (res[3] == 0).all() and (res[4] == 0).all()
    assert _untouched(res, x, u, slice(None))
    # one valve free is enough; the same valve pinned is not in the way
    assert (cmpc.plant_target(0, p, (0, 1), (0, 3), t, u, x)[2] == cmpc.CMPC_EQ_DEADZONE).all()
    assert (cmpc.plant_target(0, p, (0, 1), (0, 2), t, u, x)[2] == cmpc.CMPC_EQ_OK).all()


def test_a_valve_that_crosses_into_the_dead_zone_stops():
    """The parallel plant with all four inputs free: the recycle valves start
    at 0.05 or more and some scenarios' Newton steps take one below 2e-2."""
    p, u, x, t = TC.cases(0, TC.ALL_FOUR[0], recycle=True)
    res = cmpc.plant_target(0, p, *TC.ALL_FOUR, t, u, x)
    st, it = res[2], res[3]
    print("statuses", np.bincount(st, minlength=6).tolist())
    dz = st == cmpc.CMPC_EQ_DEADZONE
    assert dz.sum() >= 2 and (it[dz] >= 1).all() and (u[:, [3, 7]] >= 0.05).all()
    assert set(st.tolist()) <= {cmpc.CMPC_EQ_OK, cmpc.CMPC_EQ_DEADZONE, cmpc.CMPC_EQ_NONFINITE}
    assert _untouched(res, x, u, st != cmpc.CMPC_EQ_OK)
    ok = st == cmpc.CMPC_EQ_OK
    assert ok.sum() >= 32
    assert np.abs(TC.outputs(0, res[0][ok]) - t[ok]).max() <= TOL_Y
    # the step before the crossing left a residual; one more iteration allowed
    # changes nothing, one fewer is NO_CONVERGENCE
    b = int(np.flatnonzero(dz)[np.argmax(it[dz])])
    one = lambda **kw: cmpc.plant_target(0, p[b:b + 1], *TC.ALL_FOUR, t[b:b + 1], u[b:b + 1], x[b:b + 1], **kw)
    alone = one()
    assert alone[2][0] == cmpc.CMPC_EQ_DEADZONE and alone[3][0] == it[b]
    assert np.array_equal(bits(alone[4]), bits(res[4][b:b + 1])) and (alone[4] > 0).all()
    assert one(max_iter=int(it[b]) - 1)[2][0] == cmpc.CMPC_EQ_NO_CONVERGENCE
    assert _untouched(alone, x[b:b + 1], u[b:b + 1], slice(None))


@pytest.mark.parametrize("plant", [0, 1])
def test_nonfinite_and_no_convergence_leave_the_inputs(plant):
    hold, free = ((0, 1), (0, 2)) if plant == 0 else ((1, 3), (0, 2))
    p, u, x, t = TC.cases(plant, hold, B=8)
    q = p.copy()
    q[0] = EC.NO_EQUILIBRIUM
    res = cmpc.plant_target(plant, q, hold, free, t, u, x)
    keep = np.arange(8) != 0
    assert res[2][0] == cmpc.CMPC_EQ_NONFINITE and (res[2][keep] == cmpc.CMPC_EQ_OK).all()
    assert _untouched(res, x, u, [0])
    good = cmpc.plant_target(plant, p, hold, free, t, u, x)
    for a, b in zip(res, good):
        assert np.array_equal(a[keep], b[keep])
    short = cmpc.plant_target(plant, p, hold, free, t, u, x, max_iter=2)
    assert (short[2] == cmpc.CMPC_EQ_NO_CONVERGENCE).all() and (short[3] == 2).all()
    assert _untouched(short, x, u, slice(None)) and (short[4].max(1) > 0).all()


def test_target_check_refuses_bad_arguments():
    lib = load_library()
    i32 = lambda v: np.ascontiguousarray(v, np.int32)
    good = dict(plant=0, nh=2, hold=i32([0, 1]), free=i32([0, 2]), max_iter=20, tol_f=1e-12, tol_y=1e-10)

    def rc(**kw):
        a = dict(good, **kw)
        return lib.cmpc_target_check(a["plant"], a["nh"], iptr(a["hold"]), iptr(a["free"]), a["max_iter"], a["tol_f"],
                                     a["tol_y"])

    assert rc() == 0
    assert rc(nh=0) == 0 and rc(nh=4, hold=i32([3, 2, 1, 0]), free=i32([1, 0, 3, 2])) == 0
    for kw, word in ((dict(plant=2), "plant"), (dict(plant=-1), "plant"), (dict(nh=-1), "nh"), (dict(nh=5), "nh"),
                     (dict(hold=i32([0, 0])), "hold_idx repeats"), (dict(free=i32([2, 2])), "free_idx repeats"),
                     (dict(hold=i32([0, 4])), "hold_idx[1]"), (dict(hold=i32([-1, 1])), "hold_idx[0]"),
                     (dict(free=i32([0, 4])), "free_idx[1]"), (dict(free=i32([-1, 2])), "free_idx[0]"),
                     (dict(max_iter=-1), "max_iter"), (dict(max_iter=65), "max_iter"),
                     (dict(tol_f=0.0), "tol_f"), (dict(tol_f=float("nan")), "tol_f"),
                     (dict(tol_f=float("inf")), "tol_f"), (dict(tol_y=-1.0), "tol_y"),
                     (dict(tol_y=float("nan")), "tol_y")):
        assert rc(**kw) < 0, kw
        msg = lib.cmpc_last_error().decode()
        assert "cmpc_target_check" in msg and word in msg, (kw, msg)
    assert lib.cmpc_target_check(0, 1, None, None, 20, 1e-12, 1e-10) < 0
    # the host entry point runs the same check before it touches anything
    p, u, x = EC.cases(0, B=2)
    with pytest.raises(RuntimeError, match="hold_idx repeats"):
        cmpc.plant_target(0, p, (1, 1), (0, 2), [4.5, 4.5], u, x)
    with pytest.raises(ValueError):
        cmpc.plant_target(0, p, (0, 1), (0,), [4.5, 4.5], u, x)
    with pytest.raises(ValueError):
        cmpc.plant_target(0, p, (0, 1), (0, 2), [4.5], u, x)
    st, it, r = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(4)
    h, f, t = i32([0, 1]), i32([0, 2]), np.full((2, 2), 4.5)
    xx, uu = x.copy(), u.copy()
    assert lib.cmpc_plant_target_host(0, 0, dptr(p), 2, iptr(h), iptr(f), dptr(t), dptr(uu), dptr(xx), 20, 1e-12, 1e-10,
                                      iptr(st), iptr(it), dptr(r)) < 0
    assert lib.cmpc_plant_target_host(0, 2, dptr(p), 2, iptr(h), iptr(f), None, dptr(uu), dptr(xx), 20, 1e-12, 1e-10,
                                      iptr(st), iptr(it), dptr(r)) < 0
    assert "null" in lib.cmpc_last_error().decode()
    assert np.array_equal(xx, x) and np.array_equal(uu, u)


def test_host_body_under_sanitizers():
    """csrc/target_body.h built with AddressSanitizer and UndefinedBehaviorSanitizer
    as a stand-alone program (host code only; tests/cpp/target_asan.cpp) and
    run for both plants and nh = 0 .. 4."""
    here = os.path.join(ROOT, "tests", "cpp")
    exe = os.path.join(here, "target_asan")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--cuda-host-only", "-O1", "-g",
                           "-std=c++17", "-Wall", "-ffp-contract=off", "-fno-omit-frame-pointer", "-Xarch_host",
                           "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined", "-o", exe,
                           os.path.join(here, "target_asan.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("target_asan ok"), r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-2000:]
