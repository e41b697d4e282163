"""Plant equilibrium on the host (cmpc_plant_equilibrium_host,
cmpc_plant_derivative, include/cmpc.h) against the oracle's
derivative and linearisation: the residual of the result, the statuses of
scenarios that do not converge, one Newton step against a dense model, and the
refusals.  No device."""
import ctypes

import numpy as np
import pytest

import cmpc
import equilibrium_cases as EC
from cmpc._abi import dptr, iptr, load_library

PLANTS = (0, 1)

# One Newton step, float64 numpy.linalg.solve against the long-double model,
# largest rel_diff over the 64 cases of equilibrium_cases.cases: parallel
# 1.61e-16, serial 1.31e-16 (the product's own step against the same model:
# 1.40e-16 and 1.04e-16).  The test measures the figure again and allows the
# product STEP_FACTOR times it.
STEP_FACTOR = 8.0


def _solve(plant, p, u, x0, max_iter=20, tol=1e-12):
    """The raw call: (rc, x, status, iters, resid)."""
    lib = load_library()
    c = lambda a: np.ascontiguousarray(a, np.float64)
    p, u, x = c(p), c(u), np.array(x0, dtype=np.float64, order="C")
    B = len(x)
    st, it, r = np.full(B, -7, np.int32), np.full(B, -7, np.int32), np.full(B, -7.0)
    rc = lib.cmpc_plant_equilibrium_host(plant, B, dptr(p), dptr(u), dptr(x), max_iter, tol, iptr(st), iptr(it),
                                         dptr(r))
    return rc, x, st, it, r


@pytest.mark.parametrize("plant", PLANTS)
def test_residual_against_the_oracle(plant):
    """B = 64 seeded cases from cmpc_plant_default: every status OK within 6
    iterations (plain Newton with LAPACK needs at most 5; one more for the
    different rounding of the product's own elimination), and the ORACLE's
    derivative at the returned state is within 1e-12."""
    p, u, x0 = EC.cases(plant)
    x, st, it, r = cmpc.plant_equilibrium(plant, p, u, x0)
    print("iters max", it.max(), "resid max", r.max())
    assert (st == cmpc.CMPC_EQ_OK).all(), st
    assert it.max() <= 6, it
    worst = max(np.abs(EC.or_derivative(plant, x[b], u[b], *p[b])).max() for b in range(len(x)))
    print("oracle max|f|", worst)
    assert worst <= 1e-12
    assert (r <= 1e-12).all()
    # the start is no equilibrium, so the solve has moved every state
    assert all(np.abs(EC.or_derivative(plant, x0[b], u[b], *p[b])).max() > 1e-3 for b in range(len(x)))


@pytest.mark.parametrize("plant", PLANTS)
def test_non_convergence_is_a_status(plant):
    x0, u0 = cmpc.plant_default(plant)
    # no forward-flow equilibrium: NONFINITE, the state untouched, no error
    rc, x, st, it, r = _solve(plant, [EC.NO_EQUILIBRIUM], [u0], [x0])
    assert rc == 0
    assert st[0] == cmpc.CMPC_EQ_NONFINITE and it[0] >= 1
    assert np.array_equal(x[0].view(np.uint64), x0.view(np.uint64))
    # one step from the default state is not enough: NO_CONVERGENCE, x restored
    rc, x, st, it, r = _solve(plant, [[1.0, 1.0]], [u0], [x0], max_iter=1)
    assert rc == 0
    assert st[0] == cmpc.CMPC_EQ_NO_CONVERGENCE and it[0] == 1 and 1e-12 < r[0] < 1e-2
    assert np.array_equal(x[0].view(np.uint64), x0.view(np.uint64))
    # max_iter = 0 only tests the state given
    rc, xe, st, it, r = _solve(plant, [[1.0, 1.0]], [u0], [x0])
    assert rc == 0 and st[0] == cmpc.CMPC_EQ_OK
    rc, x, st, it, r2 = _solve(plant, [[1.0, 1.0]], [u0], xe, max_iter=0)
    assert rc == 0 and st[0] == cmpc.CMPC_EQ_OK and it[0] == 0 and r2[0] == r[0]
    assert np.array_equal(x.view(np.uint64), xe.view(np.uint64))
    rc, x, st, it, r = _solve(plant, [[1.0, 1.0]], [u0], [x0], max_iter=0)
    assert rc == 0 and st[0] == cmpc.CMPC_EQ_NO_CONVERGENCE and it[0] == 0


def test_a_failing_scenario_is_contained_on_the_host():
    """Scenario 3 of 8 has no equilibrium: the other seven are what they are
    with scenario 3 at (1, 1)."""
    for plant in PLANTS:
        p, u, x0 = EC.cases(plant, B=8)
        q = p.copy()
        q[3] = EC.NO_EQUILIBRIUM
        p[3] = (1.0, 1.0)
        xa, sa, ia, ra = cmpc.plant_equilibrium(plant, p, u, x0)
        xb, sb, ib, rb = cmpc.plant_equilibrium(plant, q, u, x0)
        keep = np.arange(8) != 3
        assert sb[3] == cmpc.CMPC_EQ_NONFINITE and np.array_equal(xb[3], x0[3])
        assert (sa == cmpc.CMPC_EQ_OK).all() and (sb[keep] == cmpc.CMPC_EQ_OK).all()
        assert np.array_equal(xa[keep].view(np.uint64), xb[keep].view(np.uint64))
        assert np.array_equal(ia[keep], ib[keep]) and np.array_equal(ra[keep], rb[keep])


@pytest.mark.parametrize("plant", PLANTS)
def test_one_newton_step_against_a_dense_model(plant):
    """The state after exactly one Newton step from the default state against
    x - numpy.linalg.solve(A, f) with the oracle's A and f.  A call returns
    that state when tol lies between r(x0) and r(x1): r(x1) is at most 0.33
    r(x0) over these cases, so tol = r(x0) / 2 gives status OK with iters = 1.
    Tolerance: STEP_FACTOR times the largest distance of numpy's float64 step
    from the long-double step over the same cases (measured here)."""
    p, u, x0 = EC.cases(plant)
    measured = product = 0.0
    for b in range(len(x0)):
        r0 = np.abs(EC.or_derivative(plant, x0[b], u[b], *p[b])).max()
        rc, x, st, it, r = _solve(plant, p[b:b + 1], u[b:b + 1], x0[b:b + 1], max_iter=1, tol=0.5 * r0)
        assert rc == 0 and st[0] == cmpc.CMPC_EQ_OK and it[0] == 1, (b, st, it, r, r0)
        x64, xld = EC.newton_step_models(plant, x0[b], u[b], *p[b])
        measured = max(measured, EC.rel_diff(x64, xld))
        product = max(product, EC.rel_diff(x[0], xld))
    print("float64 numpy against long double", measured, "product against long double", product)
    assert measured > 0
    assert product <= STEP_FACTOR * measured


def test_argument_errors_are_refused():
    lib = load_library()
    plant = 0
    p, u, x0 = EC.cases(plant, B=2)
    st, it, r = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2)
    x = x0.copy()
    good = [plant, 2, dptr(p), dptr(u), dptr(x), 20, 1e-12, iptr(st), iptr(it), dptr(r)]

    def refused(i, v, word):
        a = list(good)
        a[i] = v
        assert lib.cmpc_plant_equilibrium_host(*a) < 0
        msg = lib.cmpc_last_error().decode()
        assert "cmpc_plant_equilibrium_host" in msg and word in msg, msg
        assert np.array_equal(x, x0)

    for i in (2, 3, 4, 7, 8, 9):
        refused(i, None, "null")
    refused(5, 65, "max_iter")
    refused(5, -1, "max_iter")
    refused(6, 0.0, "tol")
    refused(6, float("nan"), "tol")
    refused(6, float("inf"), "tol")
    refused(6, -1e-12, "tol")
    refused(0, 2, "plant")
    refused(1, 0, "B")
    assert lib.cmpc_plant_equilibrium_host(*good) == 0
    # the boundary values are accepted
    for mi in (0, 64):
        a = list(good)
        a[5] = mi
        assert lib.cmpc_plant_equilibrium_host(*a) == 0
    # the Python wrappers check the shapes
    with pytest.raises(ValueError):
        cmpc.plant_equilibrium(plant, p, u[:, :-1], x0)
    with pytest.raises(ValueError):
        cmpc.plant_derivative(plant, x0[0][:-1], u[0])
    x1, u1 = cmpc.plant_default(1)
    dx = np.zeros(10)
    assert lib.cmpc_plant_derivative(1, 1.0, 1.0, None, dptr(u1), dptr(dx)) < 0
    assert lib.cmpc_plant_derivative(2, 1.0, 1.0, dptr(x1), dptr(u1), dptr(dx)) < 0


@pytest.mark.parametrize("plant", PLANTS)
def test_derivative_equals_the_oracle_bit_for_bit(plant):
    rng = np.random.default_rng(EC.SEED + 10 + plant)
    x0, u0 = cmpc.plant_default(plant)
    for _ in range(16):
        x = x0 * (1 + 0.02 * rng.uniform(-1, 1, len(x0)))
        u = u0 + rng.uniform(-0.02, 0.02, len(u0)) * (u0 != 0)
        p_in, p_out = rng.uniform(0.95, 1.05, 2)
        a = cmpc.plant_derivative(plant, x, u, p_in, p_out)
        b = EC.or_derivative(plant, x, u, p_in, p_out)
        assert np.abs(b).max() > 0
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
