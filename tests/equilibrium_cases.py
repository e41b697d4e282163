"""Inputs and models of the equilibrium tests (tests/test_equilibrium.py,
tests/test_gpu_equilibrium.py): the seeded pressure and input-offset cases, the
oracle's derivative and linearisation, and one Newton step in numpy's float64
and in long double.  TEST INFRASTRUCTURE ONLY."""
import ctypes

import numpy as np

import _oracle as O
import cmpc

SEED = 20261021
NS = {0: 11, 1: 10}
NI = {0: 9, 1: 8}
# the three pressure classes of the per-scenario and closed-loop tests
CLASSES = np.array([[1.0, 1.0], [0.97, 1.02], [1.03, 0.98]])
NO_EQUILIBRIUM = (1.0, 1.2)   # no forward-flow equilibrium: f is non-finite after a step or two


def oracle():
    """liboracle.so with the signatures of or_plant_derivative and
    or_plant_linearize (tests/_oracle.py declares neither for direct use)."""
    L = O.lib()
    P, d = ctypes.POINTER, ctypes.c_double
    L.or_plant_derivative.argtypes = [ctypes.c_int, d, d, P(d), P(d), P(d)]
    L.or_plant_linearize.argtypes = [ctypes.c_int, d, d, P(d), P(d), P(d), P(d), P(d), P(d)]
    return L


def or_derivative(plant, x, u, p_in=1.0, p_out=1.0):
    dx = np.zeros(NS[plant])
    oracle().or_plant_derivative(plant, p_in, p_out, O.dptr(np.ascontiguousarray(x, np.float64)),
                                 O.dptr(np.ascontiguousarray(u, np.float64)), O.dptr(dx))
    return dx


def or_linearize(plant, x, u, p_in=1.0, p_out=1.0):
    """(A ns x ns, f ns) of the oracle's continuous linearisation."""
    ns = NS[plant]
    A, B, C, f = np.zeros(ns * ns), np.zeros(ns * 4), np.zeros(4 * ns), np.zeros(ns)
    oracle().or_plant_linearize(plant, p_in, p_out, O.dptr(np.ascontiguousarray(x, np.float64)),
                                O.dptr(np.ascontiguousarray(u, np.float64)), O.dptr(A), O.dptr(B), O.dptr(C),
                                O.dptr(f))
    return A.reshape(ns, ns), f


def cases(plant, B=64, seed=SEED):
    """(pressures (B, 2), u_full (B, ni), x0 (B, ns)): pressures uniform in
    [0.95, 1.05]^2, an offset within 0.02 on every input that is nonzero in
    the default (the others stay zero), every scenario at cmpc_plant_default."""
    rng = np.random.default_rng(seed + plant)
    x0, u0 = cmpc.plant_default(plant)
    p = rng.uniform(0.95, 1.05, (B, 2))
    u = np.tile(u0, (B, 1)) + rng.uniform(-0.02, 0.02, (B, len(u0))) * (u0 != 0)
    return p, u, np.tile(x0, (B, 1))


def class_pressures(B):
    """The three classes dealt round-robin, (B, 2)."""
    return np.ascontiguousarray(CLASSES[np.arange(B) % len(CLASSES)])


def solve_longdouble(A, b):
    """Gaussian elimination with partial pivoting in numpy.longdouble."""
    A = np.array(A, dtype=np.longdouble)
    b = np.array(b, dtype=np.longdouble)
    n = len(b)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            b[[k, p]] = b[[p, k]]
        for i in range(k + 1, n):
            m = A[i, k] / A[k, k]
            A[i, k:] -= m * A[k, k:]
            b[i] -= m * b[k]
    x = np.zeros(n, dtype=np.longdouble)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def newton_step_models(plant, x, u, p_in, p_out):
    """x - A^-1 f from the oracle's linearisation: (numpy float64, long double)."""
    A, f = or_linearize(plant, x, u, p_in, p_out)
    x64 = x - np.linalg.solve(A, f)
    xld = np.asarray(x, dtype=np.longdouble) - solve_longdouble(A, f)
    return x64, xld


def rel_diff(a, b):
    """The largest |a_i - b_i| / |b_i| over the components with b_i != 0; a
    component that is zero in b must be zero in a."""
    a = np.asarray(a, dtype=np.longdouble)
    b = np.asarray(b, dtype=np.longdouble)
    nz = b != 0
    assert np.all(a[~nz] == 0)
    return float(np.max(np.abs(a[nz] - b[nz]) / np.abs(b[nz])))
