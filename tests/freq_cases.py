"""Inputs and models of the frequency-response tests (tests/test_freq.py,
tests/test_gpu_freq.py): the cases are those of
tests/gains_cases.py, the grid runs from rest past every pole of the plant, and
the models are C (j w I - A)^-1 [B | E] from the oracle's linearisation, in
numpy's complex128 and by a complex long-double elimination.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

import gains_cases as GC
import target_cases as TC

ALL = GC.ALL
bits = GC.bits
NAN_BITS = GC.NAN_BITS
cases = GC.cases
# rad/s: rest, then two decades either side of the poles (|lambda| = 0.14 .. 9.8)
GRID = np.array([0.0, 1e-2, 1e-1, 1.0, 3.16, 5.62, 10.0, 17.8, 31.6, 56.2, 100.0, 1000.0])
GRID.setflags(write=False)
# the bands of DESIGN.md §3.23's accuracy table, as index lists into GRID
BANDS = (("0 - 3.16", (0, 1, 2, 3, 4)), ("5.62 - 31.6", (5, 6, 7, 8)), ("56.2 - 100", (9, 10)), ("1000", (11,)))


def solve_longdouble(M, R):
    """M^-1 R for complex M (n, n) and R (n, k) in long double: Gaussian
    elimination with partial pivoting on |.|."""
    M = np.array(M, dtype=np.clongdouble)
    R = np.array(R, dtype=np.clongdouble)
    n = len(M)
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
            R[[k, p]] = R[[p, k]]
        for i in range(k + 1, n):
            m = M[i, k] / M[k, k]
            M[i, k:] -= m * M[k, k:]
            R[i] -= m * R[k]
    for k in range(n - 1, -1, -1):
        R[k] = (R[k] - M[k, k + 1:] @ R[k + 1:]) / M[k, k]
    return R


_lin = {}


def matrices(plant, b):
    """(A, B, C, E) of case b from the oracle's linearisation, E differenced at
    gains_body.h's step.  Computed once per case; read-only."""
    if (plant, b) not in _lin:
        p, u, x = cases(plant)
        A, Bm, C, _ = TC.or_linearize_full(plant, x[b], u[b], *p[b])
        E = GC.or_pressure_matrix(plant, x[b], u[b], *p[b])
        for m in (A, Bm, C, E):
            m.setflags(write=False)
        _lin[(plant, b)] = (A, Bm, C, E)
    return _lin[(plant, b)]


def model64(A, Bm, C, E, w):
    """[G | Gp] (4 x 6) at w through np.linalg.solve in complex128."""
    return C @ np.linalg.solve(1j * w * np.eye(len(A)) - A, np.hstack([Bm, E]).astype(np.complex128))


def model_ld(A, Bm, C, E, w):
    """The same by the long-double elimination."""
    n = len(A)
    M = (1j * np.longdouble(w)) * np.eye(n, dtype=np.clongdouble) - np.asarray(A, dtype=np.clongdouble)
    return np.asarray(C, dtype=np.clongdouble) @ solve_longdouble(M, np.hstack([Bm, E]))


def scaled_diff(a, b):
    """max |a - b| over max |b|, complex: the error scaled by the block's largest entry."""
    a = np.asarray(a, dtype=np.clongdouble)
    b = np.asarray(b, dtype=np.clongdouble)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def block(res, b, k):
    """[G | Gp] of scenario b at frequency k from a FreqResponse of the 4 x 4 selection."""
    return np.concatenate([res.G[b, k], res.Gp[b, k]], axis=1)
