"""Inputs and models of the plant-mode tests (tests/test_modes.py,
tests/test_gpu_modes.py): the exact spectrum by mpmath at 50 digits, the
greedy matching of computed to exact eigenvalues, the error rule, the hard
matrices, and the summary's formulas in numpy.  TEST INFRASTRUCTURE ONLY."""
import mpmath
import numpy as np

SEED = 20261022
EPS = 2.0 ** -52
# The product's largest error may be EIG_FACTOR times the larger of numpy's
# largest error on the same matrix (measured again by every test) and a floor:
# the margin this project gives its own elimination over LAPACK (STEP_FACTOR
# in tests/test_equilibrium.py).
EIG_FACTOR = 8.0
NAN_BITS = np.uint64(0x7ff8000000000000)


def exact_spectrum(A):
    """The eigenvalues of A as mpmath numbers, from mpmath.eig at 50 digits."""
    if len(A) == 1:
        return [mpmath.mpc(float(np.asarray(A)[0][0]))]
    with mpmath.workdps(50):
        E = mpmath.eig(mpmath.matrix(np.asarray(A, dtype=np.float64).tolist()), left=False, right=False)
        return [mpmath.mpc(e) for e in E]


def match_errors(w, exact):
    """|w_k - e_k| as floats and the matched exact values, computed and exact
    eigenvalues matched greedily by nearest distance."""
    with mpmath.workdps(50):
        w = [mpmath.mpc(float(np.real(v)), float(np.imag(v))) for v in w]
        left = list(exact)
        assert len(w) == len(left)
        d = [[abs(a - b) for b in left] for a in w]
        rows, cols = set(range(len(w))), set(range(len(left)))
        err, at = [], []
        while rows:
            _, i, j = min((d[i][j], i, j) for i in rows for j in cols)
            err.append(float(d[i][j]))
            at.append(left[j])
            rows.discard(i)
            cols.discard(j)
        return np.array(err), at


def worst_error(w, exact, relative):
    err, at = match_errors(w, exact)
    if relative:
        err = err / np.array([float(abs(e)) for e in at])
    return float(err.max())


def allowed(A, exact, relative):
    """(bound, numpy's figure): EIG_FACTOR times the larger of numpy's own
    largest error and the floor n eps rho (rho the exact spectral radius; the
    backward-stable bound of a balanced matrix).  Under the relative rule
    every error is divided by its eigenvalue's modulus and the floor is n eps:
    the same bound relative to rho, the smallest it can be for any eigenvalue."""
    n = len(A)
    rho = max(float(abs(e)) for e in exact)
    ref = worst_error(np.linalg.eigvals(np.asarray(A, dtype=np.float64)), exact, relative)
    floor = n * EPS * (1.0 if relative else rho)
    return EIG_FACTOR * max(ref, floor), ref


def embed(H, n):
    """H in the leading block of an otherwise diagonal n x n matrix whose fill
    is distinct negative numbers."""
    H = np.atleast_2d(np.asarray(H, dtype=np.float64))
    k = len(H)
    A = np.zeros((n, n))
    A[:k, :k] = H
    for i in range(k, n):
        A[i, i] = -(3.0 + 0.5 * i)
    return A


def rot_blocks(ab):
    """Block diagonal of [[a, b], [-b, a]]."""
    n = 2 * len(ab)
    A = np.zeros((n, n))
    for k, (a, b) in enumerate(ab):
        A[2 * k:2 * k + 2, 2 * k:2 * k + 2] = [[a, b], [-b, a]]
    return A


def cycle(n):
    """The n-cycle permutation matrix: the plain double shift stalls on it."""
    P = np.zeros((n, n))
    for i in range(n):
        P[(i + 1) % n, i] = 1.0
    return P


def gaussian(n, seed=SEED):
    return np.random.default_rng(seed).standard_normal((n, n))


def badly_scaled(n, seed=SEED):
    """(M, D^-1 M D) with D = diag(2^k), k seeded in [-20, 20]: the scaling is
    exact, so both have M's spectrum."""
    rng = np.random.default_rng(seed + 1)
    M = gaussian(n, seed)
    d = 2.0 ** rng.integers(-20, 21, n)
    return M, M * d[None, :] / d[:, None]


def jordan(rotated, seed=SEED):
    """The 3 x 3 Jordan block at 2; rotated by a seeded orthogonal matrix."""
    J = np.array([[2.0, 1.0, 0.0], [0.0, 2.0, 1.0], [0.0, 0.0, 2.0]])
    if not rotated:
        return J
    Q, _ = np.linalg.qr(np.random.default_rng(seed + 2).standard_normal((3, 3)))
    return Q @ J @ Q.T


def triangular(k, seed=SEED):
    return np.triu(np.random.default_rng(seed + 3).standard_normal((k, k)))


BLOCKS = ((-0.5, 2.0), (-1.25, 0.75), (0.25, 3.0), (-2.0, 0.125), (1.5, 1.0))


def hard_matrices(n):
    """{name: n x n matrix} of the hard cases: the small ones embedded, the
    seeded Gaussian matrix and its badly scaled twin n x n."""
    M, S = badly_scaled(n)
    return {
        "zero": embed(np.zeros((4, 4)), n),
        "triangular": embed(triangular(6), n),
        "blocks": embed(rot_blocks(BLOCKS), n),
        "perm4": embed(cycle(4), n),
        "jordan": embed(jordan(False), n),
        "jordan_rotated": embed(jordan(True), n),
        "gaussian": M,
        "scaled": S,
    }


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def summary_numpy(wr, wi):
    """The six summary values of include/cmpc.h for one ordered spectrum, by
    the same operations in numpy's float64."""
    wr, wi = np.asarray(wr, np.float64), np.asarray(wi, np.float64)
    zeta, wd, wn, have = 1.0, 0.0, 0.0, False
    for a, b in zip(wr, wi):
        if b > 0:
            mod = np.sqrt(a * a + b * b)
            z = -a / mod
            if not have or z < zeta:
                zeta, wd, wn, have = z, b, mod, True
    return np.array([wr.max(), float((wr > 0).sum()), zeta, wd, wn, wr.min()])


def assert_order(wr, wi):
    """Real part descending, then imaginary part descending; a conjugate pair
    adjacent, + first, real parts bit-equal, imaginary parts negated."""
    n = len(wr)
    for k in range(n - 1):
        assert (wr[k], wi[k]) >= (wr[k + 1], wi[k + 1]), (k, wr, wi)
    k = 0
    while k < n:
        if wi[k] != 0:
            assert wi[k] > 0 and k + 1 < n, (k, wi)
            assert bits(wr[k]) == bits(wr[k + 1]) and bits(wi[k + 1]) == bits(-wi[k]), (k, wr, wi)
            k += 2
        else:
            k += 1
