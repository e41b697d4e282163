"""Eigenvalues of small matrices and the plant's modes on the host
(cmpc_eig_host, cmpc_plant_modes_host, cmpc_modes_summary_host, include/cmpc.h,
DESIGN.md §3.20) against the exact spectrum from mpmath at 50 digits, with
numpy.linalg.eigvals as the yardstick (tests/modes_cases.py has the rule).
No device.

numpy's own largest error against mpmath, as measured when this was written
(the tests measure it again): plant cases 4.9e-15 (parallel) and 6.4e-15
(serial), relative; random 11 x 11 2.7e-15; D^-1 M D 2.7e-15; perm4 4.5e-16;
the rotated Jordan block 2.5e-6.  The product's figures: DESIGN.md §3.20."""
import os
import subprocess

import numpy as np
import pytest

import cmpc
import equilibrium_cases as EC
import modes_cases as MC
from cmpc._abi import dptr, iptr, load_library

PLANTS = (0, 1)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PLANT_CASES = 32   # of the 64 of equilibrium_cases.cases: mpmath takes most of the time


def trimmed(plant, B=64):
    p, u, x0 = EC.cases(plant, B=B)
    x, st, _, _ = cmpc.plant_equilibrium(plant, p, u, x0)
    assert (st == cmpc.CMPC_EQ_OK).all()
    return p, u, x


@pytest.mark.parametrize("plant", PLANTS)
def test_plant_modes_against_the_exact_spectrum(plant):
    """The seeded cases at their equilibria: status OK everywhere, every
    eigenvalue within the relative rule of the exact spectrum of the ORACLE's
    Jacobian, and what was observed of these plants: stable, two oscillatory
    pairs, the least damping ratio inside (0.2, 0.7)."""
    p, u, x = trimmed(plant)
    w, sm, st, it = cmpc.plant_modes(plant, p, u, x)
    assert (st == cmpc.CMPC_EIG_OK).all(), st
    assert (it <= 30 * EC.NS[plant]).all() and it.min() >= 4
    assert (sm[:, 1] == 0).all()                       # n_unstable
    assert ((w.imag > 0).sum(axis=1) == 2).all()
    assert ((sm[:, 2] > 0.2) & (sm[:, 2] < 0.7)).all(), sm[:, 2]
    assert (sm[:, 0] < -0.05).all() and (sm[:, 0] > -0.2).all()
    product = yard = smallest = 0.0
    for b in range(N_PLANT_CASES):
        A, _ = EC.or_linearize(plant, x[b], u[b], *p[b])
        exact = MC.exact_spectrum(A)
        bound, ref = MC.allowed(A, exact, relative=True)
        err = MC.worst_error(w[b], exact, relative=True)
        product, yard = max(product, err), max(yard, ref)
        smallest = min([smallest or 1.0] + [float(abs(e)) for e in exact])
        assert err <= bound, (b, err, bound)
    print("relative error against mpmath: product", product, "numpy", yard, "smallest modulus", smallest)
    assert smallest > 0.05


def test_damping_falls_with_the_discharge_pressure():
    """The parallel plant at (p_in, p_out) = (1.0, 1.1) is closer to surge than
    at (1.0, 0.9)."""
    x0, u0 = cmpc.plant_default(0)
    p = np.array([[1.0, 0.9], [1.0, 1.1]])
    u, xs = np.tile(u0, (2, 1)), np.tile(x0, (2, 1))
    x, st, _, _ = cmpc.plant_equilibrium(0, p, u, xs)
    assert (st == cmpc.CMPC_EQ_OK).all()
    _, sm, st, _ = cmpc.plant_modes(0, p, u, x)
    assert (st == cmpc.CMPC_EIG_OK).all()
    print("zeta_min at p_out 0.9 and 1.1:", sm[:, 2])
    assert sm[1, 2] < sm[0, 2]


HARD = ("zero", "triangular", "blocks", "perm4", "jordan", "jordan_rotated", "gaussian", "scaled")


@pytest.mark.parametrize("n", [10, 11])
@pytest.mark.parametrize("name", HARD)
def test_hard_matrices(name, n):
    A = MC.hard_matrices(n)[name]
    w, st, it = cmpc.eig_batch(A[None])
    assert st[0] == cmpc.CMPC_EIG_OK and 0 <= it[0] <= 30 * n
    MC.assert_order(w[0].real, w[0].imag)
    if name in ("zero", "triangular"):
        # exactly the diagonal, as numpy returns it
        want = np.linalg.eigvals(A)
        assert np.array_equal(np.sort(want), np.sort(np.diag(A))) and it[0] == 0
        assert np.array_equal(MC.bits(np.sort(w[0].real)), MC.bits(np.sort(want)))
        assert (w[0].imag == 0).all()
        return
    exact = MC.exact_spectrum(MC.badly_scaled(n)[0] if name == "scaled" else A)
    bound, ref = MC.allowed(A, exact, relative=False)
    err = MC.worst_error(w[0], exact, relative=False)
    print(name, n, "absolute error against mpmath: product", err, "numpy", ref, "allowed", bound, "iters", it[0])
    assert err <= bound
    if name == "perm4":
        roots = sorted(w[0][:4], key=lambda v: (-v.real, -v.imag))
        assert np.allclose(roots, [1, 1j, -1j, -1], atol=1e-14)
        assert it[0] > 10     # the plain double shift alone does not get there
    if name == "scaled":
        assert bound < 2e-13


@pytest.mark.parametrize("n", [1, 2, 3, 12])
def test_the_edges_of_the_size_range(n):
    mats = [MC.gaussian(n), np.zeros((n, n)), MC.cycle(n), MC.badly_scaled(n)[1]]
    w, st, it = cmpc.eig_batch(np.stack(mats))
    assert (st == cmpc.CMPC_EIG_OK).all() and (it <= 30 * n).all()
    for k, A in enumerate(mats):
        MC.assert_order(w[k].real, w[k].imag)
        exact = MC.exact_spectrum(MC.badly_scaled(n)[0] if k == 3 else A)
        bound, _ = MC.allowed(A, exact, relative=False)
        assert MC.worst_error(w[k], exact, relative=False) <= bound, (n, k)
    assert (w[1] == 0).all()


def test_order_and_summary():
    """Pairs adjacent, + first; the summary bit for bit by the same formulas
    in numpy; a known count of right-half-plane eigenvalues."""
    p, u, x = trimmed(0, B=8)
    w, sm, st, _ = cmpc.plant_modes(0, p, u, x)
    for b in range(8):
        MC.assert_order(w[b].real, w[b].imag)
        assert np.array_equal(MC.bits(sm[b]), MC.bits(MC.summary_numpy(w[b].real, w[b].imag)))
    assert np.array_equal(MC.bits(cmpc.modes_summary(w, st)), MC.bits(sm))
    # diag(1, 2, -1, ...) and one unstable rotation block: four in the right half plane
    A = np.diag([1.0, 2.0, -1.0, -1.5, -2.5, -3.0, -4.0, -5.0, 0.0, 0.0])
    A[8:, 8:] = [[0.5, 3.0], [-3.0, 0.5]]
    w, st, _ = cmpc.eig_batch(A[None])
    s = cmpc.modes_summary(w, st)[0]
    MC.assert_order(w[0].real, w[0].imag)
    assert np.array_equal(MC.bits(s), MC.bits(MC.summary_numpy(w[0].real, w[0].imag)))
    assert s[1] == 4 and s[0] == 2.0 and s[5] == -5.0
    assert s[3] == 3.0 and s[2] == -0.5 / np.sqrt(0.25 + 9.0) and s[4] == np.sqrt(0.25 + 9.0)
    # no oscillatory mode: zeta 1, both frequencies 0
    w, st, _ = cmpc.eig_batch(np.diag([-1.0, -2.0, 3.0])[None])
    assert np.array_equal(cmpc.modes_summary(w, st)[0], [3.0, 1.0, 1.0, 0.0, 0.0, -2.0])


def test_statuses():
    n = 11
    M = MC.gaussian(n)
    for bad in (np.nan, np.inf, -np.inf):
        batch = np.stack([M, M, M.T])
        good = cmpc.eig_batch(batch)
        batch[1, 4, 7] = bad
        w, st, it = cmpc.eig_batch(batch)
        assert list(st) == [cmpc.CMPC_EIG_OK, cmpc.CMPC_EIG_NONFINITE, cmpc.CMPC_EIG_OK] and it[1] == 0
        assert (MC.bits(w[1].real) == MC.NAN_BITS).all() and (MC.bits(w[1].imag) == MC.NAN_BITS).all()
        assert (MC.bits(cmpc.modes_summary(w, st)[1]) == MC.NAN_BITS).all()
        # the neighbours are what they are without it
        for k in (0, 2):
            assert np.array_equal(MC.bits(w[k].real), MC.bits(good[0][k].real))
            assert np.array_equal(MC.bits(w[k].imag), MC.bits(good[0][k].imag))
            assert it[k] == good[2][k]
    w, st, it = cmpc.eig_batch(M[None], max_iter=1)
    assert st[0] == cmpc.CMPC_EIG_NO_CONVERGENCE and it[0] == 1
    assert (MC.bits(w[0].real) == MC.NAN_BITS).all() and (MC.bits(w[0].imag) == MC.NAN_BITS).all()
    assert (MC.bits(cmpc.modes_summary(w, st)[0]) == MC.NAN_BITS).all()
    full = cmpc.eig_batch(M[None])[2][0]
    for cap in (2, 5, full - 1, full, cmpc.CMPC_EIG_MAX_ITER):
        w, st, it = cmpc.eig_batch(M[None], max_iter=cap)
        assert it[0] <= cap and (st[0] == cmpc.CMPC_EIG_OK) == (cap >= full)
    # a state that is not finite: the plant's Jacobian is not either
    x0, u0 = cmpc.plant_default(1)
    xs = np.stack([x0, x0])
    xs[1, 2] = np.nan
    w, sm, st, it = cmpc.plant_modes(1, np.ones((2, 2)), np.stack([u0, u0]), xs)
    assert list(st) == [cmpc.CMPC_EIG_OK, cmpc.CMPC_EIG_NONFINITE]
    assert (MC.bits(sm[1]) == MC.NAN_BITS).all() and (MC.bits(w[1].real) == MC.NAN_BITS).all()


def test_argument_errors_are_refused():
    lib = load_library()
    n, B = 11, 2
    A = np.stack([MC.gaussian(n), MC.gaussian(n).T])
    wr, wi = np.zeros((B, n)), np.zeros((B, n))
    st, it = np.zeros(B, np.int32), np.zeros(B, np.int32)

    def refused(fn, name, good, i, v, word):
        a = list(good)
        a[i] = v
        assert fn(*a) < 0
        msg = lib.cmpc_last_error().decode()
        assert name in msg and word in msg, msg

    good = [n, B, dptr(A), 30 * n, dptr(wr), dptr(wi), iptr(st), iptr(it)]
    for i in (2, 4, 5, 6, 7):
        refused(lib.cmpc_eig_host, "cmpc_eig_host", good, i, None, "null")
    for v in (0, 13, -1):
        refused(lib.cmpc_eig_host, "cmpc_eig_host", good, 0, v, "n must")
    refused(lib.cmpc_eig_host, "cmpc_eig_host", good, 1, 0, "B")
    for v in (0, -1, cmpc.CMPC_EIG_MAX_ITER + 1):
        refused(lib.cmpc_eig_host, "cmpc_eig_host", good, 3, v, "max_iter")
    assert (wr == 0).all() and (st == 0).all()
    for mi in (1, cmpc.CMPC_EIG_MAX_ITER):
        a = list(good)
        a[3] = mi
        assert lib.cmpc_eig_host(*a) == 0

    plant = 0
    p, u, x = EC.cases(plant, B=B)
    sm = np.zeros((B, 6))
    good = [plant, B, dptr(p), dptr(u), dptr(x), 330, dptr(wr), dptr(wi), dptr(sm), iptr(st), iptr(it)]
    name = "cmpc_plant_modes_host"
    for i in (2, 3, 4, 6, 7, 8, 9, 10):
        refused(lib.cmpc_plant_modes_host, name, good, i, None, "null")
    refused(lib.cmpc_plant_modes_host, name, good, 0, 2, "plant")
    refused(lib.cmpc_plant_modes_host, name, good, 1, 0, "B")
    for v in (0, 361):
        refused(lib.cmpc_plant_modes_host, name, good, 5, v, "max_iter")
    assert lib.cmpc_plant_modes_host(*good) == 0

    good = [n, B, dptr(wr), dptr(wi), iptr(st), dptr(sm)]
    name = "cmpc_modes_summary_host"
    for i in (2, 3, 4, 5):
        refused(lib.cmpc_modes_summary_host, name, good, i, None, "null")
    refused(lib.cmpc_modes_summary_host, name, good, 0, 13, "n must")
    refused(lib.cmpc_modes_summary_host, name, good, 1, 0, "B")
    assert lib.cmpc_modes_summary_host(*good) == 0

    # the device entry points refuse before they touch a device
    refused(lib.cmpc_eig_device, "cmpc_eig_device", [n, B, None, 330, None, None, None, None, None], 0, 12, "n must")
    refused(lib.cmpc_eig_device, "cmpc_eig_device", [n, B, None, 330, None, None, None, None, None], 0, n, "null")
    assert lib.cmpc_sim_modes(None, 330) < 0 and "cmpc_sim_modes" in lib.cmpc_last_error().decode()
    assert lib.cmpc_sim_modes_download(None, None, None, None, None, None) < 0
    assert lib.cmpc_sim_modes_status(None) is None

    # the Python wrappers check the shapes
    with pytest.raises(ValueError):
        cmpc.eig_batch(np.zeros((2, 3, 4)))
    with pytest.raises(ValueError):
        cmpc.eig_batch(np.zeros((3, 3)))
    with pytest.raises(ValueError):
        cmpc.eig_batch(np.zeros((1, 13, 13)))
    with pytest.raises(ValueError):
        cmpc.plant_modes(plant, p, u[:, :-1], x)
    with pytest.raises(ValueError):
        cmpc.plant_modes(plant, p[:1], u, x)
    with pytest.raises(ValueError):
        cmpc.modes_summary(np.zeros((2, 3), complex), np.zeros(3, np.int32))
    with pytest.raises(RuntimeError, match="max_iter"):
        cmpc.eig_batch(A, max_iter=0)


def test_host_body_under_sanitizers():
    """csrc/eig_body.h built with AddressSanitizer and UndefinedBehaviorSanitizer
    as a stand-alone program (host code only; tests/cpp/eig_asan.cpp) and run
    over random and hard matrices for every n from 1 to 12."""
    here = os.path.join(ROOT, "tests", "cpp")
    exe = os.path.join(here, "eig_asan")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--cuda-host-only", "-O1", "-g",
                           "-std=c++17", "-Wall", "-ffp-contract=off", "-fno-omit-frame-pointer", "-Xarch_host",
                           "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined", "-o", exe,
                           os.path.join(here, "eig_asan.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("eig_asan ok"), r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-2000:]
