"""The plant frequency responses on the host (cmpc_plant_freq_host,
cmpc_freq_host, csrc/freq_body.h): G(jw) and Gp(jw) against
the oracle's linearisation solved by numpy and by a complex long-double
elimination, the same without the balancing (reported), w = 0 against the
steady-state gains, the structure of the record and the summary for every
selection shape, the order of the list, analytic systems through the
matrix-level call, every status, every refusal of cmpc_freq_check, and the body
under ASan + UBSan.  CPU only.

Measured on the 64 seeded cases per plant, 4 x 4 selection, the error of
[G | Gp] against long double scaled by the block's largest entry, the worst
case of both plants per band of the grid (DESIGN.md §3.23 has the reading):
  band (rad/s)   unbalanced   numpy complex128   the product
  0 - 3.16       8.5e-15      1.3e-15            1.4e-15
  5.62 - 31.6    8.2e-14      1.8e-14            8.2e-16
  56.2 - 100     3.6e-16      1.3e-13            3.8e-16
  1000           2.4e-16      4.8e-16            3.3e-16
(unbalanced: the same elimination in Python floats on 16 cases per plant.)
"""
import os
import subprocess

import numpy as np
import pytest

import cmpc
import freq_cases as FC
import gains_cases as GC
from cmpc._abi import dptr, iptr, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_FACTOR = 8.0    # the product against numpy's measured error or ns eps (DESIGN.md §3.20's rule and margin)
EPS = 2.0 ** -52
OK = cmpc.CMPC_EQ_OK
bits = GC.bits
ALL = GC.ALL


def _all_nan(a):
    return bool((bits(a) == GC.NAN_BITS).all())


def _parts(z):
    """(re, im) of a complex array as one float array, for bit comparisons."""
    z = np.asarray(z)
    return np.stack([z.real, z.imag], axis=-1)


_full = {}


def full(plant):
    """The 4 x 4 response of every case on the grid.  Computed once; read-only."""
    if plant not in _full:
        p, u, x = GC.cases(plant)
        _full[plant] = cmpc.plant_freq_response(plant, p, u, x, FC.GRID, ALL, ALL)
    return _full[plant]


def unbalanced(A, Bm, C, E, w):
    """[G | Gp] at w by the product's elimination as it stands on A - j w I,
    no balancing: the adjoint solve with the first largest |re| + |im| as
    pivot, in Python's complex floats.  A restatement for DESIGN.md's table."""
    n = len(A)
    col = [[complex(A[j][i]) - (1j * w if i == j else 0) for i in range(n)] for j in range(n)]
    col += [[complex(C[r][i]) for i in range(n)] for r in range(4)]
    for k in range(n):
        p = max(range(k, n), key=lambda i: (abs(col[k][i].real) + abs(col[k][i].imag), -i))
        for c in col[k:]:
            c[k], c[p] = c[p], c[k]
        for i in range(k + 1, n):
            m = col[k][i] / col[k][k]
            for c in col[k + 1:]:
                c[i] -= m * c[k]
    R = np.hstack([Bm, E])
    out = np.zeros((4, 6), np.complex128)
    for r in range(4):
        z = col[n + r]
        for k in range(n - 1, -1, -1):
            z[k] = z[k] / col[k][k]
            for i in range(k):
                z[i] -= col[k][i] * z[k]
        for q in range(6):
            out[r, q] = -sum(z[k] * R[k, q] for k in range(n))
    return out


@pytest.mark.parametrize("plant", [0, 1])
def test_response_against_the_oracle_linearisation(plant):
    """[G | Gp] of the 4 x 4 selection at every grid frequency against the
    same from the oracle's A, B, C and its differenced E.  Tolerance, per
    frequency: MODEL_FACTOR times the larger of numpy's distance from the
    long-double result over the same cases (measured here) and ns eps, all
    scaled by the block's largest entry."""
    res = full(plant)
    assert (res.status == OK).all(), res.status
    assert (res.resid <= 1e-12).all()
    ns = 11 if plant == 0 else 10
    nw = len(FC.GRID)
    measured, product, plain = np.zeros(nw), np.zeros(nw), np.zeros(nw)
    for b in range(64):
        mats = FC.matrices(plant, b)
        for k, w in enumerate(FC.GRID):
            ld = FC.model_ld(*mats, w)
            measured[k] = max(measured[k], FC.scaled_diff(FC.model64(*mats, w), ld))
            product[k] = max(product[k], FC.scaled_diff(FC.block(res, b, k), ld))
            if b < 16:
                plain[k] = max(plain[k], FC.scaled_diff(unbalanced(*mats, w), ld))
    for name, idx in FC.BANDS:
        idx = list(idx)
        print(f"plant {plant} band {name}: unbalanced {plain[idx].max():.1e}, numpy complex128 "
              f"{measured[idx].max():.1e}, product {product[idx].max():.1e}")
    for k, w in enumerate(FC.GRID):
        assert measured[k] > 0
        assert product[k] <= MODEL_FACTOR * max(measured[k], ns * EPS), (w, product[k], measured[k])


@pytest.mark.parametrize("plant", [0, 1])
def test_rest_is_the_steady_state_gains(plant):
    """w = 0: every imaginary part is a zero, and the real parts are the
    steady-state gains' G and Gp within the sum of the two tests' allowances
    (each MODEL_FACTOR times numpy's own error, measured here; for the response
    not less than ns eps)."""
    p, u, x = GC.cases(plant)
    res, g = full(plant), cmpc.plant_gains(plant, p, u, x, ALL, ALL)
    ns = x.shape[1]
    assert (res.G[:, 0].imag == 0).all() and (res.Gp[:, 0].imag == 0).all()
    gain_err, freq_err = {"G": 0.0, "Gp": 0.0}, 0.0
    for b in range(64):
        m64, mld = GC.gain_models(plant, x[b], u[b], *p[b])
        for key in gain_err:
            gain_err[key] = max(gain_err[key], GC.scaled_diff(m64[key], mld[key]))
        mats = FC.matrices(plant, b)
        freq_err = max(freq_err, FC.scaled_diff(FC.model64(*mats, 0.0), FC.model_ld(*mats, 0.0)))
    for key, got in (("G", res.G[:, 0].real), ("Gp", res.Gp[:, 0].real)):
        allow = MODEL_FACTOR * gain_err[key] + MODEL_FACTOR * max(freq_err, ns * EPS)
        worst = max(GC.scaled_diff(got[b], getattr(g, key)[b]) for b in range(64))
        print(f"plant {plant} {key} at rest: {worst:.2e} from plant_gains, allowed {allow:.2e}")
        assert worst <= allow


@pytest.mark.parametrize("plant", [0, 1])
def test_record_layout_of_every_selection(plant):
    """A sub-selection's entries are the 4 x 4 result's bit for bit at every
    frequency (the balancing and each column of Z do not depend on the
    selection); everything outside ny / nu is the one quiet NaN."""
    p, u, x = GC.cases(plant)
    whole = full(plant)
    assert not np.isnan(whole.record).any() and not np.isnan(whole.summary).any()
    nw = len(FC.GRID)
    for outs, ins in GC.SELECTIONS + (((2, 0), (3, 1)), ((3,), (2,)), ((1, 3), (0, 1, 2))):
        ny, nu = len(outs), len(ins)
        res = cmpc.plant_freq_response(plant, p, u, x, FC.GRID, outs, ins)
        assert (res.status == OK).all(), (outs, ins, res.status)
        assert res.G.shape == (64, nw, ny, nu) and res.Gp.shape == (64, nw, ny, 2)
        assert res.peak.shape == res.peak_omega.shape == (64, ny, nu)
        assert res.peak_p.shape == res.peak_p_omega.shape == (64, ny, 2)
        sub = lambda a: a[..., list(outs), :]
        assert np.array_equal(bits(_parts(res.G)), bits(_parts(sub(whole.G)[..., list(ins)])))
        assert np.array_equal(bits(_parts(res.Gp)), bits(_parts(sub(whole.Gp))))
        assert np.array_equal(bits(res.peak), bits(sub(whole.peak)[..., list(ins)]))
        assert np.array_equal(bits(res.peak_omega), bits(sub(whole.peak_omega)[..., list(ins)]))
        assert np.array_equal(bits(res.peak_p), bits(sub(whole.peak_p)))
        assert np.array_equal(bits(res.peak_p_omega), bits(sub(whole.peak_p_omega)))
        assert np.array_equal(bits(res.resid), bits(whole.resid))
        G4, Gp4 = res.record[..., :32].reshape(64, nw, 4, 4, 2), res.record[..., 32:].reshape(64, nw, 4, 2, 2)
        assert _all_nan(G4[:, :, ny:]) and _all_nan(G4[:, :, :, nu:]) and _all_nan(Gp4[:, :, ny:])
        assert not np.isnan(G4[:, :, :ny, :nu]).any() and not np.isnan(Gp4[:, :, :ny]).any()
        for lo in (0, 24):
            S4, Sp4 = res.summary[:, lo:lo + 16].reshape(64, 4, 4), res.summary[:, lo + 16:lo + 24].reshape(64, 4, 2)
            assert _all_nan(S4[:, ny:]) and _all_nan(S4[:, :, nu:]) and _all_nan(Sp4[:, ny:])
            assert not np.isnan(S4[:, :ny, :nu]).any() and not np.isnan(Sp4[:, :ny]).any()
        # the peak is the largest re re + im im of the list, its index the first that has it
        m2 = res.G.real * res.G.real + res.G.imag * res.G.imag
        assert np.array_equal(res.summary[:, :16].reshape(64, 4, 4)[:, :ny, :nu], m2.max(axis=1))
        assert np.array_equal(res.summary[:, 24:40].reshape(64, 4, 4)[:, :ny, :nu], m2.argmax(axis=1))


@pytest.mark.parametrize("plant", [0, 1])
def test_the_order_of_the_list_is_the_order_of_the_record(plant):
    p, u, x = GC.cases(plant, B=8)
    sel = GC.SELECTIONS[1]
    base = cmpc.plant_freq_response(plant, p, u, x, FC.GRID, *sel)
    perm = np.random.default_rng(5).permutation(len(FC.GRID))
    mixed = cmpc.plant_freq_response(plant, p, u, x, FC.GRID[perm], *sel)
    assert np.array_equal(bits(mixed.record), bits(base.record[:, perm]))
    assert np.array_equal(bits(mixed.summary[:, :24]), bits(base.summary[:, :24]))
    assert np.array_equal(bits(mixed.peak_omega), bits(base.peak_omega))
    # a repeated frequency: equal records, and the peak keeps the lower index
    twice = cmpc.plant_freq_response(plant, p, u, x, np.concatenate([FC.GRID, FC.GRID]), *sel)
    assert np.array_equal(bits(twice.record[:, :12]), bits(base.record))
    assert np.array_equal(bits(twice.record[:, 12:]), bits(base.record))
    assert np.array_equal(bits(twice.summary), bits(base.summary))
    same = cmpc.plant_freq_response(plant, p, u, x, [5.62, 5.62, 5.62], *sel)
    assert (same.summary[:, 24:48][~np.isnan(same.summary[:, 24:48])] == 0).all()


def _scaled(got, want):
    return float(np.max(np.abs(np.asarray(got, np.clongdouble) - want)) / np.max(np.abs(want)))


def test_first_order_lag():
    a = 2.0
    w = FC.GRID
    res = cmpc.freq_response([[-a]], [[1.0]], [[1.0]], np.zeros((1, 2)), w)
    assert res.status.tolist() == [OK] and res.G.shape == (1, 12, 1, 1) and res.resid[0] == 0
    want = 1 / (1j * w.astype(np.longdouble) + a)
    for k in range(len(w)):
        assert _scaled(res.G[0, k, 0, 0], want[k]) <= MODEL_FACTOR * 1 * EPS, w[k]
    assert (res.Gp == 0).all() and res.peak[0, 0, 0] == 0.5 and res.peak_omega[0, 0, 0] == 0.0
    assert _all_nan(res.record[0, :, 2:32]) and _all_nan(res.record[0, :, 36:])


@pytest.mark.parametrize("shift", [0, 20])
def test_second_order_resonance(shift):
    """x'' + 2 zeta wn x' + wn^2 x = u, zeta = 0.1, wn = 5; with shift = 20 the
    second state is measured in units 2^20 times smaller (D = diag(1, 2^20)),
    which the balancing undoes: the same accuracy."""
    wn, zeta, d = 5.0, 0.1, 2.0 ** shift
    A = np.array([[0, 1.0], [-wn * wn, -2 * zeta * wn]])
    Bm, C = np.array([[0.0], [1.0]]), np.array([[1.0, 0.0]])
    D, Di = np.diag([1.0, d]), np.diag([1.0, 1 / d])
    w = FC.GRID
    res = cmpc.freq_response(Di @ A @ D, Di @ Bm, C @ D, np.zeros((2, 2)), w)
    assert res.status.tolist() == [OK]
    wl = w.astype(np.longdouble)
    want = 1 / (np.longdouble(wn) ** 2 - wl * wl + 2j * np.longdouble(zeta) * wn * wl)
    errs = [_scaled(res.G[0, k, 0, 0], want[k]) for k in range(len(w))]
    print(f"second order, shift {shift}: worst {max(errs):.2e} of {MODEL_FACTOR * 2 * EPS:.2e}")
    assert max(errs) <= MODEL_FACTOR * 2 * EPS, errs
    nearest = int(np.argmin(np.abs(w - wn * np.sqrt(1 - 2 * zeta * zeta))))
    assert res.summary[0, 24] == nearest and res.peak_omega[0, 0, 0] == w[nearest] == 5.62
    g = res.G[0, :, 0, 0]
    assert res.peak[0, 0, 0] == np.sqrt(g.real * g.real + g.imag * g.imag).max()


def test_a_frequency_on_a_pole_is_singular():
    """The undamped oscillator at w = 1: the second pivot cancels exactly.
    One such frequency in the list is the scenario's status, all NaN."""
    A = [[0, 1.0], [-1.0, 0]]
    args = (A, [[0.0], [1.0]], [[1.0, 0.0]], np.zeros((2, 2)))
    res = cmpc.freq_response(*args, [0.5, 1.0, 2.0])
    assert res.status.tolist() == [cmpc.CMPC_EQ_SINGULAR] and _all_nan(res.record) and _all_nan(res.summary)
    off = cmpc.freq_response(*args, [0.5, 2.0])
    assert off.status.tolist() == [OK]
    assert _scaled(off.G[0, :, 0, 0], 1 / (1 - np.array([0.25, 4.0], np.longdouble))) <= MODEL_FACTOR * 2 * EPS


def test_a_nan_entry_is_nonfinite():
    A = np.array([[-1.0, 0.5], [0.25, -2.0]])
    Bm, C, E = np.ones((2, 2)), np.ones((3, 2)), np.ones((2, 2))
    good = cmpc.freq_response(A, Bm, C, E, [1.0])
    assert good.status.tolist() == [OK] and good.G.shape == (1, 1, 3, 2) and not np.isnan(good.Gp.real).any()
    for which in range(4):
        mats = [A.copy(), Bm.copy(), C.copy(), E.copy()]
        mats[which][1, 0] = np.nan if which % 2 else np.inf
        res = cmpc.freq_response(*mats, [1.0])
        assert res.status.tolist() == [cmpc.CMPC_EQ_NONFINITE] and _all_nan(res.record) and _all_nan(res.summary)
    # an entry that overflows when the balancing scales it
    big = cmpc.freq_response([[-1.0, 2.0 ** 900], [2.0 ** -900, -1.0]], [[1e300], [1e300]], [[1e300, 1e300]],
                             np.zeros((2, 2)), [1.0])
    assert big.status.tolist() == [cmpc.CMPC_EQ_NONFINITE] and _all_nan(big.record)
    # a batch keeps its members apart
    both = cmpc.freq_response(np.stack([A, np.full((2, 2), np.nan)]), np.stack([Bm, Bm]), np.stack([C, C]),
                              np.stack([E, E]), [1.0])
    assert both.status.tolist() == [OK, cmpc.CMPC_EQ_NONFINITE]
    assert np.array_equal(bits(both.record[0]), bits(good.record[0]))


def test_a_selected_recycle_valve_in_the_dead_zone():
    p, u, x = GC.cases(0, B=8)
    u = u.copy()
    u[:, 3] = 0.01
    res = cmpc.plant_freq_response(0, p, u, x, FC.GRID, (0, 1), (0, 1))
    assert (res.status == cmpc.CMPC_EQ_DEADZONE).all() and _all_nan(res.record) and _all_nan(res.summary)
    ps, us, xs = GC.cases(1, B=8)
    us = us.copy()
    us[:, 7] = 0.0
    assert (cmpc.plant_freq_response(1, ps, us, xs, [1.0], ALL, ALL).status == cmpc.CMPC_EQ_DEADZONE).all()
    assert (cmpc.plant_freq_response(1, ps, us, xs, [1.0], ALL, (0, 1, 2)).status == OK).all()
    # the same valve not selected is not in the way: its B column is never read
    free = cmpc.plant_freq_response(0, p, u, x, FC.GRID, (0, 1), (0, 2))
    assert (free.status == OK).all() and not np.isnan(free.G.real).any() and (free.resid > 0).all()


@pytest.mark.parametrize("plant", [0, 1])
def test_a_nan_state_is_nonfinite(plant):
    p, u, x = GC.cases(plant, B=8)
    x = x.copy()
    x[2, 3] = np.nan
    x[5, 0] = np.inf
    res = cmpc.plant_freq_response(plant, p, u, x, FC.GRID, (0, 1), (0, 2))
    bad = np.isin(np.arange(8), (2, 5))
    assert (res.status[bad] == cmpc.CMPC_EQ_NONFINITE).all() and (res.status[~bad] == OK).all()
    assert _all_nan(res.record[bad]) and _all_nan(res.summary[bad])
    good = cmpc.plant_freq_response(plant, p, u, GC.cases(plant, B=8)[2], FC.GRID, (0, 1), (0, 2))
    assert np.array_equal(bits(res.record[~bad]), bits(good.record[~bad]))
    assert np.array_equal(bits(res.summary[~bad]), bits(good.summary[~bad]))


def test_freq_check_refuses_bad_arguments():
    lib = load_library()
    i32 = lambda v: np.ascontiguousarray(v, np.int32)
    f64 = lambda v: np.ascontiguousarray(v, np.float64)
    good = dict(plant=0, ny=2, out=i32([0, 1]), nu=2, inp=i32([0, 2]), nw=3, om=f64([0.0, 1.0, 1.0]))

    def rc(**kw):
        a = dict(good, **kw)
        return lib.cmpc_freq_check(a["plant"], a["ny"], iptr(a["out"]), a["nu"], iptr(a["inp"]), a["nw"],
                                   dptr(a["om"]) if a["om"] is not None else None)

    assert rc() == 0 and rc(nw=64, om=f64(np.arange(64.0))) == 0 and rc(nw=1, om=f64([1e300])) == 0
    for kw, word in ((dict(plant=2), "plant"), (dict(ny=0), "ny"), (dict(ny=5), "ny"), (dict(nu=0), "nu"),
                     (dict(nu=5), "nu"), (dict(out=i32([0, 0])), "out_idx repeats"),
                     (dict(inp=i32([2, 2])), "in_idx repeats"), (dict(out=i32([0, 4])), "out_idx[1]"),
                     (dict(inp=i32([-1, 2])), "in_idx[0]"), (dict(nw=0), "nw"),
                     (dict(nw=65, om=f64(np.ones(65))), "nw"),
                     (dict(nw=-1), "nw"), (dict(om=None), "null omega"), (dict(om=f64([0.0, -1.0, 1.0])), "omega[1]"),
                     (dict(om=f64([np.nan, 1.0, 1.0])), "omega[0]"), (dict(om=f64([0.0, 1.0, np.inf])), "omega[2]"),
                     (dict(om=f64([0.0, -np.inf, 1.0])), "omega[1]")):
        assert rc(**kw) < 0, kw
        msg = lib.cmpc_last_error().decode()
        assert "cmpc_freq_check" in msg and word in msg, (kw, msg)
    # the entry points run the same check before they touch anything
    p, u, x = GC.cases(0, B=2)
    with pytest.raises(RuntimeError, match="out_idx repeats"):
        cmpc.plant_freq_response(0, p, u, x, [1.0], (1, 1), (0, 2))
    with pytest.raises(RuntimeError, match="nw"):
        cmpc.plant_freq_response(0, p, u, x, [], (0, 1), (0, 2))
    with pytest.raises(ValueError):
        cmpc.plant_freq_response(0, p, u[:, :8], x, [1.0], (0, 1), (0, 2))
    rec, sm = np.full((2, 3, cmpc.CMPC_FREQ_LEN), 7.0), np.full((2, cmpc.CMPC_FREQ_NSUM), 7.0)
    st = np.full(2, 9, np.int32)
    o, i = i32([0, 1]), i32([0, 2])
    host = lambda B=2, xs=x, outs=o, nw=3, om=good["om"]: lib.cmpc_plant_freq_host(
        0, B, dptr(p), dptr(u), dptr(xs) if xs is not None else None, 2, iptr(outs), 2, iptr(i), nw,
        dptr(om) if om is not None else None, dptr(rec), dptr(sm), iptr(st))
    for kw in (dict(B=0), dict(xs=None), dict(outs=i32([1, 1])), dict(nw=0), dict(nw=65), dict(om=None),
               dict(om=f64([0.0, -1.0, 1.0])), dict(om=f64([0.0, np.nan, 1.0])), dict(om=f64([np.inf, 0.0, 1.0]))):
        assert host(**kw) < 0, kw
        assert (rec == 7.0).all() and (sm == 7.0).all() and (st == 9).all(), kw
    assert host() == 0 and (st == OK).all() and not (rec == 7.0).any()
    # the matrix-level call
    A, Bm, C, E = f64(-np.eye(2)), f64(np.ones((2, 4))), f64(np.ones((4, 2))), f64(np.ones((2, 2)))
    rec[:], sm[:], st[:] = 7.0, 7.0, 9
    mat = lambda n=2, B=1, ny=1, nu=1, nw=3, om=good["om"], Am=A: lib.cmpc_freq_host(
        n, B, dptr(Am) if Am is not None else None, dptr(Bm), dptr(C), dptr(E), ny, nu, nw,
        dptr(om) if om is not None else None, dptr(rec), dptr(sm), iptr(st))
    for kw, word in ((dict(n=0), "n must"), (dict(n=13), "n must"), (dict(B=0), "B must"), (dict(ny=0), "ny"),
                     (dict(nu=5), "nu"), (dict(nw=0), "nw"), (dict(nw=65), "nw"), (dict(om=None), "null omega"),
                     (dict(om=f64([0.0, -1.0, 1.0])), "omega[1]"), (dict(Am=None), "null argument")):
        assert mat(**kw) < 0, kw
        assert "cmpc_freq_host" in lib.cmpc_last_error().decode() and word in lib.cmpc_last_error().decode(), kw
        assert (rec == 7.0).all() and (sm == 7.0).all() and (st == 9).all(), kw
    assert mat() == 0 and st[0] == OK and st[1] == 9
    with pytest.raises(ValueError):
        cmpc.freq_response(np.eye(13), np.ones((13, 1)), np.ones((1, 13)), np.zeros((13, 2)), [1.0])
    with pytest.raises(ValueError):
        cmpc.freq_response(np.eye(2), np.ones((2, 5)), np.ones((1, 2)), np.zeros((2, 2)), [1.0])


def test_host_body_under_sanitizers():
    """csrc/freq_body.h built with AddressSanitizer and UndefinedBehaviorSanitizer
    as a stand-alone program (host code only; tests/cpp/freq_asan.cpp,
    freq_asan.mk) and run for both plants, every selection size, one frequency
    and 64, every status, and the matrix-level body at n = 1, 2 and 12."""
    here = os.path.join(ROOT, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-C", here, "-f", "freq_asan.mk", "freq_asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(here, "freq_asan")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("freq_asan ok"), r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-2000:]
