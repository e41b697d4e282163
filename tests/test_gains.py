"""The steady-state gains on the host (cmpc_plant_gains_host,
csrc/gains_body.h): G, Gp, RGA and K_ff against the oracle's
linearisation solved by numpy and by a long-double elimination, G and Gp
against central differences of the nonlinear plant's equilibria, the structure
of the record for every selection shape, every status that a plant case
reaches, every refusal of cmpc_gain_check, and the body under ASan + UBSan.
CPU only.

Measured on the 64 seeded cases per plant (parallel, serial), errors scaled by
the matrix's largest entry (DESIGN.md §3.22 has the reading):
  against long double, numpy float64 / the product
    G     6.8e-16 / 2.0e-15    9.4e-16 / 7.3e-15
    Gp    7.2e-16 / 1.8e-15    1.4e-15 / 2.7e-15
    RGA   7.3e-16 / 3.4e-15    1.5e-15 / 2.4e-15
    K_ff  1.0e-15 / 4.5e-15    1.0e-15 / 6.3e-15
  against the nonlinear differences, numpy's model and the product alike
    G     3.2e-10              5.5e-10
    Gp    3.7e-10              2.3e-10
"""
import os
import subprocess

import numpy as np
import pytest

import cmpc
import gains_cases as GC
from cmpc._abi import dptr, iptr, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_FACTOR = 8.0    # the product against numpy's measured error (DESIGN.md §3.19's rule)
PLANT_FACTOR = 4.0    # the product against the model's differencing error
OK = cmpc.CMPC_EQ_OK


def _all_nan(a):
    return bool((GC.bits(a) == GC.NAN_BITS).all())


@pytest.mark.parametrize("plant", [0, 1])
def test_gains_against_the_oracle_linearisation(plant):
    """G, Gp, RGA and K_ff of the 4 x 4 selection against the same from the
    oracle's A, B, C and its E differenced at the same h.  Tolerance:
    MODEL_FACTOR times the largest distance of numpy's float64 result from the
    long-double one over the same cases (measured here), both scaled by the
    matrix's largest entry."""
    p, u, x = GC.cases(plant)
    res = cmpc.plant_gains(plant, p, u, x, GC.ALL, GC.ALL)
    assert (res.status == OK).all(), res.status
    assert (res.resid <= 1e-12).all()
    measured = dict.fromkeys(("G", "Gp", "rga", "k_ff"), 0.0)
    product = dict(measured)
    for b in range(len(x)):
        m64, mld = GC.gain_models(plant, x[b], u[b], *p[b])
        for key in measured:
            measured[key] = max(measured[key], GC.scaled_diff(m64[key], mld[key]))
            product[key] = max(product[key], GC.scaled_diff(getattr(res, key)[b], mld[key]))
    for key in measured:
        print(f"plant {plant} {key}: float64 numpy against long double {measured[key]:.2e}, "
              f"product against long double {product[key]:.2e}")
    for key in measured:
        assert measured[key] > 0
        assert product[key] <= MODEL_FACTOR * measured[key], key


@pytest.mark.parametrize("plant", [0, 1])
def test_gains_against_the_nonlinear_plant(plant):
    """G against central differences (+-1e-5 per control input) of host-solved
    equilibria, Gp against the same in each pressure, scaled by the matrix's
    largest entry.  The numpy model's error against the same differences is
    the differencing error; the product may have PLANT_FACTOR times it."""
    p, u, x = GC.cases(plant)
    Gfd, Gpfd = GC.nonlinear_gains(plant)
    res = cmpc.plant_gains(plant, p, u, x, GC.ALL, GC.ALL)
    assert (res.status == OK).all(), res.status
    model = {"G": 0.0, "Gp": 0.0}
    product = dict(model)
    for b in range(len(x)):
        m64, _ = GC.gain_models(plant, x[b], u[b], *p[b])
        for key, fd in (("G", Gfd[b]), ("Gp", Gpfd[b])):
            model[key] = max(model[key], GC.scaled_diff(m64[key], fd))
            product[key] = max(product[key], GC.scaled_diff(getattr(res, key)[b], fd))
    for key in model:
        print(f"plant {plant} {key}: numpy model against the nonlinear differences {model[key]:.2e}, "
              f"product {product[key]:.2e}")
    for key in model:
        assert model[key] > 0
        assert product[key] <= PLANT_FACTOR * model[key], key


@pytest.mark.parametrize("plant", [0, 1])
def test_rga_rows_and_columns_sum_to_one(plant):
    """The largest distance of a row or column sum from 1 against the same of
    numpy's RGA on the same cases, by the MODEL_FACTOR rule; 4 x 4 and 2 x 2."""
    p, u, x = GC.cases(plant)
    for outs, ins in (GC.SELECTIONS[2], GC.SELECTIONS[1]):
        res = cmpc.plant_gains(plant, p, u, x, outs, ins)
        assert (res.status == OK).all()
        dev = lambda r: max(np.abs(r.sum(-1) - 1).max(), np.abs(r.sum(-2) - 1).max())
        model = max(dev(GC.gain_models(plant, x[b], u[b], *p[b], outs, ins)[0]["rga"]) for b in range(len(x)))
        product = dev(res.rga)
        print(f"plant {plant} {len(outs)} x {len(ins)}: RGA sums off 1 by {product:.2e} (product), {model:.2e} (numpy)")
        assert model > 0
        assert product <= MODEL_FACTOR * model
    one = cmpc.plant_gains(plant, p, u, x, (0,), (0,))
    # 1 x 1: g * (1 / g), two roundings of 2^-53 each
    assert (one.status == OK).all() and np.abs(one.rga - 1.0).max() <= 2.0 ** -52


@pytest.mark.parametrize("plant", [0, 1])
def test_record_layout_of_every_selection(plant):
    p, u, x = GC.cases(plant)
    full = cmpc.plant_gains(plant, p, u, x, GC.ALL, GC.ALL)
    assert not np.isnan(full.record).any()
    for outs, ins in GC.SELECTIONS + (((2, 0), (3, 1)), ((3,), (2,)), ((1, 3), (0, 1, 2))):
        ny, nu = len(outs), len(ins)
        res = cmpc.plant_gains(plant, p, u, x, outs, ins)
        assert (res.status == OK).all(), (outs, ins, res.status)
        assert res.G.shape == (64, ny, nu) and res.Gp.shape == (64, ny, 2)
        assert res.rga.shape == (64, ny, nu) and res.k_ff.shape == (64, nu, 2)
        # Z does not depend on the input selection, nor a column of it on the other outputs
        assert np.array_equal(GC.bits(res.G), GC.bits(full.G[:, list(outs)][:, :, list(ins)]))
        assert np.array_equal(GC.bits(res.Gp), GC.bits(full.Gp[:, list(outs)]))
        assert np.array_equal(GC.bits(res.resid), GC.bits(full.resid))
        # outside ny / nu: the one quiet NaN
        G4, Gp4 = res.record[:, :16].reshape(-1, 4, 4), res.record[:, 16:24].reshape(-1, 4, 2)
        R4, K4 = res.record[:, 24:40].reshape(-1, 4, 4), res.record[:, 40:48].reshape(-1, 4, 2)
        assert _all_nan(G4[:, ny:]) and _all_nan(G4[:, :, nu:]) and _all_nan(Gp4[:, ny:])
        if ny == nu:
            assert not np.isnan(res.rga).any() and not np.isnan(res.k_ff).any()
            assert _all_nan(R4[:, ny:]) and _all_nan(R4[:, :, nu:]) and _all_nan(K4[:, nu:])
        else:
            assert _all_nan(R4) and _all_nan(K4)


def test_a_selected_recycle_valve_in_the_dead_zone():
    p, u, x = GC.cases(0, B=8)
    u = u.copy()
    u[:, 3] = 0.01
    res = cmpc.plant_gains(0, p, u, x, (0, 1), (0, 1))
    assert (res.status == cmpc.CMPC_EQ_DEADZONE).all() and _all_nan(res.record)
    assert (cmpc.plant_gains(0, p, u, x, GC.ALL, GC.ALL).status == cmpc.CMPC_EQ_DEADZONE).all()
    # the same valve not selected is not in the way: its B column is never read
    free = cmpc.plant_gains(0, p, u, x, (0, 1), (0, 2))
    assert (free.status == OK).all() and not np.isnan(free.G).any() and (free.resid > 0).all()
    u[:, 3] = 0.0
    assert (cmpc.plant_gains(0, p, u, x, (0, 1), (0, 3)).status == OK).all()


def test_a_rank_deficient_selection_is_singular_g():
    """Parallel plant, outputs (0, 3) against both inputs of the second
    compressor: torque and recycle valve reach the first compressor's surge
    distance and the tank only through the second compressor's outlet flow, so
    G has rank 1.  Where the second pivot cancels to exactly zero the status is
    CMPC_GAIN_SINGULAR_G: G, Gp and r_f stand, RGA and K_ff are the NaN.
    Where it is left rounding-sized the status is OK and the RGA is huge."""
    p, u, x = GC.cases(0)
    outs, ins = (0, 3), (2, 3)
    res = cmpc.plant_gains(0, p, u, x, outs, ins)
    full = cmpc.plant_gains(0, p, u, x, GC.ALL, GC.ALL)
    print("statuses", np.bincount(res.status, minlength=7).tolist())
    sg = res.status == cmpc.CMPC_GAIN_SINGULAR_G
    assert set(res.status.tolist()) == {OK, cmpc.CMPC_GAIN_SINGULAR_G} and sg.sum() >= 4 and (~sg).sum() >= 4
    assert np.array_equal(GC.bits(res.G), GC.bits(full.G[:, list(outs)][:, :, list(ins)]))
    assert np.array_equal(GC.bits(res.Gp), GC.bits(full.Gp[:, list(outs)]))
    assert np.array_equal(GC.bits(res.resid), GC.bits(full.resid))
    assert _all_nan(res.record[sg, 24:48]) and _all_nan(res.record[sg][:, [2, 3, 6, 7] + list(range(8, 16))])
    det = res.G[:, 0, 0] * res.G[:, 1, 1] - res.G[:, 0, 1] * res.G[:, 1, 0]
    # each entry carries the elimination's rounding, of order 1e-14 of max|G|, which is some 60 times
    # the smallest entry here: the determinant cancels to 1e-12 of its terms or better, the RGA is their ratio
    assert (np.abs(det) <= 1e-12 * np.abs(res.G[:, 0, 0] * res.G[:, 1, 1])).all()
    assert (np.abs(res.rga[~sg]).max(axis=(1, 2)) > 1e10).all()


@pytest.mark.parametrize("plant", [0, 1])
def test_a_nan_state_is_nonfinite(plant):
    p, u, x = GC.cases(plant, B=8)
    x = x.copy()
    x[2, 3] = np.nan
    x[5, 0] = np.inf
    res = cmpc.plant_gains(plant, p, u, x, (0, 1), (0, 2))
    bad = np.isin(np.arange(8), (2, 5))
    assert (res.status[bad] == cmpc.CMPC_EQ_NONFINITE).all() and (res.status[~bad] == OK).all()
    assert _all_nan(res.record[bad])
    good = cmpc.plant_gains(plant, p, u, GC.cases(plant, B=8)[2], (0, 1), (0, 2))
    assert np.array_equal(GC.bits(res.record[~bad]), GC.bits(good.record[~bad]))


def test_gain_check_refuses_bad_arguments():
    lib = load_library()
    i32 = lambda v: np.ascontiguousarray(v, np.int32)
    good = dict(plant=0, ny=2, out=i32([0, 1]), nu=2, inp=i32([0, 2]))

    def rc(**kw):
        a = dict(good, **kw)
        return lib.cmpc_gain_check(a["plant"], a["ny"], iptr(a["out"]), a["nu"], iptr(a["inp"]))

    assert rc() == 0
    assert rc(ny=4, out=i32([3, 2, 1, 0]), nu=1) == 0 and rc(plant=1, nu=4, inp=i32([1, 0, 3, 2])) == 0
    for kw, word in ((dict(plant=2), "plant"), (dict(plant=-1), "plant"), (dict(ny=0), "ny"), (dict(ny=5), "ny"),
                     (dict(nu=0), "nu"), (dict(nu=5), "nu"), (dict(ny=-1), "ny"),
                     (dict(out=i32([0, 0])), "out_idx repeats"), (dict(inp=i32([2, 2])), "in_idx repeats"),
                     (dict(out=i32([0, 4])), "out_idx[1]"), (dict(out=i32([-1, 1])), "out_idx[0]"),
                     (dict(inp=i32([0, 4])), "in_idx[1]"), (dict(inp=i32([-1, 2])), "in_idx[0]")):
        assert rc(**kw) < 0, kw
        msg = lib.cmpc_last_error().decode()
        assert "cmpc_gain_check" in msg and word in msg, (kw, msg)
    assert lib.cmpc_gain_check(0, 1, None, 1, iptr(i32([0]))) < 0
    assert lib.cmpc_gain_check(0, 1, iptr(i32([0])), 1, None) < 0
    assert "null" in lib.cmpc_last_error().decode()
    # the host entry point runs the same check before it touches anything
    p, u, x = GC.cases(0, B=2)
    with pytest.raises(RuntimeError, match="out_idx repeats"):
        cmpc.plant_gains(0, p, u, x, (1, 1), (0, 2))
    with pytest.raises(ValueError):
        cmpc.plant_gains(0, p, u[:, :8], x, (0, 1), (0, 2))
    rec, st = np.full((2, cmpc.CMPC_GAIN_LEN), 7.0), np.full(2, 9, np.int32)
    o, i = i32([0, 1]), i32([0, 2])
    assert lib.cmpc_plant_gains_host(0, 0, dptr(p), dptr(u), dptr(x), 2, iptr(o), 2, iptr(i), dptr(rec), iptr(st)) < 0
    assert lib.cmpc_plant_gains_host(0, 2, dptr(p), dptr(u), None, 2, iptr(o), 2, iptr(i), dptr(rec), iptr(st)) < 0
    assert "null" in lib.cmpc_last_error().decode()
    assert (rec == 7.0).all() and (st == 9).all()


def test_host_body_under_sanitizers():
    """csrc/gains_body.h built with AddressSanitizer and UndefinedBehaviorSanitizer
    as a stand-alone program (host code only; tests/cpp/gains_asan.cpp,
    gains_asan.mk) and run for both plants and every selection size."""
    here = os.path.join(ROOT, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-C", here, "-f", "gains_asan.mk", "gains_asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(here, "gains_asan")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("gains_asan ok"), r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-2000:]
