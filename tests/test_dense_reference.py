"""The oracle on dense data against a long-double model (tests/dense_ref.py).
CPU only.

Every other problem the suite feeds the build, predict and step paths is a
linearisation of the two compressor plants with the setup files' weights and
references: records with exact zeros in A, Bin and Csel, diagonal weights and
a reference that is the same at every horizon row.  An index error that reads
the wrong one of two zeros, a transposed weight factor or a horizon index off
by one is invisible there.  Here the oracle (oracle/or_condense.c) builds the
QP and the prediction matrices from dense records with dense SPD weights and
an independent reference per horizon row, and must agree with a model of the
record contract that shares no code and no algorithm with it: the plant
equations stepped forward in numpy.longdouble, Su from unit plans.

Bound: the project's (test_gpu_build_matches_oracle), scaled by the Gram part
  |H - H_ref| <= 1e-11 sH, sH = max|H_ref - R|;  f, G as there with this sH;
  predicted outputs 1e-11 max|y_ref| per slot, costs 1e-11 relative.
The oracle has to stay within a TENTH of it (the GPU tests hold the kernels to
the whole bound against both the oracle and the long-double reference).

Measured (x86-64, 80-bit long double), worst over the slots as a fraction of
the bound:
  dense, 96 cases (8 dimension sets x 4 delay sets x p = 7, 23, 50, B = 3):
    H 2.7e-4, f 3.3e-4, G 8.8e-4, y_pred 3.0e-4, costs 2.4e-4
  plant data, the six reference configurations (p = 100, B = 4):
    H 2.5e-4, f 1.5e-4, G 2.4e-4, Su 2.0e-4, y_pred 1.7e-4, costs 2.6e-4
  the B = 47 problems of test_gpu_dense_parity.py (41 build, 32 predict cases):
    H 3.7e-4, f 3.4e-4, G 8.9e-3, y_pred 3.4e-4, costs 3.1e-4
so the oracle's own error is 9e-14 of the scale at the worst, a factor of ten
inside the tenth, and 4e-15 for everything but G.  max|H - R| of the dense QPs
is 1e3 to 1e7 against max|R| of 3 to 20: R does not set the tolerance.
"""
import numpy as np
import pytest

import _oracle as O
import cmpc
import dense_ref as DR
import golden_cases as GC
import predict_ref as PR
from cmpc.synthetic import synthetic_batch

NEAR_TIE = 1e-9            # tests/test_gpu_parity.py
TENTH = 0.1

DELAY_SETS = [(0, 40, 0, 40), (0, 10, 0, 25), (0, 2, 0, 63), (0, 50, 0, 57)]   # the last: both delays >= p
HORIZONS = [7, 23, 50]


def oracle_predictions(cfg, arr, lin, u_old, du, d):
    dims = DR.dims_of(cfg, 1)
    return PR.oracle_batch(cfg, dims, O.layout(dims), arr, lin, u_old, du, d)


# ---- the record layout --------------------------------------------------------

@pytest.mark.parametrize("dimset", list(DR.DIM_SETS))
@pytest.mark.parametrize("delays", DELAY_SETS + [(0, 0, 0, 5), (3, 0, 0, 0)])
def test_layout_from_the_contract_matches_the_oracle(dimset, delays):
    cfg = DR.config_for(dimset, 23, delays)
    L, Lo = DR.Layout(cfg), O.layout(DR.dims_of(cfg, 1))
    for k in ("nd", "naug", "nobs", "nV", "nuo", "nVo", "off_A", "off_B", "off_C", "off_f", "off_x", "off_y",
              "rec_len"):
        assert getattr(L, k) == getattr(Lo, k), k


# ---- anchoring: plant data ------------------------------------------------------

@pytest.mark.parametrize("name", GC.NAMES)
def test_long_double_reference_matches_oracle_on_plant_data(name):
    """The six reference configurations (p = 100, the setup files' weights
    and references): what the goldens pin through the oracle pins the
    long-double reference too."""
    cfg, setup, arr, _ = GC.case(name)
    B = 4
    lin, u_old, _, _ = synthetic_batch(cfg, B, seed=77)
    Hr, fr, Gr, gram = DR.ref_qp(cfg, lin, u_old, arr)
    Ho, fo, Go = DR.oracle_qps(cfg, arr, lin, u_old)
    w = DR.qp_error_ratios(Ho, fo, Go, Hr, fr, Gr, gram)
    # or_generate_prediction's Su and Su_other
    _, Su, Suo = DR.ref_matrices(cfg, lin, u_old)
    dims = DR.dims_of(cfg, 1)
    w_su = 0.0
    for q in range(lin.shape[0]):
        So, _, _, Soo = O.generate_prediction(dims, lin[q])
        w_su = max(w_su, float(np.abs(So - Su[q]).max() / (1e-11 * np.abs(Su[q]).max())))
        if cfg.nVo:
            w_su = max(w_su, float(np.abs(Soo - Suo[q]).max() / (1e-11 * np.abs(Suo[q]).max())))
    rng = np.random.default_rng(5)
    du = rng.uniform(-0.1, 0.1, (B * cfg.S, cfg.nV))
    d = rng.uniform(-0.1, 0.1, (B * cfg.S, cfg.nVo))
    Yo, Jo = oracle_predictions(cfg, arr, lin, u_old, du, d)
    wy, wj = DR.prediction_error_ratios(Yo, Jo, *DR.ref_prediction(cfg, lin, u_old, arr, du, d))
    print(f"{name}: oracle error / bound: H {w['H']:.2e} f {w['f']:.2e} G {w['G']:.2e} Su {w_su:.2e} "
          f"y_pred {wy:.2e} costs {wj:.2e}")
    assert max(w["H"], w["f"], w["G"], w_su, wy, wj) <= TENTH


# ---- dense data -----------------------------------------------------------------

@pytest.mark.parametrize("p", HORIZONS)
@pytest.mark.parametrize("delays", DELAY_SETS)
@pytest.mark.parametrize("dimset", list(DR.DIM_SETS))
def test_oracle_matches_long_double_reference_on_dense_data(dimset, delays, p):
    c = DR.predict_case(dimset, p, delays, B=3)
    cfg = c["cfg"]
    DR.assert_dense(cfg, c["lin"], c["u_old"], c["arr"])
    w = c["ratios"]
    Yo, Jo = oracle_predictions(cfg, c["arr"], c["lin"], c["u_old"], c["du"], c["d"])
    wy, wj = DR.prediction_error_ratios(Yo, Jo, *c["given"])
    print(f"{dimset} delays {delays} p {p}: oracle error / bound: H {w['H']:.2e} f {w['f']:.2e} G {w['G']:.2e} "
          f"y_pred {wy:.2e} costs {wj:.2e}; max|H - R| {float(np.abs(c['gram']).max()):.3g}")
    assert max(w["H"], w["f"], w["G"], wy, wj) <= TENTH


def test_oracle_within_a_tenth_on_the_gpu_files_problems():
    """The B = 47 problems test_gpu_dense_parity.py feeds the kernels: the
    oracle alone stays within a tenth of the bound on each of them, so a
    kernel that meets the bound against one reference cannot miss it against
    the other by more than that."""
    worst = {"H": 0.0, "f": 0.0, "G": 0.0, "y_pred": 0.0, "costs": 0.0}
    for dimset, p, delays in DR.GPU_BUILD_CASES:
        for k, v in DR.build_case(dimset, p, delays)["ratios"].items():
            worst[k] = max(worst[k], v)
    for dimset, p, delays in DR.GPU_PREDICT_CASES:
        c = DR.predict_case(dimset, p, delays)
        Yo, Jo = oracle_predictions(c["cfg"], c["arr"], c["lin"], c["u_old"], c["du"], c["d"])
        wy, wj = DR.prediction_error_ratios(Yo, Jo, *c["given"])
        worst["y_pred"], worst["costs"] = max(worst["y_pred"], wy), max(worst["costs"], wj)
    print("oracle error / bound, worst over the GPU cases:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) <= TENTH


def test_dense_draw_properties():
    """No zero entry anywhere, off-diagonal weights non-zero, the reference
    different at every horizon row, the same draw for the same seed."""
    for dimset, p, delays in [((11, 3, 2, 2), 50, (0, 40, 0, 40)), ((10, 4, 4, 2), 23, (0, 2, 0, 63)),
                              ((11, 3, 2, 3), 7, (0, 50, 0, 57)), ((10, 2, 2, 2), 50, (0, 10, 0, 25))]:
        cfg = DR.config_for(dimset, p, delays)
        for scale in (1.0, DR.STEP_SCALE):
            lin, u_old, arr = DR.dense_problem(cfg, 5, seed=9, scale=scale)
            DR.assert_dense(cfg, lin, u_old, arr)
            L = DR.Layout(cfg)
            assert lin.shape == (5 * cfg.S, L.rec_len) and u_old.shape == (5 * cfg.S, cfg.nu_tot)
            yr = arr.y_ref.reshape(cfg.S, p, cfg.ny)
            assert np.all(yr[:, 1:, :] != yr[:, :-1, :])
            for s in range(cfg.S):
                for W in (arr.ywt[s], arr.uwt[s]):
                    off = W[~np.eye(W.shape[0], dtype=bool)]
                    assert np.all(off != 0.0) and np.abs(off).max() > 0.05
                # inside the limits: every QP of a step is feasible
                uo = u_old.reshape(5, cfg.S, cfg.nu_tot)[:, s, :cfg.nu]
                assert np.all(uo > arr.lower[s]) and np.all(uo < arr.upper[s])
            lin2, u2, arr2 = DR.dense_problem(cfg, 5, seed=9, scale=scale)
            assert np.array_equal(lin, lin2) and np.array_equal(u_old, u2) and np.array_equal(arr.y_ref, arr2.y_ref)
            lin3, _, _ = DR.dense_problem(cfg, 5, seed=10, scale=scale)
            assert not np.array_equal(lin, lin3)


@pytest.mark.parametrize("name", list(DR.STEP_CASES))
def test_dense_step_cases_meet_their_conditions(name):
    """The step problems of test_gpu_dense_parity.py on the oracle alone: at
    least a quarter of the QPs end with an active constraint, the oracle's
    margins flag at most 1/64 of the scenarios as near-ties, every status 0."""
    c = DR.step_case(name)
    cfg = c["cfg"]
    du, st, nw, ws, tr, ntr = c["oracle"]
    B = c["lin"].shape[0] // cfg.S
    flagged = int((c["margin"] < NEAR_TIE).reshape(B, cfg.S).any(1).sum())
    active = float((ws != 0).mean())
    print(f"{name}: active {active:.2f}, scenarios flagged {flagged} of {B}, smallest margin {c['margin'].min():.2g}, "
          f"working-set changes {int(ntr.sum())}")
    assert (st == 0).all()
    assert active >= 0.25
    assert flagged <= B // 64
    assert not np.array_equal(c["u_after"], c["u_old"])
