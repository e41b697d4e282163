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
import refprofile_ref as RP
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


# ---- per-scenario settings on dense data -------------------------------------------
# Offsets dy, profiles dref, per-slot weights and limits and the paired draw
# (dense_ref.scenario_case and its kin), for tests/test_gpu_dense_scenarios.py.
#
# Measured (x86-64, 80-bit long double), worst over the slots as a fraction of
# the bound:
#   72 cases (8 dimension sets x 3 delay sets x p = 7, 23, 50, B = 3), per-slot
#   dense weights, dy and dref all in force:
#     H 2.6e-4, f 7.1e-5, G 3.2e-3, y_pred 1.9e-4, costs 3.3e-4; against ref_shift,
#     as a fraction of 1e-11 max|g|: the oracle's Su' w 7.1e-4, the numpy sweep 8.9e-4
#   the problems of test_gpu_dense_scenarios.py (B = 5 and 9):
#     H 3.3e-4, f 1.0e-3, G 8.9e-3, shift 3.9e-3, y_pred 1.3e-4, costs 1.4e-4;
#     smallest max|g| / max|f| over the slots with a profile in force: 0.81
#   each of the four errors the GPU file is there for (a transposed L_W'[q], dref
#   one horizon row off, Bin rotated by nu +- 1 columns, the neighbouring slot's
#   dy), put into the oracle's inputs, misses the bound by more than 1e3

SCN_DELAY_SETS = DELAY_SETS[:3]


def all_gpu_scenario_cases():
    """(label, case, parts of the reference in force) for every build problem
    test_gpu_dense_scenarios.py feeds the kernels"""
    out = []
    for case in DR.SCN_OFFSET_CASES:
        for B in (DR.B_WAVE, DR.B_ROWS):
            out.append(("offsets", DR.scenario_case(*case, B=B, scale=1.0), dict(dy=True)))
    for case in DR.SCN_PROFILE_CASES:
        for B in (DR.B_WAVE, DR.B_ROWS):
            out.append(("profiles", DR.scenario_case(*case, B=B), dict(dref=True)))
    for case in DR.SCN_WEIGHT_CASES:
        out.append(("weights", DR.scenario_case(*case, weights=True, scale=1.0), dict()))
        out.append(("weights+dy+dref", DR.scenario_case(*case, weights=True), dict(dy=True, dref=True)))
    for p in DR.PAIR_HORIZONS:
        out.append(("pair", DR.pair_case(p), dict()))
        out.append(("pair+dy+dref", DR.pair_case(p), dict(dy=True, dref=True)))
    return out


@pytest.mark.parametrize("p", HORIZONS)
@pytest.mark.parametrize("delays", SCN_DELAY_SETS)
@pytest.mark.parametrize("dimset", list(DR.DIM_SETS))
def test_oracle_matches_long_double_reference_with_scenario_settings(dimset, delays, p):
    """The oracle given the slot's own dense weights and y_ref + dy + dref
    against the extended model: H, f, G, the prediction and its costs within a
    tenth of the bound; the oracle's Su' w and the numpy sweep, with the dense
    per-slot ywt, within a tenth of 1e-11 max|g| of ref_shift."""
    c = DR.scenario_predict_case(dimset, p, delays, B=3)
    w = DR.scenario_refs(c, dy=True, dref=True)["ratios"]
    Yo, Jo = DR.slot_oracle_predictions(c, c["du"], c["d"])
    wy, wj = DR.prediction_error_ratios(Yo, Jo, *c["given"])
    sh = DR.scenario_shift(c)
    wo, ws = DR.shift_error_ratio(sh["oracle_g"], sh["g"]), DR.shift_error_ratio(sh["sweep_g"], sh["g"])
    print(f"{dimset} delays {delays} p {p}: oracle error / bound: H {w['H']:.2e} f {w['f']:.2e} G {w['G']:.2e} "
          f"y_pred {wy:.2e} costs {wj:.2e} shift: oracle {wo:.2e} sweep {ws:.2e}")
    assert max(w["H"], w["f"], w["G"], wy, wj, wo, ws) <= TENTH
    # the settings do reach the model: each part of the reference moves f, the weights H
    base = DR.ref_qp(c["cfg"], c["lin"], c["u_old"], c["arr"])
    full = DR.scenario_refs(c, dy=True, dref=True)["ref"]
    only_dy = DR.scenario_refs(c, dy=True)["ref"]
    for q in range(c["lin"].shape[0]):
        assert np.abs(full[0][q] - base[0][q]).max() > 1e-3 * np.abs(base[0][q]).max()
        assert np.abs(only_dy[1][q] - full[1][q]).max() > 1e-3 * np.abs(full[1][q]).max()
    assert not np.array_equal(only_dy[1], DR.scenario_refs(c)["ref"][1])


def test_model_without_settings_is_the_model_it_was():
    """ref_qp and ref_prediction with nothing given, or given the shared
    weights per slot and zero offsets, return what they did: bit for bit."""
    c = DR.predict_case((10, 4, 2, 2), 23, (0, 10, 0, 25), B=3)
    cfg, arr, lin, u_old = c["cfg"], c["arr"], c["lin"], c["u_old"]
    nq = lin.shape[0]
    s_of = np.arange(nq) % cfg.S
    kw = dict(ywt=arr.ywt[s_of], uwt=arr.uwt[s_of], dy=np.zeros((nq, cfg.ny)), dref=np.zeros((nq, cfg.p, cfg.ny)))
    for a, b in zip(DR.ref_qp(cfg, lin, u_old, arr, **kw), (*c["ref"], c["gram"])):
        assert np.array_equal(a, b)
    for a, b in zip(DR.ref_prediction(cfg, lin, u_old, arr, c["du"], c["d"], **kw), c["given"]):
        assert np.array_equal(a, b)
    # ref_shift is the difference of the two f's it is not computed from
    dref = np.random.default_rng(3).standard_normal((nq, cfg.p, cfg.ny))
    g = DR.ref_shift(cfg, lin, u_old, arr, dref)
    f1 = DR.ref_qp(cfg, lin, u_old, arr, dref=dref)[1]
    for q in range(nq):
        assert np.abs((c["ref"][1][q] - f1[q]) - g[q]).max() <= 1e-15 * max(np.abs(c["ref"][1][q]).max(),
                                                                              np.abs(g[q]).max())


def test_oracle_within_a_tenth_on_the_gpu_scenario_problems():
    """Every build and predict problem of test_gpu_dense_scenarios.py: the
    oracle stays within a tenth of the bound, and where a profile is in force
    max|g| >= 0.1 max|f| in every slot, so that the difference of two f's the
    shift test takes still holds g to the precision it asks for."""
    worst = {"H": 0.0, "f": 0.0, "G": 0.0, "shift": 0.0, "y_pred": 0.0, "costs": 0.0}
    least = np.inf
    for label, c, parts in all_gpu_scenario_cases():
        r = DR.scenario_refs(c, **parts)
        for k, v in r["ratios"].items():
            worst[k] = max(worst[k], v)
        if parts.get("dref"):
            sh = DR.scenario_shift(c)
            worst["shift"] = max(worst["shift"], DR.shift_error_ratio(sh["oracle_g"], sh["g"]),
                                 DR.shift_error_ratio(sh["sweep_g"], sh["g"]))
            ratio = DR.shift_to_f(r["ref"][1], sh["g"])
            least = min(least, ratio)
            assert ratio >= 0.1, (label, c["key"], ratio)
    for case in DR.SCN_PREDICT_CASES:
        c = DR.scenario_predict_case(*case, weights=True)
        for plans, ref in ((c["d"], c["given"]), (c["d_gathered"], c["gathered"])):
            wy, wj = DR.prediction_error_ratios(*DR.slot_oracle_predictions(c, c["du"], plans), *ref)
            worst["y_pred"], worst["costs"] = max(worst["y_pred"], wy), max(worst["costs"], wj)
    print("oracle error / bound, worst over the GPU scenario cases:", {k: f"{v:.2e}" for k, v in worst.items()},
          f"; smallest max|g| / max|f| {least:.3g}")
    assert max(worst.values()) <= TENTH


@pytest.mark.parametrize("p", DR.PAIR_HORIZONS)
def test_paired_draw(p):
    """The premises of build pairing hold bit for bit, the draw is still dense,
    and the pair is no trivial one: the scenario's two QPs differ in H, f and G
    (Bin's rotation, uwt, y_ref, the tails), u_old lies inside each slot's own
    limits and those differ from the shared ones."""
    c = DR.pair_case(p)
    cfg = c["cfg"]
    DR.assert_dense(cfg, c["lin"], c["u_old"], c["arr"])
    DR.assert_paired(cfg, c["lin"], c["u_old"], c["arr"])
    dims = DR.dims_of(cfg, DR.B_ROWS)
    lw = [cmpc.weight_factor(c["arr"].ywt[s]) for s in range(2)]
    assert cmpc.build_pairing_reason(dims, *lw) == ""
    for parts in (dict(), dict(dy=True, dref=True)):
        H, f, G = DR.scenario_refs(c, **parts)["ref"]
        for b in range(DR.B_ROWS):
            # (slot 1's G is slot 0's transposed, own and other inputs exchanged: the diagonals agree)
            for a, least in ((H, 1e-3), (f, 1e-3), (G, 1e-6)):
                assert np.abs(a[2 * b] - a[2 * b + 1]).max() > least * np.abs(a[2 * b]).max()
    lo, up, rlo, rup = c["limits"]
    own = c["u_old"][:, :cfg.nu]
    assert np.all(own > lo) and np.all(own < up)
    assert np.all(up != np.tile(c["arr"].upper, (DR.B_ROWS, 1))) and not np.array_equal(up[0::2], up[1::2])
    # the altered batch: two entries differ, and the QPs of exactly those two slots
    a = DR.pair_altered_case(p)
    rows = np.flatnonzero((a["lin"] != c["lin"]).any(axis=1))
    assert rows.tolist() == [2 * b + 1 for b in DR.PAIR_ALTERED]
    assert max(a["oracle"][0][q].tobytes() != DR.scenario_refs(c)["oracle"][0][q].tobytes() for q in rows)
    w = DR.qp_error_ratios(*a["oracle"], *a["ref"], a["gram"])
    assert max(w.values()) <= TENTH, w


@pytest.mark.parametrize("name", list(DR.SCN_STEP_CASES))
def test_scenario_step_cases_meet_their_conditions(name):
    """The step problems of test_gpu_dense_scenarios.py on the oracle alone, as
    step_case's: at least a quarter of the QPs end with an active constraint, no
    scenario flagged as a near-tie (B // 32 = 0 at B = 9), every status 0; and
    at least one slot ends on a limit of its own that differs from the shared
    one, so that a solve which ignored the per-slot block would not pass."""
    c = DR.scenario_step_case(name)
    cfg = c["cfg"]
    du, st, nw, ws, tr, ntr = c["oracle"]
    B = c["lin"].shape[0] // cfg.S
    flagged = int((c["margin"] < NEAR_TIE).reshape(B, cfg.S).any(1).sum())
    active = float((ws != 0).mean())
    own = DR.on_own_limit(cfg, c, du)
    print(f"{name}: active {active:.2f}, scenarios flagged {flagged} of {B}, smallest margin {c['margin'].min():.2g}, "
          f"working-set changes {int(ntr.sum())}, slots on a limit of their own {int(own.sum())} of {own.size}")
    assert B == DR.B_ROWS and (st == 0).all()
    assert active >= 0.25
    assert flagged <= B // 32
    assert own.any()
    assert not np.array_equal(c["u_after"], c["u_old"])


# ---- each GPU assertion fails for the error it is there for --------------------------
# The corruption goes into the oracle's inputs (no kernel is broken to show it):
# the corrupted oracle must miss the bound against the long-double reference.

def _cases_for_corruption():
    return [DR.scenario_case(ds, 17, weights=True) for ds in DR.DIM_SETS]


def test_transposed_weight_factor_misses_the_bound():
    """L_W' read transposed: the weight becomes L_W' L_W in place of
    ywt = L_W L_W'.  With the setup files' diagonal ywt the two are equal."""
    for c in _cases_for_corruption():
        cfg, nq = c["cfg"], c["lin"].shape[0]
        lw = np.stack([cmpc.weight_factor(c["ywt"][q]) for q in range(nq)])
        wrong = np.ascontiguousarray(lw @ np.transpose(lw, (0, 2, 1)))
        assert np.abs(np.transpose(lw, (0, 2, 1)) @ lw - c["ywt"]).max() <= 1e-13 * np.abs(c["ywt"]).max()
        r = DR.scenario_refs(c, dy=True, dref=True)
        Ho, fo, Go = DR.slot_oracle_qps(cfg, c["arr"], c["lin"], c["u_old"], wrong, c["uwt"], c["dy"], c["dref"])
        w = DR.qp_error_ratios(Ho, fo, Go, *r["ref"], r["gram"])
        assert min(w["H"], w["f"]) > 1e3, w
        g = DR.scenario_shift(c)["g"]
        dims = DR.dims_of(cfg, 1)
        gw = np.stack([RP.oracle_g(cfg, dims, c["lin"][q], wrong[q], c["dref"][q]) for q in range(nq)])
        assert DR.shift_error_ratio(gw, g) > 1e3
        diag = np.stack([np.diag(np.diag(c["ywt"][q])) for q in range(nq)])
        ld = np.stack([cmpc.weight_factor(diag[q]) for q in range(nq)])
        assert np.array_equal(ld @ np.transpose(ld, (0, 2, 1)), np.transpose(ld, (0, 2, 1)) @ ld)


def test_profile_off_by_one_row_misses_the_bound():
    for c in _cases_for_corruption():
        cfg = c["cfg"]
        r = DR.scenario_refs(c, dy=True, dref=True)
        for shift in (1, -1):
            wrong = np.ascontiguousarray(np.roll(c["dref"], shift, axis=1))
            Ho, fo, Go = DR.slot_oracle_qps(cfg, c["arr"], c["lin"], c["u_old"], c["ywt"], c["uwt"], c["dy"], wrong)
            assert DR.qp_error_ratios(Ho, fo, Go, *r["ref"], r["gram"])["f"] > 1e3
    # and the prediction's tracking cost
    c = DR.scenario_predict_case((11, 3, 2, 2), 17)
    wrong = dict(c, dref=np.ascontiguousarray(np.roll(c["dref"], 1, axis=1)))
    _, wj = DR.prediction_error_ratios(*DR.slot_oracle_predictions(wrong, c["du"], c["d"]), *c["given"])
    assert wj > 1e3


def test_offset_of_the_neighbouring_slot_misses_the_bound():
    for c in _cases_for_corruption() + [DR.scenario_case(*DR.SCN_OFFSET_CASES[0], B=DR.B_ROWS, scale=1.0)]:
        cfg = c["cfg"]
        r = DR.scenario_refs(c, dy=True)
        for shift in (1, -1):
            wrong = np.ascontiguousarray(np.roll(c["dy"], shift, axis=0))
            Ho, fo, Go = DR.slot_oracle_qps(cfg, c["arr"], c["lin"], c["u_old"], c["ywt"], c["uwt"], wrong)
            assert DR.qp_error_ratios(Ho, fo, Go, *r["ref"], r["gram"])["f"] > 1e3


def test_weights_of_the_neighbouring_slot_miss_the_bound():
    for c in _cases_for_corruption():
        r = DR.scenario_refs(c)
        Ho, fo, Go = DR.slot_oracle_qps(c["cfg"], c["arr"], c["lin"], c["u_old"], np.roll(c["ywt"], 1, axis=0),
                                        np.roll(c["uwt"], 1, axis=0))
        assert DR.qp_error_ratios(Ho, fo, Go, *r["ref"], r["gram"])["H"] > 1e3


@pytest.mark.parametrize("p", DR.PAIR_HORIZONS)
def test_pair_rotated_by_one_column_more_or_less_misses_the_bound(p):
    """Slot 1's Bin taken as slot 0's rolled by nu +- 1 columns instead of nu"""
    c = DR.pair_case(p)
    cfg, L = c["cfg"], DR.Layout(c["cfg"])
    r = DR.scenario_refs(c)
    for off in (1, -1):
        lin = c["lin"].copy()
        B0 = lin[0::2, L.off_B:L.off_C].reshape(-1, cfg.ns, cfg.nu_tot)
        lin[1::2, L.off_B:L.off_C] = np.roll(B0, -(cfg.nu + off), axis=2).reshape(B0.shape[0], -1)
        Ho, fo, Go = DR.slot_oracle_qps(cfg, c["arr"], lin, c["u_old"])
        w = DR.qp_error_ratios(Ho, fo, Go, *r["ref"], r["gram"])
        assert w["H"] > 1e3 and w["f"] > 1e3, w
