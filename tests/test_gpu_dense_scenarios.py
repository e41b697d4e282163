"""GPU parity on dense data for the per-scenario settings and the paired row
build: offsets dy_ref, per-slot limits, reference profiles, per-slot weights
and build pairing, against the oracle AND against the long-double model of
tests/dense_ref.py.  Marked gpu; runs on an MI355X.

The GPU files of these features (test_gpu_scenario_config.py,
test_gpu_reference_profile.py, test_gpu_scenario_weights.py,
test_gpu_build_pairing.py) run on plant records: exact zeros in A, Bin and
Csel, the setup files' diagonal ywt, a reference constant over the horizon,
and bars scaled by max|H| (the uwt scale) or max|f|.  There a transposed
L_W'[q], a profile read one horizon row off, Bin rotated by nu +- 1 columns or
the offset of the neighbouring slot can pass.  Here nothing is zero, every
weight is dense, the reference differs at every row and slot, and each of
those four errors, put into the oracle's inputs on the CPU, misses the bound
by more than 1e3 (tests/test_dense_reference.py).

B = 5 for the one-QP-per-wave, split, predict and refshift paths (10 or 5
slots: refshift's workgroup of four rows ends partly filled), B = 9 wherever
the row or the paired build runs (two whole groups of four scenarios and a
partial one).

Bounds (conditions, not measurements; the oracle stays within a tenth of each
against the long-double reference on every problem here, checked on the CPU):
  build    dense_ref.qp_error_ratios <= 1 against both references (the Gram
           part scales H, f and G); H exactly symmetric; bit-identity wherever
           include/cmpc.h promises it
  shift    f_unset - f_profile within 1e-11 max|g| of the long-double
           g = Su' W dref; the problems are drawn so that max|g| >= 0.1 max|f|
  predict  dense_ref.prediction_error_ratios <= 1
  step     fused, build + iterate, paired and unpaired bit-identical; against
           the oracle's step as test_gpu_dense_step (compare_step, NEAR_TIE),
           no scenario flagged (B // 32 = 0), every status 0

Measured on an MI355X, worst over all cases and kernels as a fraction of the
bound (97 tests, 4 s):
  offsets and profiles, WAVE / SPLIT / ROWS: H 4.5e-4, f 6.2e-4, G 1.4e-2
    (either reference), shift 1.2e-3
  per-slot weights, alone and with dy and dref: H 4.6e-4, f 1.2e-4, G 4.6e-4,
    shift 6.4e-4 (the shared ywt in refshift would miss it by 1e11)
  predict with all three: y_pred 1.9e-4, costs 1.1e-4
  paired row build: H 2.9e-4, f 4.2e-5, G 9.0e-4, shift 2.5e-4; paired and
    unpaired bit-identical, the altered batch shares 4 of 9 scenarios
  steps: no scenario differs from the oracle, none is flagged; 10 of 18
    (pair), 12 of 18 (coop-par) and 6 of 9 (cent-par) slots end on a limit of
    their own that differs from the shared one
"""
import numpy as np
import pytest

import cmpc
import dense_ref as DR
from cmpc._abi import CmpcDims
from test_gpu_dense_parity import VARIANT_NAMES, build_variants, case_id, dense_ctx, dev
from test_gpu_parity import NEAR_TIE, compare_step

pytestmark = pytest.mark.gpu
WAVE, ROWS = cmpc.CMPC_BUILD_WAVE, cmpc.CMPC_BUILD_ROWS
ON, OFF = cmpc.CMPC_PAIRING_ON, cmpc.CMPC_PAIRING_OFF
B5, B9 = DR.B_WAVE, DR.B_ROWS


def batch_of(variant):
    return B9 if variant == ROWS else B5


def variants_of(case):
    """WAVE and SPLIT everywhere, ROWS where the plan has it: every m <= 2 set"""
    vs = build_variants(DR.config_for(*case), B9)
    assert (ROWS in vs) == (case[0][3] <= 2)
    return vs


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_qp(qp, refs, what):
    """H, f, G finite, H exactly symmetric, within the bound of both references;
    returns the worst ratios"""
    H, f, G = qp
    assert np.isfinite(H).all() and np.isfinite(f).all() and np.isfinite(G).all(), what
    assert np.array_equal(H, np.transpose(H, (0, 2, 1))), f"{what}: H must be exactly symmetric"
    worst = {}
    for name in ("oracle", "ref"):
        w = DR.qp_error_ratios(H, f, G, *refs[name], refs["gram"])
        print(f"{what} vs {'long double' if name == 'ref' else name}: error / bound H {w['H']:.2e} f {w['f']:.2e} "
              f"G {w['G']:.2e}")
        worst[name] = w
    for name, w in worst.items():
        assert max(w.values()) <= 1.0, (what, name, w)
    return worst


# ---- 1. offsets ------------------------------------------------------------------

@pytest.mark.parametrize("case", DR.SCN_OFFSET_CASES, ids=case_id)
def test_gpu_dense_offsets(case):
    """cmpc_set_scenario_reference(dy): H, f, G against both references; H and
    G those of the build without dy and the whole QP that of a build without
    dy from records whose y_prev is y_prev - dy, bit for bit."""
    for v in variants_of(case):
        B = batch_of(v)
        c = DR.scenario_case(*case, B=B, scale=1.0)
        cfg, L = c["cfg"], DR.Layout(c["cfg"])
        refs = DR.scenario_refs(c, dy=True)
        shifted = c["lin"].copy()
        shifted[:, L.off_y:L.off_y + cfg.ny] = c["lin"][:, L.off_y:L.off_y + cfg.ny] - c["dy"]   # one FP64 subtraction
        with dense_ctx(c, B) as ctx:
            ctx.set_build_variant(v)
            ctx.build()
            plain = ctx.download_qp()
            ctx.set_scenario_reference(c["dy"])
            ctx.build()
            assert ctx.last_build_kernel() == v
            got = ctx.download_qp()
            ctx.set_scenario_reference(None)
            ctx.upload_lin(shifted)
            ctx.build()
            from_shifted = ctx.download_qp()
        what = f"{case_id(case)} {VARIANT_NAMES[v]} B={B}"
        assert_qp(got, refs, what)
        assert bits_equal(got[0], plain[0]) and bits_equal(got[2], plain[2]), f"{what}: dy moved H or G"
        for a, b, name in zip(got, from_shifted, "HfG"):
            assert bits_equal(a, b), f"{what}: {name} is not that of the records with y_prev - dy"
        assert all(not np.array_equal(got[1][q], plain[1][q]) for q in range(B * cfg.S))


# ---- 2. profiles -----------------------------------------------------------------

@pytest.mark.parametrize("case", DR.SCN_PROFILE_CASES, ids=case_id)
def test_gpu_dense_profile(case):
    """cmpc_set_scenario_reference_profile(dref) with the shared dense ywt: f
    against both references, H and G untouched bit for bit, the shift itself
    against the long-double g, inputs delayed by >= p untouched bit for bit."""
    for v in variants_of(case):
        B = batch_of(v)
        c = DR.scenario_case(*case, B=B)
        cfg = c["cfg"]
        assert cmpc.reference_profile_available(CmpcDims.from_config(cfg, B))
        refs, g = DR.scenario_refs(c, dref=True), DR.scenario_shift(c)["g"]
        assert DR.shift_to_f(refs["ref"][1], g) >= 0.1
        with dense_ctx(c, B) as ctx:
            ctx.set_build_variant(v)
            ctx.build()
            H0, f0, G0 = ctx.download_qp()
            ctx.set_scenario_reference_profile(c["dref"])
            ctx.build()
            assert ctx.last_build_kernel() == v
            H, f, G = ctx.download_qp()
        what = f"{case_id(case)} {VARIANT_NAMES[v]} B={B}"
        ws = DR.shift_error_ratio(f0 - f, g)
        print(f"{what}: shift error / bound {ws:.2e}")
        assert_qp((H, f, G), refs, what)
        assert bits_equal(H, H0) and bits_equal(G, G0), f"{what}: the profile moved H or G"
        assert ws <= 1.0, what
        late = [k for k in range(cfg.nu) if cfg.delays[k] >= cfg.p]
        assert bool(late) == (cfg.p <= 17)
        for k in late:
            assert bits_equal(f[:, k::cfg.nu], f0[:, k::cfg.nu]), f"{what}: input {k} never arrives"
        for k in set(range(cfg.nu)) - set(late):
            assert not np.array_equal(f[:, k::cfg.nu], f0[:, k::cfg.nu])


# ---- 3. weights ------------------------------------------------------------------

@pytest.mark.parametrize("case", DR.SCN_WEIGHT_CASES, ids=case_id)
def test_gpu_dense_weights(case):
    """cmpc_set_scenario_weights, dense per slot: the build AUTO chooses is
    WAVE; H, f, G against both references; a slot whose block is the shared
    one gets WAVE's QP bit for bit."""
    c = DR.scenario_case(*case, weights=True, scale=1.0)
    cfg, nq = c["cfg"], B5 * c["cfg"].S
    assert cmpc.scenario_weights_available(CmpcDims.from_config(cfg, B5))
    s_of = np.arange(nq) % cfg.S
    some = np.arange(nq) % 3 == 1    # these slots keep the shared block
    uwt, ywt = c["uwt"].copy(), c["ywt"].copy()
    uwt[some], ywt[some] = c["arr"].uwt[s_of][some], c["arr"].ywt[s_of][some]
    with dense_ctx(c, B5) as ctx:
        ctx.set_build_variant(WAVE)
        ctx.build()
        shared = ctx.download_qp()
        ctx.set_build_variant(cmpc.CMPC_BUILD_AUTO)
        ctx.set_scenario_weights(c["uwt"], c["ywt"])
        ctx.build()
        assert ctx.last_build_kernel() == WAVE
        got = ctx.download_qp()
        ctx.set_scenario_weights(uwt, ywt)
        ctx.build()
        assert ctx.last_build_kernel() == WAVE
        mixed = ctx.download_qp()
    assert_qp(got, DR.scenario_refs(c), f"{case_id(case)} weights")
    for a, b, m, name in zip(got, shared, mixed, "HfG"):
        if a.shape[-1] == 0:
            continue
        assert bits_equal(m[some], b[some]), f"{name}: a slot with the shared block is not WAVE's"
        assert bits_equal(m[~some], a[~some]), name
        assert all(not np.array_equal(a[q], b[q]) for q in range(nq)), name


@pytest.mark.parametrize("case", DR.SCN_WEIGHT_CASES, ids=case_id)
def test_gpu_dense_weights_offsets_and_profile(case):
    """Weights, dy and dref together: refshift reads ywt[q].  f and the shift
    against the long-double model."""
    c = DR.scenario_case(*case, weights=True)
    cfg = c["cfg"]
    refs, g = DR.scenario_refs(c, dy=True, dref=True), DR.scenario_shift(c)["g"]
    assert DR.shift_to_f(refs["ref"][1], g) >= 0.1
    with dense_ctx(c, B5) as ctx:
        ctx.set_scenario_weights(c["uwt"], c["ywt"])
        ctx.set_scenario_reference(c["dy"])
        ctx.build()
        H0, f0, G0 = ctx.download_qp()
        ctx.set_scenario_reference_profile(c["dref"])
        ctx.build()
        assert ctx.last_build_kernel() == WAVE
        H, f, G = ctx.download_qp()
    what = f"{case_id(case)} weights + dy + dref"
    ws = DR.shift_error_ratio(f0 - f, g)
    g_shared = DR.scenario_shift(c, weights=False)["g"]
    print(f"{what}: shift error / bound {ws:.2e} (with the shared ywt instead it would be "
          f"{DR.shift_error_ratio(g_shared, g):.2e})")
    assert_qp((H, f, G), refs, what)
    assert bits_equal(H, H0) and bits_equal(G, G0)
    assert ws <= 1.0


# ---- 4. predict ------------------------------------------------------------------

@pytest.mark.parametrize("case", DR.SCN_PREDICT_CASES, ids=case_id)
def test_gpu_dense_predict_with_settings(case):
    """cmpc_predict with per-slot weights, dy and dref in force, predict_case's
    plans: the other controllers' given in device memory, and gathered."""
    import torch
    torch.cuda.init()
    c = DR.scenario_predict_case(*case)
    cfg = c["cfg"]
    assert cmpc.predict_available(CmpcDims.from_config(cfg, B5))
    t_du, t_d = dev(c["du"]), dev(c["d"])
    with dense_ctx(c, B5) as ctx:
        ctx.set_scenario_weights(c["uwt"], c["ywt"])
        ctx.set_scenario_reference(c["dy"])
        ctx.set_scenario_reference_profile(c["dref"])
        ctx.build()
        ctx.predict(t_du.data_ptr(), t_d.data_ptr() if cfg.nVo else 0)
        Y, J = ctx.download_prediction()
        ctx.predict(t_du.data_ptr(), 0)
        Yg, Jg = ctx.download_prediction()
    assert Y.shape == (B5 * cfg.S, cfg.p, cfg.ny) and J.shape == (B5 * cfg.S, 2)
    wy, wj = DR.prediction_error_ratios(Y, J, *c["given"])
    wyg, wjg = DR.prediction_error_ratios(Yg, Jg, *c["gathered"])
    print(f"{case_id(case)}: error / bound, plans given: y_pred {wy:.2e} costs {wj:.2e}; gathered: y_pred {wyg:.2e} "
          f"costs {wjg:.2e}")
    assert np.isfinite(Y).all() and np.isfinite(Yg).all() and np.isfinite(J).all() and np.isfinite(Jg).all()
    assert max(wy, wj, wyg, wjg) <= 1.0


# ---- 5. the paired build ---------------------------------------------------------

def pair_build(c, mode, lin=None, settings=False, profile=True):
    """(H, f, G) and the coverage counter of one forced row build; settings: dy,
    per-slot limits and (profile) dref in force"""
    with dense_ctx(c, B9) as ctx:
        if lin is not None:
            ctx.upload_lin(lin)
        ctx.set_build_variant(ROWS)
        ctx.set_build_pairing(mode)
        if settings:
            ctx.set_scenario_reference(c["dy"])
            ctx.set_scenario_constraints(*c["limits"])
            if profile:
                ctx.set_scenario_reference_profile(c["dref"])
        ctx.build()
        assert ctx.last_build_kernel() == ROWS
        shared = ctx.last_build_shared_scenarios()
        return ctx.download_qp(), shared


def assert_same_bits(on, off):
    for name, a, b in zip("HfG", on, off):
        a, b = np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)
        bad = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=1))
        assert bad.size == 0, f"{name} differs in QP slots {bad.tolist()}"


@pytest.mark.parametrize("p", DR.PAIR_HORIZONS)
def test_gpu_dense_pair_build(p):
    """CMPC_PAIRING_ON against CMPC_PAIRING_OFF bit for bit on the paired dense
    draw, every scenario in the shared form, and both within the bound of the
    oracle and of the long-double reference: plain, and with dy, dref and
    per-slot limits in force."""
    c = DR.pair_case(p)
    for settings in (False, True):
        refs = DR.scenario_refs(c, dy=settings, dref=settings)
        off, n_off = pair_build(c, OFF, settings=settings)
        on, n_on = pair_build(c, ON, settings=settings)
        assert n_off == -1 and n_on == B9
        assert_same_bits(on, off)
        what = f"pair p={p}" + (" dy + dref + limits" if settings else "")
        assert_qp(on, refs, what + " paired")
        assert_qp(off, refs, what + " unpaired")
        if settings:
            g = DR.scenario_shift(c)["g"]
            assert DR.shift_to_f(refs["ref"][1], g) >= 0.1
            f_dy = pair_build(c, ON, settings=True, profile=False)[0][1]
            ws = DR.shift_error_ratio(f_dy - on[1], g)
            print(f"{what}: shift error / bound {ws:.2e}")
            assert ws <= 1.0


def test_gpu_dense_pair_mixed_batch():
    """One entry of slot 1's A one ulp off in scenarios 2 and 8: still the
    unpaired QP buffer bit for bit, the shared count exactly the scenarios
    outside those scenarios' groups of four, and within the bound of the
    long-double reference of the ALTERED records."""
    c, a = DR.pair_case(50), DR.pair_altered_case(50)
    off, n_off = pair_build(c, OFF, lin=a["lin"])
    on, n_on = pair_build(c, ON, lin=a["lin"])
    assert_same_bits(on, off)
    groups = {b // 4 for b in DR.PAIR_ALTERED}
    assert n_off == -1 and n_on == sum(1 for b in range(B9) if b // 4 not in groups) == 4
    assert_qp(on, a, "pair p=50, scenarios 2 and 8 altered")
    plain, _ = pair_build(c, ON)
    rows = [np.flatnonzero((x != y).reshape(x.shape[0], -1).any(axis=1)).tolist() for x, y in zip(on, plain)]
    assert set(rows[0]) <= {2 * b + 1 for b in DR.PAIR_ALTERED}, rows


STEP_NAMES = ("du", "status", "nwsr", "trace", "ntrace", "u_old", "du_old", "ws")


def assert_step_matches_oracle(c, run, what):
    cfg, K = c["cfg"], DR.STEP_K
    B = c["lin"].shape[0] // cfg.S
    du, st, nw, tr, ntr, u_g, du_g, ws_g = run
    odu, ost, onw, ows, otr, ontr = c["oracle"]
    assert (st == 0).all(), what
    bad, flagged = compare_step(B, cfg.S, K, (du, st, nw, ws_g, tr, ntr), (odu, ost, onw, ows, otr, ontr),
                                c["margin"], np.zeros(B, bool))
    own = DR.on_own_limit(cfg, c, du)
    print(f"{what}: active {(ws_g != 0).mean():.2f}, scenarios differing at a flagged near-tie {flagged.sum()}, "
          f"unflagged {bad.sum()}, smallest oracle margin {c['margin'].min():.3g} (NEAR_TIE {NEAR_TIE:g}), slots on a "
          f"limit of their own {int(own.sum())} of {own.size}")
    assert not bad.any(), np.flatnonzero(bad)[:10]
    assert flagged.sum() <= B // 32, flagged.sum()
    np.testing.assert_allclose(du, odu, rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(u_g, c["u_after"], rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(du_g, odu, rtol=1e-9, atol=1e-10)
    assert (ws_g != 0).mean() >= 0.25
    assert own.any(), "no slot ends on a limit of its own: a solve that ignored the per-slot block would pass"


def test_gpu_dense_pair_step():
    """cmpc_step, K = 3, the first move applied, the unfused step on the row
    build with dy, dref and per-slot limits in force: paired against unpaired
    bit for bit, and against the oracle's step."""
    c = DR.scenario_step_case("pair")
    flags = cmpc.CMPC_APPLY_MOVE | cmpc.CMPC_TRACE
    runs = {}
    for mode in (ON, OFF):
        with dense_ctx(c, B9) as ctx:
            ctx.set_scenario_reference(c["dy"])
            ctx.set_scenario_constraints(*c["limits"])
            ctx.set_scenario_reference_profile(c["dref"])
            ctx.set_build_variant(ROWS)
            ctx.set_build_pairing(mode)
            ctx.set_step_variant(cmpc.CMPC_STEP_SPLIT)
            ctx.step(DR.STEP_K, flags)
            assert ctx.last_build_kernel() == ROWS and not ctx.last_step_fused()
            assert ctx.last_build_shared_scenarios() == (B9 if mode == ON else -1)
            runs[mode] = (*ctx.download(), *ctx.download_trace(DR.STEP_K), *ctx.get_state())
    for a, b, name in zip(runs[ON], runs[OFF], STEP_NAMES):
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), f"paired, unpaired: {name}"
    assert_step_matches_oracle(c, runs[ON], "pair step")


# ---- 6. per-slot limits in the solve ---------------------------------------------

@pytest.mark.parametrize("name", ["coop-par", "cent-par"])
def test_gpu_dense_step_with_per_slot_limits(name):
    """The dense step cases re-drawn with per-slot limits and dy: the fused
    launch and cmpc_build + cmpc_iterate on the same build kernel bit for bit,
    both against the oracle's step run with each slot's own limits, and at
    least one slot ending on a limit of its own that is not the shared one."""
    c = DR.scenario_step_case(name)
    cfg, K = c["cfg"], DR.STEP_K
    flags = cmpc.CMPC_APPLY_MOVE | cmpc.CMPC_TRACE
    runs = {}
    with dense_ctx(c, B9) as ctx:
        ctx.set_scenario_reference(c["dy"])
        ctx.set_scenario_constraints(*c["limits"])
        ctx.set_step_variant(cmpc.CMPC_STEP_FUSED)
        ctx.step(K, flags)
        assert ctx.last_step_fused()
        kernel = ctx.last_build_kernel()
        runs["fused"] = (*ctx.download(), *ctx.download_trace(K), *ctx.get_state())
    with dense_ctx(c, B9) as ctx:
        ctx.set_scenario_reference(c["dy"])
        ctx.set_scenario_constraints(*c["limits"])
        ctx.set_build_variant(kernel)
        ctx.build()
        assert ctx.last_build_kernel() == kernel
        ctx.iterate(K, flags)
        runs["split"] = (*ctx.download(), *ctx.download_trace(K), *ctx.get_state())
    for a, b, what in zip(runs["fused"], runs["split"], STEP_NAMES):
        assert np.array_equal(a, b), f"fused and build + iterate differ in {what}"
    for mode, run in runs.items():
        assert_step_matches_oracle(c, run, f"{name} {mode}")
