"""GPU parity on dense data: the build, predict and step kernels against the
oracle AND against the long-double model of tests/dense_ref.py.  Marked gpu;
runs on an MI355X.

The problems (dense_ref.dense_problem) have no zero entry in any record
field, dense SPD weights and a reference that differs at every horizon row,
so a lane or index that reads the wrong entry, a transposed L_W or a horizon
index off by one changes the result; on the plant data of the other GPU files
each of these is invisible (tests/test_dense_reference.py).
B = 47: 47 or 94 QP slots, the last row group partial.

Bounds (conditions, not measurements; the oracle itself stays within a tenth
of each against the long-double reference, checked on the CPU):
  build    |H - H_ref| <= 1e-11 sH with sH = max|H_ref - R| (the Gram part:
           R does not widen it); f: 1e-10 max(max|f_ref|, 1e-6 sH);
           G: 1e-11 max(max|G_ref|, 1e-6 sH); against both references.
           H exactly symmetric; SPLIT bit-identical to WAVE.
  predict  test_gpu_predict.py's: y_pred 1e-11 max|y_ref| per slot, J_track and
           J_move 1e-11 relative, against the long-double reference.
  step     fused and build + iterate bit-identical; against the oracle's step
           as test_gpu_step_matches_oracle (compare_step, NEAR_TIE), at most
           1/32 of the scenarios flagged, every status 0.

Measured on an MI355X, worst over all cases and kernels as a fraction of the
bound: build H 4.8e-4, f 4.7e-4, G 1.1e-2 (either reference); Gram part on
plant data 6.0e-4 (the oracle's own 4.9e-4); predict y_pred 2.0e-4, costs
2.5e-4; step: no scenario differs from the oracle, none is flagged.
"""
import numpy as np
import pytest

import cmpc
import dense_ref as DR
import golden_cases as GC
from cmpc._abi import CmpcDims
from cmpc.synthetic import synthetic_batch
from test_gpu_parity import NEAR_TIE, compare_step, make_ctx, oracle_qps

pytestmark = pytest.mark.gpu
B = 47
VARIANT_NAMES = {cmpc.CMPC_BUILD_WAVE: "wave", cmpc.CMPC_BUILD_SPLIT: "split", cmpc.CMPC_BUILD_ROWS: "rows"}


def device_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def dense_ctx(c, B=B):
    cfg = c["cfg"]
    nq = B * cfg.S
    return make_ctx(cfg, c["arr"], B, c["lin"], c["u_old"], np.zeros((nq, cfg.nV)), np.zeros(nq, np.uint32))


def build_variants(cfg, B=B):
    """WAVE and SPLIT everywhere, ROWS where the library's plan has it"""
    out = [cmpc.CMPC_BUILD_WAVE, cmpc.CMPC_BUILD_SPLIT]
    if cmpc.plan(CmpcDims.from_config(cfg, B), device_cus(), build=cmpc.CMPC_BUILD_ROWS).build_error == 0:
        out.append(cmpc.CMPC_BUILD_ROWS)
    return out


def case_id(case):
    ds, p, dl = case
    return "-".join(map(str, ds)) + f"-p{p}-d" + "_".join(map(str, dl))


# ---- 1. build ------------------------------------------------------------------

@pytest.mark.parametrize("case", DR.GPU_BUILD_CASES, ids=case_id)
def test_gpu_dense_build(case):
    c = DR.build_case(*case)
    cfg = c["cfg"]
    assert max(c["ratios"].values()) <= 0.1, c["ratios"]     # the oracle against the long-double reference
    got = {}
    with dense_ctx(c) as ctx:
        for v in build_variants(cfg):
            ctx.set_build_variant(v)
            ctx.build()
            assert ctx.last_build_kernel() == v
            got[v] = ctx.download_qp()
    if case[0][3] <= 2:
        assert cmpc.CMPC_BUILD_ROWS in got, "the row build is instantiated for every m <= 2 dimension set"
    worst = {}
    for v, (H, f, G) in got.items():
        for name, ref in (("oracle", c["oracle"]), ("long double", c["ref"])):
            worst[v, name] = DR.qp_error_ratios(H, f, G, *ref, c["gram"])
    for (v, name), w in worst.items():
        print(f"{case_id(case)} {VARIANT_NAMES[v]} vs {name}: error / bound H {w['H']:.2e} f {w['f']:.2e} G {w['G']:.2e}")
    for v, (H, f, G) in got.items():
        assert np.isfinite(H).all() and np.isfinite(f).all() and np.isfinite(G).all()
        assert np.array_equal(H, np.transpose(H, (0, 2, 1))), f"{VARIANT_NAMES[v]}: H must be exactly symmetric"
    for a, b in zip(got[cmpc.CMPC_BUILD_WAVE], got[cmpc.CMPC_BUILD_SPLIT]):
        assert np.array_equal(a, b), "SPLIT must equal WAVE bit for bit"
    for (v, name), w in worst.items():
        assert max(w.values()) <= 1.0, (VARIANT_NAMES[v], name, w)


# ---- 2. the Gram part on plant data ---------------------------------------------

@pytest.mark.parametrize("plant", ["par", "ser"])
def test_gpu_gram_part_on_plant_data(plant):
    """The existing plant-data batch (coop, p = 50), H - R compared at
    1e-11 max|H_oracle - R|: 6e-8 absolute where the 1e-11 max|H| of
    test_gpu_build_matches_oracle allows 2e-6, since max|H| is uwt."""
    _, setup, _, _ = GC.case(f"coop-{plant}")
    cfg = cmpc.reference_config(plant, "coop", p=50)
    arr = cmpc.controller_arrays(cfg, setup)
    lin, u_old, du_old, ws = synthetic_batch(cfg, B, seed=61)
    Ho, _, _ = oracle_qps(cfg, arr, lin, u_old)
    _, _, _, gram_ld = DR.ref_qp(cfg, lin, u_old, arr)
    nq, nu, m = B * cfg.S, cfg.nu, cfg.m
    R = np.zeros((nq, cfg.nV, cfg.nV))
    for mv in range(m):
        R[:, mv * nu:(mv + 1) * nu, mv * nu:(mv + 1) * nu] = arr.uwt[np.arange(nq) % cfg.S]
    gram_o = Ho - R
    scale = np.abs(gram_o).max(axis=(1, 2))
    own = float((np.abs(gram_o - gram_ld).max(axis=(1, 2)) / (1e-11 * scale)).max())
    print(f"{plant}-coop: max|H - R| {scale.max():.4g}, max|R| {np.abs(R).max():.4g}; oracle's own error against the "
          f"long-double Gram part {own:.2e} of the bound")
    worst = {}
    with make_ctx(cfg, arr, B, lin, u_old, du_old, ws) as ctx:
        for v in build_variants(cfg):
            ctx.set_build_variant(v)
            ctx.build()
            assert ctx.last_build_kernel() == v
            H, _, _ = ctx.download_qp()
            worst[v] = float((np.abs((H - R) - gram_o).max(axis=(1, 2)) / (1e-11 * scale)).max())
            print(f"{plant}-coop {VARIANT_NAMES[v]}: |(H - R) - (H_oracle - R)| / (1e-11 max|H_oracle - R|) = {worst[v]:.2e}")
    assert len(worst) == 3
    assert max(worst.values()) <= 1.0, worst


# ---- 3. predict ------------------------------------------------------------------

def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")


@pytest.mark.parametrize("case", DR.GPU_PREDICT_CASES, ids=case_id)
def test_gpu_dense_predict(case):
    """Random plans: the other controllers' given in device memory, and
    gathered by the kernel from the scenario's other slots."""
    import torch
    torch.cuda.init()
    c = DR.predict_case(*case)
    cfg = c["cfg"]
    assert cmpc.predict_available(CmpcDims.from_config(cfg, B))
    t_du, t_d = dev(c["du"]), dev(c["d"])
    with dense_ctx(c) as ctx:
        ctx.build()
        ctx.predict(t_du.data_ptr(), t_d.data_ptr() if cfg.nVo else 0)
        Y, J = ctx.download_prediction()
        ctx.predict(t_du.data_ptr(), 0)
        Yg, Jg = ctx.download_prediction()
    assert Y.shape == (B * cfg.S, cfg.p, cfg.ny) and J.shape == (B * cfg.S, 2)
    wy, wj = DR.prediction_error_ratios(Y, J, *c["given"])
    wyg, wjg = DR.prediction_error_ratios(Yg, Jg, *c["gathered"])
    print(f"{case_id(case)}: error / bound, plans given: y_pred {wy:.2e} costs {wj:.2e}; gathered: y_pred {wyg:.2e} "
          f"costs {wjg:.2e}")
    assert np.isfinite(Y).all() and np.isfinite(Yg).all()
    if cfg.nVo:
        assert not np.array_equal(Y, Yg)      # the two sets of other plans differ
    else:
        assert np.array_equal(Y, Yg) and np.array_equal(J, Jg)
    assert max(wy, wj, wyg, wjg) <= 1.0


# ---- 4. step ---------------------------------------------------------------------

@pytest.mark.parametrize("name", list(DR.STEP_CASES))
def test_gpu_dense_step(name):
    """cmpc_step, K = 3, the first move applied: one fused launch and
    cmpc_build + cmpc_iterate on the same build kernel give the same plans,
    statuses, nWSR, working sets, change sequences and u_old bit for bit, and
    both match the oracle's step."""
    c = DR.step_case(name)
    cfg, K = c["cfg"], DR.STEP_K
    flags = cmpc.CMPC_APPLY_MOVE | cmpc.CMPC_TRACE
    runs = {}
    with dense_ctx(c) as ctx:
        ctx.set_step_variant(cmpc.CMPC_STEP_FUSED)
        ctx.step(K, flags)
        assert ctx.last_step_fused()
        kernel = ctx.last_build_kernel()
        runs["fused"] = (*ctx.download(), *ctx.download_trace(K), *ctx.get_state())
    with dense_ctx(c) as ctx:
        ctx.set_build_variant(kernel)
        ctx.build()
        assert ctx.last_build_kernel() == kernel
        ctx.iterate(K, flags)
        runs["split"] = (*ctx.download(), *ctx.download_trace(K), *ctx.get_state())
    for a, b, what in zip(runs["fused"], runs["split"],
                          ("du", "status", "nwsr", "trace", "ntrace", "u_old", "du_old", "ws")):
        assert np.array_equal(a, b), f"fused and build + iterate differ in {what}"
    odu, ost, onw, ows, otr, ontr = c["oracle"]
    for mode, (du, st, nw, tr, ntr, u_g, du_g, ws_g) in runs.items():
        assert (st == 0).all(), mode
        bad, flagged = compare_step(B, cfg.S, K, (du, st, nw, ws_g, tr, ntr), (odu, ost, onw, ows, otr, ontr),
                                    c["margin"], np.zeros(B, bool))
        print(f"{name} {mode}: active {(ws_g != 0).mean():.2f}, scenarios differing at a flagged near-tie "
              f"{flagged.sum()}, unflagged {bad.sum()}, smallest oracle margin {c['margin'].min():.3g} "
              f"(NEAR_TIE {NEAR_TIE:g})")
        assert not bad.any(), np.flatnonzero(bad)[:10]
        assert flagged.sum() <= B // 32, flagged.sum()
        keep = np.repeat(~flagged, cfg.S)
        np.testing.assert_allclose(du[keep], odu[keep], rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(u_g[keep], c["u_after"][keep], rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(du_g[keep], odu[keep], rtol=1e-9, atol=1e-10)
        assert (ws_g != 0).mean() >= 0.25
