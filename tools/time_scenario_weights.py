"""Time cmpc_build with per-scenario weights (cmpc_set_scenario_weights, the
SCW instances of build_wave_body in csrc/cmpc_kernels.hip) at the bench shape
(coop-par, p = 50, 65 536 scenarios = 131 072 QP slots by default): device
events around windows of back-to-back builds on the context's stream, after a
settle loop, the three configurations alternating over several rounds.

(a) per-slot weights in force (the build is the one-QP-per-wave kernel's
    weights instance) against CMPC_BUILD_WAVE forced with shared weights: the
    price of the per-wave tables (13 doubles loaded and (p + 1) ny (ny + 1) / 2
    multiply-adds per QP, and the LDS they take).  The plain instances' code
    is byte for byte that of the commit before per-slot weights existed
    (tools/kernel_hash.py over both libraries), so the forced build is that
    commit's.
(b) the same against the unset CMPC_BUILD_AUTO build (the row build, at this
    size its shared form): the price of a weight sweep in one batch while the
    row build does not take per-slot weights.

    python tools/time_scenario_weights.py [B] [p]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "compressor-mpc_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import cmpc  # noqa: E402
from cmpc.configs import reference_setup  # noqa: E402
from cmpc.synthetic import synthetic_batch  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
P = int(sys.argv[2]) if len(sys.argv) > 2 else 50
PLANT, CTYPE = os.environ.get("CMPC_TSW_CASE", "par-coop").split("-")
N, ROUNDS = int(os.environ.get("CMPC_TSW_N", "30")), int(os.environ.get("CMPC_TSW_ROUNDS", "5"))
KERNEL = {cmpc.CMPC_BUILD_WAVE: "wave", cmpc.CMPC_BUILD_ROWS: "rows", cmpc.CMPC_BUILD_SPLIT: "split"}


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def draw(rng, cfg, arr, nq):
    """dense SPD ywt and symmetric positive uwt per slot, on the shared weights' scale"""
    ny, nu = cfg.ny, cfg.nu
    s = np.arange(nq) % cfg.S
    ys = np.abs(arr.ywt).reshape(cfg.S, -1).max(axis=1)[s][:, None, None]
    us = np.abs(arr.uwt).reshape(cfg.S, -1).max(axis=1)[s][:, None, None]
    R = rng.uniform(-1.0, 1.0, (nq, ny, ny))
    ywt = ys * (np.einsum("qij,qkj->qik", R, R) / ny + 0.5 * np.eye(ny))
    Q = rng.uniform(0.1, 0.4, (nq, nu, nu))
    uwt = us * (0.5 * (Q + Q.transpose(0, 2, 1)) + nu * np.eye(nu))
    return np.ascontiguousarray(uwt), np.ascontiguousarray(ywt)


def main():
    torch.cuda.init()
    cfg = cmpc.reference_config(PLANT, CTYPE, p=P)
    arr = cmpc.controller_arrays(cfg, reference_setup(PLANT, CTYPE))
    lin, u, du, ws = synthetic_batch(cfg, B, seed=7, n_distinct=256)
    nq = B * cfg.S
    uwt, ywt = draw(np.random.default_rng(3), cfg, arr, nq)
    with cmpc.Context(cfg, B) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.configure(arr)
        ctx.set_state(u, du, ws)
        ctx.upload_lin(lin)
        ctx.set_scenario_weights(uwt, ywt)
        u_dev, lw_dev = ctx.get_scenario_weights()
        packed = torch.from_numpy(np.concatenate([lw_dev.reshape(nq, -1), u_dev.reshape(nq, -1)], axis=1)).cuda()

        def config(kind):
            ctx.bind_scenario_weights(packed.data_ptr() if kind == "weights" else 0)
            ctx.set_build_variant(cmpc.CMPC_BUILD_WAVE if kind == "wave" else cmpc.CMPC_BUILD_AUTO)

        kinds = ("weights", "wave", "auto")
        seen = {}
        t_end = time.perf_counter() + 0.3   # the clock ramps over the first tens of ms of load
        while time.perf_counter() < t_end:
            for kind in kinds:
                config(kind)
                for _ in range(4):
                    ctx.build()
                seen[kind] = KERNEL[ctx.last_build_kernel()]
            ctx.synchronize()
        t = {k: [] for k in kinds}
        for _ in range(ROUNDS):
            for kind in kinds:
                config(kind)
                ctx.build()
                t[kind].append(window(ctx.build, N))
        H, f, G = ctx.download_qp()
        assert np.isfinite(H).all() and np.isfinite(f).all()
        shared = ctx.last_build_shared_scenarios()
    med = lambda v: float(np.median(v))
    rounds = lambda v: " ".join(f"{x * 1e3:.1f}" for x in v)
    print(f"{PLANT}-{CTYPE} p={cfg.p} B={B} ({nq} QP slots), {ROUNDS} rounds x {N} builds, the three configurations "
          f"alternating")
    names = {"weights": f"per-slot weights ({seen['weights']}, weights instance)",
             "wave": f"shared weights, WAVE forced ({seen['wave']})",
             "auto": f"shared weights, AUTO ({seen['auto']}" + (", shared form" if shared >= 0 else "") + ")"}
    for kind in kinds:
        print(f"    {names[kind]:58s} per build: median {med(t[kind]) * 1e3:8.1f} us   rounds {rounds(t[kind])}")
    w, v, a = med(t["weights"]), med(t["wave"]), med(t["auto"])
    print(f"(a) per-slot weights / WAVE forced: {w / v:.3f}  ({(w - v) * 1e3:+.1f} us, {(w / v - 1) * 100:+.1f} %)")
    print(f"(b) per-slot weights / AUTO:        {w / a:.3f}  ({(w - a) * 1e3:+.1f} us)")


if __name__ == "__main__":
    main()
