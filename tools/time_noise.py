"""Time the seeded noise and the ensemble statistics:

  1. cmpc_noise_step at one batch size (65 536 scenarios by default) for n = 4
     and n = the plant's input count, white and AR(1), beside the algorithmic
     bytes (sigma, base read, out written; rho read and w read and written for
     the AR(1)) over 8 TB/s as the floor;
  2. a ClosedLoop.step without noise and with measurement noise and an AR(1)
     input disturbance in force (a library without set_noise, an earlier
     commit's, times the plain step alone);
  3. cmpc_score_ensemble per call on that loop's record.

Device events around windows of back-to-back calls on torch's stream, after a
settle loop, the variants alternating over several rounds; medians.
score_ensemble ends with a small copy to the host and a stream synchronisation,
so its window measures launch-to-result latency of one call after another.

    python tools/time_noise.py [B] [loop B]
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
from cmpc.driver import ClosedLoop  # noqa: E402

HBM_BYTES_PER_S = 8e12
B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
LOOP_B = int(sys.argv[2]) if len(sys.argv) > 2 else B
N, ROUNDS = int(os.environ.get("CMPC_TN_N", "50")), int(os.environ.get("CMPC_TN_ROUNDS", "5"))
LOOP_N = int(os.environ.get("CMPC_TN_LOOP_N", "10"))
SEED = 20261020


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def alternate(fns, n):
    t_end = time.perf_counter() + 0.3   # the clock ramps over the first tens of ms of load
    while time.perf_counter() < t_end:
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            t[k].append(window(fn, n))
    return t


def report(t, extra=lambda k: ""):
    for k, v in t.items():
        print(f"{k:22s} per call: median {np.median(v) * 1e3:8.1f} us   rounds " +
              " ".join(f"{x * 1e3:.1f}" for x in v) + extra(k))


def time_kernel(ni):
    if not hasattr(cmpc, "noise_step"):
        return
    fns, bytes_ = {}, {}
    keep = []
    for n in sorted({4, ni}):
        new = lambda: torch.rand(B, n, dtype=torch.float64, device="cuda:0")
        sigma, rho, w, base, out = new(), new(), new(), new(), new()
        keep.append((sigma, rho, w, base, out))
        step = [0]

        def white(sigma=sigma, base=base, out=out):
            step[0] += 1
            cmpc.noise_step(SEED, step[0], out, sigma=sigma, base=base)

        def ar1(sigma=sigma, rho=rho, w=w, base=base, out=out):
            step[0] += 1
            cmpc.noise_step(SEED, step[0], out, sigma=sigma, rho=rho, w=w, base=base, stream=1)

        fns[f"n={n} white"], bytes_[f"n={n} white"] = white, 8 * B * n * 3
        fns[f"n={n} AR(1)"], bytes_[f"n={n} AR(1)"] = ar1, 8 * B * n * 6
    t = alternate(fns, N)
    print(f"cmpc_noise_step, B = {B}, {ROUNDS} rounds x {N} calls each, alternating")
    report(t, lambda k: f"   {bytes_[k] / 1e6:.1f} MB, floor at 8 TB/s {bytes_[k] / HBM_BYTES_PER_S * 1e6:.2f} us")


def time_loop():
    cfg = cmpc.reference_config("par", "coop", p=50)
    arr = cmpc.controller_arrays(cfg, reference_setup("par", "coop"))
    x0, u_def = cmpc.plant_default(cfg.plant)
    M = cmpc.reference_observer_gain(cfg)
    Bl = LOOP_B

    def make(noise):
        loop = ClosedLoop(cfg, arr, [M] * cfg.S, np.tile(x0, (Bl, 1)), np.tile(u_def, (Bl, 1)), 9)
        if noise:
            loop.set_noise(SEED, sigma_y=np.full(4, 2e-4), sigma_u=np.full(len(u_def), 2e-3),
                           rho_u=np.full(len(u_def), 0.8))
        loop.enable_scores(band=np.full((cfg.S, cfg.ny), 1e-3))
        loop.initialize()
        return loop

    loops = {"step": make(False)}
    if hasattr(ClosedLoop, "set_noise"):
        loops["step with noise"] = make(True)
    fns = {k: (lambda l=l: l.step()) for k, l in loops.items()}
    t = alternate(fns, LOOP_N)
    print(f"ClosedLoop.step (scored), par-coop p = 50, K = 9, B = {Bl}, {ROUNDS} rounds x {LOOP_N} steps each, "
          "alternating")
    report(t)
    loop = loops["step"]
    if hasattr(loop, "score_ensemble"):
        dims = loop.ctx.dims
        thr = np.zeros(cmpc.score_len(dims))
        te = alternate({"score_ensemble": lambda: loop.score_ensemble(thr)}, N)
        rows = cmpc.score_len(dims) * cfg.S
        print(f"cmpc_score_ensemble: record {cmpc.score_len(dims)} x {Bl * cfg.S} doubles "
              f"({8 * cmpc.score_len(dims) * Bl * cfg.S / 1e6:.1f} MB, read twice), {rows} rows x 6 out")
        report(te)
    for l in loops.values():
        l.close()


if __name__ == "__main__":
    torch.cuda.init()
    time_kernel(len(cmpc.plant_default(cmpc.reference_config("par", "coop", p=50).plant)[1]))
    time_loop()
