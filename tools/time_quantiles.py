"""Time the exact ensemble quantiles and the envelope:

  1. cmpc_score_quantiles with 3 levels (and with 8) on a closed loop's score
     record, beside cmpc_score_ensemble on the same record in the same process;
  2. a ClosedLoop.step with the envelope off and on (3 levels, and the
     statistics alone).

Device events around windows of back-to-back calls on torch's stream, after a
settle loop, the variants alternating over several rounds; medians and the
rounds.  score_quantiles and score_ensemble end with a small copy to the host
and a stream synchronisation, so their windows measure the launch-to-result
latency of one call after another.

    python tools/time_quantiles.py [loop B]
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

LOOP_B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
N, ROUNDS = int(os.environ.get("CMPC_TQ_N", "50")), int(os.environ.get("CMPC_TQ_ROUNDS", "5"))
LOOP_N = int(os.environ.get("CMPC_TQ_LOOP_N", "10"))
LEVELS3 = (0.05, 0.5, 0.95)
LEVELS8 = (0.0, 0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99)


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


def report(t):
    for k, v in t.items():
        print(f"{k:28s} per call: median {np.median(v) * 1e3:8.1f} us   range {min(v) * 1e3:.1f} .. "
              f"{max(v) * 1e3:.1f}   rounds " + " ".join(f"{x * 1e3:.1f}" for x in v))


def main():
    cfg = cmpc.reference_config("par", "coop", p=50)
    arr = cmpc.controller_arrays(cfg, reference_setup("par", "coop"))
    x0, u_def = cmpc.plant_default(cfg.plant)
    M = cmpc.reference_observer_gain(cfg)
    Bl = LOOP_B

    def make(levels):
        loop = ClosedLoop(cfg, arr, [M] * cfg.S, np.tile(x0, (Bl, 1)), np.tile(u_def, (Bl, 1)), 9)
        loop.enable_scores(band=np.full((cfg.S, cfg.ny), 1e-3))
        if levels is not None:
            loop.enable_envelope(1 << 14, levels)   # (more rows than the run has steps: none is dropped)
        loop.initialize()
        return loop

    loops = {"step": make(None), "step + envelope, 3 levels": make(LEVELS3), "step + envelope, 0 levels": make(())}
    fns = {k: (lambda l=l: l.step()) for k, l in loops.items()}
    t = alternate(fns, LOOP_N)
    print(f"ClosedLoop.step (scored), par-coop p = 50, K = 9, B = {Bl}, {ROUNDS} rounds x {LOOP_N} steps each, "
          "alternating")
    report(t)
    loop = loops["step"]
    dims = loop.ctx.dims
    n = cmpc.score_len(dims)
    thr = np.zeros(n)
    mb = 8 * n * Bl * cfg.S / 1e6
    print(f"score record {n} x {Bl * cfg.S} doubles ({mb:.1f} MB), {n * cfg.S} rows; {ROUNDS} rounds x {N} calls "
          "each, alternating")
    print(f"  cmpc_score_ensemble: 3 launches, the record read twice; cmpc_score_quantiles: 18 launches, the record "
          f"read 9 times ({9 * mb:.0f} MB)")
    report(alternate({"score_ensemble": lambda: loop.score_ensemble(thr),
                      "score_quantiles, 3 levels": lambda: loop.score_quantiles(LEVELS3),
                      "score_quantiles, 8 levels": lambda: loop.score_quantiles(LEVELS8)}, N))
    for l in loops.values():
        l.close()


if __name__ == "__main__":
    torch.cuda.init()
    main()
