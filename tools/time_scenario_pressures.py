"""Time a closed-loop step (cmpc/driver.py ClosedLoop.step: plant output,
observe_step, build, K iterations, observe_apply, delay line, one plant
interval) with per-scenario boundary pressures in force against unset, at one
batch size (coop-par, p = 50, K = 9, 1024 scenarios by default): device events
around windows of back-to-back steps, after a settle loop, the configurations
alternating over several rounds, one ClosedLoop each.

  unset     the scalars (1, 1): the scalar sim instance, the producer's pointer null
  set       plant and model arrays bound (the model follows the plant)
  schedule  the same with a plant schedule: one (B, 2) device copy more per step

    python tools/time_scenario_pressures.py [B] [p]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "compressor-mpc_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import cmpc  # noqa: E402
from cmpc.configs import reference_setup  # noqa: E402
from cmpc.driver import ClosedLoop  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
P = int(sys.argv[2]) if len(sys.argv) > 2 else 50
PLANT, CTYPE = os.environ.get("CMPC_TSP_CASE", "par-coop").split("-")
N, ROUNDS, K = int(os.environ.get("CMPC_TSP_N", "50")), int(os.environ.get("CMPC_TSP_ROUNDS", "5")), 9


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main():
    torch.cuda.init()
    cfg = cmpc.reference_config(PLANT, CTYPE, p=P)
    arr = cmpc.controller_arrays(cfg, reference_setup(PLANT, CTYPE))
    rng = np.random.default_rng(5)
    x0, u_def = cmpc.plant_default(cfg.plant)
    xs = x0[None, :] * (1 + 0.002 * rng.uniform(-1, 1, (B, len(x0))))
    press = 0.95 + 0.1 * (rng.permutation(2 * B) + 0.5).reshape(B, 2) / (2 * B)
    M = [cmpc.reference_observer_gain(cfg)] * cfg.S
    kinds = {"unset": {}, "set": dict(pressures=press), "schedule": dict(pressures=press)}
    loops = {}
    for kind, kw in kinds.items():
        loops[kind] = ClosedLoop(cfg, arr, M, xs, np.tile(u_def, (B, 1)), K, **kw)
        if kind == "schedule":
            loops[kind].set_pressure_schedule(np.repeat(press[:, None, :], 4, axis=1))
        loops[kind].initialize()
    try:
        for _ in range(3):                    # settle: clocks, allocations, first launches
            for loop in loops.values():
                for _ in range(20):
                    loop.step()
        torch.cuda.synchronize()
        t = {k: [] for k in kinds}
        for _ in range(ROUNDS):
            for kind, loop in loops.items():
                t[kind].append(window(loop.step, N))
        for kind, loop in loops.items():
            nfail, _ = loop.plant_failures()
            assert nfail == 0, (kind, nfail)
    finally:
        for loop in loops.values():
            loop.close()
    med = lambda v: float(np.median(v))
    print(f"{PLANT}-{CTYPE} p={cfg.p} K={K} B={B} ({B * cfg.S} QP slots), {ROUNDS} rounds x {N} closed-loop steps, "
          f"the configurations alternating")
    for kind in kinds:
        print(f"    {kind:9s} per step: median {med(t[kind]) * 1e3:8.1f} us   rounds "
              + " ".join(f"{x * 1e3:.1f}" for x in t[kind]))
    u = med(t["unset"])
    for kind in ("set", "schedule"):
        print(f"{kind} / unset: {med(t[kind]) / u:.3f}  ({(med(t[kind]) - u) * 1e3:+.1f} us)")


if __name__ == "__main__":
    main()
