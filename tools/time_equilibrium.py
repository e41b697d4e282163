"""Time the plant equilibrium solve: cmpc_sim_equilibrium at
one batch size (65 536 scenarios by default) for both plants, from
cmpc_plant_default at seeded per-scenario pressures and input offsets (the
cases of tests/equilibrium_cases.py), and again from the equilibrium itself
(every scenario returns at iteration 0: one linearisation and one elimination
pass, the loop's floor).

The solve moves the state, so every timed call starts from a fresh
cmpc_sim_reset (which synchronises); a pair of device events on torch's
stream brackets the one launch.  After a settle loop, medians over the calls.

    python tools/time_equilibrium.py [B]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "compressor-mpc_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import cmpc  # noqa: E402
from cmpc._abi import check, iptr  # noqa: E402
from cmpc.sim import EQ_MAX_ITER, EQ_TOL, PlantSimulator  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
N = int(os.environ.get("CMPC_TE_N", "20"))
SEED = 20261021


def cases(plant):
    rng = np.random.default_rng(SEED + plant)
    x0, u0 = cmpc.plant_default(plant)
    p = rng.uniform(0.95, 1.05, (B, 2))
    u = np.tile(u0, (B, 1)) + rng.uniform(-0.02, 0.02, (B, len(u0))) * (u0 != 0)
    return p, u, np.tile(x0, (B, 1))


def main():
    torch.cuda.init()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    for plant, name in ((0, "parallel"), (1, "serial")):
        p, u, x0 = cases(plant)
        tp, tu, tx = dev(p), dev(u), dev(x0)
        with PlantSimulator(plant, B) as sim:
            sim.bind_pressures(tp.data_ptr())

            def solve(x):
                sim.reset(x, tu)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                check(sim.lib.cmpc_sim_equilibrium(sim._h, EQ_MAX_ITER, EQ_TOL), "cmpc_sim_equilibrium")
                b.record()
                b.synchronize()
                return a.elapsed_time(b) * 1e3

            t_end = time.perf_counter() + 0.3
            while time.perf_counter() < t_end:
                solve(tx)
            cold = [solve(tx) for _ in range(N)]
            st, it = np.zeros(B, np.int32), np.zeros(B, np.int32)
            check(sim.lib.cmpc_sim_equilibrium_download(sim._h, iptr(st), iptr(it), None),
                  "cmpc_sim_equilibrium_download")
            x_eq = dev(sim.download()[0])
            warm = [solve(x_eq) for _ in range(N)]
            print(f"cmpc_sim_equilibrium, {name} plant, B = {B}, {N} calls: statuses {np.bincount(st).tolist()}, "
                  f"iterations {np.bincount(it).tolist()}")
            print(f"  from cmpc_plant_default: median {np.median(cold):8.1f} us (min {min(cold):.1f}, max {max(cold):.1f})")
            print(f"  from the equilibrium:    median {np.median(warm):8.1f} us (min {min(warm):.1f}, max {max(warm):.1f})")


if __name__ == "__main__":
    main()
