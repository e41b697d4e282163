"""Time the steady-state gains: cmpc_sim_gains at one batch
size (65 536 scenarios by default) for both plants, at seeded per-scenario
pressures with every scenario first brought to its equilibrium, outputs 0 and
1 against both torques (2 x 2) and all four against all four, beside
cmpc_sim_equilibrium on the same batch in the same process.

cmpc_sim_gains writes nothing of the simulator, so the timed calls repeat on
one state; the equilibrium solve moves the state, so each of its timed calls
starts from a fresh cmpc_sim_reset at cmpc_plant_default (which
synchronises).  A pair of device events on torch's stream brackets the one
launch.  After a settle loop: median and range over the calls and the
statuses.

    python tools/time_gains.py [B]
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
N = int(os.environ.get("CMPC_TG_N", "20"))
SEED = 20261021
SELECTIONS = ((np.array([0, 1], np.int32), np.array([0, 2], np.int32)),
              (np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int32)))


def main():
    torch.cuda.init()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    for plant, name in ((0, "parallel"), (1, "serial")):
        rng = np.random.default_rng(SEED + plant)
        x0, u0 = cmpc.plant_default(plant)
        u0 = u0.copy()
        u0[[3, 7]] = 0.1                      # both recycle valves open: every B column is exact
        tp = dev(rng.uniform(0.95, 1.05, (B, 2)))
        tu, tx = dev(np.tile(u0, (B, 1))), dev(np.tile(x0, (B, 1)))
        with PlantSimulator(plant, B) as sim:
            sim.bind_pressures(tp.data_ptr())

            def timed(launch, reset):
                if reset:
                    sim.reset(tx, tu)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch()
                b.record()
                b.synchronize()
                return a.elapsed_time(b) * 1e3

            rest = lambda: check(sim.lib.cmpc_sim_equilibrium(sim._h, EQ_MAX_ITER, EQ_TOL), "cmpc_sim_equilibrium")
            gains = [(lambda o=o, i=i: check(sim.lib.cmpc_sim_gains(sim._h, len(o), iptr(o), len(i), iptr(i)),
                                             "cmpc_sim_gains")) for o, i in SELECTIONS]
            t_end = time.perf_counter() + 0.3
            while time.perf_counter() < t_end:
                timed(rest, True)
                for g in gains:
                    timed(g, False)
            us = [timed(rest, True) for _ in range(N)]          # the last one leaves every scenario at rest
            st = np.zeros(B, np.int32)
            check(sim.lib.cmpc_sim_equilibrium_download(sim._h, iptr(st), None, None), "cmpc_sim_equilibrium_download")
            print(f"cmpc_sim_equilibrium, {name} plant, B = {B}, {N} calls: median {np.median(us):8.1f} us "
                  f"(min {min(us):.1f}, max {max(us):.1f}); statuses {np.bincount(st).tolist()}")
            for (o, i), g in zip(SELECTIONS, gains):
                us = [timed(g, False) for _ in range(N)]
                check(sim.lib.cmpc_sim_gains_download(sim._h, None, iptr(st)), "cmpc_sim_gains_download")
                print(f"cmpc_sim_gains {len(o)} x {len(i)}, {name} plant, B = {B}, {N} calls: median "
                      f"{np.median(us):8.1f} us (min {min(us):.1f}, max {max(us):.1f}); statuses "
                      f"{np.bincount(st).tolist()}")


if __name__ == "__main__":
    main()
