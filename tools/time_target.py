"""Time the steady-state target solve: cmpc_sim_target at one
batch size (65 536 scenarios by default) for both plants, from
cmpc_plant_default at seeded per-scenario pressures, holding outputs 0 and 1 at
the values they have in the default state with both torques free, beside
cmpc_sim_equilibrium on the same batch in the same process.

Both solves move the state, so every timed call starts from a fresh
cmpc_sim_reset (which synchronises); a pair of device events on torch's
stream brackets the one launch.  After a settle loop: median and range over
the calls, the statuses and the split of the scenarios by iteration count.

    python tools/time_target.py [B]
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
from cmpc.sim import EQ_MAX_ITER, EQ_TOL, TARGET_TOL_Y, PlantSimulator  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
N = int(os.environ.get("CMPC_TT_N", "20"))
SEED = 20261021
HOLD = np.array([0, 1], np.int32)
FREE = np.array([0, 2], np.int32)   # the torques


def main():
    torch.cuda.init()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    for plant, name in ((0, "parallel"), (1, "serial")):
        rng = np.random.default_rng(SEED + plant)
        x0, u0 = cmpc.plant_default(plant)
        tp = dev(rng.uniform(0.95, 1.05, (B, 2)))
        tu, tx = dev(np.tile(u0, (B, 1))), dev(np.tile(x0, (B, 1)))
        tt = dev(np.tile(cmpc.plant_output(plant, x0)[HOLD], (B, 1)))
        with PlantSimulator(plant, B) as sim:
            sim.bind_pressures(tp.data_ptr())

            def timed(launch):
                sim.reset(tx, tu)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch()
                b.record()
                b.synchronize()
                return a.elapsed_time(b) * 1e3

            target = lambda: check(sim.lib.cmpc_sim_target(sim._h, 2, iptr(HOLD), iptr(FREE), tt.data_ptr(), EQ_MAX_ITER,
                                                           EQ_TOL, TARGET_TOL_Y), "cmpc_sim_target")
            rest = lambda: check(sim.lib.cmpc_sim_equilibrium(sim._h, EQ_MAX_ITER, EQ_TOL), "cmpc_sim_equilibrium")
            t_end = time.perf_counter() + 0.3
            while time.perf_counter() < t_end:
                timed(target)
                timed(rest)
            for what, launch, download in (("cmpc_sim_target", target, sim.lib.cmpc_sim_target_download),
                                           ("cmpc_sim_equilibrium", rest, sim.lib.cmpc_sim_equilibrium_download)):
                us = [timed(launch) for _ in range(N)]
                st, it = np.zeros(B, np.int32), np.zeros(B, np.int32)
                check(download(sim._h, iptr(st), iptr(it), None), what + "_download")
                print(f"{what}, {name} plant, B = {B}, {N} calls: median {np.median(us):8.1f} us "
                      f"(min {min(us):.1f}, max {max(us):.1f})")
                print(f"  statuses {np.bincount(st).tolist()}, iterations {np.bincount(it).tolist()}")


if __name__ == "__main__":
    main()
