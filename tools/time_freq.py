"""Time the plant frequency responses: cmpc_sim_freq at one
batch size (65 536 scenarios by default) for both plants, at seeded
per-scenario pressures with every scenario first brought to its equilibrium,
all four outputs against all four inputs, at one frequency and at 32 (a
logarithmic grid from 1e-2 to 1e2 rad/s), beside cmpc_sim_gains on the same
batch in the same process.

Neither call writes anything of the simulator, so the timed calls repeat on
one state.  The frequencies are uploaded inside the call; a pair of device
events on torch's stream brackets the upload and the one launch.  After a
settle loop: median and range over the calls and the statuses.

    python tools/time_freq.py [B]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "compressor-mpc_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import cmpc  # noqa: E402
from cmpc._abi import check, dptr, iptr  # noqa: E402
from cmpc.sim import EQ_MAX_ITER, EQ_TOL, PlantSimulator  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
N = int(os.environ.get("CMPC_TF_N", "20"))
SEED = 20261021
ALL = np.arange(4, dtype=np.int32)
LISTS = (np.array([31.6]), np.logspace(-2, 2, 32))


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
            sim.reset(tx, tu)
            check(sim.lib.cmpc_sim_equilibrium(sim._h, EQ_MAX_ITER, EQ_TOL), "cmpc_sim_equilibrium")
            st = np.zeros(B, np.int32)
            check(sim.lib.cmpc_sim_equilibrium_download(sim._h, iptr(st), None, None), "cmpc_sim_equilibrium_download")
            print(f"{name} plant, B = {B}: at rest, statuses {np.bincount(st).tolist()}")

            def timed(launch):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch()
                b.record()
                b.synchronize()
                return a.elapsed_time(b) * 1e3

            gains = lambda: check(sim.lib.cmpc_sim_gains(sim._h, 4, iptr(ALL), 4, iptr(ALL)), "cmpc_sim_gains")
            freq = [(lambda w=w: check(sim.lib.cmpc_sim_freq(sim._h, 4, iptr(ALL), 4, iptr(ALL), len(w), dptr(w)),
                                       "cmpc_sim_freq")) for w in LISTS]
            t_end = time.perf_counter() + 0.3
            while time.perf_counter() < t_end:
                timed(gains)
                timed(freq[0])
            timed(freq[1])                                      # (the record grows here, not in a timed call)
            us = [timed(gains) for _ in range(N)]
            check(sim.lib.cmpc_sim_gains_download(sim._h, None, iptr(st)), "cmpc_sim_gains_download")
            print(f"cmpc_sim_gains 4 x 4, {name} plant, B = {B}, {N} calls: median {np.median(us):8.1f} us "
                  f"(min {min(us):.1f}, max {max(us):.1f}); statuses {np.bincount(st).tolist()}")
            for w, f in zip(LISTS, freq):
                us = [timed(f) for _ in range(N)]
                check(sim.lib.cmpc_sim_freq_download(sim._h, None, None, iptr(st)), "cmpc_sim_freq_download")
                print(f"cmpc_sim_freq 4 x 4, nw = {len(w)}, {name} plant, B = {B}, {N} calls: median "
                      f"{np.median(us):8.1f} us (min {min(us):.1f}, max {max(us):.1f}); statuses "
                      f"{np.bincount(st).tolist()}")


if __name__ == "__main__":
    main()
