"""Time the plant-mode analysis: cmpc_sim_modes at one batch
size (65 536 scenarios by default) for both plants, at the equilibria of the
seeded per-scenario pressures and input offsets (the cases of
tests/equilibrium_cases.py), and cmpc_eig_device on the same number of seeded
Gaussian matrices.

The analysis writes nothing of the simulator, so the calls follow one another;
a pair of device events on torch's stream brackets the one launch.  After a
settle loop, medians and ranges over the calls.

    python tools/time_modes.py [B]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "compressor-mpc_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import cmpc  # noqa: E402
from cmpc._abi import check  # noqa: E402
from cmpc.sim import PlantSimulator  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
N = int(os.environ.get("CMPC_TM_N", "20"))
SEED = 20261021


def cases(plant):
    rng = np.random.default_rng(SEED + plant)
    x0, u0 = cmpc.plant_default(plant)
    p = rng.uniform(0.95, 1.05, (B, 2))
    u = np.tile(u0, (B, 1)) + rng.uniform(-0.02, 0.02, (B, len(u0))) * (u0 != 0)
    return p, u, np.tile(x0, (B, 1))


def timed(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def report(what, call):
    t_end = time.perf_counter() + 0.3
    while time.perf_counter() < t_end:
        timed(call)
    t = [timed(call) for _ in range(N)]
    print(f"  {what}: median {np.median(t):8.1f} us (min {min(t):.1f}, max {max(t):.1f})")


def main():
    torch.cuda.init()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    for plant, name in ((0, "parallel"), (1, "serial")):
        p, u, x0 = cases(plant)
        tp, tu, tx = dev(p), dev(u), dev(x0)
        with PlantSimulator(plant, B) as sim:
            sim.bind_pressures(tp.data_ptr())
            sim.reset(tx, tu)
            st_eq = sim.equilibrium()[0]
            w, sm, st, it = sim.modes()
            print(f"cmpc_sim_modes, {name} plant, B = {B}, {N} calls: equilibrium statuses "
                  f"{np.bincount(st_eq).tolist()}, statuses {np.bincount(st).tolist()}, sweeps {it.min()} to "
                  f"{it.max()} (mean {it.mean():.1f}), zeta_min {np.nanmin(sm[:, 2]):.3f} to {np.nanmax(sm[:, 2]):.3f}, "
                  f"abscissa {np.nanmin(sm[:, 0]):.4f} to {np.nanmax(sm[:, 0]):.4f}")
            report("at the equilibria", lambda: check(sim.lib.cmpc_sim_modes(sim._h, 30 * sim.ns), "cmpc_sim_modes"))
    for n in (10, 11):
        A = torch.from_numpy(np.random.default_rng(SEED).standard_normal((B, n, n))).cuda()
        wr, wi, st, it = cmpc.eig_batch_device(A)
        torch.cuda.synchronize()
        it = it.cpu().numpy()
        print(f"cmpc_eig_device, n = {n}, B = {B} Gaussian matrices: statuses {np.bincount(st.cpu().numpy()).tolist()}, "
              f"sweeps {it.min()} to {it.max()} (mean {it.mean():.1f})")
        report("one launch", lambda: cmpc.eig_batch_device(A))


if __name__ == "__main__":
    main()
