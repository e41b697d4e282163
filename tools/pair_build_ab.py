#!/usr/bin/env python3
"""A/B of the forced row build with pairing on (the shared form,
build_pair_kernel.h) between several libcmpc builds: alternating rounds, each
arm in a process of its own, the build kernel by events over --builds launches
after a clock settle, and the QP buffer (H, f, G) of every arm compared bit
for bit with the first arm's.  GPU only.
usage: python tools/pair_build_ab.py NAME=LIB [NAME=LIB ...] [--rounds 5] [--builds 40] [-p 50] [-B 65536]
       [--pairing on|off]"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import sys, time, numpy as np
sys.path.insert(0, sys.argv[1])
import cmpc
from cmpc.configs import reference_setup
from cmpc.synthetic import synthetic_batch
p, B, builds, pairing, out = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5], sys.argv[6]
cfg = cmpc.reference_config("par", "coop", p=p)
arr = cmpc.controller_arrays(cfg, reference_setup("par", "coop"))
lin, u, du, ws = synthetic_batch(cfg, B, seed=7, n_distinct=min(B, 256))
with cmpc.Context(cfg, B) as ctx:
    ctx.configure(arr); ctx.set_state(u, du, ws); ctx.upload_lin(lin)
    ctx.set_build_variant(cmpc.CMPC_BUILD_ROWS)
    ctx.set_build_pairing(cmpc.CMPC_PAIRING_ON if pairing == "on" else cmpc.CMPC_PAIRING_OFF)
    t_end = time.perf_counter() + 0.3  # settle at the steady clock (DESIGN section 7)
    while time.perf_counter() < t_end:
        for _ in range(16):
            ctx.build()
        ctx.synchronize()
    ctx.enable_timing(True, only=(cmpc.CMPC_KERNEL_BUILD,))
    for _ in range(builds):
        ctx.build()
    ctx.synchronize()
    ms, n = ctx.kernel_time(cmpc.CMPC_KERNEL_BUILD)
    shared = ctx.last_build_shared_scenarios()
    H, f, G = ctx.download_qp()
np.savez(out, H=H, f=f, G=G)
print(f"{ms / n * 1e3:.2f} {shared}")
'''


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("arms", nargs="+", help="NAME=LIB")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--builds", type=int, default=40)
    ap.add_argument("-p", type=int, default=50)
    ap.add_argument("-B", type=int, default=65536)
    ap.add_argument("--pairing", default="on", choices=("on", "off"))
    a = ap.parse_args()
    arms = [x.split("=", 1) for x in a.arms]
    first, bad = None, 0
    times = {n: [] for n, _ in arms}
    with tempfile.TemporaryDirectory() as td:
        for rnd in range(a.rounds):
            for name, lib in arms:
                out = os.path.join(td, "qp.npz")
                env = dict(os.environ, CMPC_LIBRARY=os.path.abspath(lib))
                r = subprocess.run([sys.executable, "-c", CHILD, os.path.join(ROOT, "compressor-mpc_amd"), str(a.p),
                                    str(a.B), str(a.builds), a.pairing, out], env=env, check=True, timeout=300,
                                   stdout=subprocess.PIPE, text=True)
                us, shared = r.stdout.split()[-2:]
                qp = np.load(out)
                qp = {k: qp[k].view(np.uint64) for k in ("H", "f", "G")}
                if first is None:
                    first = qp
                same = all(np.array_equal(first[k], qp[k]) for k in first)
                bad += not same
                times[name].append(float(us))
                print(f"p={a.p} B={a.B} pairing={a.pairing} round={rnd} {name} build_us={us} shared={shared} "
                      f"qp_same_as_first={same}", flush=True)
    for name, t in times.items():
        print(f"{name}: {min(t):.2f}-{max(t):.2f} us (median {np.median(t):.2f})")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
