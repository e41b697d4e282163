"""Time cmpc_predict beside cmpc_build at the bench shape (coop-par, p = 50,
65 536 scenarios = 131 072 QP slots by default): device events around windows
of back-to-back calls on the context's stream, after a settle loop, the two
kernels alternating over several rounds.  Prints the time per call, the
predict kernel's algorithmic bytes (records, state and plans read; y_pred and
cost written) over 8 TB/s as its floor, the ratio of the measured time to
that floor, and the kernel's registers, scratch, LDS and occupancy as the
compiler reports them.

    python tools/time_predict.py [B] [p]
"""
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "compressor-mpc_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import cmpc  # noqa: E402
from cmpc.configs import reference_setup  # noqa: E402
from cmpc.synthetic import synthetic_batch  # noqa: E402

HBM_BYTES_PER_S = 8e12
B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
P = int(sys.argv[2]) if len(sys.argv) > 2 else 50
PLANT, CTYPE = os.environ.get("CMPC_TP_CASE", "par-coop").split("-")
N, ROUNDS = int(os.environ.get("CMPC_TP_N", "50")), int(os.environ.get("CMPC_TP_ROUNDS", "5"))


def resource_usage(ns, ny, nu, m):
    """the compiler's report for the instance, or None without hipcc"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        return None
    csrc = os.path.join(ROOT, "compressor-mpc_amd", "csrc")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-c",
                          "predict.hip", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                         cwd=csrc, capture_output=True, text=True).stderr
    tag = f"cmpc_predict_kernelILi{ns}ELi{ny}ELi{nu}ELi{m}E"
    got, on = {}, False
    for ln in out.splitlines():
        if "Function Name" in ln:
            on = tag in ln
        elif on:
            mt = re.search(r"remark:\s+(VGPRs|AGPRs|SGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                           r"LDS Size \[bytes/block\]): (\d+)", ln)
            if mt:
                got[mt.group(1)] = int(mt.group(2))
    return got or None


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
    lin, u, du, ws = synthetic_batch(cfg, B, seed=7, n_distinct=256)
    nq = B * cfg.S
    with cmpc.Context(cfg, B) as ctx:
        L = ctx.layout
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.configure(arr)
        ctx.set_state(u, du, ws)
        ctx.upload_lin(lin)
        ctx.build()
        ctx.init_warmstart()
        ctx.iterate(3, 0)
        ctx.predict()
        ctx.synchronize()
        t_end = time.perf_counter() + 0.3   # the clock ramps over the first tens of ms of load
        while time.perf_counter() < t_end:
            for _ in range(8):
                ctx.build()
                ctx.predict()
            ctx.synchronize()
        tb, tp = [], []
        for _ in range(ROUNDS):
            tb.append(window(ctx.build, N))
            tp.append(window(ctx.predict, N))
        y, cost = ctx.download_prediction()
        assert np.isfinite(y).all() and np.isfinite(cost).all()
        kernel = {cmpc.CMPC_BUILD_WAVE: "wave", cmpc.CMPC_BUILD_ROWS: "rows",
                  cmpc.CMPC_BUILD_SPLIT: "split"}[ctx.last_build_kernel()]
    read = 8 * nq * (L.rec_len + cfg.nu_tot + L.nV + L.nVo)
    written = 8 * nq * (cfg.p * cfg.ny + 2)
    floor_ms = (read + written) / HBM_BYTES_PER_S * 1e3
    med_b, med_p = float(np.median(tb)), float(np.median(tp))
    print(f"{PLANT}-{CTYPE} p={cfg.p} B={B} ({nq} QP slots), {ROUNDS} rounds x {N} calls per kernel, alternating")
    print(f"build   ({kernel}) per call: median {med_b * 1e3:8.1f} us   rounds " +
          " ".join(f"{v * 1e3:.1f}" for v in tb))
    print(f"predict        per call: median {med_p * 1e3:8.1f} us   rounds " +
          " ".join(f"{v * 1e3:.1f}" for v in tp))
    print(f"predict algorithmic bytes: {read / 1e6:.1f} MB read + {written / 1e6:.1f} MB written = "
          f"{(read + written) / 1e6:.1f} MB; floor at 8 TB/s {floor_ms * 1e3:.1f} us")
    print(f"predict measured / floor: {med_p / floor_ms:.2f}   ({(read + written) / med_p / 1e9:.2f} TB/s achieved)")
    ru = resource_usage(cfg.ns, cfg.ny, cfg.nu, cfg.m)
    print(f"predict kernel <{cfg.ns}, {cfg.ny}, {cfg.nu}, {cfg.m}> resources: " +
          (", ".join(f"{k} {v}" for k, v in ru.items()) if ru else "not available (no hipcc)"))


if __name__ == "__main__":
    main()
