"""Time the reference-profile correction (cmpc_set_scenario_reference_profile,
csrc/refshift.hip) at the bench shape (coop-par, p = 50, 65 536 scenarios =
131 072 QP slots by default): device events around windows of back-to-back
calls on the context's stream, after a settle loop, profile bound and unset
alternating over several rounds.

(a) cmpc_build with the profile bound against unset: the difference is the
    correction kernel, which cmpc_build launches right after its build kernel
    on the same stream.  Beside it cmpc_predict (the same dependent-chain
    length), the kernel's byte floor at 8 TB/s (per slot the record, p*ny*8
    bytes of profile and an nV*8 read-modify-write of f) and the compiler's
    resource report.
(b) the headline step, cmpc_step(9, CMPC_APPLY_MOVE) with CMPC_STEP_SPLIT
    forced, profile bound against unset.

    python tools/time_reference_profile.py [B] [p]
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
from cmpc._abi import CMPC_STEP_SPLIT  # noqa: E402
from cmpc.configs import reference_setup  # noqa: E402
from cmpc.synthetic import synthetic_batch  # noqa: E402

HBM_BYTES_PER_S = 8e12
B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
P = int(sys.argv[2]) if len(sys.argv) > 2 else 50
PLANT, CTYPE = os.environ.get("CMPC_TRP_CASE", "par-coop").split("-")
N, ROUNDS = int(os.environ.get("CMPC_TRP_N", "50")), int(os.environ.get("CMPC_TRP_ROUNDS", "5"))
K = 9


def resource_usage(ns, ny, nu, m):
    """the compiler's report for the instance, or None without hipcc"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        return None
    csrc = os.path.join(ROOT, "compressor-mpc_amd", "csrc")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-c",
                          "refshift.hip", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                         cwd=csrc, capture_output=True, text=True).stderr
    tag = f"cmpc_refshift_kernelILi{ns}ELi{ny}ELi{nu}ELi{m}E"
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
    dref = torch.empty(nq, cfg.p, cfg.ny, dtype=torch.float64, device="cuda").uniform_(-0.02, 0.02)
    with cmpc.Context(cfg, B) as ctx:
        L = ctx.layout
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.configure(arr)
        ctx.set_step_variant(CMPC_STEP_SPLIT)
        ctx.set_state(u, du, ws)
        ctx.upload_lin(lin)
        ctx.build()
        ctx.init_warmstart()
        ctx.iterate(3, 0)
        ctx.predict()
        ctx.synchronize()
        bound = lambda on: ctx.bind_scenario_reference_profile(dref.data_ptr() if on else 0)
        step = lambda: ctx.step(K, cmpc.CMPC_APPLY_MOVE)
        t_end = time.perf_counter() + 0.3   # the clock ramps over the first tens of ms of load
        while time.perf_counter() < t_end:
            for on in (True, False):
                bound(on)
                for _ in range(4):
                    ctx.build()
                    ctx.predict()
            ctx.synchronize()
        tb = {True: [], False: []}
        ts = {True: [], False: []}
        tp = []
        for _ in range(ROUNDS):
            for on in (True, False):
                bound(on)
                tb[on].append(window(ctx.build, N))
            tp.append(window(ctx.predict, N))
        for _ in range(ROUNDS):
            for on in (True, False):
                bound(on)
                ctx.set_state(u, du, ws)
                step()
                ts[on].append(window(step, N))
        du_out, status, _ = ctx.download()
        assert np.isfinite(du_out).all()
        kernel = {cmpc.CMPC_BUILD_WAVE: "wave", cmpc.CMPC_BUILD_ROWS: "rows",
                  cmpc.CMPC_BUILD_SPLIT: "split"}[ctx.last_build_kernel()]
    med = lambda v: float(np.median(v))
    rounds = lambda v: " ".join(f"{x * 1e3:.1f}" for x in v)
    nbytes = 8 * nq * (L.rec_len + cfg.p * cfg.ny + 2 * L.nV)
    floor_ms = nbytes / HBM_BYTES_PER_S * 1e3
    shift = med(tb[True]) - med(tb[False])
    print(f"{PLANT}-{CTYPE} p={cfg.p} B={B} ({nq} QP slots), {ROUNDS} rounds x {N} calls, profile bound / unset "
          f"alternating")
    print(f"(a) build ({kernel}) unset   per call: median {med(tb[False]) * 1e3:8.1f} us   rounds {rounds(tb[False])}")
    print(f"    build + correction   per call: median {med(tb[True]) * 1e3:8.1f} us   rounds {rounds(tb[True])}")
    print(f"    correction kernel (difference of the medians): {shift * 1e3:.1f} us")
    print(f"    predict              per call: median {med(tp) * 1e3:8.1f} us   rounds {rounds(tp)}")
    print(f"    correction algorithmic bytes: {nbytes / 1e6:.1f} MB (records, profile, f read and written); "
          f"floor at 8 TB/s {floor_ms * 1e3:.1f} us")
    print(f"    correction measured / floor: {shift / floor_ms:.2f}   ({nbytes / shift / 1e9:.2f} TB/s achieved); "
          f"correction / predict: {shift / med(tp):.2f}")
    print(f"(b) step K={K} split, unset  per call: median {med(ts[False]) * 1e3:8.1f} us   rounds {rounds(ts[False])}")
    print(f"    step K={K} split, bound  per call: median {med(ts[True]) * 1e3:8.1f} us   rounds {rounds(ts[True])}")
    print(f"    bound - unset: {(med(ts[True]) - med(ts[False])) * 1e3:.1f} us "
          f"({(med(ts[True]) / med(ts[False]) - 1) * 100:+.1f} %)")
    ru = resource_usage(cfg.ns, cfg.ny, cfg.nu, cfg.m)
    print(f"correction kernel <{cfg.ns}, {cfg.ny}, {cfg.nu}, {cfg.m}> resources: " +
          (", ".join(f"{k} {v}" for k, v in ru.items()) if ru else "not available (no hipcc)"))


if __name__ == "__main__":
    main()
