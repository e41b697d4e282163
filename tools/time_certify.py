"""Time cmpc_certify and cmpc_certify_summary beside the
iterate's K = 0 launch, which reads the same QP buffer, at one batch size
(coop-par, p = 50, 65 536 scenarios = 131 072 QP slots by default): device
events around windows of back-to-back calls on the context's stream, after a
settle loop, the three alternating over several rounds.  Prints the time per
call, the certify kernel's algorithmic bytes (the QP record, plans, state,
limits, working-set and status words read; the record written) over 8 TB/s as
its floor, and the fraction of that peak the measured time reaches.

cmpc_certify_summary ends with a 64-byte copy to the host and a stream
synchronisation, so its window measures launch-to-result latency of one call
after another, not back-to-back kernels.

    python tools/time_certify.py [B] [p]
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
from cmpc.synthetic import synthetic_batch  # noqa: E402

HBM_BYTES_PER_S = 8e12
B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
P = int(sys.argv[2]) if len(sys.argv) > 2 else 50
PLANT, CTYPE = os.environ.get("CMPC_TC_CASE", "par-coop").split("-")
N, ROUNDS, K = int(os.environ.get("CMPC_TC_N", "50")), int(os.environ.get("CMPC_TC_ROUNDS", "5")), 9


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
        ctx.iterate(K, 0)
        ctx.certify()
        summary = ctx.certify_summary(1e-9)
        fns = {"certify": ctx.certify, "summary": lambda: ctx.certify_summary(1e-9),
               "iterate K=0": lambda: ctx.iterate(0, 0)}
        t_end = time.perf_counter() + 0.3   # the clock ramps over the first tens of ms of load
        while time.perf_counter() < t_end:
            for _ in range(8):
                for fn in fns.values():
                    fn()
            ctx.synchronize()
        t = {k: [] for k in fns}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                t[k].append(window(fn, N))
        rec = ctx.certify_download()
        assert all(np.isfinite(v).all() for v in rec.values())
    qp_len = L.nV * L.nV + L.nV + L.nV * L.nVo
    read = nq * (8 * (qp_len + L.nV + L.nVo + cfg.nu) + 4 * 2)   # (shared limits: the cfg block stays in cache)
    written = 8 * nq * cmpc.certify_len(cmpc.CmpcDims.from_config(cfg, B))
    floor_ms = (read + written) / HBM_BYTES_PER_S * 1e3
    med = {k: float(np.median(v)) for k, v in t.items()}
    print(f"{PLANT}-{CTYPE} p={cfg.p} B={B} ({nq} QP slots), {ROUNDS} rounds x {N} calls each, alternating")
    for k in fns:
        print(f"{k:12s} per call: median {med[k] * 1e3:8.1f} us   rounds " + " ".join(f"{v * 1e3:.1f}" for v in t[k]))
    print(f"certify algorithmic bytes: {(read + written) / nq:.0f} per slot, {read / 1e6:.1f} MB read + "
          f"{written / 1e6:.1f} MB written; floor at 8 TB/s {floor_ms * 1e3:.1f} us")
    print(f"certify: {(read + written) / med['certify'] / 1e9:.2f} TB/s, {floor_ms / med['certify'] * 100:.0f} % of "
          f"HBM peak; certify / iterate K=0: {med['certify'] / med['iterate K=0']:.2f}")
    print(f"summary of the last record (tol 1e-9): {summary}")


if __name__ == "__main__":
    main()
