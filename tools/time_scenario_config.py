#!/usr/bin/env python3
"""Step time of the headline shape (par-coop, p = 50, K = 9, 65 536 scenarios,
the bench's rotation of four bound batches) with per-scenario setpoint offsets
and limits bound (cmpc_bind_scenario_reference / _constraints) against
unbound, in alternating rounds in one process.

The bound arrays hold zero offsets and the shared limits, so both arms solve
the same QPs: the difference is the cost of reading 8 (ny + 4 nu) bytes more
per QP, not of other active sets.

usage: python tools/time_scenario_config.py [--rounds 4] [--steps 200] [--out FILE]
Appends one line per round and arm ("unbound" / "bound") to FILE.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "compressor-mpc_amd"))
import cmpc  # noqa: E402
from cmpc.configs import reference_setup  # noqa: E402
from cmpc.synthetic import synthetic_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = cmpc.reference_config("par", "coop", p=50)
    arrays = cmpc.controller_arrays(cfg, reference_setup("par", "coop"))
    B, S, K, NB = args.batch, cfg.S, 9, 4
    nq = B * S
    batches, states = [], []
    for b in range(NB):
        lin, u, du, w = synthetic_batch(cfg, B, seed=1002 + b, n_distinct=min(B, 2048))
        batches.append(torch.from_numpy(lin).cuda())
        states.append(tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (u, du, w.view(np.int32))))
    dy = torch.zeros(nq, cfg.ny, dtype=torch.float64, device="cuda")
    lim = np.stack([np.tile(getattr(arrays, k), (B, 1)) for k in ("lower", "upper", "rate_lower", "rate_upper")],
                   axis=1)
    lim = torch.from_numpy(np.ascontiguousarray(lim)).cuda()   # (nq, 4, nu)
    ctx = cmpc.Context(cfg, B, device=0)
    ctx.configure(arrays)

    def arm(bound):
        ctx.bind_scenario_reference(dy.data_ptr() if bound else 0)
        ctx.bind_scenario_constraints(lim.data_ptr() if bound else 0)

    def step(i, flags=cmpc.CMPC_APPLY_MOVE):
        b = i % NB
        ctx.bind_lin(batches[b].data_ptr())
        ctx.bind_state(*(a.data_ptr() for a in states[b]))
        ctx.step(K, flags)

    for b in range(NB):
        ctx.bind_lin(batches[b].data_ptr())
        ctx.bind_state(*(a.data_ptr() for a in states[b]))
        ctx.build()
        ctx.init_warmstart()
    ctx.synchronize()
    for n in range(400):  # clock settle
        step(n, 0)
    ctx.synchronize()
    lines = []
    for r in range(1, args.rounds + 1):
        for bound in (False, True):
            arm(bound)
            for n in range(20):
                step(n, 0)
            ctx.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                step(i, 0)   # no move applied: every round of both arms solves the same QPs
            ctx.synchronize()
            ms = (time.perf_counter() - t0) / args.steps * 1e3
            line = f"{'bound' if bound else 'unbound'} {r} scenario_config " + json.dumps(
                {"ms_per_step": ms, "steps": args.steps, "scenarios": B, "qp_per_s": nq * K / (ms * 1e-3)})
            print(line, flush=True)
            lines.append(line)
    st = ctx.download()[1]
    print("status ok fraction", float((st == 0).mean()), flush=True)
    ctx.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
