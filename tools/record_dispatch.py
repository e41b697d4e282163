#!/usr/bin/env python3
"""Record which kernels a library launches over a grid of batches (GPU).

Drives the library named by CMPC_LIBRARY (default: the in-tree one) through
the Python API and writes, per case, what cmpc_last_build_kernel /
cmpc_last_solve_kernel / cmpc_last_step_fused report after build(),
iterate(K), step(K) and control_step(K), or the error text of the call, plus
the device's CU count.  tests/test_dispatch.py checks that cmpc.plan
reproduces tests/golden/dispatch_parent.json, recorded from the library
before the selection moved into csrc/dispatch.cpp; recording the current
library must give the same file.

The grid: both plants x three controller types, p = 20, 50, 200, batches
at and beside every switch point of the selection (in units of the CU count),
B = 1 and 65 536; AUTO, each forced build and solve variant and the fused
step; K = 0, 1, 9; the control step at B = 1 and 13.

usage: record_dispatch.py OUT.json
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "compressor-mpc_amd"))

import cmpc  # noqa: E402
from cmpc.synthetic import synthetic_batch, synthetic_operating_points  # noqa: E402

CONFIGS = [(pl, ct) for pl in ("par", "ser") for ct in ("coop", "ncoop", "cent")]
HORIZONS = (20, 50, 200)
KS = (0, 1, 9)
# (build, solve, step) variant settings
VARIANTS = [(cmpc.CMPC_BUILD_AUTO, cmpc.CMPC_SOLVE_AUTO, cmpc.CMPC_STEP_AUTO),
            (cmpc.CMPC_BUILD_WAVE, cmpc.CMPC_SOLVE_AUTO, cmpc.CMPC_STEP_AUTO),
            (cmpc.CMPC_BUILD_ROWS, cmpc.CMPC_SOLVE_AUTO, cmpc.CMPC_STEP_AUTO),
            (cmpc.CMPC_BUILD_SPLIT, cmpc.CMPC_SOLVE_AUTO, cmpc.CMPC_STEP_AUTO),
            (cmpc.CMPC_BUILD_AUTO, cmpc.CMPC_SOLVE_LANE, cmpc.CMPC_STEP_AUTO),
            (cmpc.CMPC_BUILD_AUTO, cmpc.CMPC_SOLVE_ROWS, cmpc.CMPC_STEP_AUTO),
            (cmpc.CMPC_BUILD_AUTO, cmpc.CMPC_SOLVE_AUTO, cmpc.CMPC_STEP_FUSED)]
CONTROL_B = (1, 13)


def batches(S: int, cus: int):
    """Scenario counts that put nqp = B * S at and just past every threshold
    of the selection: cus, 4 cus (fused step, split build, control step),
    16 cus - 4 (a row group per SIMD), 16 cus (nV < 6 row solve), 16 384
    (nV >= 6 row solve)."""
    out = {1, 65536}
    for nqp in (cus, 4 * cus, 16 * cus - 4, 16 * cus, 16383, 16384):
        lo = nqp // S                   # the last batch at or below nqp
        out.update((max(lo, 1), lo + 1))
    return sorted(out)


def outcome(call, read):
    """read() after call(), or the library's error text."""
    try:
        call()
    except RuntimeError as e:
        return "error: " + str(e).split("): ", 1)[1]
    return read()


def warm_start(ctx) -> bool:
    """The first build and InitializeQPProblem.  False where no build kernel
    takes the dimensions (ser-coop and ser-cent at p = 200: the horizon is too
    long for the LDS): no QP exists then, and the grid leaves iterate out."""
    try:
        ctx.build()
    except RuntimeError:
        return False
    ctx.init_warmstart()
    return True


def triple(ctx):
    return [ctx.last_build_kernel(), ctx.last_solve_kernel(), int(ctx.last_step_fused())]


def record(out_path: str):
    import torch
    torch.cuda.init()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows, control = [], []
    for plant, ctype in CONFIGS:
        for p in HORIZONS:
            cfg = cmpc.reference_config(plant, ctype, p=p)
            arr = cmpc.controller_arrays(cfg, cmpc.reference_setup(plant, ctype))
            lin4, u4, du4, ws4 = synthetic_batch(cfg, 4, seed=3, n_distinct=4)
            for B in batches(cfg.S, cus):
                idx = np.arange(B * cfg.S) % (4 * cfg.S)
                with cmpc.Context(cfg, B) as ctx:
                    ctx.configure(arr)
                    ctx.set_state(u4[idx], du4[idx], ws4[idx])
                    ctx.upload_lin(lin4[idx])
                    built = warm_start(ctx)
                    for bv, sv, stv in VARIANTS:
                        ctx.set_build_variant(bv)
                        ctx.set_solve_variant(sv)
                        ctx.set_step_variant(stv)
                        for K in KS:
                            rows.append([plant, ctype, p, B, bv, sv, stv, K,
                                         outcome(ctx.build, ctx.last_build_kernel),
                                         outcome(lambda: ctx.iterate(K), ctx.last_solve_kernel) if built else None,
                                         outcome(lambda: ctx.step(K), lambda: triple(ctx))])
                    ctx.synchronize()
            for B in CONTROL_B:
                x, u, y = synthetic_operating_points(cfg, B, seed=3, n_distinct=min(B, 4))
                tx, tu, ty = (torch.from_numpy(a).to("cuda:0") for a in (x, u, y))
                nq = B * cfg.S
                rng = np.random.default_rng(5)
                with cmpc.Context(cfg, B) as ctx:
                    ctx.configure(arr)
                    ctx.set_state(np.zeros((nq, cfg.nu_tot)), np.zeros((nq, cfg.nV)), np.zeros(nq, np.uint32))
                    for s in range(cfg.S):
                        ctx.set_observer(s, 0.01 * rng.normal(size=(ctx.layout.nobs, y.shape[1])))
                    ctx.observer_init(tx.data_ptr(), tu.data_ptr(), ty.data_ptr())
                    warm_start(ctx)
                    for bv, sv, stv in VARIANTS + [(cmpc.CMPC_BUILD_AUTO, cmpc.CMPC_SOLVE_AUTO, cmpc.CMPC_STEP_SPLIT)]:
                        ctx.set_build_variant(bv)
                        ctx.set_solve_variant(sv)
                        ctx.set_step_variant(stv)
                        for K in KS:
                            control.append([plant, ctype, p, B, bv, sv, stv, K,
                                            outcome(lambda: ctx.control_step(tu.data_ptr(), ty.data_ptr(), K),
                                                    lambda: triple(ctx))])
                    ctx.synchronize()
            print(f"{plant} {ctype} p = {p}: {len(rows)} + {len(control)} cases", flush=True)
    write(out_path, cus, rows, control)
    print(f"{len(rows)} + {len(control)} cases on {cus} CUs -> {out_path}")


def factored(rows):
    """The cases [plant, controller, p, B, build, solve, step variant, K,
    outcome...] as one line per configuration and variant setting,
    [plant, controller, p, build, solve, step variant, segments]: a segment
    [Ks, Bs, outcome...] says that every K of Ks with every B of Bs gave that
    outcome (the selection changes at a few batch sizes only)."""
    groups = {}
    for plant, ctype, p, B, bv, sv, stv, K, *outcome in rows:
        groups.setdefault((plant, ctype, p, bv, sv, stv), {}).setdefault(K, []).append((B, outcome))
    lines = []
    for key, by_k in groups.items():
        same = {}  # the Ks that share one B -> outcome list
        for K, cases in by_k.items():
            same.setdefault(json.dumps(cases), (cases, []))[1].append(K)
        segments = []
        for cases, Ks in same.values():
            for B, outcome in cases:
                if segments and segments[-1][0] is Ks and segments[-1][2:] == outcome:
                    segments[-1][1].append(B)
                else:
                    segments.append([Ks, [B], *outcome])
        lines.append([*key, segments])
    return lines


def expanded(lines):
    """the cases of factored() lines"""
    for plant, ctype, p, bv, sv, stv, segments in lines:
        for Ks, Bs, *outcome in segments:
            for K in Ks:
                for B in Bs:
                    yield [plant, ctype, p, B, bv, sv, stv, K, *outcome]


def write(out_path, cus, rows, control):
    dump = lambda lines: ",\n".join(json.dumps(r, separators=(",", ":")) for r in lines)
    with open(out_path, "w") as f:
        f.write('{"cus": %d,\n "format": "[plant, controller, p, build_variant, solve_variant, step_variant, '
                '[[Ks, Bs, outcome...], ...]]: tools/record_dispatch.py, factored()",\n'
                ' "outcome": ["after build", "after iterate", "after step"],\n "rows": [\n' % cus)
        f.write(dump(factored(rows)))
        f.write('\n ],\n "control_outcome": ["after control_step"],\n "control_rows": [\n')
        f.write(dump(factored(control)))
        f.write("\n ]\n}\n")


if __name__ == "__main__":
    record(sys.argv[1])
