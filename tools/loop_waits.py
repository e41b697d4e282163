#!/usr/bin/env python3
"""Per-basic-block arithmetic, LDS traffic and wait sequence of one kernel.

Compiles one translation unit of compressor-mpc_amd/csrc to gfx950 device
assembly with the flags its Makefile rule uses (HIPFLAGS plus the rule's
SOLVERFLAGS / ROWSFLAGS) and prints, for every basic block of the named kernel
that holds at least --min-valu VALU instructions:

  fma     FMA instructions (v_fma*/v_fmac*)
  valu    the other VALU instructions, by opcode
  lds     ds_* instructions, by opcode
  waits   the s_waitcnt operands in program order; `|` marks a run of at least
          --gap FMAs between two waits, so the step structure of an unrolled
          block can be read off the line

and after the blocks the kernel's register, scratch and occupancy figures.

usage: python tools/loop_waits.py UNIT.hip KERNEL_SUBSTRING [--min-valu N] [--gap N] [-D NAME=VALUE ...] [--asm FILE.s]
  -D    adds a preprocessor definition to the Makefile's flags (a kernel's compile-time switch)
  --asm reads an existing assembly file instead of compiling."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "compressor-mpc_amd", "csrc")


def make_vars():
    """The Makefile's simple `NAME = value` / `NAME ?= value` assignments."""
    out = {}
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(r"^([A-Z]+)\s*\??=\s*(.*)$", line.rstrip("\n"))
        if m:
            out[m.group(1)] = m.group(2)
    return out


def rule_flags(unit, mv):
    """Flags of the rule that compiles `unit`: the $(...) variables of its recipe."""
    obj = os.path.splitext(os.path.basename(unit))[0] + ".o"
    lines = open(os.path.join(CSRC, "Makefile")).read().split("\n")
    for i, line in enumerate(lines):
        if line.startswith(obj + ":"):
            names = re.findall(r"\$\(([A-Z]+)\)", lines[i + 1])
            flags = []
            for n in names:
                if n.endswith("FLAGS"):
                    flags += re.sub(r"\$\(([A-Z]+)\)", lambda k: mv[k.group(1)], mv[n]).split()
            return flags
    sys.exit(f"no Makefile rule for {obj}")


def compile_asm(unit, out, defines):
    mv = make_vars()
    hipcc = os.environ.get("HIPCC", mv["HIPCC"])
    cmd = [hipcc] + rule_flags(unit, mv) + ["-D" + d for d in defines] + ["--cuda-device-only", "-S", os.path.basename(unit), "-o", out]
    r = subprocess.run(cmd, cwd=CSRC, stderr=subprocess.PIPE, text=True)
    if r.returncode:
        sys.exit(r.stderr)


def kernel_text(src, key):
    m = re.search(r"^(\S*" + re.escape(key) + r"\S*):", src, re.M)
    if not m:
        sys.exit(f"kernel {key} not found")
    i = m.end()
    j = src.index(".Lfunc_end", i)
    k = src.find(".end_amdhsa_kernel", j)
    return m.group(1), src[i:j], src[j:k if k > 0 else len(src)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("unit")
    ap.add_argument("kernel")
    ap.add_argument("--min-valu", type=int, default=40)
    ap.add_argument("--gap", type=int, default=20)
    ap.add_argument("-D", dest="defines", action="append", default=[])
    ap.add_argument("--asm")
    a = ap.parse_args()
    if a.asm:
        src = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "unit.s")
            compile_asm(a.unit, path, a.defines)
            src = open(path).read()
    sym, body, desc = kernel_text(src, a.kernel)
    print(f"kernel {sym}")

    blocks, cur = [], None

    def new(name):
        nonlocal cur
        cur = {"name": name, "fma": 0, "valu": collections.Counter(), "lds": collections.Counter(),
               "waits": [], "run": 0}
        blocks.append(cur)

    new("entry")
    for line in body.split("\n"):
        lm = re.match(r"^(\.LBB\d+_\d+):", line)
        if lm:
            new(lm.group(1))
            continue
        t = line.split(";")[0].strip()
        if not t or t.startswith("."):
            continue
        op = t.split()[0]
        if op == "s_waitcnt":
            if cur["run"] >= a.gap and cur["waits"]:
                cur["waits"].append("|")
            cur["run"] = 0
            cur["waits"].append(" ".join(t.split()[1:]))
        elif op.startswith("v_fma"):
            cur["fma"] += 1
            cur["run"] += 1
        elif op.startswith("v_"):
            cur["valu"][op] += 1
        elif op.startswith("ds_"):
            cur["lds"][op] += 1
    for b in blocks:
        nv = b["fma"] + sum(b["valu"].values())
        if nv < a.min_valu:
            continue
        print(f"\n{b['name']}: {b['fma']} FMA, {sum(b['valu'].values())} other VALU, {sum(b['lds'].values())} LDS")
        if b["valu"]:
            print("  valu : " + ", ".join(f"{k} x{v}" for k, v in sorted(b["valu"].items())))
        if b["lds"]:
            print("  lds  : " + ", ".join(f"{k} x{v}" for k, v in sorted(b["lds"].items())))
        print("  waits: " + " ".join(b["waits"]))
        print(f"  lgkmcnt(0) waits: {sum('lgkmcnt(0)' in w for w in b['waits'])}")
    print()
    for key in (".amdhsa_next_free_vgpr", ".amdhsa_accum_offset", ".amdhsa_private_segment_fixed_size"):
        m = re.search(re.escape(key) + r"\s+(\S+)", desc)
        if m:
            print(f"{key[8:]} {m.group(1)}")
    for key in ("NumVgprs", "NumAgprs", "TotalNumVgprs", "ScratchSize", "Occupancy"):
        m = re.search(r";\s*" + key + r":\s*(\S+)", desc)
        if m:
            print(f"{key} {m.group(1)}")


if __name__ == "__main__":
    main()
