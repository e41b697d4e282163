#!/usr/bin/env python3
"""bench.py — QP solves/sec (whole node) of the cooperative-parallel MPC hot
path at horizon p = 50 (BASELINE.json metric) on MI355X.

One step = one batched NerveCenter control step over B scenarios per GPU
(2-compressor cooperative-parallel plant, S = 2 sub-controllers each, m = 2):
condensed-QP build of every sub-controller (cmpc_build) + K = 9 Jacobi
iterations of warm-started QP re-solves with the plan exchange, the first
move applied to u_old (cmpc_iterate with CMPC_APPLY_MOVE: SURVEY §8(a)
a1-a13).  QP solves per step = B * S * K per GPU.

Inputs are resident in HBM before the timed region: NB distinct synthetic
batches of B scenarios are uploaded once, each with its own
controller state (u_old, move plans, warm-start working sets).  Step i binds
batch i % NB's records (cmpc_bind_lin) and state (cmpc_bind_state), so
consecutive steps solve different QPs (the 327 MB of records per batch are
read from HBM, not from the 256 MB Infinity Cache) and every QP is
warm-started from its own scenario's previous step, as each reference
controller hot-starts its own QProblem.

Multi-GPU: one process per GPU (torch.distributed.run), scenarios sharded
across ranks with no data-path collective (weak scaling); the barrier and
the max-over-ranks of the elapsed time use torch.distributed (RCCL).  A plain
`python bench.py --gpus N` (no launcher environment) starts the N ranks itself:
a torch.distributed.run child process, rank 0's line relayed, the child's exit
code returned; fewer than N visible GPUs is an error.  The `coupled` section
beside the metric runs SURVEY config 4 on the same ranks: S_local = 8
sub-controllers per GPU of S_total = 8 x world per scenario, the plans
all-gathered over RCCL once per Jacobi iteration; `coupled_s64` runs config
4's own 64-sub-controller system at every world size (64 / world per GPU).

A plain run (`bench.py --gpus N --steps K --warmup W`) sets up, warms up,
times the K steps, writes the last timed step's outputs with --dump-outputs
DIR, and prints the result line.  Everything else measured here (the iterate
kernel's own pass, working-set traces, the harder-QP, K = 1, closed-loop,
SURVEY-config, recorded-run and coupled sections, the CPU baseline, the PMC
traffic lookup) runs after that with --full; their keys are null in a plain
run's line (`cpu_baseline` is left out, as with --no-cpu).

Prints ONE JSON line (rank 0).
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "compressor-mpc_amd"))

import numpy as np  # noqa: E402

FP64_PEAK_TFLOPS = 78.6   # MI355X dense FP64 (vector = matrix), spec
HBM_PEAK_GBS = 8000.0


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def build_flops(cfg, naug: int, nd: int) -> float:
    """Algorithmic FLOPs of one sub-controller build (FMA = 2)."""
    p, ny, ns, nu_tot, nV = cfg.p, cfg.ny, cfg.ns, cfg.nu_tot, cfg.nV
    return (p * 2 * ny * ns * (ns + nd) + p * 2 * ny * ns * (nu_tot - nd) + p * ny * nu_tot +
            p * ny * ns + 2 * p * ny * ny * nV + 2 * nV * nV * p * ny +
            2 * p * ny * (ns + naug) + p * ny + 2 * p * ny * nV)


def iterate_flops(cfg) -> float:
    """Algorithmic FLOPs of one Jacobi iteration of one sub-controller
    (ApplyOtherInput's (p ny)-long products + the plan
    update; the QP solve itself is not counted, a lower bound)."""
    p, ny, m, nV = cfg.p, cfg.ny, cfg.m, cfg.nV
    nuo = cfg.nu_tot - cfg.nu
    return 2 * p * ny * m * nuo + 2 * p * ny * nV


def applied_iterate_flops(cfg) -> float:
    """FLOPs one Jacobi iteration of this build performs before the solve:
    f_k = f + G du_other, G nV x nVo (built once per step in the build
    kernel)."""
    nuo = cfg.nu_tot - cfg.nu
    return 2.0 * cfg.nV * cfg.m * nuo


def build_bytes(cfg, L) -> float:
    """Algorithmic HBM bytes of one sub-controller build: its lin record
    (Aorig, Bin, Csel, f, dx_aug, y_prev) + u_old in, the condensed QP out."""
    ns, ny, nu_tot = cfg.ns, cfg.ny, cfg.nu_tot
    rec = ns * ns + ns * nu_tot + ny * L.nobs + ns + L.naug + ny
    out = L.nV * L.nV + L.nV + L.nV * L.nVo
    return 8.0 * (rec + nu_tot + out)


# the bench's build-kernel instantiation (cmpc_build_rows_kernel<NS=11, NY=3,
# NUT=4, NU=2, M=2, ND=2, WPG=4, RING=false, WPE=3, FUSE=0>)
BENCH_KERNEL_SYMBOL = "cmpc_build_rows_kernelILi11ELi3ELi4ELi2ELi2ELi2ELi4ELb0ELi3ELi0EE"


def bench_kernel_code_hash():
    """sha256 of the bench build kernel's gfx950 machine code in the loaded
    library (tools/kernel_hash.py): ties a PMC traffic figure under profiles/
    to the code it was measured on; other instantiations, comments and the
    solve kernels do not change it."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_hash
    from cmpc._abi import LIB_PATH
    blob = open(LIB_PATH, "rb").read()
    for co in kernel_hash.code_objects(blob):
        r = kernel_hash.kernel_bytes(co, BENCH_KERNEL_SYMBOL)
        if r:
            return hashlib.sha256(r[1]).hexdigest()[:16]
    return None


def pmc_traffic(B: int, kernel: str):
    """(bytes per launch, provenance) from profiles/pmc_build_coop_p50.json
    when it was measured on this batch, this kernel and this kernel's machine
    code; (None, reason) otherwise."""
    path = os.path.join(ROOT, "profiles", "pmc_build_coop_p50.json")
    try:
        rec = json.load(open(path))
    except (OSError, ValueError):
        return None, {"file": "profiles/pmc_build_coop_p50.json", "status": "missing"}
    try:
        cur = bench_kernel_code_hash()
    except Exception as e:  # noqa: BLE001 -- reported, never required
        cur = None
        log(f"kernel code hash failed: {e}")
    prov = {"file": "profiles/pmc_build_coop_p50.json", "pmc_source": rec.get("source"),
            "round": rec.get("round"), "measured_code_hash": rec.get("build_kernel_code_hash"),
            "current_code_hash": cur,
            "hash_of": "gfx950 machine code of " + BENCH_KERNEL_SYMBOL + " in the loaded libcmpc.so"}
    if rec.get("batch") != B or rec.get("kernel") != kernel:
        prov["status"] = "not this workload"
        return None, prov
    if cur is None or rec.get("build_kernel_code_hash") != cur:
        prov["status"] = "stale: measured on another build of the bench kernel"
        return None, prov
    prov["status"] = "measured on this machine code (rocprofv3 --pmc FETCH_SIZE, WRITE_SIZE passes)"
    return rec.get("hbm_bytes_per_launch"), prov


def cpu_quota():
    """CPUs this process may use: affinity mask and cgroup v2 quota."""
    out = {}
    try:
        out["affinity_cpus"] = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        pass
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        out["cgroup_cpu_quota"] = None if q == "max" else int(q) / int(per)
    except (OSError, ValueError):
        pass
    return out


def cpu_baseline(cfg, arrays, lin, u_old, K, target_s):
    """The oracle (CPU restatement of the reference path: O(p^2) Su loop,
    dense products, the build's active-set solver) on a bounded sample of
    the bench's batch 0, in three legs: one thread; as many threads as the
    process may run at once (affinity mask and cgroup CPU quota, the value);
    and os.cpu_count() threads (all host cores) when that is
    more.  The single-thread leg runs first: idle OpenMP workers of a wide
    leg spin and eat the quota of whatever runs after them."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _oracle as O
    from cmpc._abi import CmpcDims
    S = cfg.S

    def run(nb, th, reps):
        dims = CmpcDims.from_config(cfg, nb)
        sl = slice(0, nb * S)
        lin_s = np.ascontiguousarray(lin[sl])
        u_s = np.ascontiguousarray(u_old[sl])
        du_s = np.zeros((nb * S, cfg.nV))
        ws_s = np.zeros(nb * S, np.uint32)
        O.step(dims, arrays, lin_s, K, u_s.copy(), du_s.copy(), ws_s.copy(), init=True, threads=th)
        t0 = time.perf_counter()
        for _ in range(reps):
            O.step(dims, arrays, lin_s, K, u_s, du_s, ws_s, threads=th)
        return (time.perf_counter() - t0) / reps

    def leg(threads, seconds):
        probe = min(64, lin.shape[0] // S)
        t1 = run(probe, threads, 1)
        nb = int(min(lin.shape[0] // S, max(probe, probe * seconds / max(t1, 1e-6))))
        t_pass = run(nb, threads, 1)
        reps = max(1, int(round(seconds / max(t_pass, 1e-6))))
        dt = run(nb, threads, reps)
        return {"value": nb * S * K / dt, "threads": threads, "scenarios": nb, "steps": reps,
                "seconds": dt * reps, "us_per_scenario_step": dt / nb * 1e6}

    share = cpu_quota()
    host = os.cpu_count() or 1
    usable = min([host] + [int(v) for v in (share.get("affinity_cpus"), share.get("cgroup_cpu_quota"))
                           if v])
    single = leg(1, min(5.0, target_s / 2))
    main_leg = leg(usable, target_s)
    all_leg = leg(host, target_s / 2) if host > usable else None
    model = ""
    try:
        with open("/proc/cpuinfo") as fh:
            model = next((ln.split(":", 1)[1].strip() for ln in fh if ln.startswith("model name")), "")
    except OSError:
        pass
    return {
        "value": main_leg["value"],
        "unit": "QP solves/s",
        "cores": usable,
        "kind": "port",
        "cpu_model": model,
        "host_cpus": host,
        "cpu_share": share,
        "sample": (f"{main_leg['steps']} control steps of {main_leg['scenarios']} scenarios x {S} "
                   f"sub-controllers x K={K} Jacobi iterations (build + solves) of batch 0, "
                   f"oracle/liboracle.so (reference op order, -O3, OpenMP over scenarios, {usable} "
                   f"threads), {main_leg['seconds']:.1f} s"),
        "single_thread": single,
        "all_host_cpus": all_leg,
        "threads_note": ("value: as many OpenMP threads as the process may run at once (the smaller "
                         "of the affinity mask and the cgroup CPU quota); all_host_cpus: "
                         "os.cpu_count() threads as BASELINE.md §2 asks, which the quota time-slices"),
        "reference_recorded": {
            "note": "context, not comparison (BASELINE.md §1): the reference's own per-step wall "
                    "times from results/parallel/run*/coop{1,9}.dat, p = 100, one thread, CPU unrecorded",
            "coop9_step_us": 900.4, "coop1_step_us": 727.2, "build_us_per_subcontroller": 349.0,
            "resolve_us_per_qp": 10.7, "qp_solves_per_s_k9": 20.0e3},
    }


def traced_changes(ctx, K, bind, steps):
    """Working-set changes per step summed over all K Jacobi iterations and all
    QPs (the trace counts of CMPC_TRACE), over `steps` steps bound by bind(i)
    (untimed; the caller restores the states afterwards)."""
    import cmpc
    tot = []
    for i in steps:
        bind(i)
        ctx.step(K, cmpc.CMPC_APPLY_MOVE | cmpc.CMPC_TRACE)
        _, ntr = ctx.download_trace(K)
        tot.append(int(ntr.sum()))
    return float(np.mean(tot)), tot


def time_config(name, plant, ctype, p, B, K, local, settle_seconds, steps, NB=2, seed=4000, markers=False):
    """One SURVEY §8(d) configuration on this GPU: NB resident batches of B
    scenarios, each with its own controller state, step i on batch i % NB
    (build + K Jacobi iterations, first move applied: cmpc_step, fused into
    one launch where CMPC_STEP_AUTO picks that); then the build kernel alone
    with events for its roofline fraction.  markers: a torch.cuda._sleep
    launch before and after the event-timed pass, so that a kernel trace of
    the run can be cut to that pass (tools/configs_pass_stats.py)."""
    import torch
    import cmpc
    from cmpc.configs import reference_setup
    from cmpc.synthetic import synthetic_batch
    cfg = cmpc.reference_config(plant, ctype, p=p)
    arrays = cmpc.controller_arrays(cfg, reference_setup(plant, ctype))
    dev = f"cuda:{local}"
    recs, sts = [], []
    for b in range(NB):
        lin, u, du, w = synthetic_batch(cfg, B, seed=seed + 31 * b, n_distinct=min(B, 1024))
        recs.append(torch.from_numpy(lin).to(dev))
        sts.append(tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (u, du, w.view(np.int32))))
    ctx = cmpc.Context(cfg, B, device=local)
    try:
        ctx.configure(arrays)

        def bind(i):
            st_ = sts[i % NB]
            ctx.bind_lin(recs[i % NB].data_ptr())
            ctx.bind_state(st_[0].data_ptr(), st_[1].data_ptr(), st_[2].data_ptr())

        for b in range(NB):
            bind(b)
            ctx.build()
            ctx.init_warmstart()
        i = 0
        t_end = time.perf_counter() + settle_seconds
        while time.perf_counter() < t_end or i < 8:
            bind(i)
            ctx.step(K, 0)
            i += 1
            if i % 16 == 0:
                ctx.synchronize()
        ctx.synchronize()
        torch.cuda.synchronize(local)
        # every pass below starts from this snapshot (the same steps on the
        # same states: the applied moves of one pass do not shift the working
        # sets of the next), after build-only launches that hold the clock
        # (builds write only the QP buffer, no controller state)
        snap = [tuple(a.clone() for a in st_) for st_ in sts]

        def restore():
            for st_, sn in zip(sts, snap):
                for a, a0 in zip(st_, sn):
                    a.copy_(a0)
            torch.cuda.synchronize(local)
            t_w = time.perf_counter()
            while time.perf_counter() - t_w < 0.05:
                for k in range(8):
                    bind(i + k)
                    ctx.build()
                ctx.synchronize()

        restore()
        t0 = time.perf_counter()
        for k in range(steps):
            bind(i + k)
            ctx.step(K, cmpc.CMPC_APPLY_MOVE)
        ctx.synchronize()
        dt = (time.perf_counter() - t0) / steps
        fused = ctx.last_step_fused()
        # one step at a time (host waits for each): the latency view
        restore()
        t0 = time.perf_counter()
        for k in range(steps):
            bind(i + k)
            ctx.step(K, cmpc.CMPC_APPLY_MOVE)
            ctx.synchronize()
        dt_sync = (time.perf_counter() - t0) / steps
        # device time of the step's kernels (events), then the build alone
        restore()
        if markers:
            torch.cuda._sleep(1000)
        ctx.enable_timing(True)
        for k in range(steps):
            bind(i + k)
            ctx.step(K, cmpc.CMPC_APPLY_MOVE)
        if markers:  # (the marker runs on torch's stream: after the pass's kernels)
            ctx.synchronize()
            torch.cuda._sleep(1000)
        kt = {}
        for kn, kid in (("build", cmpc.CMPC_KERNEL_BUILD), ("iterate", cmpc.CMPC_KERNEL_ITERATE),
                        ("fused_step", cmpc.CMPC_KERNEL_STEP)):
            ms, n = ctx.kernel_time(kid)
            if n:
                kt[kn] = ms / n
        restore()
        ctx.enable_timing(True, only=(cmpc.CMPC_KERNEL_BUILD,))
        for k in range(steps):
            bind(i + k)
            ctx.build()
        bms, bn = ctx.kernel_time(cmpc.CMPC_KERNEL_BUILD)
        ctx.enable_timing(False)
        bkern = {cmpc.CMPC_BUILD_ROWS: "cmpc_build_rows_kernel",
                 getattr(cmpc, "CMPC_BUILD_SPLIT", -1): "cmpc_build_split_kernel"}.get(ctx.last_build_kernel(),
                                                                                     "cmpc_build_kernel")
        L = ctx.layout
        restore()
        changes, _ = traced_changes(ctx, K, bind, range(i, i + steps))  # the timed steps, replayed
        for st_, sn in zip(sts, snap):
            for a, a0 in zip(st_, sn):
                a.copy_(a0)
        _, st, _ = ctx.download()
    finally:
        ctx.close()
    f_b = build_flops(cfg, L.naug, L.nd)
    b_s = bms / max(bn, 1) / 1e3
    return {"config": name, "plant": plant, "controller": ctype, "p": p, "B": B, "qp": B * cfg.S, "K": K,
            "qp_solves_per_s": B * cfg.S * K / dt, "ms_per_step": dt * 1e3,
            "ms_per_step_synchronised": dt_sync * 1e3, "step_fused": fused, "kernels_ms": kt,
            "build_kernel": bkern, "build_ms": b_s * 1e3,
            "build_roofline": {"flops_per_qp": f_b, "achieved_tflops": B * cfg.S * f_b / b_s / 1e12,
                               "frac": B * cfg.S * f_b / b_s / 1e12 / FP64_PEAK_TFLOPS,
                               "peak": FP64_PEAK_TFLOPS, "bound": "fp64-valu"},
            "working_set_changes_per_step": changes, "qp_status_ok_fraction": float((st == 0).mean()),
            "note": "back-to-back, synchronised and event-timed passes each run the same steps from the same "
                    "snapshot of the states, after build-only launches that hold the clock"}


def cpp_step_latency(plant, ctype, p, steps=400):
    """B = 1 step latency through the C++ adapter (tests/cpp/nerve_center_latency:
    NerveCenter::GetNextInput with the device observer, host clock per call)."""
    import subprocess
    import tempfile
    from cmpc.configs import reference_setup
    exe = os.path.join(ROOT, "tests", "cpp", "nerve_center_latency")
    if not os.path.exists(exe):
        return {"error": "tests/cpp/nerve_center_latency not built (make -C tests/cpp)"}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, f"setup-{ctype}-{plant}")
        with open(path, "w") as fh:
            fh.write(reference_setup(plant, ctype).text())
        r = subprocess.run([exe, path, plant, ctype, str(p), str(steps)], capture_output=True, text=True,
                           timeout=120)
    if r.returncode:
        return {"error": r.stderr.strip()[-300:]}
    out = json.loads(r.stdout.strip().splitlines()[-1])
    out.update({"plant": plant, "controller": ctype, "p": p, "B": 1,
                "note": "NerveCenter::GetNextInput (observer a posteriori + linearisation, build, K Jacobi "
                        "iterations, download, a-priori update) through include/cmpc/nerve_center.hpp, one "
                        "scenario, host clock per call; the reference recorded 371.3 us (cent-ser) and "
                        "900.4 us (coop-par K = 9) per step at p = 100 on its CPU"})
    return out


def recorded_run_changes(local, n_steps=10000):
    """The solver load of the reference's own recorded run: the device closed
    loop that reproduces results/parallel/run1/coop9.dat record for record
    (cooperative parallel, p = 100, K = 9, the setup file's input step at
    50 s, observer gain [0; I]; tests/test_closed_loop_golden.py), one
    scenario, with the Jacobi iterations' working-set changes counted
    (CMPC_TRACE) at every one of its n_steps instants."""
    import cmpc
    from cmpc.configs import reference_setup
    from cmpc.driver import ClosedLoop
    cfg = cmpc.reference_config("par", "coop")
    setup = reference_setup("par", "coop")
    arr = cmpc.controller_arrays(cfg, setup)
    x0, u_def = cmpc.plant_default(cfg.plant)
    M = cmpc.reference_observer_gain(cfg)
    K = setup.n_iterations
    loop = ClosedLoop(cfg, arr, [M] * cfg.S, x0[None, :], u_def[None, :], K, device=local)
    per_step = []
    t0 = time.perf_counter()
    try:
        loop.set_segments(setup.segments, u_def)
        loop.initialize()
        for _ in range(n_steps):
            loop.step(trace=True)
            per_step.append(loop.last_changes)
        n_fail, _ = loop.plant_failures()
    finally:
        loop.close()
    a = np.asarray(per_step)
    return {"run": "results/parallel/run1/coop9.dat (cooperative parallel, p = 100, K = 9)",
            "instants": int(n_steps), "S": cfg.S, "K": K,
            "working_set_changes_total": int(a.sum()),
            "working_set_changes_per_qp_step": float(a.sum()) / (n_steps * cfg.S),
            "working_set_changes_per_qp_solve": float(a.sum()) / (n_steps * cfg.S * K),
            "instants_with_a_change": int((a > 0).sum()),
            "changes_first_100_instants": int(a[:100].sum()),
            "plant_failures": n_fail, "seconds": time.perf_counter() - t0,
            "note": "per_qp_step: changes summed over the K Jacobi iterations of one sub-controller's "
                    "control step, averaged over the run's instants and sub-controllers (the synthetic "
                    "headline's working_set_changes_per_qp_step is the same quantity)"}


def run_configs(local, settle_seconds, steps, with_cpp=True, markers=False):
    """SURVEY §8(d) / BASELINE.json configs 2, 3 and 5 at their batch sizes on
    this GPU, and (with_cpp) config 1 and the coop-par B = 1 step through the
    C++ adapter; each entry failure-tolerant."""
    configs = {}
    for key, (pl, ct, p_, B_, K_) in {"2": ("par", "coop", 20, 4096, 9),
                                     "3": ("par", "ncoop", 50, 65536, 1),
                                     "5": ("par", "cent", 200, 1024, 1)}.items():
        try:
            configs[key] = time_config(key, pl, ct, p_, B_, K_, local, settle_seconds, max(20, steps),
                                       markers=markers)
        except Exception as e:  # reported, never required
            log(f"config {key} failed: {e}")
            configs[key] = {"error": str(e)[:300]}
    if with_cpp:
        for key, (pl, ct, p_) in {"1": ("ser", "cent", 100), "b1_coop_par": ("par", "coop", 50)}.items():
            try:
                configs[key] = cpp_step_latency(pl, ct, p_)
            except Exception as e:  # reported, never required
                log(f"config {key} failed: {e}")
                configs[key] = {"error": str(e)[:300]}
    return configs


SELF_LAUNCH_ENV = "CMPC_BENCH_SELF_LAUNCHED"


def launch_plan(gpus: int, backend: str, env, device_count):
    """How `bench.py --gpus N` runs.

    Returns ("here", None) when this process is a rank already (a launcher set
    WORLD_SIZE) or N = 1, or ("spawn", N) when the parent must start N ranks
    itself: the driver's plain `python3 bench.py --gpus N` then measures N GPUs
    instead of one.  Raises SystemExit (non-zero) when the ranks cannot match
    the request: WORLD_SIZE differs from --gpus, or fewer than N devices are
    visible for RCCL (one rank per GPU; gloo rehearsals may share a GPU).
    device_count is a callable, asked only when needed; the caller passes one
    that does not initialise the GPU (torch.cuda.device_count() on this image)."""
    if "WORLD_SIZE" in env:
        world = int(env["WORLD_SIZE"])
        if world != gpus:
            raise SystemExit(f"bench.py: WORLD_SIZE={world} but --gpus={gpus}: the launcher and the "
                             "request disagree")
        return "here", None
    if gpus <= 1:
        return "here", None
    if backend == "nccl":
        n = device_count()
        if n < gpus:
            raise SystemExit(f"bench.py: --gpus {gpus} needs {gpus} visible GPUs for one RCCL rank per "
                             f"GPU, {n} visible")
    return "spawn", gpus


def free_port() -> int:
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks(n: int, argv, script=None) -> int:
    """Start `python -m torch.distributed.run --nproc-per-node n bench.py argv`
    as a child process (never exec: this process stays the parent), relay its
    stdout (rank 0's JSON line) and return its exit code."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", f"--master-port={free_port()}",
           script or os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env[SELF_LAUNCH_ENV] = "1"
    log("bench.py: starting " + " ".join(cmd[1:]))
    import signal
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, text=True)

    def forward(signum, _frame):  # a time limit on this process reaches the ranks
        p.send_signal(signum)

    old = {s: signal.signal(s, forward) for s in (signal.SIGTERM, signal.SIGINT)}
    try:
        for line in p.stdout:
            sys.stdout.write(line)
            sys.stdout.flush()
        return p.wait()
    finally:
        for s, h in old.items():
            signal.signal(s, h)


DUMP_LIMIT_BYTES = 60 * 10**6   # all files of one --dump-outputs directory


def dump_outputs(path, rank, world, arrays):
    """--dump-outputs: each array (one row per QP) as path/<name>.npy in
    float64 (rank r > 0: <name>.rank<r>.npy).  Past this rank's share of
    DUMP_LIMIT_BYTES the same fixed, seeded sample of rows of every array,
    their indices in rows.npy."""
    os.makedirs(path, exist_ok=True)
    n = len(next(iter(arrays.values())))
    row_bytes = 8 + sum(8 * (a.size // n) for a in arrays.values())
    keep = None
    limit = DUMP_LIMIT_BYTES // world
    if n * row_bytes > limit:
        keep = np.sort(np.random.default_rng(6401).choice(n, limit // row_bytes, replace=False))
        arrays = dict(arrays, rows=keep)
    for name, a in arrays.items():
        a = np.asarray(a, dtype=np.float64)
        if keep is not None and name != "rows":
            a = a[keep]
        np.save(os.path.join(path, name + (f".rank{rank}" if rank else "") + ".npy"), a)
    log(f"[rank {rank}] outputs of the last timed step: {sorted(arrays)} in {path}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=65536, help="scenarios per GPU")
    ap.add_argument("--p", type=int, default=50)
    ap.add_argument("--K", type=int, default=9)
    ap.add_argument("--input-batches", type=int, default=4)
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--settle-seconds", type=float, default=0.25,
                    help="untimed steps after the W warmup steps until this much wall time has "
                         "passed: the chip ramps its clock over the first ~40 ms of this load "
                         "(tools/time_clock_ramp.py), and the metric is the steady state")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, everything else the benchmark measures: the iterate "
                         "kernel's own pass, working-set traces, harder-QP, K = 1, closed-loop, SURVEY "
                         "configs, recorded-run, coupled and CPU-baseline sections and the PMC traffic "
                         "lookup.  Off by default: a plain run sets up, warms up, times --steps steps, "
                         "writes --dump-outputs and prints the result line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (move plans, "
                         "QP status, working-set changes, and its batch's u_old with the first move "
                         "applied and the working sets it leaves for the next step) "
                         "as DIR/<name>.npy, float64")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--headline-only", action="store_true",
                    help="with --full: only the metric's steps and the kernels' own passes (no K = 1, "
                         "closed-loop, coupled or CPU sections): "
                         "profiler runs, so that every build launch in the trace is a headline one")
    ap.add_argument("--markers", action="store_true",
                    help="a torch.cuda._sleep launch before and after the timed steps and before and "
                         "after the iterate's event pass, so that a kernel trace of the run can be cut "
                         "to exactly those launches (tools/headline_pass_stats.py)")
    ap.add_argument("--build-events", choices=("timed", "separate"), default="timed",
                    help="timed: the build's HIP events ride on the timed steps (the roofline's "
                         "launch time is the timed launches'); separate: the timed steps run without "
                         "events and the build's launch time comes from a second pass of the same "
                         "steps (A/B of the events' own cost)")
    ap.add_argument("--build-event-stride", type=int, default=0,
                    help="with --build-events timed: event-stamp every n-th timed build launch only "
                         "(cmpc_set_timing_stride; the roofline's launch time is the mean of those). "
                         "0 (default): min(5, steps // 4), at least 1, so that >= 4 launches are "
                         "sampled; an event-stamped launch costs the stream ~4 us after the kernel "
                         "(every launch stamped: +1.6 %% per step, profiles/r6f_stride_u10_ab/)")
    ap.add_argument("--no-coupled", action="store_true", help="skip the config-4 (coupled) section")
    ap.add_argument("--configs-only", action="store_true",
                    help="only the SURVEY-config section's GPU configs (2, 3, 5), one JSON line: "
                         "profiler runs, so that the kernel statistics are the configs' own")
    ap.add_argument("--no-configs", action="store_true",
                    help="skip the SURVEY-config section (configs 1, 2, 3, 5 on this GPU)")
    ap.add_argument("--coupled-batch", type=int, default=4096, help="config-4 scenarios per GPU")
    ap.add_argument("--coupled-tiles", type=int, default=1,
                    help="config-4 scenario tiles per GPU, each on its own stream: a tile's "
                         "all-gather overlaps another tile's Jacobi iteration (1 = no overlap)")
    ap.add_argument("--dist-backend", default="nccl", choices=("nccl", "gloo"),
                    help="process-group backend for the barrier and the max over ranks "
                         "(nccl = RCCL; gloo only to rehearse several ranks on one GPU)")
    ap.add_argument("--force-dist", action="store_true",
                    help="set up the process group and run the collectives even at world size 1 "
                         "(an RCCL communicator of one rank: exercises the multi-GPU code path "
                         "on a one-GPU box)")
    args = ap.parse_args()
    if not args.full and (args.headline_only or args.configs_only or args.build_events == "separate"):
        ap.error("--headline-only, --configs-only and --build-events separate select among the "
                 "sections of a --full run: pass --full with them")
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    def device_count():
        import torch  # device_count() does not initialise the GPU (no HIP context)
        return torch.cuda.device_count()

    mode, n = launch_plan(args.gpus, args.dist_backend, os.environ, device_count)
    if mode == "spawn":
        sys.exit(spawn_ranks(n, sys.argv[1:]))

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    launch = ("torch.distributed.run child started by bench.py --gpus N" if os.environ.get(SELF_LAUNCH_ENV)
              else "external launcher (WORLD_SIZE set)" if "WORLD_SIZE" in os.environ else "single process")

    import torch
    if args.dist_backend == "nccl" and local >= torch.cuda.device_count():
        raise SystemExit(f"bench.py: rank {rank} has LOCAL_RANK {local}, {torch.cuda.device_count()} GPUs visible")
    if args.dist_backend == "gloo":
        local = local % max(1, torch.cuda.device_count())  # rehearsal: ranks may share a GPU
    torch.cuda.set_device(local)
    dist = None
    if world > 1 or args.force_dist:
        import torch.distributed as dist
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group("gloo")

    if args.configs_only:
        print(json.dumps({"configs": run_configs(local, args.settle_seconds, args.steps, with_cpp=False,
                                                 markers=True)}),
              flush=True)
        return

    import cmpc
    from cmpc.configs import reference_setup
    from cmpc.synthetic import synthetic_batch

    cfg = cmpc.reference_config("par", "coop", p=args.p)
    arrays = cmpc.controller_arrays(cfg, reference_setup("par", "coop"))
    B, S, K, NB = args.batch, cfg.S, args.K, args.input_batches
    t0 = time.time()
    batches, states = [], []
    u_old = du_old = ws = None
    dev = f"cuda:{local}"
    for b in range(NB):
        lin, u, du, w = synthetic_batch(cfg, B, seed=1002 + 101 * rank + b, n_distinct=min(B, 2048))
        if b == 0:
            u_old, du_old, ws, lin0 = u, du, w, lin
        batches.append(torch.from_numpy(lin).to(dev))
        # each batch is its own set of B scenarios with its own controller
        # state (u_old, move plans, warm-start working sets), resident in HBM
        states.append(tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                            for a in (u, du, w.view(np.int32))))
    torch.cuda.synchronize()
    log(f"[rank {rank}] synthetic inputs: {NB} x {B} scenarios in {time.time() - t0:.1f} s")

    ctx = cmpc.Context(cfg, B, device=local)
    ctx.configure(arrays)
    ctx.set_state(u_old, du_old, ws)

    def bind(i):
        """Step i runs on batch i % NB: its records and its own state, so every
        QP is warm-started from its own scenario's previous step (the reference
        hot-starts each controller's own QProblem, libs/mpc_qp_solver.cc:42-75)."""
        st_ = states[i % NB]
        ctx.bind_lin(batches[i % NB].data_ptr())
        ctx.bind_state(st_[0].data_ptr(), st_[1].data_ptr(), st_[2].data_ptr())

    for b in range(NB):  # InitializeQPProblem of every batch's controllers
        bind(b)
        ctx.build()
        ctx.init_warmstart()
    for i in range(args.warmup):
        bind(i)
        ctx.step(K, 0)
    ctx.synchronize()
    # clock settle (time the steady state): from a cold start the
    # step runs ~15 % slower for the first ~40 ms while the clock ramps up
    settle_steps, t_settle = 0, time.perf_counter()
    while time.perf_counter() - t_settle < args.settle_seconds:
        for _ in range(16):
            bind(args.warmup + settle_steps)
            ctx.step(K, 0)
            settle_steps += 1
        ctx.synchronize()
    # whole rotations of the batches (already so when NB divides 16): the timed
    # steps then start on the same batch in every run, whatever the settle
    # phase's step count was, and so does their last step (--dump-outputs)
    while settle_steps % NB:
        bind(args.warmup + settle_steps)
        ctx.step(K, 0)
        settle_steps += 1
    ctx.synchronize()
    t_settle = time.perf_counter() - t_settle
    # the timed steps continue the batch rotation where the warmup left it
    first = args.warmup + settle_steps

    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    # the roofline kernel (build) carries dispatch-stamped HIP events in the
    # timed steps; the iterate kernel is timed in its own pass afterwards.
    # The timed steps apply the first move (UpdateUOld):
    # each batch's u_old moves from its drawn state over the timed steps (the
    # warmup and settle steps leave it unchanged) and is restored after.
    snap = [tuple(a.clone() for a in st_) for st_ in states]

    def marker():
        """A short kernel on torch's stream with the library's stream idle: a
        kernel trace is cut between two of them (--markers)."""
        if args.markers:
            torch.cuda.synchronize()
            torch.cuda._sleep(1000)
            torch.cuda.synchronize()

    marker()
    torch.cuda.synchronize()
    ev_stride = args.build_event_stride or max(1, min(5, args.steps // 4))
    ctx.set_timing_stride(ev_stride)
    ctx.enable_timing(args.build_events == "timed", only=(cmpc.CMPC_KERNEL_BUILD,))
    t_start = time.perf_counter()
    for i in range(args.steps):
        bind(first + i)
        ctx.step(K, cmpc.CMPC_APPLY_MOVE)
    ctx.synchronize()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t_start
    marker()
    if dist:
        dist.barrier()
    build_ms, n_build = ctx.kernel_time(cmpc.CMPC_KERNEL_BUILD)
    ctx.set_timing_stride(1)
    if args.full and n_build == 0 and args.build_events == "timed":
        # the steps ran fused (a small --batch, CMPC_STEP_AUTO): the build
        # kernel's own launch time from a build-only pass for the roofline
        # (a plain run reports no build roofline then)
        ctx.enable_timing(True, only=(cmpc.CMPC_KERNEL_BUILD,))
        for i in range(args.steps):
            bind(first + i)
            ctx.build()
        ctx.synchronize()
        build_ms, n_build = ctx.kernel_time(cmpc.CMPC_KERNEL_BUILD)
        ctx.enable_timing(True, only=(cmpc.CMPC_KERNEL_BUILD,))
    t = torch.tensor([elapsed], dtype=torch.float64,
                     device=f"cuda:{local}" if args.dist_backend == "nccl" else "cpu")
    rank_elapsed = [elapsed]
    if dist:
        # every rank's own time (the balance of the shards), then the max
        parts = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(parts, t)
        rank_elapsed = [float(x.item()) for x in parts]
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed_max = float(t.item())

    du, st, nw = ctx.download()
    u_drift = max(float((st_[0] - sn[0]).abs().max()) for st_, sn in zip(states, snap))
    last = states[(first + args.steps - 1) % NB]  # the last step's batch
    ws_now = last[2].cpu().numpy()
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, rank, world,
                     {"du": du, "status": st, "working_set_changes": nw, "u_old": last[0].cpu().numpy(),
                      "working_set": ws_now.view(np.uint32)})
    # a plain run ends with its result line; everything below measures more
    extras = args.full and not args.headline_only

    def restore(warm=False):
        """The states of the timed steps' start; warm: then build-only
        launches (no controller state written) until the clock is back at
        the steady state, so that the pass that follows is timed like the
        headline's steps."""
        for st_, sn in zip(states, snap):
            for a, a0 in zip(st_, sn):
                a.copy_(a0)
        torch.cuda.synchronize()
        if warm:
            t_w = time.perf_counter()
            while time.perf_counter() - t_w < args.settle_seconds:
                for k in range(8):
                    bind(first + k)
                    ctx.build()
                ctx.synchronize()

    # the iterate kernel's own time: the same step loop from the same states,
    # events on the iterate only (after the headline measurement, untimed for
    # `value`)
    iter_ms, n_iter = 0.0, 0
    if args.full:
        restore(warm=True)
        marker()
        ctx.enable_timing(True, only=(cmpc.CMPC_KERNEL_ITERATE,))
        for i in range(args.steps):
            bind(first + i)
            ctx.step(K, cmpc.CMPC_APPLY_MOVE)
        ctx.synchronize()
        iter_ms, n_iter = ctx.kernel_time(cmpc.CMPC_KERNEL_ITERATE)
        marker()
    if args.build_events == "separate":
        # the build's launch time from a second pass of the timed steps
        restore(warm=True)
        ctx.enable_timing(True, only=(cmpc.CMPC_KERNEL_BUILD,))
        for i in range(args.steps):
            bind(first + i)
            ctx.step(K, cmpc.CMPC_APPLY_MOVE)
        ctx.synchronize()
        build_ms, n_build = ctx.kernel_time(cmpc.CMPC_KERNEL_BUILD)
    ctx.enable_timing(False)
    if args.full:
        restore()
    # working-set changes of the timed workload, summed over the K Jacobi
    # iterations and all QPs of a step (CMPC_TRACE counts, untimed pass over
    # one rotation of the batches)
    ws_changes = ws_changes_steps = None
    if extras:  # (profiler runs: every build launch a headline one, no traced solves)
        # a traced replay of the timed steps from the same states: the moves
        # applied over the timed steps shift u_old, so the later steps change
        # working sets that the first rotation does not
        ws_changes, ws_changes_steps = traced_changes(ctx, K, bind, range(first, first + args.steps))
        restore()

    # harder_qp: every state set meets other records at each of its steps
    # (step i: state i % NB, records (i + i // NB) % NB), so each QP's warm
    # start comes from another QP's solution and the active sets move
    harder = None
    if extras:
        def bind_h(i):
            st_ = states[i % NB]
            ctx.bind_lin(batches[(i + i // NB) % NB].data_ptr())
            ctx.bind_state(st_[0].data_ptr(), st_[1].data_ptr(), st_[2].data_ptr())
        try:
            for i in range(2 * NB):
                bind_h(i)
                ctx.step(K, 0)
            ctx.synchronize()
            restore(warm=True)
            t0 = time.perf_counter()
            for i in range(args.steps):
                bind_h(first + i)
                ctx.step(K, cmpc.CMPC_APPLY_MOVE)
            ctx.synchronize()
            t_h = (time.perf_counter() - t0) / args.steps
            restore(warm=True)
            ctx.enable_timing(True, only=(cmpc.CMPC_KERNEL_ITERATE,))
            for i in range(args.steps):
                bind_h(first + i)
                ctx.step(K, cmpc.CMPC_APPLY_MOVE)
            ctx.synchronize()
            ims_h, nih = ctx.kernel_time(cmpc.CMPC_KERNEL_ITERATE)
            ctx.enable_timing(False)
            restore()
            ch_h, _ = traced_changes(ctx, K, bind_h, range(first, first + NB))
            restore()
            harder = {"ms_per_step": t_h * 1e3, "qp_solves_per_s_per_gpu": B * S * K / t_h,
                      "iterate_ms": ims_h / max(nih, 1), "working_set_changes_per_step": ch_h,
                      "note": "step i binds state set i % NB to records (i + i // NB) % NB: every warm "
                              "start comes from the solution of another QP (the reference's hotstart "
                              "after its QP changed, libs/mpc_qp_solver.cc:62-64)"}
        except Exception as e:  # reported, never required
            log(f"harder_qp variant failed: {e}")
        finally:
            restore()
    # the sections below run on the context's own state buffers
    if args.full:
        ctx.bind_state()
        ctx.bind_lin(0)
        ctx.set_state(u_old, du_old, ws)

    def warm():
        """Build launches on a resident batch for --settle-seconds, then the
        context's own record buffer is bound again: the clock drops while
        the GPU waits on host work (state snapshots, input set-up) and ramps
        back over ~40 ms of load, so every timed section below
        starts at the steady clock.  Builds write only the QP buffer, which
        the timed section rebuilds: no controller state changes."""
        t_w = time.perf_counter()
        ctx.bind_lin(batches[0].data_ptr())
        while time.perf_counter() - t_w < args.settle_seconds:
            for _ in range(16):
                ctx.build()
            ctx.synchronize()
        ctx.bind_lin(0)

    # K = 1 (the build-dominated figure beside the K = 9 headline),
    # this rank, after the headline measurement
    k1 = None
    if extras:
        try:
            warm()
            for i in range(2):
                bind(i)
                ctx.step(1, 0)
            ctx.synchronize()
            reps1 = max(10, args.steps // 2)
            t0 = time.perf_counter()
            for i in range(reps1):
                bind(i)
                ctx.step(1, 0)
            ctx.synchronize()
            t_k1 = (time.perf_counter() - t0) / reps1
            k1 = {"qp_solves_per_s_per_gpu": B * S / t_k1, "ms_per_step": t_k1 * 1e3, "steps": reps1,
                  "note": "K = 1 Jacobi iteration per step (build-dominated), this rank's GPU"}
        except Exception as e:  # reported, never required
            log(f"K=1 variant failed: {e}")
        finally:  # the sections below run on the context's own state buffers
            ctx.bind_state()
            ctx.bind_lin(0)
            restore()

        # Closed-loop variant (reported beside the metric, not in `value`): the
        # records are produced on the device from plant states each step
        # (cmpc_produce_lin), then build + K iterations with
        # the first move applied.
    closed = None
    if extras:
        try:
            from cmpc.synthetic import synthetic_operating_points, synthetic_u_old
            xs, us, ys = synthetic_operating_points(cfg, B, seed=77 + rank, n_distinct=min(B, 2048))
            tx, tu, ty = (torch.from_numpy(a).to(f"cuda:{local}") for a in (xs, us, ys))
            warm()
            ctx.set_state(synthetic_u_old(cfg, B, np.random.default_rng(78 + rank)),
                          np.zeros((B * S, cfg.nV)), np.zeros(B * S, np.uint32))
            ctx.produce_lin(tx.data_ptr(), tu.data_ptr(), ty.data_ptr())
            ctx.build()
            ctx.init_warmstart()
            ctx.produce_lin(tx.data_ptr(), tu.data_ptr(), ty.data_ptr())
            ctx.step(K, cmpc.CMPC_APPLY_MOVE)
            ctx.synchronize()
            reps = max(3, args.steps // 5)
            t0 = time.perf_counter()
            for _ in range(reps):
                ctx.produce_lin(tx.data_ptr(), tu.data_ptr(), ty.data_ptr())
            ctx.synchronize()
            t_prod = (time.perf_counter() - t0) / reps
            ctx.enable_timing(True)
            t0 = time.perf_counter()
            for _ in range(reps):
                ctx.produce_lin(tx.data_ptr(), tu.data_ptr(), ty.data_ptr())
                ctx.step(K, cmpc.CMPC_APPLY_MOVE)
            ctx.synchronize()
            t_cl = (time.perf_counter() - t0) / reps
            kms = lambda k: ctx.kernel_time(k)[0] / max(ctx.kernel_time(k)[1], 1)
            cl_kernels = {"produce": kms(cmpc.CMPC_KERNEL_PRODUCE), "build": kms(cmpc.CMPC_KERNEL_BUILD),
                          "iterate": kms(cmpc.CMPC_KERNEL_ITERATE)}
            ctx.enable_timing(False)
            _, st_cl, _ = ctx.download()
            _, _, ws_cl = ctx.get_state()
            closed = {"ms_per_step": t_cl * 1e3, "producer_ms": t_prod * 1e3,
                      "kernels_ms": cl_kernels,
                      "qp_status_ok_fraction": float((st_cl == 0).mean()),
                      "qp_active_constraint_fraction": float((ws_cl != 0).mean()),
                      "qp_solves_per_s": B * S * K / t_cl,
                      "note": "device producer (plant linearisation + discretisation + records) + build "
                              "+ K iterations with the move applied; synthetic plant states held fixed "
                              "(no plant simulation), so applied moves accumulate step to step"}
            # the full receding-horizon step with the per-sub-controller observer
            # (SURVEY §8(f) row 2): a posteriori update + linearisation at each
            # slot's x_hat, build, K iterations, a priori update + u_old += du
            try:
                # the reference runs' gain M = [0; I], identified from their records
                # (cmpc.reference_observer_gain, tests/test_closed_loop_golden.py)
                Mg = cmpc.reference_observer_gain(cfg, ys.shape[1])
                for s_ in range(S):
                    ctx.set_observer(s_, Mg)
                warm()
                ctx.set_state(synthetic_u_old(cfg, B, np.random.default_rng(78 + rank)),
                              np.zeros((B * S, cfg.nV)), np.zeros(B * S, np.uint32))
                ctx.observer_init(tx.data_ptr(), tu.data_ptr(), ty.data_ptr())
                ctx.build()
                ctx.init_warmstart()
                ctx.synchronize()
                # the isolated kernel timings below advance the observer and the
                # plans without the build/iterate between them: snapshot the
                # state and restore it before the full-step loop
                obs_snap, state_snap = ctx.observer_state(), ctx.get_state()
                t0 = time.perf_counter()
                for _ in range(reps):
                    ctx.observe_step(tu.data_ptr(), ty.data_ptr())
                ctx.synchronize()
                t_os = (time.perf_counter() - t0) / reps
                t0 = time.perf_counter()
                for _ in range(reps):
                    ctx.observe_apply()
                ctx.synchronize()
                t_oa = (time.perf_counter() - t0) / reps
                ctx.set_observer_state(obs_snap)
                ctx.set_state(*state_snap)
                warm()
                ctx.enable_timing(True)
                t0 = time.perf_counter()
                for _ in range(reps):
                    ctx.observe_step(tu.data_ptr(), ty.data_ptr())
                    ctx.build()
                    ctx.iterate(K)
                    ctx.observe_apply()
                ctx.synchronize()
                t_full = (time.perf_counter() - t0) / reps
                obs_kernels = {"observe_post_produce": kms(cmpc.CMPC_KERNEL_PRODUCE),
                               "build": kms(cmpc.CMPC_KERNEL_BUILD), "iterate": kms(cmpc.CMPC_KERNEL_ITERATE),
                               "observe_prior": kms(cmpc.CMPC_KERNEL_OBSERVE_PRIOR)}
                ctx.enable_timing(False)
                _, st_o, _ = ctx.download()
                closed["with_observer"] = {
                    "ms_per_step": t_full * 1e3, "kernels_ms": obs_kernels, "observe_step_ms": t_os * 1e3,
                    "observe_apply_ms": t_oa * 1e3,
                    "qp_status_ok_fraction": float((st_o == 0).mean()),
                    "qp_solves_per_s": B * S * K / t_full,
                    "note": "observe a posteriori + per-QP linearisation at x_hat (records), build, "
                            "K iterations, observe a priori + u_old update; measured y held fixed, "
                            f"the reference runs' observer gain [0; I], {reps} consecutive steps"}
            except Exception as e:
                log(f"observer closed-loop variant failed: {e}")
        except Exception as e:  # reported, never required
            log(f"closed-loop variant failed: {e}")
        # The whole closed loop of the reference's runs for B scenarios at once
        # (cmpc/driver.py: plant interval with the input delay line, observer,
        # build, K iterations, u_old update), this configuration, the reference
        # runs' observer gain, operating points 0.2 % around the default one
        if closed is not None:
            try:
                from cmpc.driver import ClosedLoop
                x_def, u_def = cmpc.plant_default(cfg.plant)
                rng_p = np.random.default_rng(79 + rank)
                x0s = x_def[None, :] * (1 + 0.002 * rng_p.uniform(-1, 1, (B, len(x_def))))
                M_ref = cmpc.reference_observer_gain(cfg)
                loop = ClosedLoop(cfg, arrays, [M_ref] * S, x0s, np.tile(u_def, (B, 1)), K, device=local)
                try:
                    loop.initialize()
                    for _ in range(3):
                        loop.step()
                    warm()
                    torch.cuda.synchronize(local)
                    reps_p = max(5, args.steps // 5)
                    t0 = time.perf_counter()
                    for _ in range(reps_p):
                        loop.step()
                    torch.cuda.synchronize(local)
                    t_p = (time.perf_counter() - t0) / reps_p
                    # the same steps again with the library's kernels event-timed
                    loop.ctx.enable_timing(True)
                    for _ in range(reps_p):
                        loop.step()
                    torch.cuda.synchronize(local)
                    lk = lambda k: loop.ctx.kernel_time(k)[0] / max(loop.ctx.kernel_time(k)[1], 1)
                    plant_kernels = {"observe_post_produce": lk(cmpc.CMPC_KERNEL_PRODUCE),
                                     "build": lk(cmpc.CMPC_KERNEL_BUILD), "iterate": lk(cmpc.CMPC_KERNEL_ITERATE),
                                     "observe_prior": lk(cmpc.CMPC_KERNEL_OBSERVE_PRIOR)}
                    loop.ctx.enable_timing(False)
                    _, st_p, _ = loop.ctx.download()
                    n_fail, _ = loop.plant_failures()   # sticky: every interval since initialize
                finally:
                    loop.close()
                closed["with_plant"] = {
                    "ms_per_step": t_p * 1e3, "scenario_steps_per_s": B / t_p, "qp_solves_per_s": B * S * K / t_p,
                    "kernels_ms": plant_kernels,
                    "qp_status_ok_fraction": float((st_p == 0).mean()), "plant_step_failures": n_fail,
                    "steps": reps_p,
                    "note": "cmpc.driver.ClosedLoop: y = plant output, observe a posteriori + per-QP "
                            "linearisation, build, K iterations, observe a priori, u_old += own first "
                            "moves, input delay line, controlled Dormand-Prince over Ts = 0.05 s; "
                            "observer gain [0; I]; the reference's recorded step (controller only, "
                            "one scenario, p = 100) is 900.4 us"}
            except Exception as e:  # reported, never required
                log(f"closed loop with the plant failed: {e}")
        # SURVEY config 4 (sub-controllers sharded over the ranks, RCCL all-gather
        # of the plans once per Jacobi iteration), beside the metric: every rank
        # takes part, so at world N it times the exchange over xGMI
    # SURVEY §8(d) / BASELINE.json configs beside the metric, this GPU:
    # 1 (cent-ser p = 100) as the reference's B = 1 call through the C++
    # adapter, 2, 3 and 5 at their batch sizes; 4 is the `coupled` section
    configs = None
    if not args.no_configs and extras and world == 1:
        configs = run_configs(local, args.settle_seconds, args.steps)
    recorded = None
    if extras and world == 1:
        try:
            recorded = recorded_run_changes(local)
        except Exception as e:  # reported, never required
            log(f"recorded-run replay failed: {e}")
    def coupled_section(S_local, S_total, note, scaling_note):
        """SURVEY config 4 on every rank (cmpc.coupled.run_coupled_bench),
        the max of the elapsed time over ranks; None when any rank failed."""
        from cmpc.coupled import run_coupled_bench
        rc = None
        try:  # reported beside the metric, never required for it
            rc = run_coupled_bench(rank, world, local, S_local=S_local, S_total=S_total, B=args.coupled_batch,
                                   p=args.p, K=K, steps=max(5, args.steps // 2),
                                   settle_seconds=args.settle_seconds, force_collective=bool(dist),
                                   tiles=args.coupled_tiles)
        except Exception as e:
            log(f"[rank {rank}] coupled section (S_total {S_total}) failed: {e}")
        # every rank joins the reduction; a failed rank reports +inf, so the
        # section is dropped everywhere
        tc = torch.tensor([rc["elapsed_s"] if rc else float("inf")], dtype=torch.float64,
                          device=f"cuda:{local}" if args.dist_backend == "nccl" else "cpu")
        if dist:
            dist.all_reduce(tc, op=dist.ReduceOp.MAX)
        el_c = float(tc.item())
        if not rc or el_c == float("inf"):
            return None
        out_c = dict(rc)
        out_c.pop("elapsed_s")
        out_c.update({
            "qp_solves_per_s": world * rc["qp_per_gpu"] * K * rc["steps"] / el_c,
            "ms_per_step": el_c / rc["steps"] * 1e3,
            "exchange": ("RCCL all_gather_into_tensor of B x S_local x nV plans per Jacobi iteration"
                         if dist and args.dist_backend == "nccl" else
                         "gloo all_gather of the plans through host memory (rehearsal only)" if dist
                         else "local copy (world size 1)"),
            "note": note, "scaling_note": scaling_note})
        return out_c

    coupled = coupled_s64 = None
    if not args.no_coupled and extras:
        common = ("step = build + K x (all-gather + coupled iteration), first move applied; with "
                  "tiles > 1 the scenarios run as that many tiles on their own streams, each tile's "
                  "all-gather overlapping another tile's iteration (cmpc.coupled.CoupledPipeline; "
                  "slower at world 1, DESIGN.md section 8); gather_ms (summed over the tiles) and "
                  "iterate_kernel_ms (G_ext_hbm_frac: G_ext bytes per iteration / that time / 8 TB/s) "
                  "from events in separate passes")
        coupled = coupled_section(
            8, 8 * world,
            "SURVEY config 4, 8 sub-controllers per GPU: S_total = 8 x world sub-controllers per "
            "scenario (synthetic coupling, cmpc/coupled.py); " + common,
            "not constant work per GPU: S_total = 8 x world, so each QP's f_k update reads nV x "
            "(S_total - 1) nV coupling entries and the gathered plans grow with world; a SCALE curve "
            "of this section is weak scaling in scenarios per GPU with per-QP work growing linearly "
            "in world size (coupled_s64 is the fixed 64-sub-controller system)")
        # BASELINE config 4's own problem at every world size (VERDICT r5,
        # next 2): S_total = 64 sub-controllers, 64 / world per GPU, B
        # scenarios: the same system at world 1, 2, 4 and 8
        if 64 % world == 0:
            coupled_s64 = coupled_section(
                64 // world, 64,
                "BASELINE config 4's system: S_total = 64 sub-controllers per scenario, S_local = "
                "64 / world per GPU (all 64 and the whole G_ext on one GPU at world 1); " + common,
                "strong scaling in sub-controllers: the same 64-sub-controller system of B scenarios "
                "at every world size, each GPU holding 64 / world of them")

    ok_frac = float((st == 0).mean())
    active_frac = float((ws_now != 0).mean())
    mean_chg = float(nw.mean())

    solves = world * B * S * K * args.steps
    value = solves / elapsed_max
    L = ctx.layout
    avg_build_s = build_ms / max(n_build, 1) / 1e3
    f_build = build_flops(cfg, L.naug, L.nd)
    # (no event-stamped build launch: a plain run whose steps ran fused)
    achieved_tf = B * S * f_build / avg_build_s / 1e12 if n_build else None
    build_kernel = ("cmpc_build_rows_kernel" if ctx.last_build_kernel() == cmpc.CMPC_BUILD_ROWS
                    else "cmpc_build_kernel")
    traffic, traffic_prov = (pmc_traffic(B, build_kernel) if args.full else
                             (None, {"file": "profiles/pmc_build_coop_p50.json",
                                     "status": "not looked up: a --full run does"}))

    out = {
        "metric": "QP solves/sec (whole node), cooperative-parallel MPC, horizon p=50",
        "value": value,
        "unit": "QP solves/s",
        "n_gpus": world,
        "gpus_requested": args.gpus,
        "launch": launch,
        "steps": args.steps,
        "warmup": args.warmup,
        "full": args.full,
        "ms_per_step": elapsed_max / args.steps * 1e3,
        "rank_ms_per_step": [e / args.steps * 1e3 for e in rank_elapsed],
        "clock_settle": {"seconds": t_settle, "steps": settle_steps,
                         "note": "untimed steps after the warmup, until the clock has ramped up"},
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic (SURVEY.md §8(d) recipe, seeded; resident in HBM)",
        "config": {
            "workload": (f"cooperative-parallel, 2 compressors, p={cfg.p}, m={cfg.m}, "
                         f"S={S} sub-controllers, K={K} Jacobi iterations, {B} scenarios/GPU"),
            "global_batch": world * B,
            "qp_per_gpu": B * S,
            "p": cfg.p, "m": cfg.m, "S": S, "K": K,
            "input_batches": NB,
            "parallelism": f"scenario-sharded replicas x{world} (no data-path collective)",
        },
        "roofline": {
            "bound": "fp64-valu",
            "pipe": "fp64 VALU (v_fmac_f64_dpp); MI355X FP64 vector peak = FP64 matrix peak",
            "kernel": build_kernel + "<NS=11,NY=3,NUT=4,NU=2,M=2,ND=2,WPG=4,RING=0,WPE=3>",
            "achieved": achieved_tf,
            "peak": FP64_PEAK_TFLOPS,
            "unit": "TFLOP/s",
            "frac": achieved_tf / FP64_PEAK_TFLOPS if n_build else None,
            "traffic": traffic,
            "traffic_provenance": traffic_prov,
            "flops_per_qp": f_build,
            "algorithmic_bytes_per_qp": build_bytes(cfg, L),
            "avg_launch_ms": avg_build_s * 1e3,
            "launches": n_build,
            "launches_note": (f"HIP events (hipExtLaunchKernel) on every {ev_stride}-th build launch of the "
                              f"{args.steps} timed steps, the mean of those" if args.build_events == "timed"
                              else "HIP events on every build launch of a second pass of the timed steps"),
        },
        "path_roofline": {
            "definition": ("whole step against the FP64 peak: the FLOPs this build performs per "
                           "sub-controller step that the reference's path also needs (F_build of "
                           "SURVEY 8(d), plus 2 nV nVo per Jacobi iteration for f_k = f + G du_other) "
                           "x B*S per GPU / measured step time (max over ranks); the QP solves "
                           "themselves are not counted"),
            "flops_per_qp_step": f_build + K * applied_iterate_flops(cfg),
            "achieved": B * S * (f_build + K * applied_iterate_flops(cfg)) / (elapsed_max / args.steps)
                        / 1e12,
            "peak": FP64_PEAK_TFLOPS,
            "unit": "TFLOP/s per GPU",
            "frac": B * S * (f_build + K * applied_iterate_flops(cfg)) / (elapsed_max / args.steps)
                    / 1e12 / FP64_PEAK_TFLOPS,
            "note": ("SURVEY 8(d)'s F_it (the reference's (p ny)-long ApplyOtherInput products, "
                     f"{iterate_flops(cfg):.0f} FLOPs per iteration) is not credited: this build "
                     "forms G = Su'W Su_other once in the build kernel and applies it with nV nVo "
                     "FMAs per iteration"),
        },
        "kernels_ms_per_step": {"build": build_ms / max(n_build, 1),
                                "iterate": iter_ms / max(n_iter, 1) if args.full else None,
                                "build_events": args.build_events,
                                "build_event_stride": ev_stride,
                                "note": "build: HIP events on every timed step (--build-events timed) or "
                                        "in a later pass of the same steps (separate); iterate: events in "
                                        "a second pass of the same step loop after the timed steps"},
        "k1": k1,
        "qp_status_ok_fraction": ok_frac,
        "qp_active_constraint_fraction": active_frac,
        "u_old_max_drift_over_timed_steps": u_drift,
        "mean_working_set_changes_last_solve": mean_chg,
        "working_set_changes_per_step": ws_changes,
        "working_set_changes_per_qp_step": None if ws_changes is None else ws_changes / (B * S),
        "working_set_changes_first_last_steps": (None if not ws_changes_steps else
                                                 [ws_changes_steps[:NB], ws_changes_steps[-NB:]]),
        "working_set_changes_note": ("summed over all K Jacobi iterations and all QPs of a timed step, "
                                     "mean over a traced replay of all the timed steps from the same "
                                     "states (CMPC_TRACE counts); per_qp_step = per step / (B S)"),
        "recorded_run": recorded,
        # the recorded run's solver load beside the synthetic headline's
        # working_set_changes_per_qp_step (the synthetic load is the higher
        # one, so no variant calibrated to the recorded rate is reported)
        "recorded_run_working_set_changes_per_qp_step": (
            recorded.get("working_set_changes_per_qp_step") if isinstance(recorded, dict) else None),
        "harder_qp": harder,
        "configs": configs,
        "closed_loop_device_resident": closed,
        "coupled": coupled,
        "coupled_s64": coupled_s64,
    }
    if rank == 0 and world == 1 and not args.no_cpu and extras:
        try:
            out["cpu_baseline"] = cpu_baseline(cfg, arrays, lin0, u_old, K, args.cpu_seconds)
        except Exception as e:  # the baseline is reported, never required
            log(f"cpu baseline failed: {e}")
            out["cpu_baseline"] = None
    if rank == 0:
        print(json.dumps(out), flush=True)
    ctx.close()
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
