"""Closed-loop driver: the reference's missing
common-simulation.inc, rebuilt from its surviving pieces and
batched over B scenarios on the device:

  per sampling instant t_k = t0 + k Ts (integrate_const's observer callback,
  simulation_system.h:48, :108-116):
    y      = plant output at x(t_k)                  SimulationSystem::GetOutput
    u      = NerveCenter::GetNextInputWithTiming(y)  nerve_center.h:134-182:
               observe a posteriori + linearise per sub-controller,
               condensed QP build, K Jacobi iterations, UpdateU (observer a
               priori + u_old), UpdateUOld (the nerve-level u_old_)
    record (t, x, u, y, ns) in the 6-line .dat format
    SetInput(u)   -> input delay line -> plant input  simulation_system.h:67-70
    integrate the plant over [t_k, t_k + Ts]          (controlled Dormand-Prince)

  The setup file's `simulation` segments are one Integrate call each, the
  plant-input offset stepped in between (SetOffset, simulation_system.h:64;
  the controller keeps its own offset, so the step is an unmeasured
  disturbance).  integrate_const observes both ends of its interval, so the
  instant at a segment boundary is observed twice: the last observation of
  one call (no integration follows), SetOffset, then the first of the next
  call at the same plant state, whose step-size control starts again from
  Ts.  The reference's records show exactly that (results/*/run1/*.dat: the
  records printed at t = 50 and 50.05 hold the same plant state, and every
  record is one controller call); the record count, not integrate_const's
  time, labels them.

Everything between two records runs on the GPU (sim.hip, observer.hip,
produce.hip, cmpc_kernels.hip); torch tensors are the device buffers.
"""
import collections
import time

import numpy as np

from . import CMPC_TRACE, Context, scenario_limits, scenario_reference_offsets
from .configs import ControllerConfig
from .sim import (EQ_MAX_ITER, EQ_TOL, REF_CONTROL_INDEX, REF_DELAYS, REF_EPS, REF_TS, TARGET_TOL_Y,
                  FreqResponse, PlantGains, PlantSimulator)  # noqa: F401

# ClosedLoop.modes: the summary's columns (include/cmpc.h, _abi.MODES_SUMMARY),
# the eigenvalues and the statuses
PlantModes = collections.namedtuple("PlantModes", ("abscissa", "n_unstable", "zeta_min", "omega_d", "omega_n",
                                                   "re_min", "w", "status"))
# ClosedLoop.trim_to_outputs: the solve's results and the free inputs in force
TrimTargets = collections.namedtuple("TrimTargets", ("status", "iters", "resid", "u_free", "du_free"))


def _fmt(v: float) -> str:
    """std::ostream default formatting of a double (precision 6, %g)."""
    return "%g" % v


def eigen_row(vals) -> str:
    """Eigen's default matrix output of a vector printed transposed: every
    coefficient right-aligned to the widest one, separated by one space."""
    s = [_fmt(float(v)) for v in vals]
    w = max(len(t) for t in s)
    return " ".join(t.rjust(w) for t in s)


class DatWriter:
    """The reference's per-sample record (results/*.dat):
    t / x / u / y / wall-ns / blank."""

    def __init__(self, path_or_file):
        self.f = open(path_or_file, "w") if isinstance(path_or_file, str) else path_or_file
        self.own = isinstance(path_or_file, str)

    def record(self, t: float, x, u, y, ns: int):
        self.f.write(f"{_fmt(t)}\n{eigen_row(x)}\n{eigen_row(u)}\n{eigen_row(y)}\n{int(ns)}\n\n")

    def close(self):
        if self.own:
            self.f.close()


class ClosedLoop:
    """B closed loops (plant + NerveCenter) of one configuration on one GPU.

    cfg, arrays    controller configuration and weights/constraints/y_ref
    M              per sub-controller observer gains ((ns + ndist) x n_outputs)
    x0, u_offset   (B, ns), (B, n_inputs) host arrays: initial plant state and
                   the input offset u_init_full (NerveCenter::Initialize)
    K              Jacobi iterations per step (n-iterations)
    y_offset       (B, n_outputs) per-scenario constant setpoint offsets per
                   plant output, or None (set_setpoints changes them later)
    limits         (lower, upper, rate_lower, rate_upper), each (B, nu_tot) in
                   plant control order: per-scenario input limits, or None
    pressures      (B, 2) per-scenario boundary pressures [p_in, p_out] of the
                   plant, or None: the scalars p_in, p_out for every scenario
    model_pressures  (B, 2) the same for the controller's model; None: the
                   model follows `pressures`.  Passing both gives a
                   plant/model mismatch study.
    All are in force before initialize (the first build and the cold solves).
    set_setpoint_schedule adds per-scenario setpoint schedules with preview,
    set_pressures and set_pressure_schedule change the pressures during a run.
    """

    def __init__(self, cfg: ControllerConfig, arrays, M, x0, u_offset, K: int, device: int = 0,
                 Ts: float = REF_TS, p_in: float = 1.0, p_out: float = 1.0, y_offset=None, limits=None,
                 pressures=None, model_pressures=None):
        import torch
        self.torch = torch
        torch.cuda.init()
        dev = torch.device("cuda", device)
        self.cfg, self.K, self.Ts, self.dev = cfg, K, Ts, dev
        self.arrays = arrays
        self.p_in, self.p_out = p_in, p_out
        B = x0.shape[0]
        self.B, S = B, cfg.S
        for a, what in ((pressures, "pressures"), (model_pressures, "model_pressures")):
            if a is not None:   # (refused before anything is allocated)
                self._pressure_check(a, what)
        self.sim = PlantSimulator(cfg.plant, B, device, p_in, p_out, REF_DELAYS, REF_CONTROL_INDEX)
        self.ctx = Context(cfg, B, device=device)
        self.ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        self.ctx.configure(arrays)
        self.ctx.set_state(np.zeros((B * S, cfg.nu_tot)), np.zeros((B * S, cfg.nV)),
                           np.zeros(B * S, np.uint32))
        for s in range(S):
            self.ctx.set_observer(s, M[s])
        self._scores = False    # enable_scores: closed-loop indices per QP slot
        self._envelope = False  # enable_envelope: the ensemble's spread per step
        self._dy_ref = None     # the setpoint offsets in force, (B*S, ny) host
        if y_offset is not None:
            self.set_setpoints(y_offset)
        if limits is not None:
            self.ctx.set_scenario_constraints(*scenario_limits(cfg, *limits))
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
        self.x0, self.u_offset = t(x0), t(u_offset)
        self.u_ctrl = torch.zeros(B, cfg.nu_tot, dtype=torch.float64, device=dev)  # NerveCenter::u_old_
        self.u_lin = torch.zeros_like(self.u_offset)   # GetPlantInput(u_old_, u_offset_)
        self.io = np.ascontiguousarray(cfg.input_order, dtype=np.int32)
        self.k = 0
        self._sched = []   # pending (t_start, plant-input offset (B, n_inputs) device)
        self._sp_sched = None   # setpoint schedule in slot order, (B, S, T, ny) device
        self._sp_window = None  # the bound reference profile, (B*S, p, ny) device
        self._pp = self._pm = None            # bound pressures of plant and model, (B, 2) device
        self._pp_sched = self._pm_sched = None  # their schedules, (B, T, 2) device
        if pressures is not None or model_pressures is not None:
            self.set_pressures(pressures, pressures if model_pressures is None else model_pressures)
        self._noise = None         # set_noise: the seed, the device arrays and the scratch tensors
        self._plant_offset = self.u_offset   # the plant's input offset in force (segment switches followed)
        self.last_measurement = None

    def set_segments(self, segments, u_default):
        """The setup file's `simulation` segments ([(offset change, end time)],
        SetupFile.segments) over the plant's default input u_default (offset
        changes and u_default may be per scenario, (B, n_inputs)): segment 0's
        offset is the initial one (call before initialize); segment i's is set
        after the last instant of segment i-1 (its end time), which no
        integration follows (module docstring)."""
        torch = self.torch
        u_default = np.asarray(u_default, dtype=np.float64)
        # per-scenario defaults and changes broadcast: (n_inputs,) or (B, n_inputs)
        shape = (self.B, u_default.shape[-1])
        offs = [np.array(np.broadcast_to(u_default + np.asarray(d, dtype=np.float64), shape)) for d, _ in segments]
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.u_offset = self._plant_offset = t(offs[0])
        self._sched = [(float(segments[i - 1][1]), t(offs[i])) for i in range(1, len(segments))]

    def set_setpoints(self, y_offset):
        """Per-scenario constant setpoint offsets, (B, n_outputs) per plant
        output, in force from the next build on; None removes them."""
        if y_offset is None:
            self.ctx.set_scenario_reference(None)
            self._dy_ref = self._score_sched = None
            return
        y_offset = np.asarray(y_offset, dtype=np.float64)
        if y_offset.ndim != 2 or y_offset.shape[0] != self.B:
            raise ValueError(f"y_offset must be (B = {self.B}, n_outputs), got {y_offset.shape}")
        self._dy_ref = scenario_reference_offsets(self.cfg, y_offset)
        self._score_sched = None
        self.ctx.set_scenario_reference(self._dy_ref)

    def set_weights_per_scenario(self, uwt, ywt):
        """Per-scenario weights for a tuning sweep: uwt (B, S, nu, nu) and ywt
        (B, S, ny, ny), scenario b's sub-controller s taking uwt[b][s] and
        ywt[b][s] in place of the shared arrays' from the next build on (call
        before initialize for the whole run); both None restores the shared
        weights.  Forwarded to Context.set_scenario_weights.  The loop's step
        is the three calls observe_step / build + iterate / observe_apply, the
        form a control step takes with per-slot weights in force."""
        if uwt is None and ywt is None:
            self.ctx.set_scenario_weights(None, None)
            return
        S, nu, ny = self.cfg.S, self.cfg.nu, self.cfg.ny
        u = np.asarray(uwt, dtype=np.float64)
        y = np.asarray(ywt, dtype=np.float64)
        if u.shape != (self.B, S, nu, nu) or y.shape != (self.B, S, ny, ny):
            raise ValueError(f"uwt must be (B = {self.B}, S = {S}, nu, nu) and ywt (B, S, ny, ny), "
                             f"got {u.shape} and {y.shape}")
        self.ctx.set_scenario_weights(u.reshape(self.B * S, nu, nu), y.reshape(self.B * S, ny, ny))

    def set_setpoint_schedule(self, schedule):
        """Per-scenario setpoint schedules with preview: (B, T, n_outputs)
        plant-output deviations per control step, in force from the next build
        on; None removes them.  At control step t slot q = b*S + s tracks, at
        horizon row r, its reference plus
        schedule[b][min(t + 1 + r, T - 1)][out_idx[s]]: row r is the output
        1 + r samples after the step's measurement (as the prediction's row 0
        is the output after the first move), and the schedule's last row is
        held past its end.  The window is gathered on the device and bound as
        the context's reference profile
        (Context.bind_scenario_reference_profile).  Independent of
        set_setpoints; the two add."""
        torch = self.torch
        self._score_sched = None
        if schedule is None:
            self.ctx.bind_scenario_reference_profile(0)
            self._sp_sched = self._sp_window = None
            return
        schedule = np.asarray(schedule, dtype=np.float64)
        n_out = int(np.max(self.cfg.out_idx)) + 1
        if schedule.ndim != 3 or schedule.shape[0] != self.B or schedule.shape[1] < 1 or schedule.shape[2] < n_out:
            raise ValueError(f"schedule must be (B = {self.B}, T >= 1, n_outputs >= {n_out}), got {schedule.shape}")
        if not np.isfinite(schedule).all():
            raise ValueError("schedule must be finite")
        oi = torch.as_tensor(np.asarray(self.cfg.out_idx, dtype=np.int64)[:, :self.cfg.ny], device=self.dev)
        sch = torch.from_numpy(np.ascontiguousarray(schedule)).to(self.dev)
        # (B, T, S, ny) -> (B, S, T, ny)
        self._sp_sched = sch[:, :, oi].permute(0, 2, 1, 3).contiguous()
        self._sp_window = torch.zeros(self.B * self.cfg.S, self.cfg.p, self.cfg.ny, dtype=torch.float64,
                                      device=self.dev)
        self._sp_rows = torch.arange(self.cfg.p, device=self.dev)
        self.ctx.bind_scenario_reference_profile(self._sp_window.data_ptr())

    def _setpoint_window(self):
        """The schedule's window of control step self.k into the bound profile."""
        if self._sp_sched is None:
            return
        T = self._sp_sched.shape[2]
        idx = (self._sp_rows + (self.k + 1)).clamp_(max=T - 1)
        self._sp_window.copy_(self._sp_sched[:, :, idx, :].reshape(self._sp_window.shape))

    def _pressure_array(self, a, what, sched=False):
        a = self._pressure_check(a, what, sched)
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def _pressure_check(self, a, what, sched=False):
        a = np.asarray(a, dtype=np.float64)
        if sched:
            if a.ndim != 3 or a.shape[0] != self.B or a.shape[1] < 1 or a.shape[2] != 2:
                raise ValueError(f"{what} must be (B = {self.B}, T >= 1, 2), got {a.shape}")
        elif a.shape != (self.B, 2):
            raise ValueError(f"{what} must be (B = {self.B}, 2), got {a.shape}")
        if not np.isfinite(a).all() or not (a > 0).all():
            raise ValueError(f"{what} must be finite and positive")
        return a

    def _bound_pressures(self, model: bool):
        """The (B, 2) device array bound to the model or the plant, made and
        bound at first use, starting from the scalars."""
        cur = self._pm if model else self._pp
        if cur is None:
            cur = self.torch.tensor([self.p_in, self.p_out], dtype=self.torch.float64,
                                    device=self.dev).repeat(self.B, 1).contiguous()
            if model:
                self._pm = cur
                self.ctx.bind_scenario_pressures(cur.data_ptr())
            else:
                self._pp = cur
                self.sim.bind_pressures(cur.data_ptr())
        return cur

    def set_pressures(self, plant=None, model=None):
        """Per-scenario boundary pressures [p_in, p_out], each (B, 2): `plant`
        for the plant's next integration, `model` for the controller's next
        linearisation.  An argument left None keeps what is in force.  The
        values go into device arrays bound to the simulator and the context
        (PlantSimulator.bind_pressures, Context.bind_scenario_pressures), so a
        call between two steps launches nothing but the copy.  A schedule
        (set_pressure_schedule) overwrites them at its next step."""
        new = [(m, self._pressure_array(a, w)) for m, a, w in ((False, plant, "plant"), (True, model, "model"))
               if a is not None]
        for m, a in new:
            self._bound_pressures(m).copy_(a)

    def set_pressure_schedule(self, plant, model=None):
        """Per-scenario pressure schedules, each (B, T, 2) of [p_in, p_out] per
        control step: at step k the controller linearises with
        model[b][min(k, T - 1)] and the plant integrates [t_k, t_k + Ts] with
        plant[b][min(k, T - 1)] (initialize linearises with row 0).  model
        None leaves the model's pressures as they are: the plant's changes are
        then an unmeasured disturbance.  The step's row is copied on the device
        into the bound arrays (set_pressures).  plant None removes both
        schedules; the arrays keep their last rows."""
        if plant is None:
            if model is not None:
                raise ValueError("a model schedule needs a plant schedule")
            self._pp_sched = self._pm_sched = None
            return
        pp = self._pressure_array(plant, "plant", sched=True)
        pm = None if model is None else self._pressure_array(model, "model", sched=True)
        self._pp_sched, self._pm_sched = pp, pm
        self._bound_pressures(False)
        if pm is not None:
            self._bound_pressures(True)

    def _pressure_rows(self):
        """The schedules' rows of control step self.k into the bound arrays."""
        for sch, model in ((self._pp_sched, False), (self._pm_sched, True)):
            if sch is not None:
                self._bound_pressures(model).copy_(sch[:, min(self.k, sch.shape[1] - 1), :])

    def enable_scores(self, band=None, capture=None, capture_steps: int = 0):
        """Keep closed-loop performance indices of every QP slot on the device
        (Context.score_*, include/cmpc.h has the field table): each step then
        scores its instant in one small launch after the moves are
        accumulated and before the plant integrates, against y_ref[s][0] +
        dy_ref[q] (+ schedule[b][min(k, T - 1)][out_idx[s]] with a setpoint
        schedule in force: the setpoint of the measured instant).  band: (S,
        ny) settling bands per controlled output, None for 0.  capture: a list
        of scenarios whose trajectories [y | u_ctrl | x] of the first
        capture_steps instants are kept too (captured()).  initialize resets
        the record.  Arguments are refused before anything is allocated."""
        from . import score_capture_check, score_check
        n_out = self.sim.no
        oi = np.asarray(self.cfg.out_idx)[:, :self.cfg.ny]
        if band is not None:
            band = np.asarray(band, dtype=np.float64)
            if band.shape != (self.cfg.S, self.cfg.ny):
                raise ValueError(f"band must be (S = {self.cfg.S}, ny = {self.cfg.ny}), got {band.shape}")
            if not np.isfinite(band).all() or (band < 0).any():
                raise ValueError("band must be finite and >= 0")
        score_check(self.ctx.dims, n_out, oi, self.Ts, band)
        sel = []
        if capture is not None and len(capture):
            sel = np.asarray(capture)
            if sel.ndim != 1 or not np.issubdtype(sel.dtype, np.integer):
                raise ValueError(f"capture must be a list of scenario indices, got {sel!r}")
            if len(set(sel.tolist())) != sel.size or sel.min() < 0 or sel.max() >= self.B:
                raise ValueError(f"capture indices must be distinct and inside [0, B = {self.B})")
            if int(capture_steps) < 1:
                raise ValueError("capture_steps must be >= 1 with a capture list")
            score_capture_check(self.ctx.dims, sel, capture_steps)
        self.ctx.score_enable(n_out, oi, self.Ts, band)
        self.ctx.score_capture(sel, int(capture_steps) if len(sel) else 0)
        self._scores = True
        self._score_sched = None   # (B, S, T, ny) device: the targets per schedule row, made at first use
        self._score_target = self.torch.zeros(self.B * self.cfg.S, self.cfg.ny, dtype=self.torch.float64,
                                              device=self.dev)

    def set_noise(self, seed, sigma_y=None, sigma_u=None, rho_u=None, scenario0: int = 0):
        """Seeded measurement noise and input disturbances, a realisation per
        scenario (cmpc.noise_step, include/cmpc.h has the arithmetic), for
        Monte Carlo runs.  sigma_y: standard deviation per plant output;
        sigma_u, rho_u: stationary standard deviation and AR(1) coefficient per
        plant input (rho_u None: white); each (n,) or (B, n).  All three None
        turns noise off.  scenario0: the global index of this batch's scenario
        0, so a shard of a larger ensemble draws what its scenarios draw in the
        whole (the draws do not depend on B).  In force, step k
          - measures y_meas = y + sigma_y z (stream 0, step k) into a tensor of
            its own, kept as self.last_measurement: the observers see y_meas,
            while step() returns the true y and the scores score the true y;
          - sets the plant's input offset to the offset in force (segment
            switches followed) + w_k before the input is applied, w the AR(1)
            (or white) draw of stream 1: the controller's own offset is
            untouched, so this is an unmeasured disturbance.
        initialize zeroes w and uses the true y(x0).  Arguments are checked
        before anything is allocated.  With no noise set a step issues exactly
        the calls it issues without this feature."""
        from . import noise_check, noise_check_params
        if sigma_y is None and sigma_u is None and rho_u is None:
            if self._noise is not None and self._noise["su"] is not None:
                self.sim.set_offset(self._plant_offset)
            self._noise = None
            self.last_measurement = None
            return
        if rho_u is not None and sigma_u is None:
            raise ValueError("rho_u needs sigma_u")
        no, ni = self.sim.no, self.sim.ni
        noise_check(seed, 0, self.B, max(no, ni), 0, scenario0)
        sy, _ = noise_check_params(self.B, no, sigma_y, None)
        su, ru = noise_check_params(self.B, ni, sigma_u, rho_u)
        torch = self.torch
        t = lambda a: None if a is None else torch.from_numpy(a).to(self.dev)
        new = lambda n: torch.zeros(self.B, n, dtype=torch.float64, device=self.dev)
        self._noise = dict(seed=int(seed), scenario0=int(scenario0), sy=t(sy), su=t(su), ru=t(ru),
                           y_meas=new(no) if sy is not None else None,
                           w=new(ni) if ru is not None else None,
                           offset=new(ni) if su is not None else None)
        self.last_measurement = self._noise["y_meas"]

    def _measure(self, y):
        """The measurement the observers see: y, or y + sigma_y z of step self.k."""
        nz = self._noise
        if nz is None or nz["sy"] is None:
            return y
        from . import CMPC_NOISE_STREAM_MEASUREMENT, noise_step
        return noise_step(nz["seed"], self.k, nz["y_meas"], sigma=nz["sy"], base=y,
                          stream=CMPC_NOISE_STREAM_MEASUREMENT, scenario0=nz["scenario0"])

    def _disturb(self):
        """The plant's input offset of step self.k: the one in force + w_k."""
        nz = self._noise
        if nz is None or nz["su"] is None:
            return
        from . import CMPC_NOISE_STREAM_INPUT, noise_step
        noise_step(nz["seed"], self.k, nz["offset"], sigma=nz["su"], rho=nz["ru"], w=nz["w"],
                   base=self._plant_offset, stream=CMPC_NOISE_STREAM_INPUT, scenario0=nz["scenario0"])
        self.sim.set_offset(nz["offset"])

    def score_ensemble(self, thresholds=None) -> dict:
        """Mean, std, min, max, argmax and count over the B scenarios of every
        row of the score record, reduced on the device (Context.score_ensemble):
        {field: {stat: (S, rows)}}."""
        return self.ctx.score_ensemble(thresholds)

    def score_quantiles(self, levels) -> dict:
        """Exact quantiles over the B scenarios of every row of the score
        record, selected on the device (Context.score_quantiles): {field:
        {"lo", "hi", "arg", "value": (n_levels, S, rows)}}."""
        return self.ctx.score_quantiles(levels)

    def enable_envelope(self, steps: int, levels=(0.05, 0.5, 0.95), thresholds=None):
        """Record, at each of the first `steps` instants after initialize, how
        the ensemble is spread (Context.envelope_*, include/cmpc.h): per plant
        output and control input the mean, std, min, max, argmax and the count
        of scenarios above the channel's threshold (thresholds: n_outputs +
        nu_tot values or None), and the quantile bands of `levels`.  A step
        then adds a few small launches where the scores' launch sits, on the
        true y and u_ctrl; nothing is copied to the host before envelope().
        Independent of enable_scores.  Arguments are refused before anything
        is allocated."""
        self.ctx.envelope_enable(self.sim.no, int(steps), levels, thresholds)
        self._envelope = True

    def envelope(self):
        """(t (n,), {"y": {...}, "u": {...}}) for the n instants recorded so
        far: per group the statistics mean, std, min, max, argmax, count as (n,
        channels) arrays (argmax and count int64) and lo, hi, value as (n,
        n_levels, channels)."""
        from . import _abi, quantile_rank, quantile_value
        rows, n = self.ctx.envelope_download()
        rows = rows[:n]
        no, lv = self.sim.no, self.ctx._env[2]
        g = np.array([quantile_rank(self.B, q)[2] for q in lv]).reshape(1, -1, 1)
        out = {}
        for name, a in (("y", rows[:, :no]), ("u", rows[:, no:])):
            d = {}
            for k, stat in enumerate(_abi.ENSEMBLE_STATS):
                v = np.ascontiguousarray(a[:, :, k])
                d[stat] = v.astype(np.int64) if stat in ("argmax", "count") else v
            pairs = a[:, :, 6:].reshape(a.shape[0], a.shape[1], lv.size, 2)
            d["lo"] = np.ascontiguousarray(pairs[..., 0].transpose(0, 2, 1))
            d["hi"] = np.ascontiguousarray(pairs[..., 1].transpose(0, 2, 1))
            d["value"] = quantile_value(d["lo"], d["hi"], g) if lv.size else d["lo"].copy()
            out[name] = d
        return np.arange(n) * self.Ts, out

    def _score_step(self, y):
        """The instant's indices (enable_scores): one launch on the step's stream."""
        tgt = 0
        if self._sp_sched is not None:
            if self._score_sched is None:
                S, ny = self.cfg.S, self.cfg.ny
                base = np.stack([np.asarray(self.arrays.y_ref[s], dtype=np.float64).reshape(self.cfg.p, ny)[0]
                                 for s in range(S)])
                base = np.broadcast_to(base, (self.B, S, ny)).copy()   # y_ref[s][0]
                if self._dy_ref is not None:
                    base = base + self._dy_ref.reshape(self.B, S, ny)
                base = self.torch.from_numpy(base).to(self.dev)
                self._score_sched = (base[:, :, None, :] + self._sp_sched).contiguous()
            T = self._score_sched.shape[2]
            self._score_target.copy_(self._score_sched[:, :, min(self.k, T - 1), :].reshape(self._score_target.shape))
            tgt = self._score_target.data_ptr()
        self.ctx.score_step(y.data_ptr(), tgt, self.sim.status_ptr() or 0,
                            self.u_ctrl.data_ptr(), self.sim.state_ptr())

    def scores(self) -> dict:
        """The indices so far: {field: (B, S) or (B, S, rows) host array} for the
        fields of include/cmpc.h's table, plus settling_time = (last_out + 1)
        Ts per controlled output."""
        rec = self.ctx.score_download()
        S = self.cfg.S
        out = {}
        for name, sl in self.ctx.score_fields().items():
            a = rec[sl].reshape(sl.stop - sl.start, self.B, S).transpose(1, 2, 0)
            scalar = name in ("n", "j_track", "j_move", "n_fail", "nwsr_sum", "plant_fail_step")
            out[name] = np.ascontiguousarray(a[:, :, 0] if scalar else a)
        out["settling_time"] = (out["last_out"] + 1.0) * self.Ts
        return out

    def captured(self):
        """(t (n,), y (n, n_sel, n_outputs), u (n, n_sel, nu_tot), x (n, n_sel,
        ns)) of the scenarios given to enable_scores(capture=...), in that
        order, for the n instants recorded so far."""
        rows, n = self.ctx.score_download_capture()
        no, nu = self.sim.no, self.cfg.nu_tot
        rows = rows[:n]
        return (np.arange(n) * self.Ts, np.ascontiguousarray(rows[:, :, :no]),
                np.ascontiguousarray(rows[:, :, no:no + nu]), np.ascontiguousarray(rows[:, :, no + nu:]))

    def trim(self, max_iter: int = EQ_MAX_ITER, tol: float = EQ_TOL):
        """Start every scenario at its own plant equilibrium (call before
        initialize): the plant is reset to x0 and u_offset, the plant's
        pressures are put in force (row 0 of a pressure schedule, the
        per-scenario array, or the scalars), PlantSimulator.equilibrium solves
        f(x, u_offset, p) = 0 from x0 on the device, and x0 becomes the
        simulator's state: the equilibrium where the scenario's status is
        CMPC_EQ_OK, its given x0 elsewhere.  Returns (status, iters, resid),
        (B,) host arrays.  initialize then starts plant and observers there
        (y_old = y(x0)); self.sim.output() gives the outputs at rest, for
        setpoints relative to them."""
        self.sim.reset(self.x0, self.u_offset, self.Ts)
        self.k = 0
        self._pressure_rows()
        out = self.sim.equilibrium(max_iter, tol)
        self.x0 = self.torch.from_numpy(self.sim.download()[0]).to(self.dev)
        return out

    def trim_to_outputs(self, hold, targets, free=None, max_iter: int = EQ_MAX_ITER, tol_f: float = EQ_TOL,
                        tol_y: float = TARGET_TOL_Y) -> "TrimTargets":
        """Start every scenario at rest with given outputs (call before
        initialize): as trim, but the plant outputs `hold`
        are brought to `targets` ((nh,) or (B, nh), plant-output units) by
        solving for as many control inputs `free` as well (columns of B: 0 and
        2 the torques, 1 and 3 the recycle valves; None: the torques, in order,
        for up to two held outputs).  The plant is reset to x0 and u_offset,
        the plant's pressures are put in force, PlantSimulator.target solves on
        the device, and where the status is CMPC_EQ_OK x0 and the free columns
        of u_offset become the solution; each scenario's change of its free
        inputs is added to every pending set_segments offset, so a later
        disturbance step keeps the trimmed inputs.  A scenario with any other
        status keeps its given x0 and offset.  Returns a TrimTargets record:
        status, iters (B,), resid (B, 2) of (max|f|, max|y - t|), u_free
        (B, nh) the free inputs in force and du_free their change."""
        hold = [int(h) for h in np.asarray(hold).reshape(-1)]
        if free is None:
            if len(hold) > 2:
                raise ValueError("trim_to_outputs: give `free` for more than two held outputs")
            free = [0, 2][:len(hold)]
        free = [int(f) for f in np.asarray(free).reshape(-1)]
        self.sim.reset(self.x0, self.u_offset, self.Ts)
        self.k = 0
        self._pressure_rows()
        before = self.u_offset.cpu().numpy()
        status, iters, resid = self.sim.target(hold, free, targets, max_iter, tol_f, tol_y)
        cols = [REF_CONTROL_INDEX[f] for f in free]
        after = self.sim.download_inputs()[0]
        du = after[:, cols] - before[:, cols]
        self.x0 = self.torch.from_numpy(self.sim.download()[0]).to(self.dev)
        self.u_offset = self._plant_offset = self.torch.from_numpy(after).to(self.dev)
        if cols:
            for _, off in self._sched:
                off[:, cols] += self.torch.from_numpy(du).to(self.dev)
        return TrimTargets(status, iters, resid, np.ascontiguousarray(after[:, cols]), du)

    def modes(self, max_iter=None) -> "PlantModes":
        """The plant's open-loop modes at the loop's current states (after
        trim or initialize), under the plant pressures in force
        (PlantSimulator.modes, one launch; nothing of the loop is written):
        a PlantModes record of (B,) arrays abscissa, n_unstable, zeta_min,
        omega_d, omega_n, re_min (include/cmpc.h has the summary), the
        eigenvalues w (B, ns) complex and status (B,)."""
        w, sm, status, _ = self.sim.modes(max_iter)
        return PlantModes(sm[:, 0].copy(), sm[:, 1].copy(), sm[:, 2].copy(), sm[:, 3].copy(), sm[:, 4].copy(),
                          sm[:, 5].copy(), w, status)

    def gains(self, outputs, inputs=(0, 2)) -> "PlantGains":
        """The plant's steady-state gains at the loop's current states (after
        trim or trim_to_outputs), under the plant pressures in force
        (PlantSimulator.gains, one launch; nothing of the loop is written;
        DESIGN.md §3.22): a PlantGains record of G (B, ny, nu) = dy/du from
        the control inputs `inputs` to the plant outputs `outputs`, Gp
        (B, ny, 2) = dy/d(p_in, p_out), and for ny == nu the relative gain
        array rga and the pressure feed-forward k_ff (B, n, 2), with resid
        (B,) = max|f| and status (B,)."""
        return self.sim.gains(outputs, inputs)

    def freq_response(self, omega, outputs, inputs=(0, 2)) -> "FreqResponse":
        """The plant's frequency responses at the loop's current states (after
        trim or trim_to_outputs), under the plant pressures in force
        (PlantSimulator.freq_response, one launch; nothing of the loop is
        written): a FreqResponse record of G (B, nw, ny, nu)
        and Gp (B, nw, ny, 2) complex at the frequencies `omega` (rad/s), the
        peak magnitude of every entry over the list with the frequency it was
        found at, resid (B,) = max|f| and status (B,)."""
        return self.sim.freq_response(omega, outputs, inputs)

    def initialize(self, dx_init=None):
        """SimulationSystem(x0, u_offset) + NerveCenter::Initialize(x0, 0,
        u_offset, y(x0), dx_init): the observers' state, the records at x0,
        the first build and the cold InitializeQPProblem solves."""
        self.sim.reset(self.x0, self.u_offset, self.Ts)
        self.k = 0
        self._plant_offset = self.u_offset
        if self._noise is not None and self._noise["w"] is not None:
            self._noise["w"].zero_()
        self._pressure_rows()
        y0 = self.sim.output()
        dx = 0 if dx_init is None else self.torch.from_numpy(np.ascontiguousarray(dx_init)).to(self.dev)
        self.ctx.observer_init(self.x0.data_ptr(), self.u_offset.data_ptr(), y0.data_ptr(),
                               dx.data_ptr() if dx_init is not None else 0, Ts=self.Ts,
                               p_in=self.p_in, p_out=self.p_out)
        self.k = 0
        self._setpoint_window()
        self.ctx.build()
        self.ctx.init_warmstart()
        self.t_seg, self.seg_step = 0.0, 0   # integrate_const's start time and step count
        if self._scores:
            self.ctx.score_reset()
        if self._envelope:
            self.ctx.envelope_reset()

    def step(self, trace: bool = False, predict: bool = False, certify=None):
        """One sampling instant: returns (t, y) of the instant; the plant has
        advanced to the next one.  trace: the Jacobi iterations record their
        working-set changes (CMPC_TRACE); self.last_changes is then their
        total over the K iterations and all QP slots of this instant.
        predict: the instant's plans are evaluated against the model they were
        computed from (Context.predict, before the move is applied);
        self.last_prediction (B*S, p, ny) and self.last_cost (B*S, 2) are then
        host arrays.  certify: at the same point the instant's multipliers and
        KKT residuals are computed (Context.certify, the other controllers'
        plans gathered from the final ones: r_stat is the Jacobi gap) and
        self.last_certificate is their summary (Context.certify_summary) at
        tolerance `certify` (True: 1e-9).  The step itself computes the same
        with or without either."""
        from ._abi import check, iptr
        t = 0.0 + self.k * self.Ts   # the record's label (record count)
        # integrate_const's own time: start_time + step * dt of the current
        # Integrate call; its interval ends at time + dt
        t_int = self.t_seg + self.seg_step * self.Ts
        self._pressure_rows()
        y = self.sim.output()
        # GetNextInputWithTiming(y): linearisation input GetPlantInput(u_old_,
        # u_offset_) with the controller's own offset (fixed at Initialize; the
        # plant's may have stepped, see set_segments)
        self.sim.plant_input_offset(self.u_ctrl, self.u_offset, self.u_lin)
        self.ctx.observe_step(self.u_lin.data_ptr(), self._measure(y).data_ptr())
        self._setpoint_window()
        self.ctx.build()
        self.ctx.iterate(self.K, CMPC_TRACE if trace else 0)
        if trace:
            _, ntr = self.ctx.download_trace(self.K)
            self.last_changes = int(ntr.sum())
        if predict:
            self.ctx.predict()
            self.last_prediction, self.last_cost = self.ctx.download_prediction()
        if certify is not None and certify is not False:
            self.ctx.certify()
            self.last_certificate = self.ctx.certify_summary(1e-9 if certify is True else float(certify))
        self.ctx.observe_apply()
        check(self.ctx.lib.cmpc_accumulate_moves(self.ctx._h, iptr(self.io),
                                                 self.torch_ptr(self.u_ctrl)), "cmpc_accumulate_moves")
        if self._scores:
            self._score_step(y)
        if self._envelope:
            self.ctx.envelope_step(y.data_ptr(), self.u_ctrl.data_ptr())
        # SetInput(u) through the delay line, then the plant over [t, t + Ts];
        # at the end of a segment's Integrate call: SetOffset and a new call
        self._disturb()
        self.sim.set_input(self.u_ctrl)
        if self._sched and t_int >= self._sched[0][0] - 1e-9:
            self.t_seg = self._sched[0][0]
            self.seg_step = 0
            self._plant_offset = self._sched.pop(0)[1]
            self.sim.set_offset(self._plant_offset)
            self.sim.restart(self.Ts)
        else:
            self.sim.integrate(t_int, t_int + self.Ts, REF_EPS, REF_EPS)
            self.seg_step += 1
        self.k += 1
        return t, y

    def plant_failures(self):
        """Scenarios whose plant integration failed in any interval since
        initialize (the simulator's status is sticky: 1 step-size control, 2
        more than 500 steps in an interval, 3 non-finite), as (count, status
        per scenario).  The reference's odeint throws and ends the run; here a
        failed scenario stops where it failed and the rest carry on."""
        st = self.sim.download()[3]
        return int((st != 0).sum()), st

    @staticmethod
    def torch_ptr(t):
        import ctypes
        return ctypes.c_void_p(t.data_ptr())

    def run(self, n_steps: int, writer: DatWriter = None, scenario: int = 0):
        """n_steps sampling instants; writes scenario `scenario`'s records
        (x and y at the instant, the controller output u) when a writer is
        given.  Returns the wall time per step (s)."""
        torch = self.torch
        t_tot = 0.0
        for _ in range(n_steps):
            x_now = self.sim.download()[0][scenario] if writer else None
            torch.cuda.synchronize(self.dev)
            t0 = time.perf_counter()
            t, y = self.step()
            torch.cuda.synchronize(self.dev)
            el = time.perf_counter() - t0
            t_tot += el
            if writer:
                writer.record(t, x_now, self.u_ctrl[scenario].cpu().numpy(), y[scenario].cpu().numpy(),
                              int(el * 1e9))
        return t_tot / max(n_steps, 1)

    def close(self):
        self.ctx.close()
        self.sim.close()
