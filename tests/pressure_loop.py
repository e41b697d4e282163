"""tests/oracle_loop.py's closed loop restated with two pairs of boundary
pressures — TEST INFRASTRUCTURE ONLY (the checker; the product never imports
this).  The plant integrates with its own [p_in, p_out] (PlantSim.p_in /
p_out), the controller linearises with the model's (the p_in / p_out arguments
of or_lin_record and or_plant_linearize, the initial C included); either may
change between instants (set_pressures, or schedules of one pair per control
step, held past their ends).  With both pairs at (1, 1) every call is
OracleClosedLoop's, in its order.
"""
import numpy as np

import _oracle as O
from cmpc._abi import CmpcDims

CTRL = (0, 3, 4, 7)   # ControlInputIndex of both plants
TS = 0.05


class PressureClosedLoop:
    def __init__(self, cfg, arrays, M, K, plant_p=(1.0, 1.0), model_p=None, segments=None, x0=None,
                 plant_schedule=None, model_schedule=None):
        self.cfg, self.arr, self.M, self.K = cfg, arrays, M, K
        self.dims = CmpcDims.from_config(cfg, 1)
        self.L = O.layout(self.dims)
        self.pp = [float(plant_p[0]), float(plant_p[1])]
        self.pm = list(self.pp) if model_p is None else [float(model_p[0]), float(model_p[1])]
        # (T, 2) each; row min(k, T - 1) holds at control step k
        self.pp_sched = None if plant_schedule is None else np.asarray(plant_schedule, dtype=np.float64)
        self.pm_sched = None if model_schedule is None else np.asarray(model_schedule, dtype=np.float64)
        self.k = 0
        self._rows()
        xd, u_def = O.plant_default(cfg.plant)
        x0 = xd if x0 is None else np.asarray(x0, dtype=np.float64)
        segs = segments or [([0.0] * len(u_def), float("inf"))]
        offs = [u_def + np.asarray(d, dtype=np.float64) for d, _ in segs]
        self.u_off = offs[0].copy()                       # the controller's (NerveCenter::Initialize)
        self.sched = [(float(segs[i - 1][1]), offs[i]) for i in range(1, len(segs))]
        self.sim = O.PlantSim(cfg.plant, x0, offs[0], p_in=self.pp[0], p_out=self.pp[1])
        nq = cfg.S
        y0 = O.plant_output(cfg.plant, x0)
        self.xh = np.repeat(x0[None, :], nq, axis=0)
        self.dx = np.zeros((nq, self.L.ntot))
        self.yo = np.repeat(y0[None, :], nq, axis=0)
        self.C = [O.plant_linearize(cfg.plant, x0, self.u_off, self.pm[0], self.pm[1])[2] for _ in range(nq)]
        self.u_old = np.zeros((nq, cfg.nu_tot))
        self.du_old = np.zeros((nq, cfg.nV))
        self.ws = np.zeros(nq, np.uint32)
        self.u_ctrl = np.zeros(cfg.nu_tot)
        self.status = np.zeros(nq, np.int32)
        self.t_seg, self.seg_step = 0.0, 0   # integrate_const's start time and step count

    def set_pressures(self, plant=None, model=None):
        if plant is not None:
            self.pp = [float(plant[0]), float(plant[1])]
        if model is not None:
            self.pm = [float(model[0]), float(model[1])]

    def _rows(self):
        for sch, dst in ((self.pp_sched, self.pp), (self.pm_sched, self.pm)):
            if sch is not None:
                dst[:] = [float(v) for v in sch[min(self.k, len(sch) - 1)]]

    def step(self):
        cfg, S = self.cfg, self.cfg.S
        t = self.t_seg + self.seg_step * TS
        self._rows()
        y = O.plant_output(cfg.plant, self.sim.x)
        u_lin = self.u_off.copy()
        u_lin[list(CTRL)] += self.u_ctrl
        recs = np.zeros((S, self.L.rec_len))
        for q in range(S):
            O.observe_post(cfg.ns, cfg.ndist, self.C[q], self.M[q], y, self.yo[q], self.dx[q], self.xh[q])
            self.C[q] = O.plant_linearize(cfg.plant, self.xh[q], u_lin, self.pm[0], self.pm[1])[2]
            r = O.lin_record(cfg, self.dims, q, self.xh[q], u_lin, p_in=self.pm[0], p_out=self.pm[1])
            r[self.L.off_x:self.L.off_x + self.L.naug] = self.dx[q, cfg.ns:]
            r[self.L.off_y:self.L.off_y + cfg.ny] = y[cfg.out_idx[q]]
            recs[q] = r
        du, st, *_ = O.step(self.dims, self.arr, np.ascontiguousarray(recs), self.K, self.u_old,
                            self.du_old, self.ws, init=(self.k == 0))
        self.status = np.asarray(st).copy()
        for q in range(S):
            O.observe_prior(self.dims, recs[q], du[q, :cfg.nu], self.u_old[q], self.dx[q])
            own = cfg.input_order[q][:cfg.nu]
            self.u_ctrl[own] += du[q, :cfg.nu]
        self.sim.set_input(self.u_ctrl)
        if self.sched and t >= self.sched[0][0] - 1e-9:
            self.t_seg, self.seg_step = self.sched[0][0], 0
            self.sim.u_offset[:] = self.sched.pop(0)[1]
            self.sim.dt[0] = TS
        else:
            self.sim.p_in, self.sim.p_out = self.pp
            self.sim.integrate(t, t + TS)
            self.seg_step += 1
        self.k += 1
        return y
