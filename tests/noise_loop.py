"""cmpc.driver.ClosedLoop's step with noise in force, written out by hand —
TEST INFRASTRUCTURE ONLY (the checker; the product never imports this).

The loop drives Context and PlantSimulator itself, in ClosedLoop's order, and
forms what set_noise adds on the host: each step it downloads the device's
plain normals z (cmpc.noise_step with nothing but out) of stream 0 and stream
1, builds y_meas = y + sigma_y z and offset = u_offset + w_k (the AR(1) or
white update) in float64 numpy in the header's operation order
(noise_ref.step_model), and uploads them.  No segments, no pressures.
"""
import ctypes

import numpy as np

import cmpc
import noise_ref as R
from cmpc._abi import check, iptr
from cmpc.sim import REF_CONTROL_INDEX, REF_DELAYS, REF_EPS, REF_TS, PlantSimulator


class NoiseLoop:
    def __init__(self, cfg, arrays, M, x0, u_offset, K, seed, sigma_y=None, sigma_u=None, rho_u=None, scenario0=0,
                 y_offset=None, limits=None, schedule=None):
        import torch
        self.torch = torch
        self.dev = dev = torch.device("cuda", 0)
        self.cfg, self.K, self.Ts = cfg, K, REF_TS
        B, S = x0.shape[0], cfg.S
        self.B = B
        self.sim = PlantSimulator(cfg.plant, B, 0, 1.0, 1.0, REF_DELAYS, REF_CONTROL_INDEX)
        self.ctx = cmpc.Context(cfg, B, device=0)
        self.ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        self.ctx.configure(arrays)
        self.ctx.set_state(np.zeros((B * S, cfg.nu_tot)), np.zeros((B * S, cfg.nV)), np.zeros(B * S, np.uint32))
        for s in range(S):
            self.ctx.set_observer(s, M[s])
        if y_offset is not None:
            self.ctx.set_scenario_reference(cmpc.scenario_reference_offsets(cfg, np.asarray(y_offset)))
        if limits is not None:
            self.ctx.set_scenario_constraints(*cmpc.scenario_limits(cfg, *limits))
        self.t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
        self.x0, self.u_offset = self.t(x0), self.t(u_offset)
        self.u_offset_host = np.ascontiguousarray(u_offset, dtype=np.float64)
        self.u_ctrl = torch.zeros(B, cfg.nu_tot, dtype=torch.float64, device=dev)
        self.u_lin = torch.zeros_like(self.u_offset)
        self.io = np.ascontiguousarray(cfg.input_order, dtype=np.int32)
        self.seed, self.scenario0 = seed, scenario0
        no, ni = self.sim.no, self.sim.ni
        bc = lambda a, n: None if a is None else np.array(np.broadcast_to(np.asarray(a, dtype=np.float64), (B, n)))
        self.sigma_y, self.sigma_u, self.rho_u = bc(sigma_y, no), bc(sigma_u, ni), bc(rho_u, ni)
        self.z_y = torch.zeros(B, no, dtype=torch.float64, device=dev)
        self.z_u = torch.zeros(B, ni, dtype=torch.float64, device=dev)
        self.y_meas = torch.zeros(B, no, dtype=torch.float64, device=dev)
        self.offset = torch.zeros(B, ni, dtype=torch.float64, device=dev)
        self.schedule = None if schedule is None else np.asarray(schedule, dtype=np.float64)
        if self.schedule is not None:
            self.window = torch.zeros(B * S, cfg.p, cfg.ny, dtype=torch.float64, device=dev)
            self.ctx.bind_scenario_reference_profile(self.window.data_ptr())
        self.k = 0

    def _window(self):
        """ClosedLoop.set_setpoint_schedule's window of control step self.k."""
        if self.schedule is None:
            return
        cfg, T = self.cfg, self.schedule.shape[1]
        idx = np.minimum(np.arange(cfg.p) + self.k + 1, T - 1)
        oi = np.asarray(cfg.out_idx, dtype=np.int64)[:, :cfg.ny]                 # (S, ny)
        win = self.schedule[:, idx][:, :, oi]                                    # (B, p, S, ny)
        self.window.copy_(self.t(win.transpose(0, 2, 1, 3).reshape(self.window.shape)))

    def initialize(self):
        self.sim.reset(self.x0, self.u_offset, self.Ts)
        self.k = 0
        y0 = self.sim.output()
        self.ctx.observer_init(self.x0.data_ptr(), self.u_offset.data_ptr(), y0.data_ptr(), 0, Ts=self.Ts,
                               p_in=1.0, p_out=1.0)
        self._window()
        self.ctx.build()
        self.ctx.init_warmstart()
        self.w = np.zeros_like(self.u_offset_host)

    def step(self):
        """Returns (y, y_meas, u_ctrl, u_lin) of the instant as host arrays."""
        t = self.k * self.Ts
        y_dev = self.sim.output()
        y = y_dev.cpu().numpy().copy()
        meas = y_dev
        y_meas = y
        if self.sigma_y is not None:
            z = cmpc.noise_step(self.seed, self.k, self.z_y, stream=0, scenario0=self.scenario0).cpu().numpy()
            y_meas = R.step_model(z, self.sigma_y, None, None, y)[1]
            self.y_meas.copy_(self.t(y_meas))
            meas = self.y_meas
        self.sim.plant_input_offset(self.u_ctrl, self.u_offset, self.u_lin)
        self.ctx.observe_step(self.u_lin.data_ptr(), meas.data_ptr())
        self._window()
        self.ctx.build()
        self.ctx.iterate(self.K, 0)
        self.ctx.observe_apply()
        check(self.ctx.lib.cmpc_accumulate_moves(self.ctx._h, iptr(self.io), ctypes.c_void_p(self.u_ctrl.data_ptr())),
              "cmpc_accumulate_moves")
        if self.sigma_u is not None:
            z = cmpc.noise_step(self.seed, self.k, self.z_u, stream=1, scenario0=self.scenario0).cpu().numpy()
            self.w, off = R.step_model(z, self.sigma_u, self.rho_u, self.w, self.u_offset_host)
            self.offset.copy_(self.t(off))
            self.sim.set_offset(self.offset)
        self.sim.set_input(self.u_ctrl)
        self.sim.integrate(t, t + self.Ts, REF_EPS, REF_EPS)
        self.k += 1
        return y, np.array(y_meas), self.u_ctrl.cpu().numpy(), self.u_lin.cpu().numpy()

    def close(self):
        self.ctx.close()
        self.sim.close()
