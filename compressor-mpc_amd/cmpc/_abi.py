"""ctypes view of the C ABI declared in include/cmpc.h.

The product library is compressor-mpc_amd/cmpc/libcmpc.so (HIP, gfx950),
built in-tree by compressor-mpc_amd/csrc/Makefile.  There is no CPU fallback:
if the library is missing or cannot be loaded, load_library() raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CMPC_LIBRARY") or os.path.join(_HERE, "libcmpc.so")

CMPC_MAX_INPUTS = 8
CMPC_MAX_NV = 8
CMPC_MAX_NS = 15
CMPC_NWSR_MAX = 10

CMPC_QP_OK = 0
CMPC_QP_MAX_NWSR = 1
CMPC_QP_INFEASIBLE = 2
CMPC_QP_NOT_PD = 3
CMPC_QP_NONFINITE = 4

CMPC_APPLY_MOVE = 1
CMPC_TRACE = 2

CMPC_KERNEL_BUILD = 0
CMPC_KERNEL_ITERATE = 1
CMPC_KERNEL_PRODUCE = 2
CMPC_KERNEL_OBSERVE_POST = 3
CMPC_KERNEL_OBSERVE_PRIOR = 4
CMPC_KERNEL_STEP = 5
CMPC_KERNEL_COUNT = 6

CMPC_BUILD_AUTO = 0
CMPC_BUILD_WAVE = 1
CMPC_BUILD_ROWS = 2
CMPC_BUILD_SPLIT = 3
CMPC_PAIRING_AUTO = 0
CMPC_PAIRING_OFF = 1
CMPC_PAIRING_ON = 2
CMPC_SOLVE_AUTO = 0
CMPC_SOLVE_LANE = 1
CMPC_SOLVE_ROWS = 2
CMPC_STEP_AUTO = 0
CMPC_STEP_SPLIT = 1
CMPC_STEP_FUSED = 2

CMPC_PLAN_DU_OTHER = 0x100
CMPC_PLAN_REF_PROFILE = 0x200
CMPC_PLAN_OK = 0
CMPC_PLAN_NO_ROWS_BUILD = 1
CMPC_PLAN_NO_BUILD = 2
CMPC_PLAN_NO_ROWS_SOLVE = 3
CMPC_PLAN_NO_SOLVE = 4
CMPC_PLAN_NO_FUSED_STEP = 5
CMPC_PLAN_PROFILE_NEEDS_SPLIT = 6
CMPC_PLAN_SCENARIO_WEIGHTS = 0x400
CMPC_PLAN_WEIGHTS_NEED_WAVE = 7
CMPC_PLAN_WEIGHTS_NEED_SPLIT = 8
CMPC_PLAN_NO_WEIGHTS_BUILD = 9


class CmpcDims(ctypes.Structure):
    _fields_ = [("ns", ctypes.c_int32), ("ndist", ctypes.c_int32),
                ("nu_tot", ctypes.c_int32), ("nu", ctypes.c_int32),
                ("ny", ctypes.c_int32), ("p", ctypes.c_int32), ("m", ctypes.c_int32),
                ("delay", ctypes.c_int32 * CMPC_MAX_INPUTS),
                ("S", ctypes.c_int32), ("B", ctypes.c_int32)]

    @classmethod
    def from_config(cls, cfg, B: int) -> "CmpcDims":
        d = cls()
        d.ns, d.ndist, d.nu_tot, d.nu, d.ny = cfg.ns, cfg.ndist, cfg.nu_tot, cfg.nu, cfg.ny
        d.p, d.m, d.S, d.B = cfg.p, cfg.m, cfg.S, B
        for i, v in enumerate(cfg.delays):
            d.delay[i] = v
        return d


class CmpcLayout(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in
                ("nd", "n_delay_states", "naug", "nobs", "ntot", "nV", "nuo", "nVo",
                 "off_A", "off_B", "off_C", "off_f", "off_x", "off_y", "rec_len")]


class CmpcPlan(ctypes.Structure):
    """cmpc_plan_t: what cmpc_build, the solve calls, cmpc_step and
    cmpc_control_step launch for a batch (include/cmpc.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in
                ("build_kernel", "build_error", "solve_kernel", "solve_error",
                 "step_fused", "step_build_kernel", "step_solve_kernel", "step_error",
                 "control_fused", "control_build_kernel", "control_solve_kernel",
                 "control_grid", "control_polled")]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


def dptr(a: np.ndarray):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def iptr(a: np.ndarray):
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def uptr(a: np.ndarray):
    assert a.dtype == np.uint32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def bptr(a: np.ndarray):
    assert a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


# Every symbol include/cmpc.h declares (checked by tests/test_abi.py).
EXPORTS = (
    "cmpc_layout_of", "cmpc_create", "cmpc_destroy", "cmpc_set_stream",
    "cmpc_last_error", "cmpc_get_layout", "cmpc_set_weights", "cmpc_set_constraints",
    "cmpc_set_reference", "cmpc_set_state", "cmpc_get_state", "cmpc_upload_lin",
    "cmpc_lin_device", "cmpc_build", "cmpc_set_build_variant", "cmpc_rows_lds_model", "cmpc_last_build_kernel", "cmpc_set_solve_variant", "cmpc_last_solve_kernel", "cmpc_set_step_variant", "cmpc_last_step_fused", "cmpc_plan", "cmpc_plan_error_string", "cmpc_init_warmstart", "cmpc_iterate", "cmpc_step",
    "cmpc_synchronize", "cmpc_download", "cmpc_download_qp", "cmpc_download_trace",
    "cmpc_enable_timing", "cmpc_kernel_time", "cmpc_set_timing_stride", "cmpc_plant_dims", "cmpc_plant_default",
    "cmpc_plant_output", "cmpc_plant_lin_record", "cmpc_qp_solve_batch", "cmpc_qp_solve_batch_map", "cmpc_bind_lin",
    "cmpc_bind_state",
    "cmpc_set_scenario_reference", "cmpc_bind_scenario_reference", "cmpc_set_scenario_constraints",
    "cmpc_bind_scenario_constraints", "cmpc_get_scenario_reference", "cmpc_get_scenario_constraints",
    "cmpc_produce_lin", "cmpc_download_lin", "cmpc_coupled_iterate", "cmpc_coupled_validate",
    "cmpc_get_input", "cmpc_get_input_host", "cmpc_update_u", "cmpc_update_u_host",
    "cmpc_set_observer", "cmpc_observer_len", "cmpc_observer_init", "cmpc_observe_step",
    "cmpc_observe_apply", "cmpc_get_observer_state", "cmpc_set_observer_state",
    "cmpc_observer_init_host", "cmpc_observe_step_host", "cmpc_control_step", "cmpc_control_step_host", "cmpc_control_step_download",
    "cmpc_sim_create", "cmpc_sim_destroy", "cmpc_sim_set_stream", "cmpc_sim_reset",
    "cmpc_sim_set_input", "cmpc_sim_set_offset", "cmpc_sim_restart", "cmpc_sim_plant_input_offset",
    "cmpc_sim_plant_input", "cmpc_sim_integrate", "cmpc_sim_output",
    "cmpc_sim_synchronize", "cmpc_sim_state", "cmpc_sim_input", "cmpc_sim_step_size",
    "cmpc_sim_status", "cmpc_accumulate_moves", "cmpc_sim_download", "cmpc_sim_reset_host",
    "cmpc_sim_set_input_host", "cmpc_sim_set_offset_host", "cmpc_sim_output_host",
    "cmpc_predict", "cmpc_predict_host", "cmpc_prediction_device", "cmpc_prediction_cost_device",
    "cmpc_download_prediction", "cmpc_predict_available",
    "cmpc_set_scenario_reference_profile", "cmpc_bind_scenario_reference_profile",
    "cmpc_get_scenario_reference_profile", "cmpc_reference_profile_available",
    "cmpc_set_build_pairing", "cmpc_build_pairing_available", "cmpc_build_pairing_reason",
    "cmpc_last_build_shared_scenarios",
    "cmpc_set_scenario_weights", "cmpc_bind_scenario_weights", "cmpc_get_scenario_weights",
    "cmpc_scenario_weights_available", "cmpc_weight_factor",
    "cmpc_set_scenario_pressures", "cmpc_bind_scenario_pressures", "cmpc_get_scenario_pressures",
    "cmpc_sim_set_pressures", "cmpc_sim_set_pressures_host", "cmpc_sim_bind_pressures",
    "cmpc_sim_get_pressures", "cmpc_check_pressures",
    "cmpc_score_len", "cmpc_score_field", "cmpc_score_check", "cmpc_score_capture_check",
    "cmpc_score_enable", "cmpc_score_bind", "cmpc_score_capture", "cmpc_score_bind_capture",
    "cmpc_score_reset", "cmpc_score_step", "cmpc_score_download", "cmpc_score_download_capture",
    "cmpc_score_disable",
    "cmpc_certify_len", "cmpc_certify_field", "cmpc_certify_available", "cmpc_certify", "cmpc_certify_host",
    "cmpc_certify_device", "cmpc_certify_download", "cmpc_certify_summary",
    "cmpc_score_ensemble",
    "cmpc_noise_check", "cmpc_noise_check_params", "cmpc_noise_uniforms_host", "cmpc_noise_step_host",
    "cmpc_noise_uniforms", "cmpc_noise_step",
    "cmpc_quantile_check", "cmpc_quantile_rank", "cmpc_quantiles_host", "cmpc_score_quantiles",
    "cmpc_envelope_check", "cmpc_envelope_len", "cmpc_envelope_enable", "cmpc_envelope_step",
    "cmpc_envelope_reset", "cmpc_envelope_bind", "cmpc_envelope_download", "cmpc_envelope_disable",
    "cmpc_plant_derivative", "cmpc_plant_equilibrium_host", "cmpc_sim_equilibrium",
    "cmpc_sim_equilibrium_download", "cmpc_sim_equilibrium_status", "cmpc_sim_equilibrium_iters",
    "cmpc_sim_equilibrium_resid",
    "cmpc_target_check", "cmpc_plant_target_host", "cmpc_sim_target", "cmpc_sim_target_host",
    "cmpc_sim_target_download", "cmpc_sim_target_status", "cmpc_sim_target_iters", "cmpc_sim_target_resid",
    "cmpc_sim_delay_len", "cmpc_sim_download_inputs",
    "cmpc_gain_check", "cmpc_plant_gains_host", "cmpc_sim_gains", "cmpc_sim_gains_download",
    "cmpc_sim_gains_record", "cmpc_sim_gains_status",
    "cmpc_freq_check", "cmpc_plant_freq_host", "cmpc_freq_host", "cmpc_sim_freq", "cmpc_sim_freq_download",
    "cmpc_sim_freq_record", "cmpc_sim_freq_summary", "cmpc_sim_freq_status",
    "cmpc_eig_host", "cmpc_eig_device", "cmpc_modes_summary_host", "cmpc_plant_modes_host", "cmpc_sim_modes",
    "cmpc_sim_modes_download", "cmpc_sim_modes_wr", "cmpc_sim_modes_wi", "cmpc_sim_modes_summary",
    "cmpc_sim_modes_status", "cmpc_sim_modes_iters",
)

# per-scenario statuses of the equilibrium solve (include/cmpc.h)
CMPC_EQ_OK = 0
CMPC_EQ_NO_CONVERGENCE = 1
CMPC_EQ_NONFINITE = 2
CMPC_EQ_SINGULAR = 3
CMPC_EQ_SKIPPED = 4
CMPC_EQ_DEADZONE = 5   # the target solve only: a free recycle valve below 2e-2
CMPC_GAIN_SINGULAR_G = 6   # the gains only: G of a square selection has no inverse
CMPC_GAIN_LEN = 49         # doubles per gains record: G 4x4, Gp 4x2, RGA 4x4, K_ff 4x2, r_f
CMPC_EQ_MAX_ITER = 64
CMPC_FREQ_MAX_NW = 64      # frequencies per frequency-response call, at most
CMPC_FREQ_MAX_N = 12       # the matrix-level host call's largest n
CMPC_FREQ_LEN = 48         # doubles per scenario and frequency: G 4x4 and Gp 4x2 as (re, im) pairs
CMPC_FREQ_NSUM = 49        # doubles per scenario: 24 peaks of re^2 + im^2, their 24 indices, r_f

# per-matrix statuses of the eigenvalue solver and the summary of the plant
# modes (include/cmpc.h)
CMPC_EIG_OK = 0
CMPC_EIG_NO_CONVERGENCE = 1
CMPC_EIG_NONFINITE = 2
CMPC_EIG_SKIPPED = 3
CMPC_EIG_MAX_N = 12
CMPC_EIG_MAX_ITER = 360
CMPC_MODES_NSUM = 6
MODES_SUMMARY = ("abscissa", "n_unstable", "zeta_min", "omega_d", "omega_n", "re_min")

# the fields of a slot's score record, in the record's order (cmpc_score_field
# gives each one's rows; include/cmpc.h has the table)
SCORE_FIELDS = ("n", "ise", "iae", "peak", "last_out", "j_track", "j_move", "tv", "sat_bound", "sat_rate",
                "n_fail", "nwsr_sum", "plant_fail_step")

# the fields of a slot's certificate record, in the record's order
# (cmpc_certify_field gives each one's rows; include/cmpc.h has the table)
CERTIFY_FIELDS = ("lam", "r_stat", "r_prim", "r_dual", "r_comp", "obj", "scale", "n_active", "status", "rank_def")


class CmpcCertifySummary(ctypes.Structure):
    """cmpc_certify_summary_t (include/cmpc.h)."""
    _fields_ = ([(n, ctypes.c_double) for n in ("r_stat", "r_prim", "r_dual", "r_comp")] +
                [(n, ctypes.c_int32) for n in ("slot_stat", "slot_prim", "slot_dual", "slot_comp",
                                               "n_above", "n_not_ok")])

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


# the statistics of Context.score_ensemble, in the order cmpc_score_ensemble writes them
ENSEMBLE_STATS = ("mean", "std", "min", "max", "argmax", "count")

# levels per quantile call (include/cmpc.h)
CMPC_QUANTILE_MAX_LEVELS = 8

# the noise streams the closed loop uses (include/cmpc.h); the others are the caller's
CMPC_NOISE_STREAM_MEASUREMENT = 0
CMPC_NOISE_STREAM_INPUT = 1


class CmpcNoiseKey(ctypes.Structure):
    """cmpc_noise_key (include/cmpc.h)."""
    _fields_ = [("seed", ctypes.c_uint64), ("stream", ctypes.c_uint32), ("scenario0", ctypes.c_uint32)]


_lib = None


def load_library(path: str = LIB_PATH):
    """Load libcmpc.so.  Raises (never falls back) if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: build it with `make -C compressor-mpc_amd/csrc` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    # One HIP runtime per process: torch ships its own libamdhip64 (same
    # soname).  Loaded first, it also serves this library; loaded after ours,
    # torch brings in a second runtime that finds no GPU ("No HIP GPUs are
    # available") and whose device pointers and streams ours cannot use.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(path)
    P = ctypes.POINTER
    c_void = ctypes.c_void_p
    i32, u32, dbl = ctypes.c_int32, ctypes.c_uint32, ctypes.c_double
    sig = {
        "cmpc_layout_of": ([P(CmpcDims), P(CmpcLayout)], ctypes.c_int),
        "cmpc_create": ([P(c_void), P(CmpcDims), ctypes.c_int], ctypes.c_int),
        "cmpc_destroy": ([c_void], ctypes.c_int),
        "cmpc_set_stream": ([c_void, c_void], ctypes.c_int),
        "cmpc_last_error": ([], ctypes.c_char_p),
        "cmpc_get_layout": ([c_void, P(CmpcLayout)], ctypes.c_int),
        "cmpc_set_weights": ([c_void, ctypes.c_int, P(dbl), P(dbl)], ctypes.c_int),
        "cmpc_set_constraints": ([c_void, ctypes.c_int, P(dbl), P(dbl), P(dbl), P(dbl)],
                                 ctypes.c_int),
        "cmpc_set_reference": ([c_void, ctypes.c_int, P(dbl)], ctypes.c_int),
        "cmpc_set_state": ([c_void, P(dbl), P(dbl), P(u32)], ctypes.c_int),
        "cmpc_get_state": ([c_void, P(dbl), P(dbl), P(u32)], ctypes.c_int),
        "cmpc_upload_lin": ([c_void, P(dbl)], ctypes.c_int),
        "cmpc_lin_device": ([c_void], c_void),
        "cmpc_download_lin": ([c_void, P(dbl)], ctypes.c_int),
        "cmpc_bind_lin": ([c_void, c_void], ctypes.c_int),
        "cmpc_bind_state": ([c_void, c_void, c_void, c_void], ctypes.c_int),
        "cmpc_set_scenario_reference": ([c_void, P(dbl)], ctypes.c_int),
        "cmpc_bind_scenario_reference": ([c_void, c_void], ctypes.c_int),
        "cmpc_set_scenario_constraints": ([c_void, P(dbl), P(dbl), P(dbl), P(dbl)], ctypes.c_int),
        "cmpc_bind_scenario_constraints": ([c_void, c_void], ctypes.c_int),
        "cmpc_get_scenario_reference": ([c_void, P(dbl)], ctypes.c_int),
        "cmpc_get_scenario_constraints": ([c_void, P(dbl), P(dbl), P(dbl), P(dbl)], ctypes.c_int),
        "cmpc_build": ([c_void], ctypes.c_int),
        "cmpc_set_build_variant": ([c_void, ctypes.c_int], ctypes.c_int),
        "cmpc_last_build_kernel": ([c_void], ctypes.c_int),
        "cmpc_set_solve_variant": ([c_void, ctypes.c_int], ctypes.c_int),
        "cmpc_last_solve_kernel": ([c_void], ctypes.c_int),
        "cmpc_set_step_variant": ([c_void, ctypes.c_int], ctypes.c_int),
        "cmpc_last_step_fused": ([c_void], ctypes.c_int),
        "cmpc_plan": ([P(CmpcDims), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, u32,
                       P(CmpcPlan)], ctypes.c_int),
        "cmpc_plan_error_string": ([ctypes.c_int], ctypes.c_char_p),
        "cmpc_rows_lds_model": ([P(CmpcDims), P(dbl), P(dbl), P(ctypes.c_int32)], ctypes.c_int),
        "cmpc_init_warmstart": ([c_void], ctypes.c_int),
        "cmpc_iterate": ([c_void, ctypes.c_int, u32], ctypes.c_int),
        "cmpc_step": ([c_void, ctypes.c_int, u32], ctypes.c_int),
        "cmpc_synchronize": ([c_void], ctypes.c_int),
        "cmpc_download": ([c_void, P(dbl), P(i32), P(i32)], ctypes.c_int),
        "cmpc_download_qp": ([c_void, P(dbl), P(dbl), P(dbl)], ctypes.c_int),
        "cmpc_download_trace": ([c_void, P(ctypes.c_uint8), P(i32)], ctypes.c_int),
        "cmpc_enable_timing": ([c_void, ctypes.c_int], ctypes.c_int),
        "cmpc_set_timing_stride": ([c_void, ctypes.c_int], ctypes.c_int),
        "cmpc_kernel_time": ([c_void, ctypes.c_int, P(dbl), P(ctypes.c_int64)], ctypes.c_int),
        "cmpc_plant_dims": ([ctypes.c_int, P(ctypes.c_int), P(ctypes.c_int), P(ctypes.c_int),
                             P(ctypes.c_int)], ctypes.c_int),
        "cmpc_plant_default": ([ctypes.c_int, P(dbl), P(dbl)], ctypes.c_int),
        "cmpc_plant_output": ([ctypes.c_int, P(dbl), P(dbl)], ctypes.c_int),
        "cmpc_plant_lin_record": ([ctypes.c_int, dbl, dbl, dbl, P(dbl), P(dbl), P(i32), P(i32),
                                   P(CmpcDims), P(dbl)], ctypes.c_int),
        "cmpc_produce_lin": ([c_void, ctypes.c_int, dbl, dbl, dbl, P(i32), P(i32), c_void, c_void,
                              c_void, c_void], ctypes.c_int),
        "cmpc_set_observer": ([c_void, ctypes.c_int, ctypes.c_int, P(dbl)], ctypes.c_int),
        "cmpc_observer_len": ([c_void], ctypes.c_int),
        "cmpc_observer_init": ([c_void, ctypes.c_int, dbl, dbl, dbl, P(i32), P(i32), c_void, c_void,
                                c_void, c_void], ctypes.c_int),
        "cmpc_observe_step": ([c_void, c_void, c_void], ctypes.c_int),
        "cmpc_observe_apply": ([c_void], ctypes.c_int),
        "cmpc_control_step": ([c_void, c_void, c_void, ctypes.c_int], ctypes.c_int),
        "cmpc_control_step_host": ([c_void, P(dbl), P(dbl), ctypes.c_int], ctypes.c_int),
        "cmpc_control_step_download": ([c_void, P(dbl), P(dbl), ctypes.c_int, P(dbl), P(i32), P(i32)],
                                       ctypes.c_int),
        "cmpc_observer_init_host": ([c_void, ctypes.c_int, dbl, dbl, dbl, P(i32), P(i32), P(dbl),
                                     P(dbl), P(dbl), P(dbl)], ctypes.c_int),
        "cmpc_observe_step_host": ([c_void, P(dbl), P(dbl)], ctypes.c_int),
        "cmpc_sim_create": ([P(c_void), ctypes.c_int, ctypes.c_int, ctypes.c_int, dbl, dbl,
                             ctypes.c_int, P(i32), P(i32)], ctypes.c_int),
        "cmpc_sim_destroy": ([c_void], ctypes.c_int),
        "cmpc_sim_set_stream": ([c_void, c_void], ctypes.c_int),
        "cmpc_sim_reset": ([c_void, c_void, c_void, dbl], ctypes.c_int),
        "cmpc_sim_set_input": ([c_void, c_void], ctypes.c_int),
        "cmpc_sim_set_offset": ([c_void, c_void], ctypes.c_int),
        "cmpc_sim_restart": ([c_void, ctypes.c_double], ctypes.c_int),
        "cmpc_sim_plant_input_offset": ([c_void, c_void, c_void, c_void], ctypes.c_int),
        "cmpc_sim_plant_input": ([c_void, c_void, c_void], ctypes.c_int),
        "cmpc_sim_integrate": ([c_void, dbl, dbl, dbl, dbl], ctypes.c_int),
        "cmpc_sim_output": ([c_void, c_void], ctypes.c_int),
        "cmpc_sim_synchronize": ([c_void], ctypes.c_int),
        "cmpc_sim_download": ([c_void, P(dbl), P(dbl), P(dbl), P(i32)], ctypes.c_int),
        "cmpc_sim_reset_host": ([c_void, P(dbl), P(dbl), dbl], ctypes.c_int),
        "cmpc_sim_set_input_host": ([c_void, P(dbl)], ctypes.c_int),
        "cmpc_sim_set_offset_host": ([c_void, P(dbl)], ctypes.c_int),
        "cmpc_sim_output_host": ([c_void, P(dbl)], ctypes.c_int),
        "cmpc_sim_state": ([c_void], c_void),
        "cmpc_sim_input": ([c_void], c_void),
        "cmpc_sim_step_size": ([c_void], c_void),
        "cmpc_sim_status": ([c_void], c_void),
        "cmpc_accumulate_moves": ([c_void, P(i32), c_void], ctypes.c_int),
        "cmpc_get_observer_state": ([c_void, P(dbl)], ctypes.c_int),
        "cmpc_set_observer_state": ([c_void, P(dbl)], ctypes.c_int),
        "cmpc_get_input": ([c_void, c_void, u32], ctypes.c_int),
        "cmpc_get_input_host": ([c_void, P(dbl), u32], ctypes.c_int),
        "cmpc_update_u": ([c_void, c_void], ctypes.c_int),
        "cmpc_update_u_host": ([c_void, P(dbl)], ctypes.c_int),
        "cmpc_coupled_validate": ([P(CmpcDims), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t,
                                   ctypes.c_size_t], ctypes.c_int),
        "cmpc_coupled_iterate": ([c_void, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void, ctypes.c_size_t,
                                  c_void, ctypes.c_size_t, c_void, u32], ctypes.c_int),
        "cmpc_predict": ([c_void, c_void, c_void, u32], ctypes.c_int),
        "cmpc_predict_host": ([c_void, P(dbl), P(dbl), u32], ctypes.c_int),
        "cmpc_prediction_device": ([c_void], c_void),
        "cmpc_prediction_cost_device": ([c_void], c_void),
        "cmpc_download_prediction": ([c_void, P(dbl), P(dbl)], ctypes.c_int),
        "cmpc_predict_available": ([P(CmpcDims)], ctypes.c_int),
        "cmpc_set_scenario_reference_profile": ([c_void, P(dbl)], ctypes.c_int),
        "cmpc_bind_scenario_reference_profile": ([c_void, c_void], ctypes.c_int),
        "cmpc_get_scenario_reference_profile": ([c_void, P(dbl)], ctypes.c_int),
        "cmpc_reference_profile_available": ([P(CmpcDims)], ctypes.c_int),
        "cmpc_set_build_pairing": ([c_void, ctypes.c_int], ctypes.c_int),
        "cmpc_build_pairing_available": ([P(CmpcDims), P(dbl), P(dbl)], ctypes.c_int),
        "cmpc_build_pairing_reason": ([P(CmpcDims), P(dbl), P(dbl)], ctypes.c_char_p),
        "cmpc_last_build_shared_scenarios": ([c_void], ctypes.c_int),
        "cmpc_set_scenario_weights": ([c_void, P(dbl), P(dbl)], ctypes.c_int),
        "cmpc_bind_scenario_weights": ([c_void, c_void], ctypes.c_int),
        "cmpc_get_scenario_weights": ([c_void, P(dbl), P(dbl)], ctypes.c_int),
        "cmpc_scenario_weights_available": ([P(CmpcDims)], ctypes.c_int),
        "cmpc_weight_factor": ([ctypes.c_int, P(dbl), P(dbl)], ctypes.c_int),
        "cmpc_set_scenario_pressures": ([c_void, P(dbl)], ctypes.c_int),
        "cmpc_bind_scenario_pressures": ([c_void, c_void], ctypes.c_int),
        "cmpc_get_scenario_pressures": ([c_void, P(dbl)], ctypes.c_int),
        "cmpc_sim_set_pressures": ([c_void, c_void], ctypes.c_int),
        "cmpc_sim_set_pressures_host": ([c_void, P(dbl)], ctypes.c_int),
        "cmpc_sim_bind_pressures": ([c_void, c_void], ctypes.c_int),
        "cmpc_sim_get_pressures": ([c_void, P(dbl)], ctypes.c_int),
        "cmpc_check_pressures": ([ctypes.c_int, P(dbl)], ctypes.c_int),
        "cmpc_score_len": ([P(CmpcDims)], ctypes.c_int),
        "cmpc_score_field": ([P(CmpcDims), ctypes.c_char_p, P(ctypes.c_int), P(ctypes.c_int)], ctypes.c_int),
        "cmpc_score_check": ([P(CmpcDims), ctypes.c_int, P(i32), dbl, P(dbl)], ctypes.c_int),
        "cmpc_score_capture_check": ([P(CmpcDims), ctypes.c_int, P(i32), ctypes.c_int], ctypes.c_int),
        "cmpc_score_enable": ([c_void, ctypes.c_int, P(i32), dbl, P(dbl)], ctypes.c_int),
        "cmpc_score_bind": ([c_void, c_void], ctypes.c_int),
        "cmpc_score_capture": ([c_void, ctypes.c_int, P(i32), ctypes.c_int], ctypes.c_int),
        "cmpc_score_bind_capture": ([c_void, c_void], ctypes.c_int),
        "cmpc_score_reset": ([c_void], ctypes.c_int),
        "cmpc_score_step": ([c_void, c_void, c_void, c_void, c_void, c_void], ctypes.c_int),
        "cmpc_score_download": ([c_void, P(dbl)], ctypes.c_int),
        "cmpc_score_download_capture": ([c_void, P(dbl), P(i32)], ctypes.c_int),
        "cmpc_score_disable": ([c_void], ctypes.c_int),
        "cmpc_certify_len": ([P(CmpcDims)], ctypes.c_int),
        "cmpc_certify_field": ([P(CmpcDims), ctypes.c_char_p, P(ctypes.c_int), P(ctypes.c_int)], ctypes.c_int),
        "cmpc_certify_available": ([P(CmpcDims)], ctypes.c_int),
        "cmpc_certify": ([c_void, c_void, u32], ctypes.c_int),
        "cmpc_certify_host": ([c_void, P(dbl), u32], ctypes.c_int),
        "cmpc_certify_device": ([c_void], c_void),
        "cmpc_certify_download": ([c_void, P(dbl)], ctypes.c_int),
        "cmpc_certify_summary": ([c_void, dbl, P(CmpcCertifySummary)], ctypes.c_int),
        "cmpc_score_ensemble": ([c_void, P(dbl), P(dbl)], ctypes.c_int),
        "cmpc_noise_check": ([P(CmpcNoiseKey), ctypes.c_uint64, ctypes.c_int, ctypes.c_int], ctypes.c_int),
        "cmpc_noise_check_params": ([ctypes.c_int, ctypes.c_int, P(dbl), P(dbl)], ctypes.c_int),
        "cmpc_noise_uniforms_host": ([P(CmpcNoiseKey), ctypes.c_uint64, ctypes.c_int, ctypes.c_int, P(dbl)],
                                     ctypes.c_int),
        "cmpc_noise_step_host": ([P(CmpcNoiseKey), ctypes.c_uint64, ctypes.c_int, ctypes.c_int, P(dbl), P(dbl),
                                  P(dbl), P(dbl), P(dbl)], ctypes.c_int),
        "cmpc_noise_uniforms": ([ctypes.c_int, c_void, P(CmpcNoiseKey), ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                 c_void], ctypes.c_int),
        "cmpc_noise_step": ([ctypes.c_int, c_void, P(CmpcNoiseKey), ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                             c_void, c_void, c_void, c_void, c_void], ctypes.c_int),
        "cmpc_quantile_check": ([ctypes.c_int, ctypes.c_int, P(dbl)], ctypes.c_int),
        "cmpc_quantile_rank": ([ctypes.c_int, dbl, P(i32), P(i32), P(dbl)], ctypes.c_int),
        "cmpc_quantile_value": ([dbl, dbl, dbl], dbl),   # (returns a double: not in EXPORTS' pattern)
        "cmpc_quantiles_host": ([P(dbl), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, P(dbl), P(dbl)],
                                ctypes.c_int),
        "cmpc_score_quantiles": ([c_void, ctypes.c_int, P(dbl), P(dbl)], ctypes.c_int),
        "cmpc_envelope_check": ([P(CmpcDims), ctypes.c_int, ctypes.c_int, ctypes.c_int, P(dbl), P(dbl)],
                                ctypes.c_int),
        "cmpc_envelope_len": ([P(CmpcDims), ctypes.c_int, ctypes.c_int], ctypes.c_int),
        "cmpc_envelope_enable": ([c_void, ctypes.c_int, ctypes.c_int, ctypes.c_int, P(dbl), P(dbl)], ctypes.c_int),
        "cmpc_envelope_step": ([c_void, c_void, c_void], ctypes.c_int),
        "cmpc_envelope_reset": ([c_void], ctypes.c_int),
        "cmpc_envelope_bind": ([c_void, c_void], ctypes.c_int),
        "cmpc_envelope_download": ([c_void, P(dbl), P(i32)], ctypes.c_int),
        "cmpc_envelope_disable": ([c_void], ctypes.c_int),
        "cmpc_plant_derivative": ([ctypes.c_int, dbl, dbl, P(dbl), P(dbl), P(dbl)], ctypes.c_int),
        "cmpc_plant_equilibrium_host": ([ctypes.c_int, ctypes.c_int, P(dbl), P(dbl), P(dbl), ctypes.c_int, dbl,
                                         P(i32), P(i32), P(dbl)], ctypes.c_int),
        "cmpc_sim_equilibrium": ([c_void, ctypes.c_int, dbl], ctypes.c_int),
        "cmpc_sim_equilibrium_download": ([c_void, P(i32), P(i32), P(dbl)], ctypes.c_int),
        "cmpc_sim_equilibrium_status": ([c_void], c_void),
        "cmpc_sim_equilibrium_iters": ([c_void], c_void),
        "cmpc_sim_equilibrium_resid": ([c_void], c_void),
        "cmpc_target_check": ([ctypes.c_int, ctypes.c_int, P(i32), P(i32), ctypes.c_int, dbl, dbl], ctypes.c_int),
        "cmpc_plant_target_host": ([ctypes.c_int, ctypes.c_int, P(dbl), ctypes.c_int, P(i32), P(i32), P(dbl), P(dbl),
                                    P(dbl), ctypes.c_int, dbl, dbl, P(i32), P(i32), P(dbl)], ctypes.c_int),
        "cmpc_sim_target": ([c_void, ctypes.c_int, P(i32), P(i32), c_void, ctypes.c_int, dbl, dbl], ctypes.c_int),
        "cmpc_sim_target_host": ([c_void, ctypes.c_int, P(i32), P(i32), P(dbl), ctypes.c_int, dbl, dbl],
                                 ctypes.c_int),
        "cmpc_sim_target_download": ([c_void, P(i32), P(i32), P(dbl)], ctypes.c_int),
        "cmpc_sim_target_status": ([c_void], c_void),
        "cmpc_sim_target_iters": ([c_void], c_void),
        "cmpc_sim_target_resid": ([c_void], c_void),
        "cmpc_sim_delay_len": ([c_void], ctypes.c_int),
        "cmpc_sim_download_inputs": ([c_void, P(dbl), P(dbl)], ctypes.c_int),
        "cmpc_gain_check": ([ctypes.c_int, ctypes.c_int, P(i32), ctypes.c_int, P(i32)], ctypes.c_int),
        "cmpc_plant_gains_host": ([ctypes.c_int, ctypes.c_int, P(dbl), P(dbl), P(dbl), ctypes.c_int, P(i32),
                                   ctypes.c_int, P(i32), P(dbl), P(i32)], ctypes.c_int),
        "cmpc_sim_gains": ([c_void, ctypes.c_int, P(i32), ctypes.c_int, P(i32)], ctypes.c_int),
        "cmpc_sim_gains_download": ([c_void, P(dbl), P(i32)], ctypes.c_int),
        "cmpc_sim_gains_record": ([c_void], c_void),
        "cmpc_sim_gains_status": ([c_void], c_void),
        "cmpc_freq_check": ([ctypes.c_int, ctypes.c_int, P(i32), ctypes.c_int, P(i32), ctypes.c_int, P(dbl)],
                            ctypes.c_int),
        "cmpc_plant_freq_host": ([ctypes.c_int, ctypes.c_int, P(dbl), P(dbl), P(dbl), ctypes.c_int, P(i32),
                                  ctypes.c_int, P(i32), ctypes.c_int, P(dbl), P(dbl), P(dbl), P(i32)], ctypes.c_int),
        "cmpc_freq_host": ([ctypes.c_int, ctypes.c_int, P(dbl), P(dbl), P(dbl), P(dbl), ctypes.c_int, ctypes.c_int,
                            ctypes.c_int, P(dbl), P(dbl), P(dbl), P(i32)], ctypes.c_int),
        "cmpc_sim_freq": ([c_void, ctypes.c_int, P(i32), ctypes.c_int, P(i32), ctypes.c_int, P(dbl)], ctypes.c_int),
        "cmpc_sim_freq_download": ([c_void, P(dbl), P(dbl), P(i32)], ctypes.c_int),
        "cmpc_sim_freq_record": ([c_void], c_void),
        "cmpc_sim_freq_summary": ([c_void], c_void),
        "cmpc_sim_freq_status": ([c_void], c_void),
        "cmpc_eig_host": ([ctypes.c_int, ctypes.c_int, P(dbl), ctypes.c_int, P(dbl), P(dbl), P(i32), P(i32)],
                          ctypes.c_int),
        "cmpc_eig_device": ([ctypes.c_int, ctypes.c_int, c_void, ctypes.c_int, c_void, c_void, c_void, c_void,
                             c_void], ctypes.c_int),
        "cmpc_modes_summary_host": ([ctypes.c_int, ctypes.c_int, P(dbl), P(dbl), P(i32), P(dbl)], ctypes.c_int),
        "cmpc_plant_modes_host": ([ctypes.c_int, ctypes.c_int, P(dbl), P(dbl), P(dbl), ctypes.c_int, P(dbl), P(dbl),
                                   P(dbl), P(i32), P(i32)], ctypes.c_int),
        "cmpc_sim_modes": ([c_void, ctypes.c_int], ctypes.c_int),
        "cmpc_sim_modes_download": ([c_void, P(dbl), P(dbl), P(dbl), P(i32), P(i32)], ctypes.c_int),
        "cmpc_sim_modes_wr": ([c_void], c_void),
        "cmpc_sim_modes_wi": ([c_void], c_void),
        "cmpc_sim_modes_summary": ([c_void], c_void),
        "cmpc_sim_modes_status": ([c_void], c_void),
        "cmpc_sim_modes_iters": ([c_void], c_void),
        "cmpc_qp_solve_batch": ([ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, P(dbl),
                                 P(dbl), P(dbl), P(dbl), P(dbl), P(dbl), P(u32), ctypes.c_int,
                                 P(dbl), P(i32), P(i32), P(u32), P(ctypes.c_uint8), P(i32)],
                                ctypes.c_int),
        "cmpc_qp_solve_batch_map": ([ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     P(dbl), P(dbl), P(dbl), P(dbl), P(dbl), P(dbl), P(dbl), P(dbl), P(u32),
                                     ctypes.c_int, P(dbl), P(i32), P(i32), P(u32), P(ctypes.c_uint8), P(i32)],
                                    ctypes.c_int),
    }
    for name, (argtypes, restype) in sig.items():
        fn = getattr(lib, name, None)
        if fn is None:  # (an older library build: A/B timing runs; tests/test_abi.py checks the exports)
            continue
        fn.argtypes = argtypes
        fn.restype = restype
    _lib = lib
    return lib


def check(rc: int, what: str = "cmpc call"):
    if rc != 0:
        msg = load_library().cmpc_last_error()
        raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
