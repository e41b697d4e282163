"""cmpc — MI355X-native condensed-QP hot path of katie-jones/compressor-mpc.

Python host view of the C ABI (include/cmpc.h).  Every compute call goes to
libcmpc.so (HIP kernels for gfx950); there is no CPU fallback.

    ctx = Context(cfg, B)                 # NerveCenter/DistributedController ctors
    ctx.configure(arrays)                 # SetWeights / SetOutputReference / constraints
    ctx.set_state(u_old, du_old, ws)      # Initialize
    ctx.upload_lin(lin)                   # AugmentedLinearizedSystem::Update results
    ctx.init_warmstart()                  # InitializeQPProblem
    ctx.step(K)                           # GetNextInputWithTiming (build + K Jacobi iterations)
    du, status, nwsr = ctx.download()
"""
import ctypes

import numpy as np

from . import _abi
from ._abi import (CMPC_BUILD_AUTO, CMPC_BUILD_ROWS, CMPC_BUILD_SPLIT, CMPC_BUILD_WAVE, CMPC_PAIRING_AUTO,
                   CMPC_PAIRING_OFF, CMPC_PAIRING_ON, CMPC_SOLVE_AUTO, CMPC_SOLVE_LANE,
                   CMPC_SOLVE_ROWS, CMPC_STEP_AUTO, CMPC_STEP_FUSED, CMPC_STEP_SPLIT, CMPC_KERNEL_STEP,
                   CMPC_APPLY_MOVE, CMPC_KERNEL_BUILD, CMPC_KERNEL_ITERATE,
                   CMPC_KERNEL_PRODUCE, CMPC_KERNEL_OBSERVE_POST, CMPC_KERNEL_OBSERVE_PRIOR, CMPC_QP_INFEASIBLE,
                   CMPC_QP_MAX_NWSR, CMPC_QP_NOT_PD, CMPC_QP_NONFINITE, CMPC_QP_OK, CMPC_TRACE, CmpcDims,
                   CmpcLayout, CmpcNoiseKey, CmpcPlan, CMPC_NOISE_STREAM_INPUT, CMPC_NOISE_STREAM_MEASUREMENT,
                   CMPC_PLAN_DU_OTHER, CMPC_PLAN_REF_PROFILE, CMPC_PLAN_SCENARIO_WEIGHTS, bptr,
                   check, dptr, iptr, load_library, uptr)
from .configs import ControllerConfig, SetupFile, reference_config, reference_observer_gain, reference_setup
from .problem import ControllerArrays, controller_arrays, plant_input_from_plans
from ._abi import (CMPC_EQ_OK, CMPC_EQ_NO_CONVERGENCE, CMPC_EQ_NONFINITE, CMPC_EQ_SINGULAR,  # noqa: F401
                   CMPC_EQ_SKIPPED, CMPC_EQ_DEADZONE, CMPC_GAIN_SINGULAR_G, CMPC_GAIN_LEN,
                   CMPC_FREQ_MAX_NW, CMPC_FREQ_MAX_N, CMPC_FREQ_LEN, CMPC_FREQ_NSUM)
from ._abi import (CMPC_EIG_OK, CMPC_EIG_NO_CONVERGENCE, CMPC_EIG_NONFINITE, CMPC_EIG_SKIPPED,  # noqa: F401
                   CMPC_EIG_MAX_ITER, CMPC_MODES_NSUM)
from .sim import plant_derivative, plant_equilibrium, plant_target  # noqa: F401
from .sim import PlantGains, plant_gains  # noqa: F401
from .sim import FreqResponse, freq_response, plant_freq_response  # noqa: F401
from .sim import eig_batch, eig_batch_device, modes_summary, plant_modes  # noqa: F401

__all__ = ["Context", "ControllerConfig", "SetupFile", "reference_config", "reference_setup",
           "reference_observer_gain", "controller_arrays",
           "plant_input_from_plans", "plant_lin_record", "plant_default", "plant_output",
           "scenario_reference_offsets", "scenario_reference_profiles", "scenario_limits",
           "layout_of", "plan", "predict_available", "reference_profile_available", "CMPC_PLAN_REF_PROFILE", "plan_error_string", "rows_lds_model", "qp_solve_batch", "CMPC_APPLY_MOVE", "CMPC_TRACE", "CMPC_QP_OK",
           "CMPC_QP_MAX_NWSR", "CMPC_QP_INFEASIBLE", "CMPC_QP_NOT_PD",
           "CMPC_QP_NONFINITE", "build_pairing_available", "build_pairing_reason", "CMPC_PAIRING_AUTO",
           "CMPC_PAIRING_OFF", "CMPC_PAIRING_ON", "scenario_weights_available", "weight_factor",
           "CMPC_PLAN_SCENARIO_WEIGHTS", "score_len", "score_fields", "score_check", "score_capture_check",
           "certify_len", "certify_fields", "certify_available", "score_ensemble_unpack",
           "noise_key", "noise_check", "noise_check_params", "noise_uniforms_host", "noise_step_host",
           "noise_uniforms", "noise_step", "noise_uniforms_ptr", "noise_step_ptr",
           "CMPC_NOISE_STREAM_MEASUREMENT", "CMPC_NOISE_STREAM_INPUT",
           "quantile_check", "quantile_rank", "quantile_value", "quantiles_host", "envelope_check", "envelope_len",
           "plant_derivative", "plant_equilibrium", "CMPC_EQ_OK", "CMPC_EQ_NO_CONVERGENCE", "CMPC_EQ_NONFINITE",
           "CMPC_EQ_SINGULAR", "CMPC_EQ_SKIPPED", "CMPC_EQ_DEADZONE", "plant_target",
           "CMPC_GAIN_SINGULAR_G", "CMPC_GAIN_LEN", "PlantGains", "plant_gains",
           "CMPC_FREQ_MAX_NW", "CMPC_FREQ_MAX_N", "CMPC_FREQ_LEN", "CMPC_FREQ_NSUM", "FreqResponse", "freq_response",
           "plant_freq_response",
           "eig_batch", "eig_batch_device", "modes_summary", "plant_modes", "CMPC_EIG_OK", "CMPC_EIG_NO_CONVERGENCE",
           "CMPC_EIG_NONFINITE", "CMPC_EIG_SKIPPED", "CMPC_EIG_MAX_ITER", "CMPC_MODES_NSUM"]


def layout_of(dims: CmpcDims) -> CmpcLayout:
    L = CmpcLayout()
    check(load_library().cmpc_layout_of(ctypes.byref(dims), ctypes.byref(L)), "cmpc_layout_of")
    return L


def plan(dims: CmpcDims, cus: int, build: int = CMPC_BUILD_AUTO, solve: int = CMPC_SOLVE_AUTO,
         step: int = CMPC_STEP_AUTO, K: int = 1, flags: int = 0, scenario_weights: bool = False) -> CmpcPlan:
    """Which kernels a batch of dims.B scenarios gets on a device of `cus`
    compute units under the three variants, for calls with K iterations
    and `flags` (CMPC_TRACE, CMPC_PLAN_DU_OTHER, CMPC_PLAN_REF_PROFILE): cmpc_plan, the library's own
    selection (csrc/dispatch.cpp), answered without a device.
    scenario_weights: per-slot weights are in force (CMPC_PLAN_SCENARIO_WEIGHTS)."""
    out = CmpcPlan()
    if scenario_weights:
        flags = int(flags) | CMPC_PLAN_SCENARIO_WEIGHTS
    check(load_library().cmpc_plan(ctypes.byref(dims), int(cus), int(build), int(solve), int(step), int(K),
                                   int(flags), ctypes.byref(out)), "cmpc_plan")
    return out


def scenario_weights_available(dims: CmpcDims) -> bool:
    """Whether Context.set/bind_scenario_weights has a build kernel instance
    for dims whose LDS fits with the per-wave weight tables (host only)."""
    return bool(load_library().cmpc_scenario_weights_available(ctypes.byref(dims)))


def weight_factor(ywt) -> np.ndarray:
    """L_W' (upper triangular, ny x ny) with ywt = L_W L_W': the library's own
    factorisation of an output weight (cmpc_weight_factor), for callers that
    pack the blocks of Context.bind_scenario_weights themselves.  Raises for a
    weight that is not symmetric positive semi-definite."""
    W = np.ascontiguousarray(ywt, dtype=np.float64)
    if W.ndim != 2 or W.shape[0] != W.shape[1]:
        raise ValueError(f"ywt must be square, got {W.shape}")
    out = np.zeros_like(W)
    check(load_library().cmpc_weight_factor(W.shape[0], dptr(W), dptr(out)), "cmpc_weight_factor")
    return out


def score_len(dims: CmpcDims) -> int:
    """Rows of a QP slot's score record for dims (cmpc_score_len, host only)."""
    n = load_library().cmpc_score_len(ctypes.byref(dims))
    check(min(n, 0), "cmpc_score_len")
    return n


def score_fields(dims: CmpcDims) -> dict:
    """{field name: slice of the record's rows} for dims, from the library's
    own table (cmpc_score_field, host only).  The record is field-major: a
    download reshaped to (score_len, B*S) is indexed by these slices."""
    lib = load_library()
    out = {}
    for name in _abi.SCORE_FIELDS:
        off, cnt = ctypes.c_int(), ctypes.c_int()
        check(lib.cmpc_score_field(ctypes.byref(dims), name.encode(), ctypes.byref(off), ctypes.byref(cnt)),
              "cmpc_score_field")
        out[name] = slice(off.value, off.value + cnt.value)
    return out


def score_check(dims: CmpcDims, n_outputs: int, out_idx, Ts: float, band=None):
    """The argument check of Context.score_enable without a context (host
    only); raises with the library's message."""
    oi = np.ascontiguousarray(out_idx, dtype=np.int32).reshape(-1)
    if oi.size != dims.S * dims.ny:
        raise ValueError(f"out_idx must hold S*ny = {dims.S * dims.ny} values, got {oi.size}")
    bd = None
    if band is not None:
        bd = np.ascontiguousarray(band, dtype=np.float64).reshape(-1)
        if bd.size != dims.S * dims.ny:
            raise ValueError(f"band must hold S*ny = {dims.S * dims.ny} values, got {bd.size}")
    check(load_library().cmpc_score_check(ctypes.byref(dims), int(n_outputs), iptr(oi), float(Ts),
                                          dptr(bd) if bd is not None else None), "cmpc_score_check")
    return oi, bd


def score_capture_check(dims: CmpcDims, scenarios, t_cap: int) -> np.ndarray:
    """The argument check of Context.score_capture without a context (host
    only); raises with the library's message."""
    sel = np.ascontiguousarray(scenarios, dtype=np.int32).reshape(-1)
    check(load_library().cmpc_score_capture_check(ctypes.byref(dims), int(sel.size), iptr(sel), int(t_cap)),
          "cmpc_score_capture_check")
    return sel


def score_ensemble_unpack(dims: CmpcDims, flat) -> dict:
    """cmpc_score_ensemble's len*S*6 doubles as {field: {stat: (S, rows) array}}
    (host only): the layout is [row f][sub-controller s][stat], the stats in
    _abi.ENSEMBLE_STATS' order; argmax and count come back as int64."""
    n_stat = len(_abi.ENSEMBLE_STATS)
    a = np.asarray(flat, dtype=np.float64)
    if a.size != score_len(dims) * dims.S * n_stat:
        raise ValueError(f"expected score_len * S * {n_stat} = {score_len(dims) * dims.S * n_stat} values, got {a.size}")
    a = a.reshape(score_len(dims), dims.S, n_stat)
    out = {}
    for name, sl in score_fields(dims).items():
        out[name] = {}
        for k, stat in enumerate(_abi.ENSEMBLE_STATS):
            v = np.ascontiguousarray(a[sl, :, k].T)
            out[name][stat] = v.astype(np.int64) if stat in ("argmax", "count") else v
    return out


def quantile_check(B: int, levels) -> np.ndarray:
    """The argument check of the quantile entry points (cmpc_quantile_check,
    host only); raises with the library's message.  Returns the levels."""
    lv = np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
    check(load_library().cmpc_quantile_check(int(B), int(lv.size), dptr(lv) if lv.size else None),
          "cmpc_quantile_check")
    return lv


def quantile_rank(B: int, level: float):
    """(k_lo, k_hi, g) of a level among B values (cmpc_quantile_rank, host only):
    h = level (B - 1), k_lo = floor(h), g = h - k_lo, k_hi = k_lo + (g > 0)."""
    lo, hi, g = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
    check(load_library().cmpc_quantile_rank(int(B), float(level), ctypes.byref(lo), ctypes.byref(hi),
                                            ctypes.byref(g)), "cmpc_quantile_rank")
    return lo.value, hi.value, g.value


def quantile_value(x_lo, x_hi, g):
    """The value between two order statistics (cmpc_quantile_value, host only):
    x_lo where they are equal, else x_lo + d g for g < 0.5 and x_hi - d (1 - g)
    otherwise, d = x_hi - x_lo.  Arrays broadcast; scalars give a float."""
    fn = load_library().cmpc_quantile_value
    a, b, t = np.broadcast_arrays(np.asarray(x_lo, dtype=np.float64), np.asarray(x_hi, dtype=np.float64),
                                  np.asarray(g, dtype=np.float64))
    out = np.array([fn(float(p), float(q), float(r)) for p, q, r in zip(a.ravel(), b.ravel(), t.ravel())],
                   dtype=np.float64).reshape(a.shape)
    return out if out.ndim else float(out)


def quantiles_host(x, levels) -> dict:
    """Exact order statistics over axis 1 of a (len, B, S) host array (or (B, C):
    len = 1, S = C) by the library's own selection on host memory
    (cmpc_quantiles_host, no device): {"lo", "hi", "arg", "value"}, each
    (n_levels, len, S); arg (int64) is the lowest b holding lo."""
    a = np.ascontiguousarray(x, dtype=np.float64)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError(f"x must be (len, B, S) or (B, C), got {a.shape}")
    n, B, S = a.shape
    lv = quantile_check(B, levels)
    if n < 1 or S < 1:
        raise ValueError(f"x must not be empty, got {a.shape}")
    out = np.zeros((n, S, lv.size, 3))
    check(load_library().cmpc_quantiles_host(dptr(a), n, B, S, int(lv.size), dptr(lv), dptr(out)),
          "cmpc_quantiles_host")
    return _quantiles_unpack(out, B, lv)


def _quantiles_unpack(out, B: int, lv) -> dict:
    """(rows, S, n_levels, 3) of [x_lo, x_hi, arg] -> the dict of (n_levels, rows, S)."""
    lo, hi, arg = (np.ascontiguousarray(out[..., k].transpose(2, 0, 1)) for k in range(3))
    g = np.array([quantile_rank(B, q)[2] for q in lv])
    return {"lo": lo, "hi": hi, "arg": arg.astype(np.int64), "value": quantile_value(lo, hi, g[:, None, None])}


def envelope_check(dims: CmpcDims, n_outputs: int, t_cap: int, levels=(), thresholds=None):
    """The argument check of Context.envelope_enable without a context
    (cmpc_envelope_check, host only); raises with the library's message.
    Returns (levels, thresholds) as arrays (thresholds None stays None)."""
    lv = np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
    th = None
    if thresholds is not None:
        th = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        if th.size != int(n_outputs) + dims.nu_tot:
            raise ValueError(f"thresholds must hold n_outputs + nu_tot = {int(n_outputs) + dims.nu_tot} values, "
                             f"got {th.size}")
    check(load_library().cmpc_envelope_check(ctypes.byref(dims), int(n_outputs), int(t_cap), int(lv.size),
                                             dptr(lv) if lv.size else None, dptr(th) if th is not None else None),
          "cmpc_envelope_check")
    return lv, th


def envelope_len(dims: CmpcDims, n_outputs: int, n_levels: int) -> int:
    """Doubles per step row of the envelope, (n_outputs + nu_tot) (6 + 2
    n_levels) (cmpc_envelope_len, host only)."""
    n = load_library().cmpc_envelope_len(ctypes.byref(dims), int(n_outputs), int(n_levels))
    check(min(n, 0), "cmpc_envelope_len")
    return n


def noise_key(seed: int, stream: int = 0, scenario0: int = 0) -> CmpcNoiseKey:
    """cmpc_noise_key of (seed, stream, first global scenario of the batch)."""
    seed, stream, scenario0 = int(seed), int(stream), int(scenario0)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must be inside [0, 2^64), got {seed}")
    if not 0 <= stream < 2 ** 32 or not 0 <= scenario0 < 2 ** 32:
        raise ValueError(f"stream and scenario0 must be inside [0, 2^32), got {stream} and {scenario0}")
    return CmpcNoiseKey(seed, stream, scenario0)


def _noise_step_arg(step: int) -> int:
    step = int(step)
    if not 0 <= step < 2 ** 64:
        raise ValueError(f"step must be inside [0, 2^64), got {step}")
    return step


def noise_check(seed: int, step: int, B: int, n: int, stream: int = 0, scenario0: int = 0):
    """The argument check of every noise entry point (cmpc_noise_check, host
    only); raises with the library's message."""
    key = noise_key(seed, stream, scenario0)
    check(load_library().cmpc_noise_check(ctypes.byref(key), _noise_step_arg(step), int(B), int(n)),
          "cmpc_noise_check")
    return key


def _noise_array(a, B: int, n: int, what: str):
    """(n,) or (B, n) to a contiguous (B, n) float64 array; None stays None."""
    if a is None:
        return None
    a = np.asarray(a, dtype=np.float64)
    if a.shape not in ((n,), (B, n)):
        raise ValueError(f"{what} must be (n = {n},) or (B = {B}, n), got {a.shape}")
    return np.array(np.broadcast_to(a, (B, n)), order="C")


def noise_check_params(B: int, n: int, sigma=None, rho=None):
    """sigma finite and >= 0, rho inside [-1, 1] (cmpc_noise_check_params, host
    only), each (n,) or (B, n) or None; returns them as (B, n) arrays."""
    sg, rh = _noise_array(sigma, B, n, "sigma"), _noise_array(rho, B, n, "rho")
    check(load_library().cmpc_noise_check_params(int(B), int(n), dptr(sg) if sg is not None else None,
                                                 dptr(rh) if rh is not None else None), "cmpc_noise_check_params")
    return sg, rh


def noise_uniforms_host(seed: int, step: int, B: int, n: int, stream: int = 0, scenario0: int = 0) -> np.ndarray:
    """(B, ceil(n/2), 2): the uniforms [u1, u2] of every Box-Muller pair
    (cmpc_noise_uniforms_host, no device)."""
    key = noise_check(seed, step, B, n, stream, scenario0)
    u = np.zeros((B, (n + 1) // 2, 2))
    check(load_library().cmpc_noise_uniforms_host(ctypes.byref(key), _noise_step_arg(step), int(B), int(n), dptr(u)),
          "cmpc_noise_uniforms_host")
    return u


def noise_step_host(seed: int, step: int, B: int, n: int, sigma=None, rho=None, w=None, base=None,
                    stream: int = 0, scenario0: int = 0) -> np.ndarray:
    """(B, n): base + the step's disturbance on host arrays (cmpc_noise_step_host,
    no device; include/cmpc.h has the arithmetic).  sigma, rho, base: (n,) or
    (B, n) or None; w: the (B, n) contiguous float64 AR(1) state, updated in
    place (needed with rho)."""
    key = noise_check(seed, step, B, n, stream, scenario0)
    sg, rh, bs = (_noise_array(a, B, n, what) for a, what in ((sigma, "sigma"), (rho, "rho"), (base, "base")))
    if w is not None and (not isinstance(w, np.ndarray) or w.shape != (B, n) or w.dtype != np.float64
                          or not w.flags["C_CONTIGUOUS"]):
        raise ValueError(f"w must be a contiguous float64 array (B = {B}, n = {n})")
    out = np.zeros((B, n))
    opt = lambda a: dptr(a) if a is not None else None
    check(load_library().cmpc_noise_step_host(ctypes.byref(key), _noise_step_arg(step), int(B), int(n), opt(sg),
                                              opt(rh), opt(w), opt(bs), dptr(out)), "cmpc_noise_step_host")
    return out


def noise_uniforms_ptr(device: int, stream_ptr: int, key: CmpcNoiseKey, step: int, B: int, n: int, u_ptr: int):
    """cmpc_noise_uniforms on raw device addresses (asynchronous on the stream)."""
    check(load_library().cmpc_noise_uniforms(int(device), ctypes.c_void_p(stream_ptr or None), ctypes.byref(key),
                                             _noise_step_arg(step), int(B), int(n), ctypes.c_void_p(u_ptr or None)),
          "cmpc_noise_uniforms")


def noise_step_ptr(device: int, stream_ptr: int, key: CmpcNoiseKey, step: int, B: int, n: int, sigma_ptr: int,
                   rho_ptr: int, w_ptr: int, base_ptr: int, out_ptr: int):
    """cmpc_noise_step on raw device addresses (0: NULL; asynchronous on the stream)."""
    vp = lambda p: ctypes.c_void_p(p or None)
    check(load_library().cmpc_noise_step(int(device), vp(stream_ptr), ctypes.byref(key), _noise_step_arg(step), int(B),
                                         int(n), vp(sigma_ptr), vp(rho_ptr), vp(w_ptr), vp(base_ptr), vp(out_ptr)),
          "cmpc_noise_step")


def _noise_tensor(t, B: int, n: int, what: str, device=None):
    import torch
    if t is None:
        return 0
    if (not isinstance(t, torch.Tensor) or tuple(t.shape) != (B, n) or t.dtype != torch.float64 or not t.is_cuda
            or not t.is_contiguous() or (device is not None and t.device != device)):
        raise ValueError(f"{what} must be a contiguous float64 tensor (B = {B}, n = {n}) on the device of out")
    return t.data_ptr()


def noise_uniforms(seed: int, step: int, out, stream: int = 0, scenario0: int = 0):
    """The uniforms of a step into `out`, a contiguous float64 device tensor
    (B, ceil(n/2), 2), on torch's current stream (cmpc_noise_uniforms); n is
    taken as 2 * out.shape[1].  Returns out."""
    import torch
    if (not isinstance(out, torch.Tensor) or out.dim() != 3 or out.shape[2] != 2 or out.dtype != torch.float64
            or not out.is_cuda or not out.is_contiguous()):
        raise ValueError("out must be a contiguous float64 device tensor (B, ceil(n/2), 2)")
    B, n = int(out.shape[0]), 2 * int(out.shape[1])
    key = noise_check(seed, step, B, n, stream, scenario0)
    noise_uniforms_ptr(out.device.index, torch.cuda.current_stream(out.device).cuda_stream, key, step, B, n,
                       out.data_ptr())
    return out


def noise_step(seed: int, step: int, out, sigma=None, rho=None, w=None, base=None, stream: int = 0,
               scenario0: int = 0):
    """out = base + the step's disturbance, on the device (cmpc_noise_step, one
    launch on torch's current stream; include/cmpc.h has the arithmetic).
    out, and sigma, rho, w, base where given: contiguous float64 tensors (B, n)
    on one device.  w is the AR(1) state, updated in place (needed with rho).
    Returns out."""
    import torch
    if (not isinstance(out, torch.Tensor) or out.dim() != 2 or out.dtype != torch.float64 or not out.is_cuda
            or not out.is_contiguous()):
        raise ValueError("out must be a contiguous float64 device tensor (B, n)")
    B, n = int(out.shape[0]), int(out.shape[1])
    key = noise_check(seed, step, B, n, stream, scenario0)
    ptrs = [_noise_tensor(t, B, n, what, out.device)
            for t, what in ((sigma, "sigma"), (rho, "rho"), (w, "w"), (base, "base"))]
    noise_step_ptr(out.device.index, torch.cuda.current_stream(out.device).cuda_stream, key, step, B, n, *ptrs,
                   out.data_ptr())
    return out


def certify_len(dims: CmpcDims) -> int:
    """Rows of a QP slot's certificate record, 2 nV + 9 (cmpc_certify_len, host only)."""
    n = load_library().cmpc_certify_len(ctypes.byref(dims))
    check(min(n, 0), "cmpc_certify_len")
    return n


def certify_fields(dims: CmpcDims) -> dict:
    """{field name: slice of the record's rows} for dims, from the library's
    own table (cmpc_certify_field, host only).  The record is field-major: a
    download reshaped to (certify_len, B*S) is indexed by these slices."""
    lib = load_library()
    out = {}
    for name in _abi.CERTIFY_FIELDS:
        off, cnt = ctypes.c_int(), ctypes.c_int()
        check(lib.cmpc_certify_field(ctypes.byref(dims), name.encode(), ctypes.byref(off), ctypes.byref(cnt)),
              "cmpc_certify_field")
        out[name] = slice(off.value, off.value + cnt.value)
    return out


def certify_available(dims: CmpcDims) -> bool:
    """Whether Context.certify has a kernel instance for dims (host only)."""
    return bool(load_library().cmpc_certify_available(ctypes.byref(dims)))


def predict_available(dims: CmpcDims) -> bool:
    """Whether Context.predict has a kernel instance for dims (host only)."""
    return bool(load_library().cmpc_predict_available(ctypes.byref(dims)))


def reference_profile_available(dims: CmpcDims) -> bool:
    """Whether Context.set/bind_scenario_reference_profile has a kernel
    instance for dims (host only)."""
    return bool(load_library().cmpc_reference_profile_available(ctypes.byref(dims)))


def _lwt_pair(dims: CmpcDims, lwt_s0, lwt_s1):
    if lwt_s0 is None or lwt_s1 is None:
        return None, None, None
    n = dims.ny * dims.ny
    a = np.ascontiguousarray(lwt_s0, dtype=np.float64).reshape(-1)
    b = np.ascontiguousarray(lwt_s1, dtype=np.float64).reshape(-1)
    if a.size != n or b.size != n:
        raise ValueError("lwt tables must be ny x ny")
    dp = ctypes.POINTER(ctypes.c_double)
    return (a, b), a.ctypes.data_as(dp), b.ctypes.data_as(dp)


def build_pairing_reason(dims: CmpcDims, lwt_s0=None, lwt_s1=None) -> str:
    """Why Context.set_build_pairing(CMPC_PAIRING_ON) would refuse dims (host
    only): "" when the shared form of the row build is eligible.  lwt_s0 /
    lwt_s1: the two sub-controllers' L_W' tables (ny x ny), compared bit for
    bit; None leaves the weights out."""
    keep, pa, pb = _lwt_pair(dims, lwt_s0, lwt_s1)
    out = load_library().cmpc_build_pairing_reason(ctypes.byref(dims), pa, pb)
    del keep
    return out.decode()


def build_pairing_available(dims: CmpcDims, lwt_s0=None, lwt_s1=None) -> bool:
    """Whether the shared form of the row build is eligible for dims (host only)."""
    keep, pa, pb = _lwt_pair(dims, lwt_s0, lwt_s1)
    out = bool(load_library().cmpc_build_pairing_available(ctypes.byref(dims), pa, pb))
    del keep
    return out


def plan_error_string(code: int) -> str:
    """The text cmpc_last_error() holds after a call that failed with this plan error."""
    return load_library().cmpc_plan_error_string(int(code)).decode()


def rows_lds_model(dims: CmpcDims):
    """(packed, chosen, lds_bytes): the row build kernel's modelled extra LDS
    cycles per wave-step for regions packed back to back and for the layout
    cmpc_build uses (rows_layout.cpp), and its LDS bytes per workgroup."""
    a, b, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int32()
    check(load_library().cmpc_rows_lds_model(ctypes.byref(dims), ctypes.byref(a), ctypes.byref(b),
                                              ctypes.byref(n)), "cmpc_rows_lds_model")
    return a.value, b.value, n.value


def plant_default(plant: int):
    x = np.zeros(16)
    u = np.zeros(16)
    check(load_library().cmpc_plant_default(plant, dptr(x), dptr(u)), "cmpc_plant_default")
    ns, ni = (11, 9) if plant == 0 else (10, 8)
    return x[:ns].copy(), u[:ni].copy()


def plant_output(plant: int, x) -> np.ndarray:
    y = np.zeros(4)
    check(load_library().cmpc_plant_output(plant, dptr(np.ascontiguousarray(x, np.float64)),
                                            dptr(y)), "cmpc_plant_output")
    return y


def plant_lin_record(cfg: ControllerConfig, dims: CmpcDims, s: int, x, u_full, Ts=0.05,
                     p_in=1.0, p_out=1.0, out=None) -> np.ndarray:
    """AugmentedLinearizedSystem::Update for sub-controller s -> lin record
    (fills Aorig, Bin, Csel, fd; dx_aug and yprev are left as they are)."""
    L = layout_of(dims)
    rec = np.zeros(L.rec_len) if out is None else out
    io = np.ascontiguousarray(cfg.input_order[s], dtype=np.int32)
    oi = np.ascontiguousarray(cfg.out_idx[s], dtype=np.int32)
    check(load_library().cmpc_plant_lin_record(
        cfg.plant, p_in, p_out, Ts, dptr(np.ascontiguousarray(x, np.float64)),
        dptr(np.ascontiguousarray(u_full, np.float64)), iptr(io), iptr(oi), ctypes.byref(dims),
        dptr(rec)), "cmpc_plant_lin_record")
    return rec


def qp_solve_batch(H, g, lb, ub, lbA, ubA, nu, ws_in=None, max_chg=10, device=0):
    """The device QP solver alone over a batch (parity / known-answer tests)."""
    H = np.ascontiguousarray(H, np.float64)
    nqp, n = g.shape
    c = lambda a: np.ascontiguousarray(a, np.float64)
    ws_in = np.zeros(nqp, np.uint32) if ws_in is None else np.ascontiguousarray(ws_in, np.uint32)
    x = np.zeros((nqp, n))
    status = np.zeros(nqp, np.int32)
    nchg = np.zeros(nqp, np.int32)
    ws_out = np.zeros(nqp, np.uint32)
    trace = np.zeros((nqp, 16), np.uint8)
    ntrace = np.zeros(nqp, np.int32)
    lib = load_library()
    lib.cmpc_qp_solve_batch.restype = ctypes.c_int
    check(lib.cmpc_qp_solve_batch(device, n, nu, nqp, dptr(H), dptr(c(g)), dptr(c(lb)),
                                  dptr(c(ub)), dptr(c(lbA)), dptr(c(ubA)), uptr(ws_in), max_chg,
                                  dptr(x), iptr(status), iptr(nchg), uptr(ws_out), bptr(trace),
                                  iptr(ntrace)), "cmpc_qp_solve_batch")
    return x, status, nchg, ws_out, trace, ntrace


def qp_solve_batch_map(H, f, G, d, lb, ub, lbA, ubA, nu, ws_in=None, max_chg=10, device=0):
    """One Jacobi-iteration solve per QP in the map form (g = f + G d), the
    solve of cmpc_iterate / DistributedSolver::UpdateAndSolveQP."""
    H = np.ascontiguousarray(H, np.float64)
    nqp, n = f.shape
    G = np.ascontiguousarray(G, np.float64).reshape(nqp, n, -1)
    nvo = G.shape[2]
    c = lambda a: np.ascontiguousarray(a, np.float64)
    ws_in = np.zeros(nqp, np.uint32) if ws_in is None else np.ascontiguousarray(ws_in, np.uint32)
    x = np.zeros((nqp, n))
    status = np.zeros(nqp, np.int32)
    nchg = np.zeros(nqp, np.int32)
    ws_out = np.zeros(nqp, np.uint32)
    trace = np.zeros((nqp, 16), np.uint8)
    ntrace = np.zeros(nqp, np.int32)
    lib = load_library()
    check(lib.cmpc_qp_solve_batch_map(device, n, nu, nvo, nqp, dptr(H), dptr(c(f)), dptr(G), dptr(c(d)),
                                      dptr(c(lb)), dptr(c(ub)), dptr(c(lbA)), dptr(c(ubA)), uptr(ws_in), max_chg,
                                      dptr(x), iptr(status), iptr(nchg), uptr(ws_out), bptr(trace), iptr(ntrace)),
          "cmpc_qp_solve_batch_map")
    return x, status, nchg, ws_out, trace, ntrace


def scenario_reference_offsets(cfg: ControllerConfig, y_offset) -> np.ndarray:
    """Plant-level setpoint offsets -> slots.  y_offset: (B, n_outputs), one
    offset per scenario and plant output; returns (B*S, ny) in slot order
    q = b*S + s, sub-controller s taking its outputs cfg.out_idx[s]
    (Context.set_scenario_reference)."""
    y_offset = np.asarray(y_offset, dtype=np.float64)
    n_out = int(np.max(cfg.out_idx)) + 1
    if y_offset.ndim != 2 or y_offset.shape[1] < n_out:
        raise ValueError(f"y_offset must be (B, n_outputs) with n_outputs >= {n_out}, got {y_offset.shape}")
    oi = np.asarray(cfg.out_idx, dtype=np.int64)[:, :cfg.ny]      # (S, ny)
    return np.ascontiguousarray(y_offset[:, oi].reshape(y_offset.shape[0] * cfg.S, cfg.ny))


def scenario_reference_profiles(cfg: ControllerConfig, y_dev) -> np.ndarray:
    """Plant-level reference profiles -> slots.  y_dev: (B, p, n_outputs), one
    deviation per scenario, horizon row and plant output; returns (B*S, p, ny)
    in slot order q = b*S + s, sub-controller s taking its outputs
    cfg.out_idx[s] (Context.set_scenario_reference_profile).  The 3-D sibling
    of scenario_reference_offsets."""
    y_dev = np.asarray(y_dev, dtype=np.float64)
    n_out = int(np.max(cfg.out_idx)) + 1
    if y_dev.ndim != 3 or y_dev.shape[2] < n_out:
        raise ValueError(f"y_dev must be (B, p, n_outputs) with n_outputs >= {n_out}, got {y_dev.shape}")
    oi = np.asarray(cfg.out_idx, dtype=np.int64)[:, :cfg.ny]      # (S, ny)
    B, p = y_dev.shape[:2]
    # (B, p, S, ny) -> (B, S, p, ny)
    return np.ascontiguousarray(y_dev[:, :, oi].transpose(0, 2, 1, 3).reshape(B * cfg.S, p, cfg.ny))


def scenario_limits(cfg: ControllerConfig, lower, upper, rate_lower, rate_upper):
    """Plant-level input limits -> slots.  Each argument: (B, nu_tot) in plant
    control order; returns four (B*S, nu) arrays in slot order, sub-controller
    s taking its own inputs cfg.input_order[s][:nu]
    (Context.set_scenario_constraints)."""
    io = np.asarray(cfg.input_order, dtype=np.int64)[:, :cfg.nu]  # (S, nu)
    out = []
    B = None
    for name, a in (("lower", lower), ("upper", upper), ("rate_lower", rate_lower), ("rate_upper", rate_upper)):
        a = np.asarray(a, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != cfg.nu_tot or (B is not None and a.shape[0] != B):
            raise ValueError(f"{name} must be (B, nu_tot = {cfg.nu_tot}), got {a.shape}")
        B = a.shape[0]
        out.append(np.ascontiguousarray(a[:, io].reshape(B * cfg.S, cfg.nu)))
    return tuple(out)


def _torch_runtime_first():
    """torch bundles its own HIP runtime; when the library's runtime opens the
    device first, torch's later initialisation reports no GPUs.  If the
    caller uses torch for device buffers (it is imported), bring its runtime
    up before the library's."""
    import sys
    torch = sys.modules.get("torch")
    if torch is not None:
        try:
            if torch.cuda.is_available():
                torch.cuda.init()
        except Exception:
            pass


class Context:
    """One batched NerveCenter over B scenarios of cfg.S sub-controllers."""

    def __init__(self, cfg: ControllerConfig, B: int, device: int = 0):
        self.lib = load_library()
        self.cfg = cfg
        self.B = B
        self.dims = CmpcDims.from_config(cfg, B)
        self.layout = layout_of(self.dims)
        self.nqp = B * cfg.S
        self._h = ctypes.c_void_p()
        _torch_runtime_first()
        check(self.lib.cmpc_create(ctypes.byref(self._h), ctypes.byref(self.dims), device),
              "cmpc_create")

    # -- lifecycle -------------------------------------------------------
    def close(self):
        if self._h:
            self.lib.cmpc_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_handle: int):
        check(self.lib.cmpc_set_stream(self._h, ctypes.c_void_p(stream_handle)), "cmpc_set_stream")

    # -- configuration ---------------------------------------------------
    def configure(self, a: ControllerArrays):
        for s in range(self.cfg.S):
            check(self.lib.cmpc_set_weights(self._h, s, dptr(np.ascontiguousarray(a.uwt[s])),
                                            dptr(np.ascontiguousarray(a.ywt[s]))), "set_weights")
            check(self.lib.cmpc_set_constraints(
                self._h, s, dptr(np.ascontiguousarray(a.lower[s])),
                dptr(np.ascontiguousarray(a.upper[s])), dptr(np.ascontiguousarray(a.rate_lower[s])),
                dptr(np.ascontiguousarray(a.rate_upper[s]))), "set_constraints")
            check(self.lib.cmpc_set_reference(self._h, s, dptr(np.ascontiguousarray(a.y_ref[s]))),
                  "set_reference")

    def set_state(self, u_old=None, du_old=None, ws=None):
        c = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)
        u_old, du_old, ws = c(u_old, np.float64), c(du_old, np.float64), c(ws, np.uint32)
        check(self.lib.cmpc_set_state(self._h, dptr(u_old) if u_old is not None else None,
                                      dptr(du_old) if du_old is not None else None,
                                      uptr(ws) if ws is not None else None), "set_state")

    def get_state(self):
        u_old = np.zeros((self.nqp, self.cfg.nu_tot))
        du_old = np.zeros((self.nqp, self.layout.nV))
        ws = np.zeros(self.nqp, np.uint32)
        check(self.lib.cmpc_get_state(self._h, dptr(u_old), dptr(du_old), uptr(ws)), "get_state")
        return u_old, du_old, ws

    def upload_lin(self, lin: np.ndarray):
        lin = np.ascontiguousarray(lin, np.float64)
        assert lin.size == self.nqp * self.layout.rec_len
        check(self.lib.cmpc_upload_lin(self._h, dptr(lin)), "upload_lin")

    def lin_device_ptr(self) -> int:
        return self.lib.cmpc_lin_device(self._h)

    def bind_lin(self, device_ptr: int = 0):
        """Bind an external device-resident record array (0 = own buffer)."""
        check(self.lib.cmpc_bind_lin(self._h, ctypes.c_void_p(device_ptr or None)), "cmpc_bind_lin")

    def bind_state(self, u_old_ptr: int = 0, du_old_ptr: int = 0, ws_ptr: int = 0):
        """Bind external device-resident state arrays (u_old B*S x nu_tot f64,
        du_old B*S x nV f64, ws B*S u32; all three, or 0 for the own buffers)."""
        vp = lambda p: ctypes.c_void_p(p or None)
        check(self.lib.cmpc_bind_state(self._h, vp(u_old_ptr), vp(du_old_ptr), vp(ws_ptr)),
              "cmpc_bind_state")

    # -- per-scenario setpoints and limits (include/cmpc.h) -----------------
    def set_scenario_reference(self, dy_ref=None):
        """Per-slot constant setpoint offsets, (B*S, ny) host array in slot
        order (scenario_reference_offsets maps plant outputs to slots): slot q
        tracks y_ref[s] + dy_ref[q] over the whole horizon.  None clears."""
        if dy_ref is None:
            check(self.lib.cmpc_set_scenario_reference(self._h, None), "cmpc_set_scenario_reference")
            return
        dy = np.ascontiguousarray(dy_ref, np.float64)
        if dy.size != self.nqp * self.cfg.ny:
            raise ValueError(f"dy_ref must hold B*S*ny = {self.nqp * self.cfg.ny} values, got {dy.shape}")
        check(self.lib.cmpc_set_scenario_reference(self._h, dptr(dy)), "cmpc_set_scenario_reference")

    def bind_scenario_reference(self, device_ptr: int = 0):
        """Bind a device-resident (B*S, ny) f64 offset array (0 clears)."""
        check(self.lib.cmpc_bind_scenario_reference(self._h, ctypes.c_void_p(device_ptr or None)),
              "cmpc_bind_scenario_reference")

    def set_scenario_reference_profile(self, dref=None):
        """Per-slot reference profiles over the horizon, (B*S, p, ny) host array
        in slot order (scenario_reference_profiles maps plant outputs to
        slots): slot q tracks y_ref[s][r] + dy_ref[q] + dref[q][r] from the
        next build on.  None clears."""
        if dref is None:
            check(self.lib.cmpc_set_scenario_reference_profile(self._h, None),
                  "cmpc_set_scenario_reference_profile")
            return
        dr = np.ascontiguousarray(dref, np.float64)
        n = self.nqp * self.cfg.p * self.cfg.ny
        if dr.size != n:
            raise ValueError(f"dref must hold B*S*p*ny = {n} values, got {dr.shape}")
        check(self.lib.cmpc_set_scenario_reference_profile(self._h, dptr(dr)),
              "cmpc_set_scenario_reference_profile")

    def bind_scenario_reference_profile(self, device_ptr: int = 0):
        """Bind a device-resident (B*S, p, ny) f64 profile array (0 clears)."""
        check(self.lib.cmpc_bind_scenario_reference_profile(self._h, ctypes.c_void_p(device_ptr or None)),
              "cmpc_bind_scenario_reference_profile")

    def get_scenario_reference_profile(self) -> np.ndarray:
        """(B*S, p, ny): the profile in force (set or bound); raises if none."""
        out = np.zeros((self.nqp, self.cfg.p, self.cfg.ny))
        check(self.lib.cmpc_get_scenario_reference_profile(self._h, dptr(out)),
              "cmpc_get_scenario_reference_profile")
        return out

    # -- per-scenario weights (include/cmpc.h) -------------------------------
    def set_scenario_weights(self, uwt=None, ywt=None):
        """Per-slot weights in slot order: uwt (B*S, nu, nu) symmetric and ywt
        (B*S, ny, ny) symmetric positive semi-definite host arrays.  Slot q is
        built with its own pair in place of the sub-controller's shared one
        from the next build on.  Both None clears."""
        if uwt is None and ywt is None:
            check(self.lib.cmpc_set_scenario_weights(self._h, None, None), "cmpc_set_scenario_weights")
            return
        if uwt is None or ywt is None:
            raise ValueError("give both uwt and ywt, or neither")
        u = np.ascontiguousarray(uwt, np.float64)
        y = np.ascontiguousarray(ywt, np.float64)
        nu, ny = self.cfg.nu, self.cfg.ny
        if u.size != self.nqp * nu * nu:
            raise ValueError(f"uwt must hold B*S*nu*nu = {self.nqp * nu * nu} values, got {u.shape}")
        if y.size != self.nqp * ny * ny:
            raise ValueError(f"ywt must hold B*S*ny*ny = {self.nqp * ny * ny} values, got {y.shape}")
        check(self.lib.cmpc_set_scenario_weights(self._h, dptr(u), dptr(y)), "cmpc_set_scenario_weights")

    def bind_scenario_weights(self, device_ptr: int = 0):
        """Bind a device-resident (B*S, ny*ny + nu*nu) f64 array of per-slot
        blocks [L_W' | uwt], already factored (weight_factor); 0 clears."""
        check(self.lib.cmpc_bind_scenario_weights(self._h, ctypes.c_void_p(device_ptr or None)),
              "cmpc_bind_scenario_weights")

    def get_scenario_weights(self):
        """(uwt (B*S, nu, nu), L_W' (B*S, ny, ny)): the per-slot weights in
        force (set or bound), the output weight as its factor; raises if none."""
        nu, ny = self.cfg.nu, self.cfg.ny
        u = np.zeros((self.nqp, nu, nu))
        lw = np.zeros((self.nqp, ny, ny))
        check(self.lib.cmpc_get_scenario_weights(self._h, dptr(u), dptr(lw)), "cmpc_get_scenario_weights")
        return u, lw

    # -- per-scenario boundary pressures of the model (include/cmpc.h) -------
    def set_scenario_pressures(self, pressures=None):
        """Per-scenario boundary pressures of the controller's model, a (B, 2)
        host array of [p_in, p_out], finite and positive.  While in force the
        producer (produce_lin, observer_init, observe_step, control_step)
        linearises scenario b at its own pair and the scalar p_in / p_out
        arguments are ignored.  None clears."""
        if pressures is None:
            check(self.lib.cmpc_set_scenario_pressures(self._h, None), "cmpc_set_scenario_pressures")
            return
        p = np.ascontiguousarray(pressures, np.float64)
        if p.shape != (self.B, 2):
            raise ValueError(f"pressures must be (B = {self.B}, 2), got {p.shape}")
        check(self.lib.cmpc_set_scenario_pressures(self._h, dptr(p)), "cmpc_set_scenario_pressures")

    def bind_scenario_pressures(self, device_ptr: int = 0):
        """Bind a device-resident (B, 2) f64 array of [p_in, p_out], read at
        each launch (the caller may rewrite it between steps); 0 clears."""
        check(self.lib.cmpc_bind_scenario_pressures(self._h, ctypes.c_void_p(device_ptr or None)),
              "cmpc_bind_scenario_pressures")

    def get_scenario_pressures(self) -> np.ndarray:
        """(B, 2): the pressures in force (set or bound); raises if none."""
        out = np.zeros((self.B, 2))
        check(self.lib.cmpc_get_scenario_pressures(self._h, dptr(out)), "cmpc_get_scenario_pressures")
        return out

    def set_scenario_constraints(self, lower=None, upper=None, rate_lower=None, rate_upper=None):
        """Per-slot input limits, four (B*S, nu) host arrays in slot order
        (scenario_limits maps plant inputs to slots); all None clears."""
        arrs = [lower, upper, rate_lower, rate_upper]
        if all(a is None for a in arrs):
            check(self.lib.cmpc_set_scenario_constraints(self._h, None, None, None, None),
                  "cmpc_set_scenario_constraints")
            return
        c = []
        for a in arrs:
            if a is None:
                c.append(None)
                continue
            a = np.ascontiguousarray(a, np.float64)
            if a.size != self.nqp * self.cfg.nu:
                raise ValueError(f"each limit array must hold B*S*nu = {self.nqp * self.cfg.nu} values, got {a.shape}")
            c.append(a)
        check(self.lib.cmpc_set_scenario_constraints(self._h, *[None if a is None else dptr(a) for a in c]),
              "cmpc_set_scenario_constraints")

    def bind_scenario_constraints(self, device_ptr: int = 0):
        """Bind a device-resident (B*S, 4, nu) f64 array, per slot
        [lower | upper | rate_lower | rate_upper] (0 clears)."""
        check(self.lib.cmpc_bind_scenario_constraints(self._h, ctypes.c_void_p(device_ptr or None)),
              "cmpc_bind_scenario_constraints")

    def get_scenario_reference(self) -> np.ndarray:
        """(B*S, ny): the offsets in force (set or bound); raises if none."""
        out = np.zeros((self.nqp, self.cfg.ny))
        check(self.lib.cmpc_get_scenario_reference(self._h, dptr(out)), "cmpc_get_scenario_reference")
        return out

    def get_scenario_constraints(self):
        """Four (B*S, nu) arrays: the per-slot limits in force; raises if none."""
        out = [np.zeros((self.nqp, self.cfg.nu)) for _ in range(4)]
        check(self.lib.cmpc_get_scenario_constraints(self._h, *[dptr(a) for a in out]),
              "cmpc_get_scenario_constraints")
        return tuple(out)

    def produce_lin(self, x_ptr: int, u_full_ptr: int, y_ptr: int, dx_aug_ptr: int = 0,
                    Ts: float = 0.05, p_in: float = 1.0, p_out: float = 1.0):
        """Device producer (cmpc_produce_lin): linearise + discretise the plant
        for every scenario on the GPU and write this context's lin records.
        Arguments are device pointers (e.g. torch tensor .data_ptr())."""
        io = np.ascontiguousarray(self.cfg.input_order, dtype=np.int32)
        oi = np.ascontiguousarray(self.cfg.out_idx, dtype=np.int32)
        check(self.lib.cmpc_produce_lin(
            self._h, self.cfg.plant, p_in, p_out, Ts, iptr(io), iptr(oi), ctypes.c_void_p(x_ptr),
            ctypes.c_void_p(u_full_ptr), ctypes.c_void_p(dx_aug_ptr or None), ctypes.c_void_p(y_ptr)),
            "cmpc_produce_lin")

    # -- observer + receding-horizon update --------
    def set_observer(self, s: int, M: np.ndarray):
        """ObserverMatrix of sub-controller s, (ns + ndist) x n_outputs."""
        M = np.ascontiguousarray(M, dtype=np.float64)
        check(self.lib.cmpc_set_observer(self._h, s, M.shape[1], dptr(M)), "cmpc_set_observer")

    @property
    def observer_len(self) -> int:
        return self.lib.cmpc_observer_len(self._h)

    def observer_init(self, x_ptr: int, u_full_ptr: int, y_ptr: int, dx_init_ptr: int = 0,
                      Ts: float = 0.05, p_in: float = 1.0, p_out: float = 1.0):
        """DistributedController::Initialize for every slot: observer state at
        (x_init[b], y_init[b], dx_init) and the records at x_init (device ptrs)."""
        io = np.ascontiguousarray(self.cfg.input_order, dtype=np.int32)
        oi = np.ascontiguousarray(self.cfg.out_idx, dtype=np.int32)
        check(self.lib.cmpc_observer_init(
            self._h, self.cfg.plant, p_in, p_out, Ts, iptr(io), iptr(oi), ctypes.c_void_p(x_ptr),
            ctypes.c_void_p(u_full_ptr), ctypes.c_void_p(y_ptr), ctypes.c_void_p(dx_init_ptr or None)),
            "cmpc_observer_init")

    def observe_step(self, u_full_ptr: int, y_ptr: int):
        """ObserveAPosteriori + x_hat update, then the records at x_hat."""
        check(self.lib.cmpc_observe_step(self._h, ctypes.c_void_p(u_full_ptr), ctypes.c_void_p(y_ptr)),
              "cmpc_observe_step")

    def control_step(self, u_full_ptr: int, y_ptr: int, K: int):
        """NerveCenter::GetNextInput on the device (cmpc_control_step): observe_step,
        step(K, 0) and observe_apply, one kernel launch where the batch allows."""
        check(self.lib.cmpc_control_step(self._h, ctypes.c_void_p(u_full_ptr), ctypes.c_void_p(y_ptr), K),
              "cmpc_control_step")

    def control_step_download(self, u_full: np.ndarray, y: np.ndarray, K: int):
        """cmpc_control_step_download: the control step from host arrays and its
        plans, statuses and nWSR (polled completion for one-workgroup batches)."""
        du = np.zeros((self.nqp, self.layout.nV))
        status = np.zeros(self.nqp, np.int32)
        nwsr = np.zeros(self.nqp, np.int32)
        check(self.lib.cmpc_control_step_download(self._h, dptr(np.ascontiguousarray(u_full, np.float64)),
                                                  dptr(np.ascontiguousarray(y, np.float64)), K, dptr(du),
                                                  iptr(status), iptr(nwsr)), "cmpc_control_step_download")
        return du, status, nwsr

    def observe_apply(self):
        """UpdateU: ObserveAPriori with the own first move, then u_old += du."""
        check(self.lib.cmpc_observe_apply(self._h), "cmpc_observe_apply")

    def observer_state(self) -> np.ndarray:
        """(B*S, observer_len): [x_hat ns][dx_aug ntot][y_old n_out][C n_out x ns]."""
        out = np.zeros((self.B * self.cfg.S, self.observer_len))
        check(self.lib.cmpc_get_observer_state(self._h, dptr(out)), "cmpc_get_observer_state")
        return out

    def set_observer_state(self, st: np.ndarray):
        st = np.ascontiguousarray(st, dtype=np.float64)
        assert st.shape == (self.B * self.cfg.S, self.observer_len)
        check(self.lib.cmpc_set_observer_state(self._h, dptr(st)), "cmpc_set_observer_state")

    def download_lin(self) -> np.ndarray:
        """The context's own record buffer (B*S, rec_len), e.g. after produce_lin."""
        out = np.zeros((self.B * self.cfg.S, self.layout.rec_len))
        check(self.lib.cmpc_download_lin(self._h, dptr(out)), "cmpc_download_lin")
        return out

    # -- hot path --------------------------------------------------------
    def build(self):
        check(self.lib.cmpc_build(self._h), "cmpc_build")

    def set_build_variant(self, variant: int):
        """CMPC_BUILD_AUTO / CMPC_BUILD_WAVE (one QP per wave) / CMPC_BUILD_ROWS
        (four QPs per wave, one per DPP row) / CMPC_BUILD_SPLIT (one QP per two
        waves: chain and gather, every ny)."""
        check(self.lib.cmpc_set_build_variant(self._h, int(variant)), "cmpc_set_build_variant")

    def set_build_pairing(self, mode: int):
        """CMPC_PAIRING_AUTO / CMPC_PAIRING_OFF / CMPC_PAIRING_ON: whether the row
        build shares the Markov chain between a cooperative scenario's two QPs
        (cmpc.h).  ON raises where the configuration is not eligible."""
        check(self.lib.cmpc_set_build_pairing(self._h, int(mode)), "cmpc_set_build_pairing")

    def last_build_shared_scenarios(self) -> int:
        """Scenarios the last build() built in the shared form, -1 if that build
        was not the shared form."""
        v = self.lib.cmpc_last_build_shared_scenarios(self._h)
        check(min(v + 1, 0), "cmpc_last_build_shared_scenarios")
        return v

    def last_build_kernel(self) -> int:
        """CMPC_BUILD_WAVE / CMPC_BUILD_ROWS / CMPC_BUILD_SPLIT: the kernel the
        last build() ran."""
        v = self.lib.cmpc_last_build_kernel(self._h)
        check(min(v, 0), "cmpc_last_build_kernel")
        return v


    def set_solve_variant(self, variant: int):
        """CMPC_SOLVE_AUTO / CMPC_SOLVE_LANE (one QP per lane) / CMPC_SOLVE_ROWS
        (one QP per 16-lane row): the kernel of iterate / init_warmstart."""
        check(self.lib.cmpc_set_solve_variant(self._h, int(variant)), "cmpc_set_solve_variant")

    def last_solve_kernel(self) -> int:
        """CMPC_SOLVE_LANE / CMPC_SOLVE_ROWS: the kernel the last solve ran."""
        v = self.lib.cmpc_last_solve_kernel(self._h)
        check(min(v, 0), "cmpc_last_solve_kernel")
        return v

    def set_step_variant(self, variant: int):
        """CMPC_STEP_AUTO / CMPC_STEP_SPLIT (build + iterate launches) /
        CMPC_STEP_FUSED (one launch: the build kernel runs the iterations)."""
        check(self.lib.cmpc_set_step_variant(self._h, int(variant)), "cmpc_set_step_variant")

    def last_step_fused(self) -> bool:
        v = self.lib.cmpc_last_step_fused(self._h)
        check(min(v, 0), "cmpc_last_step_fused")
        return bool(v)
    def init_warmstart(self):
        check(self.lib.cmpc_init_warmstart(self._h), "cmpc_init_warmstart")

    def iterate(self, K: int, flags: int = 0):
        check(self.lib.cmpc_iterate(self._h, K, flags), "cmpc_iterate")

    def step(self, K: int, flags: int = 0):
        check(self.lib.cmpc_step(self._h, K, flags), "cmpc_step")

    def synchronize(self):
        check(self.lib.cmpc_synchronize(self._h), "cmpc_synchronize")

    # -- prediction (include/cmpc.h, cmpc_predict) --------------------------
    def predict(self, du_ptr: int = 0, du_other_ptr: int = 0):
        """Predicted outputs and objective values of every QP slot for the
        plans at du_ptr (device, (B*S, nV); 0: the context's current plans)
        and the other controllers' plans at du_other_ptr (device, (B*S, nVo)
        in the Jacobi iteration's order; 0: gathered from the scenario's other
        slots).  Refused unless a build has run and nothing it read has
        changed since.  Asynchronous; results through download_prediction."""
        vp = lambda p: ctypes.c_void_p(p or None)
        check(self.lib.cmpc_predict(self._h, vp(du_ptr), vp(du_other_ptr), 0), "cmpc_predict")

    def download_prediction(self):
        """(y_pred (B*S, p, ny), cost (B*S, 2) = [J_track, J_move]) of the last predict."""
        y = np.zeros((self.nqp, self.cfg.p, self.cfg.ny))
        cost = np.zeros((self.nqp, 2))
        check(self.lib.cmpc_download_prediction(self._h, dptr(y), dptr(cost)), "cmpc_download_prediction")
        return y, cost

    def prediction_ptrs(self):
        """Device addresses of (y_pred, cost); (0, 0) before the first predict."""
        return (self.lib.cmpc_prediction_device(self._h) or 0,
                self.lib.cmpc_prediction_cost_device(self._h) or 0)

    # -- multipliers and KKT certificate (include/cmpc.h, cmpc_certify*) ----
    def certify(self, du_other_ptr: int = 0):
        """Lagrange multipliers and KKT residuals of every QP slot for the
        context's current plans and the other controllers' plans at
        du_other_ptr (device, (B*S, nVo) in predict's order; 0: gathered from
        the scenario's other slots).  Refused unless a solve has written plans
        for the last build and nothing they depend on has changed since.
        Asynchronous; results through certify_download / certify_summary."""
        check(self.lib.cmpc_certify(self._h, ctypes.c_void_p(du_other_ptr or None), 0), "cmpc_certify")

    def certify_host(self, du_other=None):
        """certify with the other controllers' plans in a host array (B*S, nVo) or None."""
        d = None if du_other is None else np.ascontiguousarray(du_other, dtype=np.float64)
        check(self.lib.cmpc_certify_host(self._h, dptr(d) if d is not None and d.size else None, 0),
              "cmpc_certify_host")

    def certify_ptr(self) -> int:
        """Device address of the record; 0 before the first certify."""
        return self.lib.cmpc_certify_device(self._h) or 0

    def certify_record(self) -> np.ndarray:
        """(certify_len, B*S): the last record as stored, field-major."""
        out = np.zeros((certify_len(self.dims), self.nqp))
        check(self.lib.cmpc_certify_download(self._h, dptr(out)), "cmpc_certify_download")
        return out

    def certify_download(self) -> dict:
        """The last record by field name: lam (B*S, 2 nV), every other field (B*S,)."""
        rec = self.certify_record()
        out = {}
        for name, sl in certify_fields(self.dims).items():
            out[name] = np.ascontiguousarray(rec[sl].T) if name == "lam" else rec[sl.start].copy()
        return out

    def certify_summary(self, tol: float = 1e-9) -> dict:
        """The device's reduction of the last record over the OK slots
        (cmpc_certify_summary): the largest r_stat/scale, r_prim, r_dual/scale,
        r_comp/scale with their slots, n_above (OK slots with any of the four
        above tol) and n_not_ok."""
        out = _abi.CmpcCertifySummary()
        check(self.lib.cmpc_certify_summary(self._h, float(tol), ctypes.byref(out)), "cmpc_certify_summary")
        return out.as_dict()

    # -- closed-loop performance indices (include/cmpc.h, cmpc_score_*) -----
    def score_fields(self) -> dict:
        """{field name: slice of the record's rows} (score_fields(dims))."""
        return score_fields(self.dims)

    def score_enable(self, n_outputs: int, out_idx=None, Ts: float = 0.05, band=None):
        """Keep a running record of closed-loop indices per QP slot.  out_idx
        (S, ny): the plant output of each controlled output in the y of
        score_step (default cfg.out_idx); band (S, ny) settling bands or None
        for 0.  Allocates the record and resets it."""
        oi = np.asarray(self.cfg.out_idx if out_idx is None else out_idx)[:, :self.cfg.ny]
        oi, bd = score_check(self.dims, n_outputs, oi, Ts, band)
        check(self.lib.cmpc_score_enable(self._h, int(n_outputs), iptr(oi), float(Ts),
                                         dptr(bd) if bd is not None else None), "cmpc_score_enable")
        self._score_nout = int(n_outputs)

    def score_bind(self, device_ptr: int = 0):
        """Keep the record in a device buffer of score_len * B*S f64 (0: the
        context's own).  The buffer is taken as it is: follow with score_reset."""
        check(self.lib.cmpc_score_bind(self._h, ctypes.c_void_p(device_ptr or None)), "cmpc_score_bind")

    def score_capture(self, scenarios=(), t_cap: int = 0):
        """Also record rows [y | u_control | x] of the chosen scenarios for the
        first t_cap steps after a reset; an empty list turns it off."""
        sel = score_capture_check(self.dims, scenarios, t_cap)
        check(self.lib.cmpc_score_capture(self._h, int(sel.size), iptr(sel), int(t_cap)), "cmpc_score_capture")
        self._score_sel, self._score_tcap = int(sel.size), int(t_cap) if sel.size else 0

    def score_bind_capture(self, device_ptr: int = 0):
        """Put the captured rows into a device buffer of t_cap * n_sel * width
        f64 (0: the context's own)."""
        check(self.lib.cmpc_score_bind_capture(self._h, ctypes.c_void_p(device_ptr or None)),
              "cmpc_score_bind_capture")

    def score_reset(self):
        check(self.lib.cmpc_score_reset(self._h), "cmpc_score_reset")

    def score_step(self, y_ptr: int, target_ptr: int = 0, plant_status_ptr: int = 0, u_control_ptr: int = 0,
                   x_ptr: int = 0):
        """Score the last solve's results against the measured outputs at y_ptr
        (device, (B, n_outputs)); the other device pointers are optional
        (cmpc_score_step).  Asynchronous on the context's stream."""
        vp = lambda p: ctypes.c_void_p(p or None)
        check(self.lib.cmpc_score_step(self._h, vp(y_ptr), vp(target_ptr), vp(plant_status_ptr), vp(u_control_ptr),
                                       vp(x_ptr)), "cmpc_score_step")

    def score_download(self) -> np.ndarray:
        """(score_len, B*S): the record in force, field-major."""
        out = np.zeros((score_len(self.dims), self.nqp))
        check(self.lib.cmpc_score_download(self._h, dptr(out)), "cmpc_score_download")
        return out

    def score_download_capture(self):
        """(rows (t_cap, n_sel, n_outputs + nu_tot + ns), steps recorded)."""
        w = self._score_nout + self.cfg.nu_tot + self.cfg.ns
        rows = np.zeros((getattr(self, "_score_tcap", 0), getattr(self, "_score_sel", 0), w))
        n = np.zeros(1, np.int32)
        check(self.lib.cmpc_score_download_capture(self._h, dptr(rows) if rows.size else None, iptr(n)),
              "cmpc_score_download_capture")
        return rows, int(n[0])

    def score_disable(self):
        check(self.lib.cmpc_score_disable(self._h), "cmpc_score_disable")

    def score_ensemble(self, thresholds=None) -> dict:
        """The device's reduction of the score record in force over the B
        scenarios (cmpc_score_ensemble): {field: {stat: (S, rows) array}} with
        the stats mean, std (population, about that mean), min, max, argmax
        (the lowest scenario on a tie) and count (scenarios above the row's
        threshold).  thresholds: None (every count 0), {field: a scalar or one
        value per row of the field} (+inf for the fields left out), or
        score_len values, one per record row."""
        n = score_len(self.dims)
        thr = None
        if isinstance(thresholds, dict):
            thr = np.full(n, np.inf)
            fields = score_fields(self.dims)
            for name, v in thresholds.items():
                if name not in fields:
                    raise ValueError(f"no score field named {name!r}")
                sl = fields[name]
                thr[sl] = np.broadcast_to(np.asarray(v, dtype=np.float64), (sl.stop - sl.start,))
        elif thresholds is not None:
            thr = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
            if thr.size != n:
                raise ValueError(f"thresholds must hold score_len = {n} values, got {thr.size}")
        out = np.zeros(n * self.dims.S * len(_abi.ENSEMBLE_STATS))
        check(self.lib.cmpc_score_ensemble(self._h, dptr(thr) if thr is not None else None, dptr(out)),
              "cmpc_score_ensemble")
        return score_ensemble_unpack(self.dims, out)

    def score_quantiles(self, levels) -> dict:
        """Exact quantiles over the B scenarios of every row of the score
        record in force, selected on the device (cmpc_score_quantiles):
        {field: {"lo", "hi", "arg", "value": (n_levels, S, rows)}} with lo and
        hi the order statistics at the level's two ranks (quantile_rank), arg
        (int64) the lowest scenario holding lo, and value = quantile_value(lo,
        hi, g): numpy's quantile on finite data."""
        lv = quantile_check(self.dims.B, levels)
        n, S = score_len(self.dims), self.dims.S
        out = np.zeros((n, S, lv.size, 3))
        check(self.lib.cmpc_score_quantiles(self._h, int(lv.size), dptr(lv), dptr(out)), "cmpc_score_quantiles")
        q = _quantiles_unpack(out, self.dims.B, lv)                # (n_levels, len, S)
        return {name: {k: np.ascontiguousarray(v[:, sl, :].transpose(0, 2, 1)) for k, v in q.items()}
                for name, sl in score_fields(self.dims).items()}

    # -- the ensemble's envelope per step (include/cmpc.h, cmpc_envelope_*) --
    def envelope_enable(self, n_outputs: int, t_cap: int, levels=(), thresholds=None):
        """Record, per step, the six ensemble statistics and the quantile pairs
        of `levels` (none: the statistics only) of every plant output and
        control input over the B scenarios; thresholds: one per channel
        (n_outputs + nu_tot) for the counts, or None."""
        lv, th = envelope_check(self.dims, n_outputs, t_cap, levels, thresholds)
        check(self.lib.cmpc_envelope_enable(self._h, int(n_outputs), int(t_cap), int(lv.size),
                                            dptr(lv) if lv.size else None, dptr(th) if th is not None else None),
              "cmpc_envelope_enable")
        self._env = (int(n_outputs), int(t_cap), lv)

    def envelope_step(self, y_ptr: int, u_control_ptr: int = 0):
        """One row from the device arrays y (B, n_outputs) and u_control (B,
        nu_tot) or 0 (cmpc_envelope_step): launches on the context's stream."""
        check(self.lib.cmpc_envelope_step(self._h, ctypes.c_void_p(y_ptr or None),
                                          ctypes.c_void_p(u_control_ptr or None)), "cmpc_envelope_step")

    def envelope_reset(self):
        check(self.lib.cmpc_envelope_reset(self._h), "cmpc_envelope_reset")

    def envelope_bind(self, device_ptr: int = 0):
        """Keep the rows in a device buffer of t_cap * envelope_len f64 (0: the context's own)."""
        check(self.lib.cmpc_envelope_bind(self._h, ctypes.c_void_p(device_ptr or None)), "cmpc_envelope_bind")

    def envelope_download(self):
        """(rows (t_cap, channels, 6 + 2 n_levels), steps recorded)."""
        no, t_cap, lv = getattr(self, "_env", (0, 0, np.zeros(0)))
        rows = np.zeros((t_cap, no + self.cfg.nu_tot if t_cap else 0, 6 + 2 * lv.size))
        n = np.zeros(1, np.int32)
        check(self.lib.cmpc_envelope_download(self._h, dptr(rows) if rows.size else None, iptr(n)),
              "cmpc_envelope_download")
        return rows, int(n[0])

    def envelope_disable(self):
        check(self.lib.cmpc_envelope_disable(self._h), "cmpc_envelope_disable")
        self._env = (0, 0, np.zeros(0))

    # -- results ---------------------------------------------------------
    def download(self):
        du = np.zeros((self.nqp, self.layout.nV))
        status = np.zeros(self.nqp, np.int32)
        nwsr = np.zeros(self.nqp, np.int32)
        check(self.lib.cmpc_download(self._h, dptr(du), iptr(status), iptr(nwsr)), "download")
        return du, status, nwsr

    def download_qp(self):
        nV, nVo = self.layout.nV, self.layout.nVo
        H = np.zeros((self.nqp, nV, nV))
        f = np.zeros((self.nqp, nV))
        G = np.zeros((self.nqp, nV, max(nVo, 1)))
        check(self.lib.cmpc_download_qp(self._h, dptr(H), dptr(f), dptr(G)), "download_qp")
        return H, f, G[:, :, :nVo]

    def download_trace(self, K: int):
        trace = np.zeros((self.nqp, K, 16), np.uint8)
        ntrace = np.zeros((self.nqp, K), np.int32)
        check(self.lib.cmpc_download_trace(self._h, bptr(trace), iptr(ntrace)), "download_trace")
        return trace, ntrace

    def enable_timing(self, on: bool = True, only=None):
        """Kernel timing: every kernel (on), none, or only the kernel ids in
        `only` (CMPC_KERNEL_*)."""
        flag = int(bool(on))
        if on and only is not None:
            flag = 0
            for k in only:
                flag |= 2 << k
        check(self.lib.cmpc_enable_timing(self._h, flag), "enable_timing")

    def set_timing_stride(self, stride: int):
        """Time only every stride-th launch of each timed kernel."""
        check(self.lib.cmpc_set_timing_stride(self._h, int(stride)), "cmpc_set_timing_stride")

    def kernel_time(self, kernel: int):
        ms = ctypes.c_double()
        n = ctypes.c_int64()
        check(self.lib.cmpc_kernel_time(self._h, kernel, ctypes.byref(ms), ctypes.byref(n)),
              "kernel_time")
        return ms.value, n.value
