"""Batched plant simulation on the GPU — the
reference harness's SimulationSystem (include/simulation_system.h) for B
scenarios: input delay line (TimeDelay, time_delay.h:41-58), controlled
Dormand-Prince over one sampling interval per call (integrate_const,
simulation_system.h:108-116), plant outputs.  Arrays are torch tensors on
the device (plumbing: the simulation itself is the HIP kernel in sim.hip)."""
import collections
import ctypes

import numpy as np

from ._abi import (CMPC_EIG_MAX_N, CMPC_FREQ_LEN, CMPC_FREQ_MAX_N, CMPC_FREQ_NSUM, CMPC_GAIN_LEN, CMPC_MODES_NSUM,
                   check, dptr, iptr, load_library)

REF_DELAYS = (0, 40, 0, 40)          # Delays of both plants (control-input order)
REF_CONTROL_INDEX = (0, 3, 4, 7)     # ControlInputIndex: plant input of each control input
REF_TS = 0.05                        # sampling time of results/*.dat
REF_EPS = 1e-6                       # Integrate's max_rel_error / max_abs_error
EQ_MAX_ITER = 20                     # equilibrium solve: Newton steps allowed and the
EQ_TOL = 1e-12                       # bound on max|f|
TARGET_TOL_Y = 1e-10                 # target solve: bound on max|y - t|


def _plant_sizes(lib, plant: int):
    ns, ni = ctypes.c_int(), ctypes.c_int()
    check(lib.cmpc_plant_dims(plant, ctypes.byref(ns), ctypes.byref(ni), None, None), "cmpc_plant_dims")
    return ns.value, ni.value


def plant_derivative(plant: int, x, u_full, p_in: float = 1.0, p_out: float = 1.0) -> np.ndarray:
    """dx = f(x, u_full) of the plant at the boundary pressures (host)."""
    lib = load_library()
    ns, ni = _plant_sizes(lib, plant)
    x = np.ascontiguousarray(x, np.float64)
    u = np.ascontiguousarray(u_full, np.float64)
    if x.shape != (ns,) or u.shape != (ni,):
        raise ValueError(f"x must be ({ns},) and u_full ({ni},), got {x.shape} and {u.shape}")
    dx = np.zeros(ns)
    check(lib.cmpc_plant_derivative(plant, p_in, p_out, dptr(x), dptr(u), dptr(dx)), "cmpc_plant_derivative")
    return dx


def plant_equilibrium(plant: int, pressures, u_full, x0, max_iter: int = EQ_MAX_ITER, tol: float = EQ_TOL):
    """The plant's equilibrium for B scenarios on the host (no device):
    pressures (B, 2) of [p_in, p_out], u_full (B, n_inputs), x0 (B, ns) the
    Newton start.  Returns (x, status, iters, resid): x (B, ns) is the
    equilibrium where status is CMPC_EQ_OK and x0's row elsewhere; the
    arithmetic is PlantSimulator.equilibrium's, bit for bit."""
    lib = load_library()
    ns, ni = _plant_sizes(lib, plant)
    x = np.array(x0, dtype=np.float64, order="C")
    B = x.shape[0] if x.ndim == 2 else 0
    p = np.ascontiguousarray(pressures, np.float64)
    u = np.ascontiguousarray(u_full, np.float64)
    if B < 1 or x.shape != (B, ns) or p.shape != (B, 2) or u.shape != (B, ni):
        raise ValueError(f"x0 must be (B, {ns}), pressures (B, 2) and u_full (B, {ni}), "
                         f"got {x.shape}, {p.shape} and {u.shape}")
    status, iters, resid = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B)
    check(lib.cmpc_plant_equilibrium_host(plant, B, dptr(p), dptr(u), dptr(x), max_iter, tol, iptr(status),
                                          iptr(iters), dptr(resid)), "cmpc_plant_equilibrium_host")
    return x, status, iters, resid


def _target_indices(lib, plant: int, hold, free, max_iter: int, tol_f: float, tol_y: float):
    """hold and free as int32 arrays of one length, checked by cmpc_target_check."""
    h = np.ascontiguousarray(hold, np.int32).reshape(-1)
    f = np.ascontiguousarray(free, np.int32).reshape(-1)
    if len(h) != len(f):
        raise ValueError(f"as many free inputs as held outputs: got {len(f)} and {len(h)}")
    check(lib.cmpc_target_check(plant, len(h), iptr(h), iptr(f), max_iter, tol_f, tol_y), "cmpc_target_check")
    return h, f


def _target_array(targets, B: int, nh: int) -> np.ndarray:
    """targets as (B, nh): (nh,) holds for every scenario."""
    t = np.asarray(targets, np.float64)
    if t.shape == (nh,):
        t = np.broadcast_to(t, (B, nh))
    if t.shape != (B, nh):
        raise ValueError(f"targets must be ({nh},) or ({B}, {nh}), got {t.shape}")
    return np.ascontiguousarray(t)


def plant_target(plant: int, pressures, hold, free, targets, u_full, x0, max_iter: int = EQ_MAX_ITER,
                 tol_f: float = EQ_TOL, tol_y: float = TARGET_TOL_Y):
    """Steady states with given outputs for B scenarios on the host (no
    device): the state and the free control inputs (columns
    `free` of B: 0 and 2 the torques, 1 and 3 the recycle valves) at which
    f(x, u, p) = 0 and the plant outputs `hold` equal `targets` ((nh,) or
    (B, nh)), by Newton's method from x0 (B, ns) and u_full (B, n_inputs).
    Returns (x, u, status, iters, resid): x and u hold the solution where
    status is CMPC_EQ_OK and the rows given elsewhere, resid (B, 2) is
    (max|f|, max|y - t|); the arithmetic is PlantSimulator.target's, bit for
    bit."""
    lib = load_library()
    ns, ni = _plant_sizes(lib, plant)
    h, f = _target_indices(lib, plant, hold, free, max_iter, tol_f, tol_y)
    x = np.array(x0, dtype=np.float64, order="C")
    B = x.shape[0] if x.ndim == 2 else 0
    p = np.ascontiguousarray(pressures, np.float64)
    u = np.array(u_full, dtype=np.float64, order="C")
    if B < 1 or x.shape != (B, ns) or p.shape != (B, 2) or u.shape != (B, ni):
        raise ValueError(f"x0 must be (B, {ns}), pressures (B, 2) and u_full (B, {ni}), "
                         f"got {x.shape}, {p.shape} and {u.shape}")
    t = _target_array(targets, B, len(h))
    status, iters, resid = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros((B, 2))
    check(lib.cmpc_plant_target_host(plant, B, dptr(p), len(h), iptr(h), iptr(f), dptr(t), dptr(u), dptr(x), max_iter,
                                     tol_f, tol_y, iptr(status), iptr(iters), dptr(resid)), "cmpc_plant_target_host")
    return x, u, status, iters, resid


# plant_gains, PlantSimulator.gains, ClosedLoop.gains: the record of
# include/cmpc.h sliced to the selection, and the raw record (B, CMPC_GAIN_LEN)
PlantGains = collections.namedtuple("PlantGains", ("G", "Gp", "rga", "k_ff", "resid", "status", "record"))


def _gain_indices(lib, plant: int, outputs, inputs):
    """outputs and inputs as int32 arrays, checked by cmpc_gain_check."""
    o = np.ascontiguousarray(outputs, np.int32).reshape(-1)
    i = np.ascontiguousarray(inputs, np.int32).reshape(-1)
    check(lib.cmpc_gain_check(plant, len(o), iptr(o), len(i), iptr(i)), "cmpc_gain_check")
    return o, i


def _gain_result(record, status, ny: int, nu: int) -> "PlantGains":
    """The record's blocks, sliced to ny and nu (views of the record)."""
    B = record.shape[0]
    return PlantGains(G=record[:, 0:16].reshape(B, 4, 4)[:, :ny, :nu],
                      Gp=record[:, 16:24].reshape(B, 4, 2)[:, :ny],
                      rga=record[:, 24:40].reshape(B, 4, 4)[:, :ny, :nu],
                      k_ff=record[:, 40:48].reshape(B, 4, 2)[:, :nu],
                      resid=record[:, 48], status=status, record=record)


def plant_gains(plant: int, pressures, u_full, x, outputs, inputs=(0, 2)) -> "PlantGains":
    """Steady-state gains for B scenarios on the host (no device, DESIGN.md
    §3.22): at x (B, ns), u_full (B, n_inputs) and pressures (B, 2), the map
    from the control inputs `inputs` (columns of B: 0 and 2 the torques, 1
    and 3 the recycle valves) and from (p_in, p_out) to the plant outputs
    `outputs`.  Returns a PlantGains record: G (B, ny, nu) = dy/du, Gp
    (B, ny, 2) = dy/dp, and for ny == nu the relative gain array rga
    (B, n, n) and the feed-forward k_ff (B, n, 2) = du/dp that holds the
    outputs (NaN otherwise), resid (B,) = max|f| at x (the gains are
    steady-state gains where it is ~ 0), status (B,) and the raw record
    (B, CMPC_GAIN_LEN); everything is NaN where status is neither CMPC_EQ_OK
    nor CMPC_GAIN_SINGULAR_G.  The arithmetic is PlantSimulator.gains', bit
    for bit."""
    lib = load_library()
    ns, ni = _plant_sizes(lib, plant)
    o, i = _gain_indices(lib, plant, outputs, inputs)
    xs = np.ascontiguousarray(x, np.float64)
    B = xs.shape[0] if xs.ndim == 2 else 0
    p = np.ascontiguousarray(pressures, np.float64)
    u = np.ascontiguousarray(u_full, np.float64)
    if B < 1 or xs.shape != (B, ns) or p.shape != (B, 2) or u.shape != (B, ni):
        raise ValueError(f"x must be (B, {ns}), pressures (B, 2) and u_full (B, {ni}), "
                         f"got {xs.shape}, {p.shape} and {u.shape}")
    record, status = np.zeros((B, CMPC_GAIN_LEN)), np.zeros(B, np.int32)
    check(lib.cmpc_plant_gains_host(plant, B, dptr(p), dptr(u), dptr(xs), len(o), iptr(o), len(i), iptr(i),
                                    dptr(record), iptr(status)), "cmpc_plant_gains_host")
    return _gain_result(record, status, len(o), len(i))


def _complex(wr, wi) -> np.ndarray:
    """wr + i wi with both parts kept bit for bit (a NaN's pattern included)."""
    w = np.empty(wr.shape, np.complex128)
    w.real, w.imag = wr, wi
    return w


# plant_freq_response, freq_response, PlantSimulator.freq_response,
# ClosedLoop.freq_response: the record and the summary of include/cmpc.h sliced
# to the selection, and both raw (B, nw, CMPC_FREQ_LEN) and (B, CMPC_FREQ_NSUM)
FreqResponse = collections.namedtuple("FreqResponse", ("G", "Gp", "peak", "peak_omega", "peak_p", "peak_p_omega",
                                                       "omega", "resid", "status", "record", "summary"))


def _freq_list(omega) -> np.ndarray:
    """omega as a float64 array (nw,); cmpc_freq_check has the rules."""
    return np.ascontiguousarray(omega, np.float64).reshape(-1)


def _freq_result(record, summary, status, omega, ny: int, nu: int) -> "FreqResponse":
    """The blocks of the record and the summary, sliced to ny and nu; the
    parts of G and Gp are kept bit for bit (a NaN's pattern included)."""
    B, nw = record.shape[:2]
    pairs = record.reshape(B, nw, CMPC_FREQ_LEN // 2, 2)
    z = _complex(pairs[..., 0], pairs[..., 1])
    m2, idx = summary[:, 0:24], summary[:, 24:48]
    with np.errstate(invalid="ignore"):
        peak = np.sqrt(m2)
    at = np.full(idx.shape, np.nan)
    have = ~np.isnan(idx)
    at[have] = omega[idx[have].astype(np.int64)]
    return FreqResponse(G=z[:, :, 0:16].reshape(B, nw, 4, 4)[:, :, :ny, :nu],
                        Gp=z[:, :, 16:24].reshape(B, nw, 4, 2)[:, :, :ny],
                        peak=peak[:, 0:16].reshape(B, 4, 4)[:, :ny, :nu],
                        peak_omega=at[:, 0:16].reshape(B, 4, 4)[:, :ny, :nu],
                        peak_p=peak[:, 16:24].reshape(B, 4, 2)[:, :ny],
                        peak_p_omega=at[:, 16:24].reshape(B, 4, 2)[:, :ny],
                        omega=omega, resid=summary[:, 48], status=status, record=record, summary=summary)


def plant_freq_response(plant: int, pressures, u_full, x, omega, outputs, inputs=(0, 2)) -> "FreqResponse":
    """The plant's frequency responses for B scenarios on the host (no device,
    DESIGN.md §3.23): at x (B, ns), u_full (B, n_inputs) and pressures (B, 2),
    the response of the linearisation from the control inputs `inputs` (columns
    of B: 0 and 2 the torques, 1 and 3 the recycle valves) and from (p_in,
    p_out) to the plant outputs `outputs` at the frequencies `omega` (rad/s,
    at most 64, each finite and >= 0, any order).  Returns a FreqResponse
    record: G (B, nw, ny, nu) and Gp (B, nw, ny, 2) complex, peak (B, ny, nu)
    = max_k |G| with peak_omega the frequency it was found at (the first of
    equal ones), peak_p and peak_p_omega (B, ny, 2) the same for Gp, omega,
    resid (B,) = max|f| at x, status (B,), and the raw record (B, nw,
    CMPC_FREQ_LEN) and summary (B, CMPC_FREQ_NSUM); everything of a scenario is
    NaN where its status is not CMPC_EQ_OK.  The arithmetic is
    PlantSimulator.freq_response's, bit for bit."""
    lib = load_library()
    ns, ni = _plant_sizes(lib, plant)
    o = np.ascontiguousarray(outputs, np.int32).reshape(-1)
    i = np.ascontiguousarray(inputs, np.int32).reshape(-1)
    w = _freq_list(omega)
    check(lib.cmpc_freq_check(plant, len(o), iptr(o), len(i), iptr(i), len(w), dptr(w)), "cmpc_freq_check")
    xs = np.ascontiguousarray(x, np.float64)
    B = xs.shape[0] if xs.ndim == 2 else 0
    p = np.ascontiguousarray(pressures, np.float64)
    u = np.ascontiguousarray(u_full, np.float64)
    if B < 1 or xs.shape != (B, ns) or p.shape != (B, 2) or u.shape != (B, ni):
        raise ValueError(f"x must be (B, {ns}), pressures (B, 2) and u_full (B, {ni}), "
                         f"got {xs.shape}, {p.shape} and {u.shape}")
    record, summary = np.zeros((B, len(w), CMPC_FREQ_LEN)), np.zeros((B, CMPC_FREQ_NSUM))
    status = np.zeros(B, np.int32)
    check(lib.cmpc_plant_freq_host(plant, B, dptr(p), dptr(u), dptr(xs), len(o), iptr(o), len(i), iptr(i), len(w),
                                   dptr(w), dptr(record), dptr(summary), iptr(status)), "cmpc_plant_freq_host")
    return _freq_result(record, summary, status, w, len(o), len(i))


def freq_response(A, B, C, E, omega) -> "FreqResponse":
    """C (j w I - A)^-1 [B | E] of matrices given, on the host (cmpc_freq_host,
    the arithmetic of plant_freq_response from the balancing on): A (n, n), B
    (n, nu), C (ny, n), E (n, 2), 1 <= n <= 12, ny and nu in [1, 4], or each
    with a leading batch axis.  Returns a FreqResponse record (resid is 0)."""
    a = np.asarray(A, np.float64)
    single = a.ndim == 2
    a, b, c, e = (np.asarray(m, np.float64)[None] if single else np.asarray(m, np.float64) for m in (A, B, C, E))
    if a.ndim != 3 or b.ndim != 3 or c.ndim != 3 or e.ndim != 3:
        raise ValueError("A, B, C and E must all be matrices or all carry one batch axis")
    nb, n = a.shape[:2]
    nu, ny = b.shape[2], c.shape[1]
    if (nb < 1 or not 1 <= n <= CMPC_FREQ_MAX_N or a.shape != (nb, n, n) or b.shape != (nb, n, nu)
            or c.shape != (nb, ny, n) or e.shape != (nb, n, 2) or not 1 <= nu <= 4 or not 1 <= ny <= 4):
        raise ValueError(f"A must be (n, n) with 1 <= n <= {CMPC_FREQ_MAX_N}, B (n, nu), C (ny, n) and E (n, 2) with "
                         f"ny and nu in [1, 4], got {a.shape}, {b.shape}, {c.shape} and {e.shape}")
    b4, c4 = np.zeros((nb, n, 4)), np.zeros((nb, 4, n))
    b4[:, :, :nu], c4[:, :ny] = b, c
    a, e = np.ascontiguousarray(a), np.ascontiguousarray(e)
    w = _freq_list(omega)
    record, summary = np.zeros((nb, max(len(w), 1), CMPC_FREQ_LEN)), np.zeros((nb, CMPC_FREQ_NSUM))
    status = np.zeros(nb, np.int32)
    check(load_library().cmpc_freq_host(n, nb, dptr(a), dptr(b4), dptr(c4), dptr(e), ny, nu, len(w),
                                        dptr(w) if len(w) else None, dptr(record), dptr(summary), iptr(status)),
          "cmpc_freq_host")
    return _freq_result(record, summary, status, w, ny, nu)


def _eig_iter(max_iter, n: int) -> int:
    """The QR sweeps allowed per matrix: 30 n unless given."""
    return 30 * n if max_iter is None else int(max_iter)


def eig_batch(A, max_iter=None):
    """Eigenvalues of B real n x n matrices, 1 <= n <= 12, on the host
    (cmpc_eig_host, no device): A (B, n, n).  Returns (w, status, iters): w
    (B, n) complex128 ordered by real part descending, then imaginary part
    descending (NaN where status is not CMPC_EIG_OK), status and iters (B,)
    int32.  max_iter: QR sweeps allowed per matrix (default 30 n)."""
    a = np.ascontiguousarray(A, np.float64)
    if a.ndim != 3 or a.shape[0] < 1 or a.shape[1] != a.shape[2] or not 1 <= a.shape[1] <= CMPC_EIG_MAX_N:
        raise ValueError(f"A must be (B, n, n) with B >= 1 and 1 <= n <= {CMPC_EIG_MAX_N}, got {a.shape}")
    B, n = a.shape[:2]
    wr, wi = np.zeros((B, n)), np.zeros((B, n))
    status, iters = np.zeros(B, np.int32), np.zeros(B, np.int32)
    check(load_library().cmpc_eig_host(n, B, dptr(a), _eig_iter(max_iter, n), dptr(wr), dptr(wi), iptr(status),
                                       iptr(iters)), "cmpc_eig_host")
    return _complex(wr, wi), status, iters


def eig_batch_device(A, max_iter=None):
    """eig_batch on the device (cmpc_eig_device, one launch on torch's current
    stream): A a contiguous float64 device tensor (B, n, n), n = 10 or 11.
    Returns (wr, wi, status, iters) as device tensors ((B, n) float64 twice,
    (B,) int32 twice); the arithmetic is eig_batch's, bit for bit."""
    import torch
    if (not isinstance(A, torch.Tensor) or A.dim() != 3 or A.shape[0] < 1 or A.shape[1] != A.shape[2]
            or A.shape[1] not in (10, 11) or A.dtype != torch.float64 or not A.is_cuda or not A.is_contiguous()):
        raise ValueError("A must be a contiguous float64 device tensor (B, n, n) with n = 10 or 11")
    B, n = int(A.shape[0]), int(A.shape[1])
    wr, wi = torch.zeros(B, n, dtype=torch.float64, device=A.device), torch.zeros(B, n, dtype=torch.float64,
                                                                                  device=A.device)
    status = torch.zeros(B, dtype=torch.int32, device=A.device)
    iters = torch.zeros(B, dtype=torch.int32, device=A.device)
    vp = ctypes.c_void_p
    with torch.cuda.device(A.device):
        check(load_library().cmpc_eig_device(n, B, vp(A.data_ptr()), _eig_iter(max_iter, n), vp(wr.data_ptr()),
                                             vp(wi.data_ptr()), vp(status.data_ptr()), vp(iters.data_ptr()),
                                             vp(torch.cuda.current_stream(A.device).cuda_stream)),
              "cmpc_eig_device")
    return wr, wi, status, iters


def modes_summary(w, status) -> np.ndarray:
    """(B, 6): the summary of include/cmpc.h (_abi.MODES_SUMMARY names the
    columns) of ordered eigenvalues w (B, n) complex, NaN where status is not
    CMPC_EIG_OK (cmpc_modes_summary_host)."""
    w = np.asarray(w, np.complex128)
    st = np.ascontiguousarray(status, np.int32)
    if w.ndim != 2 or w.shape[0] < 1 or not 1 <= w.shape[1] <= CMPC_EIG_MAX_N or st.shape != (w.shape[0],):
        raise ValueError(f"w must be (B, n) with 1 <= n <= {CMPC_EIG_MAX_N} and status (B,), got {w.shape} and "
                         f"{st.shape}")
    wr, wi = np.ascontiguousarray(w.real), np.ascontiguousarray(w.imag)
    out = np.zeros((w.shape[0], CMPC_MODES_NSUM))
    check(load_library().cmpc_modes_summary_host(w.shape[1], w.shape[0], dptr(wr), dptr(wi), iptr(st), dptr(out)),
          "cmpc_modes_summary_host")
    return out


def plant_modes(plant: int, pressures, u_full, x, max_iter=None):
    """The plant's modes for B scenarios on the host (no device): the
    eigenvalues of the continuous Jacobian df/dx at x (B, ns) under pressures
    (B, 2) and the plant input u_full (B, n_inputs).  Returns (w, summary,
    status, iters): w (B, ns) complex128 in eig_batch's order, summary (B, 6)
    (_abi.MODES_SUMMARY names the columns); the arithmetic is
    PlantSimulator.modes', bit for bit."""
    lib = load_library()
    ns, ni = _plant_sizes(lib, plant)
    xs = np.ascontiguousarray(x, np.float64)
    B = xs.shape[0] if xs.ndim == 2 else 0
    p = np.ascontiguousarray(pressures, np.float64)
    u = np.ascontiguousarray(u_full, np.float64)
    if B < 1 or xs.shape != (B, ns) or p.shape != (B, 2) or u.shape != (B, ni):
        raise ValueError(f"x must be (B, {ns}), pressures (B, 2) and u_full (B, {ni}), "
                         f"got {xs.shape}, {p.shape} and {u.shape}")
    wr, wi, sm = np.zeros((B, ns)), np.zeros((B, ns)), np.zeros((B, CMPC_MODES_NSUM))
    status, iters = np.zeros(B, np.int32), np.zeros(B, np.int32)
    check(lib.cmpc_plant_modes_host(plant, B, dptr(p), dptr(u), dptr(xs), _eig_iter(max_iter, ns), dptr(wr), dptr(wi),
                                    dptr(sm), iptr(status), iptr(iters)), "cmpc_plant_modes_host")
    return _complex(wr, wi), sm, status, iters


class PlantSimulator:
    """SimulationSystem for B scenarios of one plant (0 parallel, 1 serial)."""

    def __init__(self, plant: int, B: int, device: int = 0, p_in: float = 1.0, p_out: float = 1.0,
                 delays=REF_DELAYS, control_index=REF_CONTROL_INDEX):
        import torch
        self.torch = torch
        self.lib = load_library()
        self.plant, self.B, self.device = plant, B, device
        ns, ni, no, nci = (ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int())
        check(self.lib.cmpc_plant_dims(plant, ctypes.byref(ns), ctypes.byref(ni), ctypes.byref(no),
                                       ctypes.byref(nci)), "cmpc_plant_dims")
        self.ns, self.ni, self.no = ns.value, ni.value, no.value
        self.nc = len(delays)
        d = np.ascontiguousarray(delays, dtype=np.int32)
        ci = np.ascontiguousarray(control_index, dtype=np.int32)
        if torch.cuda.is_available():
            torch.cuda.init()  # torch's HIP runtime before the library's
        self._h = ctypes.c_void_p()
        check(self.lib.cmpc_sim_create(ctypes.byref(self._h), plant, B, device, p_in, p_out, self.nc,
                                       d.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                       ci.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))),
              "cmpc_sim_create")
        self.y = torch.zeros(B, self.no, dtype=torch.float64, device=f"cuda:{device}")
        # the caller's tensors are written on torch's stream: run there too
        self.set_stream(torch.cuda.current_stream(device).cuda_stream)

    def close(self):
        if self._h:
            self.lib.cmpc_sim_destroy(self._h)
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

    def set_stream(self, stream_ptr: int):
        check(self.lib.cmpc_sim_set_stream(self._h, ctypes.c_void_p(stream_ptr)), "cmpc_sim_set_stream")

    def reset(self, x0, u_offset, dt0: float = REF_TS):
        """x0 (B, ns), u_offset (B, n_inputs): device tensors (float64)."""
        check(self.lib.cmpc_sim_reset(self._h, ctypes.c_void_p(x0.data_ptr()),
                                      ctypes.c_void_p(u_offset.data_ptr()), dt0), "cmpc_sim_reset")

    def set_input(self, u_control):
        """SetInput: u_control (B, n_control) device tensor through the delay line."""
        check(self.lib.cmpc_sim_set_input(self._h, ctypes.c_void_p(u_control.data_ptr())),
              "cmpc_sim_set_input")

    def set_offset(self, u_offset):
        """SetOffset: u_offset (B, n_inputs) device tensor; the plant input
        changes with the next set_input."""
        check(self.lib.cmpc_sim_set_offset(self._h, ctypes.c_void_p(u_offset.data_ptr())),
              "cmpc_sim_set_offset")

    def set_pressures(self, pressures=None):
        """Per-scenario boundary pressures of the plant, (B, 2) of [p_in,
        p_out], read by every later integrate in place of the constructor's
        scalars: a host array (checked finite and positive) or a device
        tensor (copied, not checked).  None restores the scalars."""
        if pressures is None:
            check(self.lib.cmpc_sim_set_pressures(self._h, None), "cmpc_sim_set_pressures")
            return
        if isinstance(pressures, self.torch.Tensor):
            if (tuple(pressures.shape) != (self.B, 2) or pressures.dtype != self.torch.float64
                    or not pressures.is_cuda or not pressures.is_contiguous()):
                raise ValueError(f"pressures must be a contiguous float64 device tensor (B = {self.B}, 2)")
            check(self.lib.cmpc_sim_set_pressures(self._h, ctypes.c_void_p(pressures.data_ptr())),
                  "cmpc_sim_set_pressures")
            return
        p = np.ascontiguousarray(pressures, np.float64)
        if p.shape != (self.B, 2):
            raise ValueError(f"pressures must be (B = {self.B}, 2), got {p.shape}")
        check(self.lib.cmpc_sim_set_pressures_host(self._h, p.ctypes.data_as(ctypes.POINTER(ctypes.c_double))),
              "cmpc_sim_set_pressures_host")

    def bind_pressures(self, device_ptr: int = 0):
        """Bind a device-resident (B, 2) f64 array of [p_in, p_out] (16-byte
        aligned), read in place by each integrate: the caller may rewrite it
        between intervals.  0 restores the scalars."""
        check(self.lib.cmpc_sim_bind_pressures(self._h, ctypes.c_void_p(device_ptr or None)),
              "cmpc_sim_bind_pressures")

    def get_pressures(self) -> np.ndarray:
        """(B, 2): the pressures the next integrate uses."""
        out = np.zeros((self.B, 2))
        check(self.lib.cmpc_sim_get_pressures(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))),
              "cmpc_sim_get_pressures")
        return out

    def restart(self, dt0: float = REF_TS):
        """A new Integrate call: the carried step size starts again at dt0."""
        check(self.lib.cmpc_sim_restart(self._h, dt0), "cmpc_sim_restart")

    def plant_input_offset(self, u_control, u_offset, out):
        """GetPlantInput over a given offset (the controller's u_offset_)."""
        check(self.lib.cmpc_sim_plant_input_offset(self._h, ctypes.c_void_p(u_control.data_ptr()),
                                                   ctypes.c_void_p(u_offset.data_ptr()),
                                                   ctypes.c_void_p(out.data_ptr())),
              "cmpc_sim_plant_input_offset")

    def plant_input(self, u_control, out):
        """GetPlantInput without the delay line into out (B, n_inputs)."""
        check(self.lib.cmpc_sim_plant_input(self._h, ctypes.c_void_p(u_control.data_ptr()),
                                            ctypes.c_void_p(out.data_ptr())), "cmpc_sim_plant_input")

    def integrate(self, t: float, t_end: float, eps_abs: float = REF_EPS, eps_rel: float = REF_EPS):
        check(self.lib.cmpc_sim_integrate(self._h, t, t_end, eps_abs, eps_rel), "cmpc_sim_integrate")

    def equilibrium(self, max_iter: int = EQ_MAX_ITER, tol: float = EQ_TOL):
        """Move every scenario to its plant equilibrium f(x, u, p) = 0 by
        Newton's method from its current state, at its current plant input and
        the pressures in force (one launch; the step sizes and the delay lines
        stay).  Returns (status, iters, resid), (B,) host arrays: the state of
        a scenario whose status is not CMPC_EQ_OK is left as it was."""
        check(self.lib.cmpc_sim_equilibrium(self._h, max_iter, tol), "cmpc_sim_equilibrium")
        status, iters, resid = np.zeros(self.B, np.int32), np.zeros(self.B, np.int32), np.zeros(self.B)
        check(self.lib.cmpc_sim_equilibrium_download(self._h, iptr(status), iptr(iters), dptr(resid)),
              "cmpc_sim_equilibrium_download")
        return status, iters, resid

    def target(self, hold, free, targets, max_iter: int = EQ_MAX_ITER, tol_f: float = EQ_TOL,
               tol_y: float = TARGET_TOL_Y):
        """Move every scenario to the steady state at which its plant outputs
        `hold` equal `targets` ((nh,) or (B, nh) host array, or a contiguous
        float64 device tensor (B, nh)), solving for the state and the control
        inputs `free` (plant_target has the meaning of both) from its current
        state and plant input at the pressures in force: one launch.  Where
        the status is CMPC_EQ_OK the state, the free entries of the plant input
        and those of the input offset are written; a scenario with any other
        status is left as it was, and the step sizes and the delay lines stay.
        Returns (status, iters, resid), host arrays (B,), (B,), (B, 2)."""
        h, f = _target_indices(self.lib, self.plant, hold, free, max_iter, tol_f, tol_y)
        nh = len(h)
        if isinstance(targets, self.torch.Tensor):
            if (tuple(targets.shape) != (self.B, nh) or targets.dtype != self.torch.float64 or not targets.is_cuda
                    or not targets.is_contiguous()):
                raise ValueError(f"targets must be a contiguous float64 device tensor (B = {self.B}, {nh})")
            check(self.lib.cmpc_sim_target(self._h, nh, iptr(h), iptr(f), ctypes.c_void_p(targets.data_ptr()),
                                           max_iter, tol_f, tol_y), "cmpc_sim_target")
        else:
            t = _target_array(targets, self.B, nh)
            check(self.lib.cmpc_sim_target_host(self._h, nh, iptr(h), iptr(f), dptr(t), max_iter, tol_f, tol_y),
                  "cmpc_sim_target_host")
        status, iters, resid = np.zeros(self.B, np.int32), np.zeros(self.B, np.int32), np.zeros((self.B, 2))
        check(self.lib.cmpc_sim_target_download(self._h, iptr(status), iptr(iters), dptr(resid)),
              "cmpc_sim_target_download")
        return status, iters, resid

    def download_inputs(self):
        """Host copies: (input offset (B, n_inputs), delay line (slots, B))."""
        off = np.zeros((self.B, self.ni))
        ring = np.zeros((self.lib.cmpc_sim_delay_len(self._h), self.B))
        check(self.lib.cmpc_sim_download_inputs(self._h, dptr(off), dptr(ring)), "cmpc_sim_download_inputs")
        return off, ring

    def gains(self, outputs, inputs=(0, 2)) -> "PlantGains":
        """The steady-state gains, relative gain array and pressure
        feed-forward at every scenario's current state, plant input and the
        pressures in force (one launch; nothing of the simulator is written).
        Returns what plant_gains returns, bit for bit; a scenario whose
        simulator status is nonzero reports CMPC_EQ_SKIPPED with NaN."""
        o, i = _gain_indices(self.lib, self.plant, outputs, inputs)
        check(self.lib.cmpc_sim_gains(self._h, len(o), iptr(o), len(i), iptr(i)), "cmpc_sim_gains")
        record, status = np.zeros((self.B, CMPC_GAIN_LEN)), np.zeros(self.B, np.int32)
        check(self.lib.cmpc_sim_gains_download(self._h, dptr(record), iptr(status)), "cmpc_sim_gains_download")
        return _gain_result(record, status, len(o), len(i))

    def freq_response(self, omega, outputs, inputs=(0, 2)) -> "FreqResponse":
        """The plant's frequency responses at every scenario's current state,
        plant input and the pressures in force, at the frequencies `omega`
        shared by all scenarios (one launch; nothing of the simulator is
        written).  Returns what plant_freq_response returns, bit for bit; a
        scenario whose simulator status is nonzero reports CMPC_EQ_SKIPPED with
        NaN."""
        o = np.ascontiguousarray(outputs, np.int32).reshape(-1)
        i = np.ascontiguousarray(inputs, np.int32).reshape(-1)
        w = _freq_list(omega)
        check(self.lib.cmpc_sim_freq(self._h, len(o), iptr(o), len(i), iptr(i), len(w), dptr(w) if len(w) else None),
              "cmpc_sim_freq")
        record, summary = np.zeros((self.B, len(w), CMPC_FREQ_LEN)), np.zeros((self.B, CMPC_FREQ_NSUM))
        status = np.zeros(self.B, np.int32)
        check(self.lib.cmpc_sim_freq_download(self._h, dptr(record), dptr(summary), iptr(status)),
              "cmpc_sim_freq_download")
        return _freq_result(record, summary, status, w, len(o), len(i))

    def modes(self, max_iter=None):
        """The plant's modes at every scenario's current state, plant input
        and the pressures in force (one launch; nothing of the simulator is
        written): the eigenvalues of the continuous Jacobian df/dx.  Returns
        (w, summary, status, iters) as plant_modes does; a scenario whose
        simulator status is nonzero reports CMPC_EIG_SKIPPED with NaN."""
        check(self.lib.cmpc_sim_modes(self._h, _eig_iter(max_iter, self.ns)), "cmpc_sim_modes")
        wr, wi, sm = np.zeros((self.B, self.ns)), np.zeros((self.B, self.ns)), np.zeros((self.B, CMPC_MODES_NSUM))
        status, iters = np.zeros(self.B, np.int32), np.zeros(self.B, np.int32)
        check(self.lib.cmpc_sim_modes_download(self._h, dptr(wr), dptr(wi), dptr(sm), iptr(status), iptr(iters)),
              "cmpc_sim_modes_download")
        return _complex(wr, wi), sm, status, iters

    def output(self, out=None):
        """GetOutput into out (B, n_outputs) (default: self.y)."""
        out = self.y if out is None else out
        check(self.lib.cmpc_sim_output(self._h, ctypes.c_void_p(out.data_ptr())), "cmpc_sim_output")
        return out

    def synchronize(self):
        check(self.lib.cmpc_sim_synchronize(self._h), "cmpc_sim_synchronize")

    def download(self):
        """Host copies: (x (B, ns), plant input (B, n_inputs), step size (B,), status (B,))."""
        x = np.zeros((self.B, self.ns))
        u = np.zeros((self.B, self.ni))
        dt = np.zeros(self.B)
        st = np.zeros(self.B, np.int32)
        P = ctypes.POINTER
        check(self.lib.cmpc_sim_download(self._h, x.ctypes.data_as(P(ctypes.c_double)),
                                         u.ctypes.data_as(P(ctypes.c_double)),
                                         dt.ctypes.data_as(P(ctypes.c_double)),
                                         st.ctypes.data_as(P(ctypes.c_int32))), "cmpc_sim_download")
        return x, u, dt, st

    def state_ptr(self) -> int:
        return self.lib.cmpc_sim_state(self._h)

    def input_ptr(self) -> int:
        return self.lib.cmpc_sim_input(self._h)

    def status_ptr(self) -> int:
        """Device address of the (B,) int32 status words (cmpc_sim_status)."""
        return self.lib.cmpc_sim_status(self._h)
