// The context's life, configuration and bound or per-slot arrays
// (include/cmpc.h): create, destroy, stream, weights, constraints, reference,
// state, records, every cmpc_*_scenario_*, kernel variants, timing.
#include "abi_ctx.h"

#include <algorithm>
#include <cmath>

using namespace cmpc_abi;

thread_local LaunchEvents cmpc_launch_events;

namespace cmpc_abi {

int rebuild_cfg(cmpc_ctx* c) {
  const cmpc_dims& d = c->d;
  const int S = d.S, ny = d.ny, nu = d.nu, p = d.p;
  for (int s = 0; s < S; ++s)
    if (!c->have_w[s] || !c->have_c[s] || !c->have_r[s])
      return fail("sub-controller " + std::to_string(s) +
                  ": weights, constraints and reference must all be set before the step");
  c->h_cfg.assign((size_t)S * c->co.len, 0.0);
  for (int s = 0; s < S; ++s) {
    double* b = c->h_cfg.data() + (size_t)s * c->co.len;
    // lwt = L_W' (upper triangular) with ywt = L_W L_W' (cmpc_weight_factor)
    double* lwt = b + c->co.lwt;
    if (const char* e = cmpc_weight_factor_error(ny, c->ywt.data() + (size_t)s * ny * ny, lwt)) return fail(e);
    // yhat = L_W' y_ref (the build kernel's per-slot-weights instances repeat
    // this order: from 0, ascending o2, a product then a sum)
    const double* yr = c->yref.data() + (size_t)s * p * ny;
    for (int r = 0; r < p; ++r)
      for (int o = 0; o < ny; ++o) {
        double v = 0;
        for (int o2 = o; o2 < ny; ++o2) v += lwt[o * ny + o2] * yr[r * ny + o2];
        b[c->co.yhat + r * ny + o] = v;
      }
    std::memcpy(b + c->co.uwt, c->uwt.data() + (size_t)s * nu * nu, sizeof(double) * nu * nu);
    std::memcpy(b + c->co.lower, c->lower.data() + (size_t)s * nu, sizeof(double) * nu);
    std::memcpy(b + c->co.upper, c->upper.data() + (size_t)s * nu, sizeof(double) * nu);
    std::memcpy(b + c->co.rlower, c->rlower.data() + (size_t)s * nu, sizeof(double) * nu);
    std::memcpy(b + c->co.rupper, c->rupper.data() + (size_t)s * nu, sizeof(double) * nu);
  }
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(c->cfg, c->h_cfg.data(), sizeof(double) * c->h_cfg.size(),
                         hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->cfg_dirty = false;
  return 0;
}

int bound_array_check(cmpc_ctx* c, const void* dev, const char* who, size_t n, const char* words) {
  if (!device_ptr_ok(c, dev, sizeof(double) * n))
    return fail(std::string(who) + ": not a device allocation of " + words + " doubles on the context's device");
  if (reinterpret_cast<uintptr_t>(dev) % 8) return fail(std::string(who) + ": misaligned array");
  return 0;
}

}  // namespace cmpc_abi

namespace {

int resolve_timing(cmpc_ctx* c) {
  for (int k = 0; k < CMPC_KERNEL_COUNT; ++k) {
    for (auto& pr : c->pending[k]) {
      HIP_TRY(hipEventSynchronize(pr.second));
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, pr.first, pr.second));
      c->tot_ms[k] += ms;
      c->event_pool.push_back(pr.first);
      c->event_pool.push_back(pr.second);
    }
    c->pending[k].clear();
  }
  return 0;
}

// A per-slot array of the context (setpoint offsets, limits, reference
// profile, weights, pressures): the pointer in force (null: none) and the
// context's own buffer, allocated by the first upload.  The host setters stage
// into the own buffer the way cmpc_set_state does; the bind variants check the
// pointer the way cmpc_bind_state does.  What a family checks of its values,
// and what it marks stale, stays in the family's functions.
struct SlotArray {
  const double*& use;
  double*& own;
};

int slot_upload(cmpc_ctx* c, SlotArray a, const double* host, size_t n) {
  HIP_TRY(hipSetDevice(c->device));
  if (ensure_device(&a.own, sizeof(double) * n)) return -1;
  HIP_TRY(hipMemcpyAsync(a.own, host, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  a.use = a.own;
  return 0;
}

// dev: n doubles on the device, or null (nothing in force)
int slot_bind(cmpc_ctx* c, SlotArray a, const double* dev, const char* who, size_t n, const char* words) {
  if (dev && bound_array_check(c, dev, who, n, words)) return -1;
  a.use = dev;
  return 0;
}

int slot_get(cmpc_ctx* c, SlotArray a, double* host, size_t n) {
  HIP_TRY(hipSetDevice(c->device));
  return direct_download(c->stream, {{a.use, host, sizeof(double) * n}});
}

SlotArray slot_dy(cmpc_ctx* c) { return {c->sc_dy, c->own_sc_dy}; }
SlotArray slot_limits(cmpc_ctx* c) { return {c->sc_limits, c->own_sc_limits}; }
SlotArray slot_dref(cmpc_ctx* c) { return {c->sc_dref, c->own_sc_dref}; }
SlotArray slot_w(cmpc_ctx* c) { return {c->sc_w, c->own_sc_w}; }
SlotArray slot_p(cmpc_ctx* c) { return {c->sc_p, c->own_sc_p}; }

const char* const kStaleProfile =
    "the reference profile has changed since the build (cmpc_set/bind_scenario_reference_profile)";
const char* const kNoProfileKernel =
    ": reference-profile kernel not instantiated for these dimensions (ns, ny, nu, m)";
const char* const kStaleWeights =
    "the per-scenario weights have changed since the build (cmpc_set/bind_scenario_weights)";

int scenario_weights_refused(cmpc_ctx* c, const char* who) {
  ensure_bp(c);
  if (c->bp_error || !cmpc_build_weights_available(c->d, c->bp))
    return fail(std::string(who) + ": " + cmpc_plan_error_string(CMPC_PLAN_NO_WEIGHTS_BUILD));
  return 0;
}

}  // namespace

extern "C" {

int cmpc_create(cmpc_ctx** out, const cmpc_dims* dims, int device) {
  if (!out || !dims) return fail("null argument");
  *out = nullptr;
  cmpc_layout L;
  if (layout_of(dims, &L)) return -1;
  const cmpc_dims& d = *dims;
  if (const char* e = cmpc_context_dims_error(d, L)) return fail(e);
  const long long nqp = (long long)d.B * d.S;
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail("no such HIP device");
  cmpc_ctx* c = new cmpc_ctx();
  c->d = d;
  c->L = L;
  c->device = device;
  c->nqp = (int)nqp;
  c->qp_len = cmpc_qp_len(L);
  int off = 0;
  c->co.lwt = off; off += d.ny * d.ny;
  c->co.yhat = off; off += d.p * d.ny;
  c->co.uwt = off; off += d.nu * d.nu;
  c->co.lower = off; off += d.nu;
  c->co.upper = off; off += d.nu;
  c->co.rlower = off; off += d.nu;
  c->co.rupper = off; off += d.nu;
  c->co.len = (off + 1) / 2 * 2;
  const int S = d.S;
  c->ywt.assign((size_t)S * d.ny * d.ny, 0);
  c->uwt.assign((size_t)S * d.nu * d.nu, 0);
  c->yref.assign((size_t)S * d.p * d.ny, 0);
  c->lower.assign((size_t)S * d.nu, 0);
  c->upper.assign((size_t)S * d.nu, 0);
  c->rlower.assign((size_t)S * d.nu, 0);
  c->rupper.assign((size_t)S * d.nu, 0);
  c->have_w.assign(S, 0);
  c->have_c.assign(S, 0);
  c->have_r.assign(S, 0);
  auto cleanup = [&](int rc) {
    cmpc_destroy(c);
    return rc;
  };
  if (hipSetDevice(device) != hipSuccess) return cleanup(fail("hipSetDevice failed"));
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess)
    return cleanup(fail("hipStreamCreate failed"));
  if (hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || c->cus < 1)
    c->cus = kCusFallback;
  c->own_stream = true;
  const size_t n = (size_t)c->nqp;
  if (hipMalloc(&c->lin, sizeof(double) * n * L.rec_len) != hipSuccess ||
      hipMalloc(&c->qp, sizeof(double) * n * c->qp_len) != hipSuccess ||
      hipMalloc(&c->cfg, sizeof(double) * (size_t)S * c->co.len) != hipSuccess ||
      hipMalloc(&c->u_old, sizeof(double) * n * d.nu_tot) != hipSuccess ||
      hipMalloc(&c->du_old, sizeof(double) * n * L.nV) != hipSuccess ||
      hipMalloc(&c->ws, sizeof(uint32_t) * n) != hipSuccess)
    return cleanup(fail("hipMalloc failed (batch too large for device memory?)"));
  c->own_u_old = c->u_old;
  c->own_du_old = c->du_old;
  c->own_ws = c->ws;
  {
    auto up16 = [](size_t v) { return (v + 15) / 16 * 16; };
    c->out_st = up16(sizeof(double) * n * L.nV);
    c->out_nw = c->out_st + up16(sizeof(int32_t) * n);
    c->out_len = c->out_nw + sizeof(int32_t) * n;
    // a few QPs (the reference's own B = 1 call pattern): the kernels write
    // du, status and nWSR straight into page-locked host memory, so
    // cmpc_download is a stream sync, no copy (a hipMemcpyAsync cost ~7 us of
    // host time and a copy kernel per step, profiles/r4e_b1_hip_api_stats.csv)
    char* dev_out = nullptr;
    if (n <= CMPC_HOST_OUT_MAX_QP) {
      void* dv = nullptr;
      const size_t done_off = up16(c->out_len);
      if (hipHostMalloc(reinterpret_cast<void**>(&c->out_block), done_off + 16, hipHostMallocCoherent) != hipSuccess ||
          hipHostGetDevicePointer(&dv, c->out_block, 0) != hipSuccess)
        return cleanup(fail("hipHostMalloc failed"));
      c->out_host = true;
      std::memset(c->out_block, 0, done_off + 16);
      dev_out = reinterpret_cast<char*>(dv);
      c->done_host = reinterpret_cast<uint32_t*>(c->out_block + done_off);
      c->done_dev = reinterpret_cast<uint32_t*>(dev_out + done_off);
    } else {
      if (hipMalloc(&c->out_block, c->out_len) != hipSuccess)
        return cleanup(fail("hipMalloc failed (batch too large for device memory?)"));
      dev_out = c->out_block;
    }
    c->du = reinterpret_cast<double*>(dev_out);
    c->status = reinterpret_cast<int32_t*>(dev_out + c->out_st);
    c->nwsr = reinterpret_cast<int32_t*>(dev_out + c->out_nw);
  }
  if (hipMemsetAsync(c->lin, 0, sizeof(double) * n * L.rec_len, c->stream) != hipSuccess ||
      hipMemsetAsync(c->qp, 0, sizeof(double) * n * c->qp_len, c->stream) != hipSuccess ||
      hipMemsetAsync(c->u_old, 0, sizeof(double) * n * d.nu_tot, c->stream) != hipSuccess ||
      hipMemsetAsync(c->du_old, 0, sizeof(double) * n * L.nV, c->stream) != hipSuccess ||
      (!c->out_host && hipMemsetAsync(c->out_block, 0, c->out_len, c->stream) != hipSuccess) ||
      hipMemsetAsync(c->ws, 0, sizeof(uint32_t) * n, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess)
    return cleanup(fail("device initialisation failed"));
  *out = c;
  return 0;
}

int cmpc_destroy(cmpc_ctx* c) {
  if (!c) return 0;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (int k = 0; k < CMPC_KERNEL_COUNT; ++k)
    for (auto& pr : c->pending[k]) {
      (void)hipEventDestroy(pr.first);
      (void)hipEventDestroy(pr.second);
    }
  for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
  pinned_free(c->pin_in);
  pinned_free(c->pin_out);
  // own state buffers (bound external ones belong to the caller); before they
  // are recorded (a failed create) the active pointers are the own ones
  if (c->out_host && c->out_block) (void)hipHostFree(c->out_block);
  void* bufs[] = {c->lin, c->qp, c->cfg,
                  c->own_u_old ? c->own_u_old : c->u_old,
                  c->own_du_old ? c->own_du_old : c->du_old,
                  c->out_host ? nullptr : c->out_block,
                  c->own_ws ? c->own_ws : c->ws,
                  c->trace, c->ntrace, c->obs, c->d_obsM,
                  c->stage, c->own_sc_dy, c->own_sc_limits, c->own_sc_dref, c->own_sc_w, c->own_sc_p, c->d_yref, c->pred_y,
                  c->pred_cost, c->cert_rec, c->cert_work,
                  c->pair_cnt, c->score_band, c->score_oi, c->score_own, c->score_map, c->score_cap_own};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return 0;
}

int cmpc_set_stream(cmpc_ctx* c, void* stream) {
  if (!c) return fail("null context");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->own_stream) (void)hipStreamDestroy(c->stream);
  c->stream = (hipStream_t)stream;
  c->own_stream = false;
  return 0;
}

int cmpc_synchronize(cmpc_ctx* c) {
  if (!c) return fail("null context");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int cmpc_get_layout(const cmpc_ctx* c, cmpc_layout* L) {
  if (!c || !L) return fail("null argument");
  *L = c->L;
  return 0;
}

int cmpc_set_weights(cmpc_ctx* c, int s, const double* uwt, const double* ywt) {
  if (!c || !uwt || !ywt) return fail("null argument");
  if (s < 0 || s >= c->d.S) return fail("sub-controller index out of range");
  const int ny = c->d.ny, nu = c->d.nu;
  std::memcpy(c->ywt.data() + (size_t)s * ny * ny, ywt, sizeof(double) * ny * ny);
  std::memcpy(c->uwt.data() + (size_t)s * nu * nu, uwt, sizeof(double) * nu * nu);
  c->have_w[s] = 1;
  c->cfg_dirty = true;
  c->pred_stale = "the weights have changed since the build (cmpc_set_weights)";
  return 0;
}

int cmpc_set_constraints(cmpc_ctx* c, int s, const double* lo, const double* up,
                         const double* rlo, const double* rup) {
  if (!c || !lo || !up || !rlo || !rup) return fail("null argument");
  if (s < 0 || s >= c->d.S) return fail("sub-controller index out of range");
  const int nu = c->d.nu;
  for (int i = 0; i < nu; ++i)
    if (!(lo[i] <= up[i]) || !(rlo[i] <= rup[i]))
      return fail("constraints must satisfy lower <= upper (NaN bounds are unset)");
  std::memcpy(c->lower.data() + (size_t)s * nu, lo, sizeof(double) * nu);
  std::memcpy(c->upper.data() + (size_t)s * nu, up, sizeof(double) * nu);
  std::memcpy(c->rlower.data() + (size_t)s * nu, rlo, sizeof(double) * nu);
  std::memcpy(c->rupper.data() + (size_t)s * nu, rup, sizeof(double) * nu);
  c->have_c[s] = 1;
  c->cfg_dirty = true;
  return 0;
}

int cmpc_set_reference(cmpc_ctx* c, int s, const double* y_ref) {
  if (!c || !y_ref) return fail("null argument");
  if (s < 0 || s >= c->d.S) return fail("sub-controller index out of range");
  const size_t n = (size_t)c->d.p * c->d.ny;
  std::memcpy(c->yref.data() + s * n, y_ref, sizeof(double) * n);
  c->have_r[s] = 1;
  c->cfg_dirty = true;
  c->yref_dirty = true;
  c->pred_stale = "the reference has changed since the build (cmpc_set_reference)";
  return 0;
}

int cmpc_set_state(cmpc_ctx* c, const double* u_old, const double* du_old, const uint32_t* ws) {
  if (!c) return fail("null context");
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)c->nqp;
  if (u_old) {
    c->pred_stale = "u_old has changed since the build (cmpc_set_state)";
    HIP_TRY(hipMemcpyAsync(c->u_old, u_old, sizeof(double) * n * c->d.nu_tot,
                           hipMemcpyHostToDevice, c->stream));
  }
  if (du_old)
    HIP_TRY(hipMemcpyAsync(c->du_old, du_old, sizeof(double) * n * c->L.nV,
                           hipMemcpyHostToDevice, c->stream));
  if (ws) HIP_TRY(hipMemcpyAsync(c->ws, ws, sizeof(uint32_t) * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int cmpc_get_state(cmpc_ctx* c, double* u_old, double* du_old, uint32_t* ws) {
  if (!c) return fail("null context");
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)c->nqp;
  return direct_download(c->stream, {{c->u_old, u_old, sizeof(double) * n * c->d.nu_tot},
                                     {c->du_old, du_old, sizeof(double) * n * c->L.nV},
                                     {c->ws, ws, sizeof(uint32_t) * n}});
}

int cmpc_upload_lin(cmpc_ctx* c, const double* lin) {
  if (!c || !lin) return fail("null argument");
  HIP_TRY(hipSetDevice(c->device));
  c->pred_stale = "the records have changed since the build (cmpc_upload_lin)";
  HIP_TRY(hipMemcpyAsync(c->lin, lin, sizeof(double) * (size_t)c->nqp * c->L.rec_len,
                         hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int cmpc_download_lin(cmpc_ctx* c, double* lin) {
  if (!c || !lin) return fail("null argument");
  HIP_TRY(hipSetDevice(c->device));
  return direct_download(c->stream, {{c->lin, lin, sizeof(double) * (size_t)c->nqp * c->L.rec_len}});
}

void* cmpc_lin_device(cmpc_ctx* c) { return c ? (void*)c->lin : nullptr; }

int cmpc_bind_lin(cmpc_ctx* c, const double* lin_device) {
  if (!c) return fail("null context");
  if (lin_device) {
    if (!device_ptr_ok(c, lin_device, sizeof(double) * (size_t)c->nqp * c->L.rec_len))
      return fail("cmpc_bind_lin: not a device allocation of nqp * rec_len doubles on the context's device");
    // the build kernels read records with 16-byte loads (LDS-DMA / double2)
    if (reinterpret_cast<uintptr_t>(lin_device) % 16 != 0)
      return fail("cmpc_bind_lin: records must be 16-byte aligned");
  }
  c->lin_bound = lin_device;
  c->pred_stale = "the records have been re-bound since the build (cmpc_bind_lin)";
  return 0;
}

int cmpc_bind_state(cmpc_ctx* c, double* u_old, double* du_old, uint32_t* ws) {
  if (!c) return fail("null context");
  const int nnull = !u_old + !du_old + !ws;
  if (nnull == 3) {
    c->pred_stale = "the state has been re-bound since the build (cmpc_bind_state)";
    c->u_old = c->own_u_old;
    c->du_old = c->own_du_old;
    c->ws = c->own_ws;
    return 0;
  }
  if (nnull != 0) return fail("cmpc_bind_state: bind all three state arrays or none");
  const size_t n = (size_t)c->nqp;
  if (!device_ptr_ok(c, u_old, sizeof(double) * n * c->d.nu_tot) ||
      !device_ptr_ok(c, du_old, sizeof(double) * n * c->L.nV) || !device_ptr_ok(c, ws, sizeof(uint32_t) * n))
    return fail("cmpc_bind_state: not device allocations of the state's size on the context's device");
  if (reinterpret_cast<uintptr_t>(u_old) % 8 || reinterpret_cast<uintptr_t>(du_old) % 8 ||
      reinterpret_cast<uintptr_t>(ws) % 4)
    return fail("cmpc_bind_state: misaligned state array");
  c->u_old = u_old;
  c->du_old = du_old;
  c->ws = ws;
  c->pred_stale = "the state has been re-bound since the build (cmpc_bind_state)";
  return 0;
}

// Per-slot setpoint offsets and limits (include/cmpc.h).
int cmpc_set_scenario_reference(cmpc_ctx* c, const double* dy_ref) {
  if (!c) return fail("null context");
  if (!dy_ref) {
    if (c->sc_dy) c->pred_stale = "the setpoint offsets have changed since the build (cmpc_set_scenario_reference)";
    c->sc_dy = nullptr;
    return 0;
  }
  const int ny = c->d.ny;
  const size_t n = (size_t)c->nqp * ny;
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(dy_ref[i]))
      return fail("cmpc_set_scenario_reference: slot " + std::to_string(i / ny) + ": offsets must be finite");
  c->pred_stale = "the setpoint offsets have changed since the build (cmpc_set_scenario_reference)";
  return slot_upload(c, slot_dy(c), dy_ref, n);
}

int cmpc_bind_scenario_reference(cmpc_ctx* c, const double* dy_ref_device) {
  if (!c) return fail("null context");
  if (slot_bind(c, slot_dy(c), dy_ref_device, "cmpc_bind_scenario_reference", (size_t)c->nqp * c->d.ny, "nqp * ny"))
    return -1;
  c->pred_stale = "the setpoint offsets have been re-bound since the build (cmpc_bind_scenario_reference)";
  return 0;
}

int cmpc_get_scenario_reference(cmpc_ctx* c, double* dy_ref) {
  if (!c || !dy_ref) return fail("null argument");
  if (!c->sc_dy) return fail("cmpc_get_scenario_reference: no per-slot offsets are set");
  return slot_get(c, slot_dy(c), dy_ref, (size_t)c->nqp * c->d.ny);
}

int cmpc_set_scenario_constraints(cmpc_ctx* c, const double* lo, const double* up, const double* rlo,
                                  const double* rup) {
  if (!c) return fail("null context");
  const int nnull = !lo + !up + !rlo + !rup;
  if (nnull == 4) {
    c->sc_limits = nullptr;
    return 0;
  }
  if (nnull != 0) return fail("cmpc_set_scenario_constraints: give all four limit arrays or none");
  const int nu = c->d.nu;
  const size_t nqp = (size_t)c->nqp;
  std::vector<double> h(nqp * 4 * nu);  // per slot [lower | upper | rate_lower | rate_upper]
  for (size_t q = 0; q < nqp; ++q)
    for (int i = 0; i < nu; ++i) {
      const double l = lo[q * nu + i], u = up[q * nu + i], rl = rlo[q * nu + i], ru = rup[q * nu + i];
      if (!std::isfinite(l) || !std::isfinite(u) || !std::isfinite(rl) || !std::isfinite(ru))
        return fail("cmpc_set_scenario_constraints: slot " + std::to_string(q) + ": limits must be finite");
      if (!(l <= u) || !(rl <= ru))
        return fail("cmpc_set_scenario_constraints: slot " + std::to_string(q) +
                    ": constraints must satisfy lower <= upper");
      double* b = h.data() + q * 4 * nu;
      b[i] = l;
      b[nu + i] = u;
      b[2 * nu + i] = rl;
      b[3 * nu + i] = ru;
    }
  return slot_upload(c, slot_limits(c), h.data(), h.size());
}

int cmpc_bind_scenario_constraints(cmpc_ctx* c, const double* limits_device) {
  if (!c) return fail("null context");
  return slot_bind(c, slot_limits(c), limits_device, "cmpc_bind_scenario_constraints", (size_t)c->nqp * 4 * c->d.nu,
                   "nqp * 4 nu");
}

int cmpc_get_scenario_constraints(cmpc_ctx* c, double* lo, double* up, double* rlo, double* rup) {
  if (!c) return fail("null context");
  if (!c->sc_limits) return fail("cmpc_get_scenario_constraints: no per-slot limits are set");
  const int nu = c->d.nu;
  const size_t nqp = (size_t)c->nqp;
  std::vector<double> h(nqp * 4 * nu);
  if (slot_get(c, slot_limits(c), h.data(), h.size())) return -1;
  double* out[4] = {lo, up, rlo, rup};
  for (int k = 0; k < 4; ++k)
    if (out[k])
      for (size_t q = 0; q < nqp; ++q)
        std::memcpy(out[k] + q * nu, h.data() + (q * 4 + k) * nu, sizeof(double) * nu);
  return 0;
}

// Per-slot reference profiles (include/cmpc.h); cmpc_build applies them
// (refshift.hip).
int cmpc_set_scenario_reference_profile(cmpc_ctx* c, const double* dref) {
  if (!c) return fail("null context");
  if (!dref) {
    if (c->sc_dref) c->pred_stale = kStaleProfile;
    c->sc_dref = nullptr;
    return 0;
  }
  if (!cmpc_refshift_instance(c->d, c->L))
    return fail(std::string("cmpc_set_scenario_reference_profile") + kNoProfileKernel);
  const size_t per = (size_t)c->d.p * c->d.ny, n = (size_t)c->nqp * per;
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(dref[i]))
      return fail("cmpc_set_scenario_reference_profile: slot " + std::to_string(i / per) +
                  ": the profile must be finite");
  c->pred_stale = kStaleProfile;
  return slot_upload(c, slot_dref(c), dref, n);
}

int cmpc_bind_scenario_reference_profile(cmpc_ctx* c, const double* dref_device) {
  if (!c) return fail("null context");
  if (dref_device && !cmpc_refshift_instance(c->d, c->L))
    return fail(std::string("cmpc_bind_scenario_reference_profile") + kNoProfileKernel);
  const bool stale = c->sc_dref || dref_device;
  if (slot_bind(c, slot_dref(c), dref_device, "cmpc_bind_scenario_reference_profile",
                (size_t)c->nqp * c->d.p * c->d.ny, "nqp * p * ny"))
    return -1;
  if (stale) c->pred_stale = kStaleProfile;
  return 0;
}

int cmpc_get_scenario_reference_profile(cmpc_ctx* c, double* dref) {
  if (!c || !dref) return fail("null argument");
  if (!c->sc_dref) return fail("cmpc_get_scenario_reference_profile: no reference profile is set");
  return slot_get(c, slot_dref(c), dref, (size_t)c->nqp * c->d.p * c->d.ny);
}

// Per-slot weights (include/cmpc.h): the build, the reference-profile
// correction and cmpc_predict read the packed blocks [L_W' | uwt].
int cmpc_set_scenario_weights(cmpc_ctx* c, const double* uwt, const double* ywt) {
  if (!c) return fail("null context");
  if (!uwt && !ywt) {
    if (c->sc_w) c->pred_stale = kStaleWeights;
    c->sc_w = nullptr;
    return 0;
  }
  if (!uwt || !ywt) return fail("cmpc_set_scenario_weights: give both weight arrays or none");
  if (scenario_weights_refused(c, "cmpc_set_scenario_weights")) return -1;
  const int ny = c->d.ny, nu = c->d.nu, nw = ny * ny + nu * nu;
  const size_t nqp = (size_t)c->nqp;
  std::vector<double> h(nqp * nw);  // per slot [L_W' | uwt]
  for (size_t q = 0; q < nqp; ++q) {
    const std::string slot = "cmpc_set_scenario_weights: slot " + std::to_string(q) + ": ";
    const double *W = ywt + q * ny * ny, *U = uwt + q * nu * nu;
    double* b = h.data() + q * nw;
    double scale = 0;
    for (int i = 0; i < ny * ny; ++i)
      if (!std::isfinite(W[i])) return fail(slot + "weights must be finite");
    for (int i = 0; i < nu * nu; ++i) {
      if (!std::isfinite(U[i])) return fail(slot + "weights must be finite");
      scale = std::max(scale, std::fabs(U[i]));
    }
    if (const char* e = cmpc_weight_factor_error(ny, W, b)) return fail(slot + e);
    for (int i = 0; i < nu; ++i)
      for (int j = 0; j < nu; ++j)
        if (std::fabs(U[i * nu + j] - U[j * nu + i]) > 1e-12 * (1 + scale)) return fail(slot + "uwt must be symmetric");
    std::memcpy(b + ny * ny, U, sizeof(double) * nu * nu);
  }
  c->pred_stale = kStaleWeights;
  return slot_upload(c, slot_w(c), h.data(), h.size());
}

int cmpc_bind_scenario_weights(cmpc_ctx* c, const double* weights_device) {
  if (!c) return fail("null context");
  if (weights_device && scenario_weights_refused(c, "cmpc_bind_scenario_weights")) return -1;
  const size_t nw = (size_t)c->d.ny * c->d.ny + (size_t)c->d.nu * c->d.nu;
  const bool stale = c->sc_w || weights_device;
  if (slot_bind(c, slot_w(c), weights_device, "cmpc_bind_scenario_weights", (size_t)c->nqp * nw,
                "nqp * (ny*ny + nu*nu)"))
    return -1;
  if (stale) c->pred_stale = kStaleWeights;
  return 0;
}

int cmpc_get_scenario_weights(cmpc_ctx* c, double* uwt, double* ywt_factor) {
  if (!c) return fail("null context");
  if (!c->sc_w) return fail("cmpc_get_scenario_weights: no per-slot weights are set");
  const int ny = c->d.ny, nu = c->d.nu, nw = ny * ny + nu * nu;
  const size_t nqp = (size_t)c->nqp;
  std::vector<double> h(nqp * nw);
  if (slot_get(c, slot_w(c), h.data(), h.size())) return -1;
  for (size_t q = 0; q < nqp; ++q) {
    if (ywt_factor) std::memcpy(ywt_factor + q * ny * ny, h.data() + q * nw, sizeof(double) * ny * ny);
    if (uwt) std::memcpy(uwt + q * nu * nu, h.data() + q * nw + ny * ny, sizeof(double) * nu * nu);
  }
  return 0;
}

// Per-scenario boundary pressures (include/cmpc.h): B x [p_in, p_out].  The
// context's are the model's (the producer reads them at each launch), the
// simulator's the plant's (cmpc_sim_set_pressures, abi_sim.cpp).
int cmpc_set_scenario_pressures(cmpc_ctx* c, const double* pressures) {
  if (!c) return fail("null context");
  if (!pressures) {
    c->sc_p = nullptr;
    return 0;
  }
  if (pressures_check("cmpc_set_scenario_pressures", pressures, (size_t)c->d.B)) return -1;
  return slot_upload(c, slot_p(c), pressures, 2 * (size_t)c->d.B);
}

int cmpc_bind_scenario_pressures(cmpc_ctx* c, const double* pressures_device) {
  if (!c) return fail("null context");
  return slot_bind(c, slot_p(c), pressures_device, "cmpc_bind_scenario_pressures", 2 * (size_t)c->d.B, "B * 2");
}

int cmpc_get_scenario_pressures(cmpc_ctx* c, double* pressures) {
  if (!c || !pressures) return fail("null argument");
  if (!c->sc_p) return fail("cmpc_get_scenario_pressures: no per-scenario pressures are set");
  return slot_get(c, slot_p(c), pressures, 2 * (size_t)c->d.B);
}

int cmpc_set_build_variant(cmpc_ctx* c, int variant) {
  if (!c) return fail("null context");
  if (variant != CMPC_BUILD_AUTO && variant != CMPC_BUILD_WAVE && variant != CMPC_BUILD_ROWS &&
      variant != CMPC_BUILD_SPLIT)
    return fail("cmpc_set_build_variant: unknown variant");
  c->build_variant = variant;
  c->plans_valid = 0;
  return 0;
}

int cmpc_last_build_kernel(cmpc_ctx* c) {
  if (!c) return fail("null context");
  return c->last_build;
}

int cmpc_set_build_pairing(cmpc_ctx* c, int mode) {
  if (!c) return fail("null context");
  if (mode != CMPC_PAIRING_AUTO && mode != CMPC_PAIRING_OFF && mode != CMPC_PAIRING_ON)
    return fail("cmpc_set_build_pairing: unknown mode");
  if (mode == CMPC_PAIRING_ON) {  // the dimensions' part now; the weights when a build has them
    ensure_bp(c);
    if (c->bp_error) return fail(c->bp_error);
    if (const char* e = cmpc_pairing_error(c->d, c->bp, nullptr, nullptr))
      return fail(std::string("cmpc_set_build_pairing: ") + e);
  }
  c->pairing = mode;
  return 0;
}

int cmpc_last_build_shared_scenarios(cmpc_ctx* c) {
  if (!c) return fail("null context") - 1;
  if (!c->last_pair || !c->pair_cnt) return -1;
  if (hipSetDevice(c->device) != hipSuccess) return fail("hipSetDevice") - 1;
  uint32_t v = 0;
  if (hipMemcpyAsync(&v, c->pair_cnt + ((c->pair_seq - 1) & 1u), sizeof v, hipMemcpyDeviceToHost, c->stream) !=
          hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess)
    return fail("cmpc_last_build_shared_scenarios: reading the counter failed") - 1;
  return (int)v;
}

int cmpc_set_solve_variant(cmpc_ctx* c, int variant) {
  if (!c) return fail("null context");
  if (variant != CMPC_SOLVE_AUTO && variant != CMPC_SOLVE_LANE && variant != CMPC_SOLVE_ROWS)
    return fail("cmpc_set_solve_variant: unknown variant");
  c->solve_variant = variant;
  c->plans_valid = 0;
  return 0;
}

int cmpc_last_solve_kernel(cmpc_ctx* c) {
  if (!c) return fail("null context");
  return c->last_solve;
}

int cmpc_set_step_variant(cmpc_ctx* c, int variant) {
  if (!c) return fail("null context");
  if (variant != CMPC_STEP_AUTO && variant != CMPC_STEP_SPLIT && variant != CMPC_STEP_FUSED)
    return fail("cmpc_set_step_variant: unknown variant");
  c->step_variant = variant;
  c->plans_valid = 0;
  return 0;
}

int cmpc_last_step_fused(cmpc_ctx* c) {
  if (!c) return fail("null context");
  return c->last_step_fused;
}

int cmpc_enable_timing(cmpc_ctx* c, int enable) {
  if (!c) return fail("null context");
  if (resolve_timing(c)) return -1;
  const int all = (1 << CMPC_KERNEL_COUNT) - 1;
  c->timing = enable == 0 ? 0 : enable == 1 ? all : (enable >> 1) & all;
  for (int k = 0; k < CMPC_KERNEL_COUNT; ++k) {
    c->tot_ms[k] = 0;
    c->launches[k] = 0;
    c->timing_seq[k] = 0;
  }
  return 0;
}

int cmpc_set_timing_stride(cmpc_ctx* c, int stride) {
  if (!c) return fail("null context");
  if (stride < 1) return fail("cmpc_set_timing_stride: stride must be >= 1");
  c->timing_stride = stride;
  return 0;
}

int cmpc_kernel_time(cmpc_ctx* c, int kernel, double* total_ms, int64_t* launches) {
  if (!c) return fail("null context");
  if (kernel < 0 || kernel >= CMPC_KERNEL_COUNT) return fail("unknown kernel id");
  HIP_TRY(hipSetDevice(c->device));
  if (resolve_timing(c)) return -1;
  if (total_ms) *total_ms = c->tot_ms[kernel];
  if (launches) *launches = c->launches[kernel];
  return 0;
}

}  // extern "C"
