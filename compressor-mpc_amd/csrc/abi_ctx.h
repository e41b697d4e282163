// The context of the C ABI (include/cmpc.h) and the helpers its translation
// units share (abi_ctx.cpp, abi_step.cpp, abi_observer.cpp, abi_score.cpp).
// What a step calls is inline here: the per-step host path is latency-bound.
//
// The context owns every batched device buffer (HBM-resident between steps):
//   lin    B*S lin records (inputs of the build kernel)
//   qp     B*S condensed QPs [H | f | G]      (build -> iterate hand-off)
//   cfg    S per-sub-controller blocks          (weights, reference, bounds)
//   state  u_old, du_old, ws                   (persist across steps, as the
//                                               reference's member state)
//   out    du, status, nwsr, trace
#pragma once
#include <utility>
#include <vector>

#include "abi_common.h"

struct cmpc_ctx {
  cmpc_dims d{};
  cmpc_layout L{};
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int nqp = 0, qp_len = 0;
  CfgOffsets co{};
  // host mirror of the configuration
  std::vector<double> ywt, uwt, yref, lower, upper, rlower, rupper;  // per s
  std::vector<double> h_cfg;
  std::vector<int> have_w, have_c, have_r;
  bool cfg_dirty = true;
  // device buffers
  const double* lin_bound = nullptr;  // external records (cmpc_bind_lin)
  double *lin = nullptr, *qp = nullptr, *cfg = nullptr, *u_old = nullptr, *du_old = nullptr,
         *du = nullptr;
  uint32_t* ws = nullptr;
  // the context's own state buffers; u_old/du_old/ws above point at them
  // unless cmpc_bind_state bound external ones
  double *own_u_old = nullptr, *own_du_old = nullptr;
  uint32_t* own_ws = nullptr;
  // per-slot setpoint offsets (nqp * ny) and limits (nqp * 4 nu) in force, or
  // null: the context's own buffers (cmpc_set_scenario_*, allocated on first
  // use) or bound ones (cmpc_bind_scenario_*)
  const double *sc_dy = nullptr, *sc_limits = nullptr;
  double *own_sc_dy = nullptr, *own_sc_limits = nullptr;
  // per-slot reference profile (nqp * p * ny) in force, or null; set or bound
  // in the same way (cmpc_set/bind_scenario_reference_profile)
  const double* sc_dref = nullptr;
  double* own_sc_dref = nullptr;
  // per-slot weights (nqp * (ny*ny + nu*nu), per slot [L_W' | uwt]) in force,
  // or null; set or bound in the same way (cmpc_set/bind_scenario_weights).
  // d_yref: the raw references [S][p][ny] their build and predict kernels read
  // (cfg holds L_W' y_ref of the shared weights only), uploaded when stale
  const double* sc_w = nullptr;
  double* own_sc_w = nullptr;
  double* d_yref = nullptr;
  bool yref_dirty = true;
  // per-scenario boundary pressures of the model (B * 2, [p_in, p_out]) in
  // force, or null: the scalar arguments; set or bound in the same way
  // (cmpc_set/bind_scenario_pressures).  The producer reads them (fill_produce).
  const double* sc_p = nullptr;
  double* own_sc_p = nullptr;
  int32_t *status = nullptr, *nwsr = nullptr, *ntrace = nullptr;
  char* out_block = nullptr;  // du | status | nwsr in one allocation: one D2H for cmpc_download
  bool out_host = false;      // out_block is page-locked host memory the kernels write in place
  uint32_t* done_host = nullptr;  // out_host: the control step's completion word (after the block)
  uint32_t* done_dev = nullptr;   // its device address
  uint32_t done_seq = 0;
  size_t out_st = 0, out_nw = 0, out_len = 0;  // byte offsets of status, nwsr; block length
  uint8_t* trace = nullptr;
  size_t trace_cap = 0;
  int trace_K = 0;
  // observer (cmpc_set_observer / cmpc_observer_init)
  int obs_nout = 0, obs_len = 0, obs_plant = -1;
  double obs_pin = 0, obs_pout = 0, obs_Ts = 0;
  std::vector<double> obsM;  // S x nobs x n_out
  std::vector<int> have_M;
  bool obsM_dirty = true;
  double *d_obsM = nullptr, *obs = nullptr;
  double* stage = nullptr;  // host-pointer observer calls: device staging
  size_t stage_cap = 0;
  cmpc_abi::PinnedIO pin_in, pin_out;  // host-array calls: page-locked staging
  int64_t obs_steps = 0;  // a-priori steps since cmpc_observer_init: the delay blocks' ring phase
  int obs_io[CMPC_MAX_S_PRODUCE][CMPC_MAX_INPUTS] = {};
  int obs_oi[CMPC_MAX_S_PRODUCE][4] = {};
  // build kernel selection (cmpc_set_build_variant)
  int build_variant = CMPC_BUILD_AUTO;
  int last_build = 0;  // kernel launched by the last cmpc_build
  // build pairing (cmpc_set_build_pairing): the mode; two coverage counters
  // used alternately by the shared-form launches (each launch clears the next
  // one's, so no launch needs a memset); whether the last build was shared
  int pairing = CMPC_PAIRING_AUTO;
  uint32_t* pair_cnt = nullptr;
  unsigned pair_seq = 0;
  bool last_pair = false;
  int solve_variant = CMPC_SOLVE_AUTO;  // cmpc_set_solve_variant
  int last_solve = 0;                   // kernel launched by the last solve
  int step_variant = CMPC_STEP_AUTO;    // cmpc_set_step_variant
  int cus = kCusFallback;               // compute units of the device (cmpc_create)
  std::vector<std::pair<const void*, size_t>> bound_ok;  // (device pointer, bytes) cmpc_bind_* validated before
  // what follows from the dimensions, the batch and the CU count, computed on
  // first use (the layout searches are host time, and the small-batch kernels
  // take tens of microseconds): the launch parameters, and the plan per kind
  // of call under the current variants (plan_of)
  bool bp_ok = false;
  BuildParams bp{};                     // cmpc_dispatch_params; bp_error: its error text
  const char* bp_error = nullptr;
  cmpc_plan_t plans[32];
  unsigned plans_valid = 0;             // bit k: plans[k] holds; cleared by cmpc_set_*_variant
  int last_step_fused = 0;
  // prediction (cmpc_predict): buffers allocated by the first call; pred_stale
  // is why a prediction would not describe the last build's QPs (null: a
  // build has run and nothing it read has changed through the ABI since)
  double *pred_y = nullptr, *pred_cost = nullptr;
  bool pred_done = false;
  bool pred_built = false;  // a build has run
  const char* pred_stale = nullptr;
  // multipliers and KKT certificate (cmpc_certify): the record and the
  // summary's work buffer are allocated by the first call; cert_plans: a solve
  // has written plans for the last build's QPs
  double* cert_rec = nullptr;
  void* cert_work = nullptr;
  bool cert_done = false;
  bool cert_plans = false;
  // closed-loop performance indices (cmpc_score_*): everything is allocated by
  // cmpc_score_enable / cmpc_score_capture and freed by cmpc_score_disable;
  // score_rec / score_cap are the buffers in force (own or bound)
  bool score_on = false;
  int score_nout = 0;
  double score_Ts = 0;
  int64_t score_k = 0;             // steps since the last reset
  double* score_band = nullptr;    // S * ny
  int32_t* score_oi = nullptr;     // S * ny
  double *score_own = nullptr, *score_rec = nullptr;
  int score_nsel = 0, score_tcap = 0;
  int32_t* score_map = nullptr;    // B: capture column or -1
  double *score_cap_own = nullptr, *score_cap = nullptr;
  // timing
  int timing = 0;  // bit k: kernel k (CMPC_KERNEL_*) is timed
  int timing_stride = 1;                        // time every stride-th launch
  int64_t timing_seq[CMPC_KERNEL_COUNT] = {};  // launches since cmpc_enable_timing
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending[CMPC_KERNEL_COUNT];
  std::vector<hipEvent_t> event_pool;  // reused so timing stays cheap in a timed loop
  double tot_ms[CMPC_KERNEL_COUNT] = {};
  int64_t launches[CMPC_KERNEL_COUNT] = {};
  // ensemble statistics of the score record (cmpc_score_ensemble): the work
  // buffer is allocated by the first call and released with the context
  // (last, so that no other member's place in the context changes)
  struct DeviceBuf {
    void* p = nullptr;
    ~DeviceBuf() {
      if (p) (void)hipFree(p);
    }
  } score_ens_work;
  // exact quantiles of the score record (cmpc_score_quantiles): the work
  // buffer, allocated by the first call.  The envelope (cmpc_envelope_*):
  // everything is allocated by cmpc_envelope_enable and released by
  // cmpc_envelope_disable or with the context; env_rows are the rows in force
  // (own or bound).  (After score_ens_work, for the same reason.)
  DeviceBuf quant_work;
  bool env_on = false;
  int env_nout = 0, env_tcap = 0;
  int64_t env_k = 0;  // steps since the last reset
  QuantileRanks env_ranks{};
  DeviceBuf env_thr, env_mom_work, env_quant_work, env_own;
  double* env_rows = nullptr;
};

namespace cmpc_abi {

int rebuild_cfg(cmpc_ctx* c);  // abi_ctx.cpp

inline int ensure_cfg(cmpc_ctx* c) { return c->cfg_dirty ? rebuild_cfg(c) : 0; }

// per-slot weights in force: the raw references [S][p][ny] beside the cfg block
inline int ensure_yref(cmpc_ctx* c) {
  if (c->d_yref && !c->yref_dirty) return 0;
  HIP_TRY(hipSetDevice(c->device));
  if (!c->d_yref) HIP_TRY(hipMalloc(&c->d_yref, sizeof(double) * c->yref.size()));
  HIP_TRY(hipMemcpyAsync(c->d_yref, c->yref.data(), sizeof(double) * c->yref.size(), hipMemcpyHostToDevice,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->yref_dirty = false;
  return 0;
}

inline hipError_t pooled_event(cmpc_ctx* c, hipEvent_t* e) {
  if (!c->event_pool.empty()) {
    *e = c->event_pool.back();
    c->event_pool.pop_back();
    return hipSuccess;
  }
  return hipEventCreate(e);
}

// A timed launch: the launcher (cmpc_launch, cmpc_internal.h) passes both
// events to hipExtLaunchKernelGGL, which writes the kernel's start and end
// into them; no marker packets go into the stream.  The guard hands the events
// to the context's pending list on end() and, on any early return (a failed
// launch), clears cmpc_launch_events and gives them back to the pool.
class TimedLaunch {
 public:
  TimedLaunch(cmpc_ctx* c, int k) : c_(c), k_(k) {}
  TimedLaunch(const TimedLaunch&) = delete;
  TimedLaunch& operator=(const TimedLaunch&) = delete;
  int begin() {
    cmpc_launch_events = LaunchEvents{};
    if (!((c_->timing >> k_) & 1)) return 0;
    if (c_->timing_seq[k_]++ % c_->timing_stride) return 0;  // a sampled launch only
    HIP_TRY(pooled_event(c_, &e0_));
    HIP_TRY(pooled_event(c_, &e1_));
    cmpc_launch_events.start = e0_;
    cmpc_launch_events.stop = e1_;
    return 0;
  }
  int end() {
    cmpc_launch_events = LaunchEvents{};
    if (e0_ && e1_) {
      c_->pending[k_].push_back({e0_, e1_});
      c_->launches[k_]++;
    }
    e0_ = e1_ = nullptr;
    return 0;
  }
  ~TimedLaunch() {
    if (!e0_ && !e1_) return;
    cmpc_launch_events = LaunchEvents{};
    if (e0_) c_->event_pool.push_back(e0_);
    if (e1_) c_->event_pool.push_back(e1_);
  }

 private:
  cmpc_ctx* c_;
  int k_;
  hipEvent_t e0_ = nullptr, e1_ = nullptr;
};

inline int solve_params(cmpc_ctx* c, SolveParams* P) {
  std::memset(P, 0, sizeof *P);
  P->qp = c->qp;
  P->cfg = c->cfg;
  P->u_old = c->u_old;
  P->du_old = c->du_old;
  P->ws = c->ws;
  P->du = c->du;
  P->status = c->status;
  P->nwsr = c->nwsr;
  P->nqp = c->nqp;
  P->S = c->d.S;
  P->nu_tot = c->d.nu_tot;
  P->qp_len = c->qp_len;
  P->co = c->co;
  P->limits = c->sc_limits;
  return 0;
}

// what follows from the dimensions, the batch and the CU count, once
inline void ensure_bp(cmpc_ctx* c) {
  if (c->bp_ok) return;
  c->bp_error = cmpc_dispatch_params(c->d, c->L, c->nqp, c->cus, &c->bp);
  c->bp.co = c->co;
  c->bp_ok = true;
}

// the build launch parameters: that part, and the buffers as they are bound now
inline int build_params(cmpc_ctx* c, BuildParams& P) {
  ensure_bp(c);
  if (c->bp_error) return fail(c->bp_error);
  P = c->bp;
  P.lin = c->lin_bound ? c->lin_bound : c->lin;
  P.cfg = c->cfg;
  P.u_old = c->u_old;
  P.qp = c->qp;
  P.dy_ref = c->sc_dy;
  return 0;
}

// The plan (cmpc_dispatch_plan) for a call with K iterations: which kernel
// each entry point launches.  Derived once per kind of call and variant
// setting, so a step pays no selection work.  (With bp_error no build kernel
// is available, and the build calls report that error first.)
inline const cmpc_plan_t& plan_of(cmpc_ctx* c, int K, bool trace, bool du_other) {
  const bool profile = c->sc_dref != nullptr;  // a reference profile is in force: no fused path
  const bool weights = c->sc_w != nullptr;     // per-slot weights are in force: the wave build, no fused path
  const unsigned k = (K > 0 ? 1u : 0u) | (trace ? 2u : 0u) | (du_other ? 4u : 0u) | (profile ? 8u : 0u) |
                     (weights ? 16u : 0u);
  if (!((c->plans_valid >> k) & 1)) {
    ensure_bp(c);
    c->plans[k] = cmpc_dispatch_plan(c->d, c->L, c->bp, c->build_variant, c->solve_variant, c->step_variant,
                                     K > 0 ? 1 : 0, trace, du_other, profile, weights);
    c->plans_valid |= 1u << k;
  }
  return c->plans[k];
}

// cmpc_ctx::pred_stale after a solve that applied its first move
constexpr const char* kStaleMove = "u_old has moved since the build (CMPC_APPLY_MOVE applied the first move)";

// p is device memory of the context's device and [p, p + bytes) lies inside
// its allocation.  A rotation over a few bound buffers (the bench binds four
// per step) queries each (pointer, size) once: the runtime's lookups are
// several microseconds of host time per call, more than a small batch's
// kernels take.  A pointer is therefore validated the first time it is bound
// to this context (include/cmpc.h, cmpc_bind_lin): a caller that frees a
// bound buffer and binds another allocation at the same address must make
// it at least as large.
inline bool device_ptr_ok(cmpc_ctx* c, const void* p, size_t bytes) {
  for (const auto& v : c->bound_ok)
    if (v.first == p && v.second >= bytes) return true;
  if (!device_range_ok(c->device, p, bytes)) return false;
  if (c->bound_ok.size() >= 64) c->bound_ok.erase(c->bound_ok.begin());
  c->bound_ok.emplace_back(p, bytes);
  return true;
}

// cmpc_bind_*'s check of an array of n doubles: device_ptr_ok and 8-byte
// alignment.  `words` is how the caller's message spells the size.
int bound_array_check(cmpc_ctx* c, const void* dev, const char* who, size_t n, const char* words);

// copies host arrays (nullptr entries skipped) into the context's staging
// buffer on its stream; returns their device addresses
// host arrays of up to this many doubles are read by the kernels in place
inline bool stage_in_place(size_t tot) { return tot <= 1024; }

inline int stage_host(cmpc_ctx* c, const double* const* host, const size_t* n, int k,
                      const double** dev) {
  size_t tot = 0;
  for (int i = 0; i < k; ++i) tot += host[i] ? (n[i] + 1) / 2 * 2 : 0;
  if (!stage_in_place(tot) && tot > c->stage_cap) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->stage) HIP_TRY(hipFree(c->stage));
    c->stage = nullptr;
    HIP_TRY(hipMalloc(&c->stage, sizeof(double) * tot));
    c->stage_cap = tot;
  }
  // one DMA from page-locked memory (the device stage is read by kernels
  // queued after the copy on the same stream); small arrays are read by the
  // kernel in place (no copy: the caller releases the buffer after the launch)
  return pinned_upload(c->pin_in, c->stream, stage_in_place(tot) ? nullptr : c->stage, host, n, k, dev);
}

// after the launch that reads what stage_host staged
inline int stage_done(cmpc_ctx* c) {
  return c->pin_in.pending ? 0 : pinned_release(c->pin_in, c->stream);
}

// a host-array variant: stages the k arrays, runs the device form on their
// device addresses, then releases the staging buffer
template <class F>
int with_staged(cmpc_ctx* c, const double* const* host, const size_t* n, int k, F&& device_form) {
  HIP_TRY(hipSetDevice(c->device));
  const double* d[4];
  if (stage_host(c, host, n, k, d)) return -1;
  const int rc = device_form(d);
  return stage_done(c) ? -1 : rc;
}

}  // namespace cmpc_abi
