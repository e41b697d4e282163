// Host implementation of the C ABI declared in include/cmpc.h.
//
// The context owns every batched device buffer (HBM-resident between steps):
//   lin    B*S lin records (inputs of the build kernel)
//   qp     B*S condensed QPs [H | f | G]      (build -> iterate hand-off)
//   cfg    S per-sub-controller blocks          (weights, reference, bounds)
//   state  u_old, du_old, ws                   (persist across steps, as the
//                                               reference's member state)
//   out    du, status, nwsr, trace
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <chrono>
#include <vector>

#include "dispatch.h"
#include "ensemble_select.h"
#include "eig_body.h"
#include "equilibrium_body.h"
#include "target_body.h"
#include "gains_body.h"
#include "noise_body.h"

namespace {

thread_local std::string g_err;

int fail(const std::string& msg) {
  g_err = msg;
  return -1;
}

#define HIP_TRY(expr)                                                              \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess)                                                          \
      return fail(std::string(#expr) + ": " + hipGetErrorString(e_));             \
  } while (0)

int layout_of(const cmpc_dims* d, cmpc_layout* L) {
  if (const char* e = cmpc_layout_error(d, L)) return fail(e);
  return 0;
}

}  // namespace

thread_local LaunchEvents cmpc_launch_events;

namespace {

// Page-locked host buffer for the host-array entry points.  A hipMemcpy from or
// to pageable memory costs ~17 us per call here: the runtime stages it through
// its own bounce buffer (rocprofv3 --hip-trace of the B = 1 harness,
// DESIGN.md §3.6).  From pinned memory it is one DMA.  `busy` is recorded after
// the copies that read the buffer, and the next writer waits on it.
struct PinnedIO {
  char* buf = nullptr;
  char* dev = nullptr;  // the device's address of buf (kernels read it in place)
  size_t cap = 0;
  hipEvent_t busy = nullptr;
  bool pending = false;
};

int pinned_acquire(PinnedIO& p, size_t bytes) {
  if (p.pending) {
    HIP_TRY(hipEventSynchronize(p.busy));
    p.pending = false;
  }
  if (bytes > p.cap) {
    if (p.buf) HIP_TRY(hipHostFree(p.buf));
    p.buf = nullptr;
    p.cap = 0;
    const size_t cap = std::max<size_t>(bytes, 4096);
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&p.buf), cap, hipHostMallocCoherent));
    p.cap = cap;
    void* dv = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&dv, p.buf, 0));
    p.dev = reinterpret_cast<char*>(dv);
  }
  return 0;
}

int pinned_release(PinnedIO& p, hipStream_t s) {
  if (!p.busy) HIP_TRY(hipEventCreateWithFlags(&p.busy, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(p.busy, s));
  p.pending = true;
  return 0;
}

void pinned_free(PinnedIO& p) {
  if (p.pending) (void)hipEventSynchronize(p.busy);
  if (p.buf) (void)hipHostFree(p.buf);
  if (p.busy) (void)hipEventDestroy(p.busy);
  p = PinnedIO{};
}

// host -> device: the k arrays (nullptr skipped) are packed into `pin` and
// copied by one DMA to `dev_base`; dev[i] receives each array's device address.
// dev_base == nullptr: no copy, the kernels read the page-locked buffer in
// place (dev[i] = its device address) and the caller calls pinned_release
// after the launch that reads it.
constexpr size_t kPad = 2;  // keep every array 16-byte aligned
int pinned_upload(PinnedIO& pin, hipStream_t s, double* dev_base, const double* const* host,
                  const size_t* n, int k, const double** dev) {
  size_t tot = 0;
  for (int i = 0; i < k; ++i) tot += host[i] ? (n[i] + kPad - 1) / kPad * kPad : 0;
  if (pinned_acquire(pin, sizeof(double) * std::max<size_t>(tot, 1))) return -1;
  double* h = reinterpret_cast<double*>(pin.buf);
  size_t off = 0;
  for (int i = 0; i < k; ++i) {
    if (dev) dev[i] = nullptr;
    if (!host[i]) continue;
    std::memcpy(h + off, host[i], sizeof(double) * n[i]);
    if (dev) dev[i] = (dev_base ? dev_base : reinterpret_cast<double*>(pin.dev)) + off;
    off += (n[i] + kPad - 1) / kPad * kPad;
  }
  if (!dev_base) return 0;
  if (off) HIP_TRY(hipMemcpyAsync(dev_base, h, sizeof(double) * off, hipMemcpyHostToDevice, s));
  return pinned_release(pin, s);
}

}  // namespace

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
  PinnedIO pin_in, pin_out;  // host-array calls: page-locked staging
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

namespace {

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

int ensure_cfg(cmpc_ctx* c) { return c->cfg_dirty ? rebuild_cfg(c) : 0; }

// per-slot weights in force: the raw references [S][p][ny] beside the cfg block
int ensure_yref(cmpc_ctx* c) {
  if (c->d_yref && !c->yref_dirty) return 0;
  HIP_TRY(hipSetDevice(c->device));
  if (!c->d_yref) HIP_TRY(hipMalloc(&c->d_yref, sizeof(double) * c->yref.size()));
  HIP_TRY(hipMemcpyAsync(c->d_yref, c->yref.data(), sizeof(double) * c->yref.size(), hipMemcpyHostToDevice,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->yref_dirty = false;
  return 0;
}

hipError_t pooled_event(cmpc_ctx* c, hipEvent_t* e) {
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

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(std::string(what) + ": " + hipGetErrorString(e));
  return 0;
}

int solve_params(cmpc_ctx* c, SolveParams* P) {
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
void ensure_bp(cmpc_ctx* c) {
  if (c->bp_ok) return;
  c->bp_error = cmpc_dispatch_params(c->d, c->L, c->nqp, c->cus, &c->bp);
  c->bp.co = c->co;
  c->bp_ok = true;
}

// the build launch parameters: that part, and the buffers as they are bound now
int build_params(cmpc_ctx* c, BuildParams& P) {
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
const cmpc_plan_t& plan_of(cmpc_ctx* c, int K, bool trace, bool du_other) {
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
const char* const kStaleMove = "u_old has moved since the build (CMPC_APPLY_MOVE applied the first move)";

int plan_mismatch(const char* what) {
  return fail(std::string("internal error: plan and launcher disagree (") + what + ")");
}

}  // namespace

extern "C" {

int cmpc_plan(const cmpc_dims* dims, int cus, int build_variant, int solve_variant, int step_variant, int K,
              uint32_t flags, cmpc_plan_t* plan) {
  if (const char* e = cmpc_plan_or_error(dims, cus, build_variant, solve_variant, step_variant, K, flags, plan))
    return fail(e);
  return 0;
}

int cmpc_layout_of(const cmpc_dims* d, cmpc_layout* L) { return layout_of(d, L); }

const char* cmpc_last_error(void) { return g_err.c_str(); }

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
  if (u_old)
    HIP_TRY(hipMemcpyAsync(u_old, c->u_old, sizeof(double) * n * c->d.nu_tot,
                           hipMemcpyDeviceToHost, c->stream));
  if (du_old)
    HIP_TRY(hipMemcpyAsync(du_old, c->du_old, sizeof(double) * n * c->L.nV,
                           hipMemcpyDeviceToHost, c->stream));
  if (ws) HIP_TRY(hipMemcpyAsync(ws, c->ws, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
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
  HIP_TRY(hipMemcpyAsync(lin, c->lin, sizeof(double) * (size_t)c->nqp * c->L.rec_len,
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

void* cmpc_lin_device(cmpc_ctx* c) { return c ? (void*)c->lin : nullptr; }

// p is device memory of the context's device and [p, p + bytes) lies inside
// its allocation.  A rotation over a few bound buffers (the bench binds four
// per step) queries each (pointer, size) once: the runtime's lookups are
// several microseconds of host time per call, more than a small batch's
// kernels take.  A pointer is therefore validated the first time it is bound
// to this context (include/cmpc.h, cmpc_bind_lin): a caller that frees a
// bound buffer and binds another allocation at the same address must make
// it at least as large.
static bool device_ptr_ok(cmpc_ctx* c, const void* p, size_t bytes) {
  for (const auto& v : c->bound_ok)
    if (v.first == p && v.second >= bytes) return true;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeDevice || a.device != c->device)
    return false;
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) == hipSuccess && base &&
      (uintptr_t)p + bytes > (uintptr_t)base + size)
    return false;
  if (c->bound_ok.size() >= 64) c->bound_ok.erase(c->bound_ok.begin());
  c->bound_ok.emplace_back(p, bytes);
  return true;
}

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

// Per-slot setpoint offsets and limits (include/cmpc.h).  The host setters
// stage into the context's own buffers the way cmpc_set_state does; the bind
// variants check the pointer the way cmpc_bind_state does.
static int scenario_upload(cmpc_ctx* c, double** own, const double* host, size_t n) {
  HIP_TRY(hipSetDevice(c->device));
  if (!*own) HIP_TRY(hipMalloc(own, sizeof(double) * n));
  HIP_TRY(hipMemcpyAsync(*own, host, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

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
  if (scenario_upload(c, &c->own_sc_dy, dy_ref, n)) return -1;
  c->sc_dy = c->own_sc_dy;
  return 0;
}

int cmpc_bind_scenario_reference(cmpc_ctx* c, const double* dy_ref_device) {
  if (!c) return fail("null context");
  if (dy_ref_device) {
    if (!device_ptr_ok(c, dy_ref_device, sizeof(double) * (size_t)c->nqp * c->d.ny)) {
      (void)hipGetLastError();  // a failed pointer query is not a later launch's error
      return fail("cmpc_bind_scenario_reference: not a device allocation of nqp * ny doubles on the context's device");
    }
    if (reinterpret_cast<uintptr_t>(dy_ref_device) % 8)
      return fail("cmpc_bind_scenario_reference: misaligned array");
  }
  c->sc_dy = dy_ref_device;
  c->pred_stale = "the setpoint offsets have been re-bound since the build (cmpc_bind_scenario_reference)";
  return 0;
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
  if (scenario_upload(c, &c->own_sc_limits, h.data(), h.size())) return -1;
  c->sc_limits = c->own_sc_limits;
  return 0;
}

int cmpc_bind_scenario_constraints(cmpc_ctx* c, const double* limits_device) {
  if (!c) return fail("null context");
  if (limits_device) {
    if (!device_ptr_ok(c, limits_device, sizeof(double) * (size_t)c->nqp * 4 * c->d.nu)) {
      (void)hipGetLastError();  // a failed pointer query is not a later launch's error
      return fail("cmpc_bind_scenario_constraints: not a device allocation of nqp * 4 nu doubles on the "
                  "context's device");
    }
    if (reinterpret_cast<uintptr_t>(limits_device) % 8)
      return fail("cmpc_bind_scenario_constraints: misaligned array");
  }
  c->sc_limits = limits_device;
  return 0;
}

int cmpc_get_scenario_reference(cmpc_ctx* c, double* dy_ref) {
  if (!c || !dy_ref) return fail("null argument");
  if (!c->sc_dy) return fail("cmpc_get_scenario_reference: no per-slot offsets are set");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(dy_ref, c->sc_dy, sizeof(double) * (size_t)c->nqp * c->d.ny, hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// Per-slot reference profiles (include/cmpc.h): set, bind and get as the
// setpoint offsets above; cmpc_build applies them (refshift.hip).
static const char* const kStaleProfile =
    "the reference profile has changed since the build (cmpc_set/bind_scenario_reference_profile)";
static const char* const kNoProfileKernel =
    ": reference-profile kernel not instantiated for these dimensions (ns, ny, nu, m)";

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
  if (scenario_upload(c, &c->own_sc_dref, dref, n)) return -1;
  c->sc_dref = c->own_sc_dref;
  return 0;
}

int cmpc_bind_scenario_reference_profile(cmpc_ctx* c, const double* dref_device) {
  if (!c) return fail("null context");
  if (dref_device) {
    if (!cmpc_refshift_instance(c->d, c->L))
      return fail(std::string("cmpc_bind_scenario_reference_profile") + kNoProfileKernel);
    if (!device_ptr_ok(c, dref_device, sizeof(double) * (size_t)c->nqp * c->d.p * c->d.ny)) {
      (void)hipGetLastError();  // a failed pointer query is not a later launch's error
      return fail("cmpc_bind_scenario_reference_profile: not a device allocation of nqp * p * ny doubles on the "
                  "context's device");
    }
    if (reinterpret_cast<uintptr_t>(dref_device) % 8)
      return fail("cmpc_bind_scenario_reference_profile: misaligned array");
  }
  if (c->sc_dref || dref_device) c->pred_stale = kStaleProfile;
  c->sc_dref = dref_device;
  return 0;
}

int cmpc_get_scenario_reference_profile(cmpc_ctx* c, double* dref) {
  if (!c || !dref) return fail("null argument");
  if (!c->sc_dref) return fail("cmpc_get_scenario_reference_profile: no reference profile is set");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(dref, c->sc_dref, sizeof(double) * (size_t)c->nqp * c->d.p * c->d.ny,
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// Per-slot weights (include/cmpc.h): set, bind and get as the families above;
// the build, the reference-profile correction and cmpc_predict read the
// packed blocks [L_W' | uwt].
static const char* const kStaleWeights =
    "the per-scenario weights have changed since the build (cmpc_set/bind_scenario_weights)";

static int scenario_weights_refused(cmpc_ctx* c, const char* who) {
  ensure_bp(c);
  if (c->bp_error || !cmpc_build_weights_available(c->d, c->bp))
    return fail(std::string(who) + ": " + cmpc_plan_error_string(CMPC_PLAN_NO_WEIGHTS_BUILD));
  return 0;
}

int cmpc_weight_factor(int ny, const double* ywt, double* lwt) {
  if (const char* e = cmpc_weight_factor_error(ny, ywt, lwt)) return fail(std::string("cmpc_weight_factor: ") + e);
  return 0;
}

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
  if (scenario_upload(c, &c->own_sc_w, h.data(), h.size())) return -1;
  c->sc_w = c->own_sc_w;
  return 0;
}

int cmpc_bind_scenario_weights(cmpc_ctx* c, const double* weights_device) {
  if (!c) return fail("null context");
  if (weights_device) {
    if (scenario_weights_refused(c, "cmpc_bind_scenario_weights")) return -1;
    const size_t nw = (size_t)c->d.ny * c->d.ny + (size_t)c->d.nu * c->d.nu;
    if (!device_ptr_ok(c, weights_device, sizeof(double) * (size_t)c->nqp * nw)) {
      (void)hipGetLastError();  // a failed pointer query is not a later launch's error
      return fail("cmpc_bind_scenario_weights: not a device allocation of nqp * (ny*ny + nu*nu) doubles on the "
                  "context's device");
    }
    if (reinterpret_cast<uintptr_t>(weights_device) % 8)
      return fail("cmpc_bind_scenario_weights: misaligned array");
  }
  if (c->sc_w || weights_device) c->pred_stale = kStaleWeights;
  c->sc_w = weights_device;
  return 0;
}

int cmpc_get_scenario_weights(cmpc_ctx* c, double* uwt, double* ywt_factor) {
  if (!c) return fail("null context");
  if (!c->sc_w) return fail("cmpc_get_scenario_weights: no per-slot weights are set");
  HIP_TRY(hipSetDevice(c->device));
  const int ny = c->d.ny, nu = c->d.nu, nw = ny * ny + nu * nu;
  const size_t nqp = (size_t)c->nqp;
  std::vector<double> h(nqp * nw);
  HIP_TRY(hipMemcpyAsync(h.data(), c->sc_w, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t q = 0; q < nqp; ++q) {
    if (ywt_factor) std::memcpy(ywt_factor + q * ny * ny, h.data() + q * nw, sizeof(double) * ny * ny);
    if (uwt) std::memcpy(uwt + q * nu * nu, h.data() + q * nw + ny * ny, sizeof(double) * nu * nu);
  }
  return 0;
}

int cmpc_get_scenario_constraints(cmpc_ctx* c, double* lo, double* up, double* rlo, double* rup) {
  if (!c) return fail("null context");
  if (!c->sc_limits) return fail("cmpc_get_scenario_constraints: no per-slot limits are set");
  HIP_TRY(hipSetDevice(c->device));
  const int nu = c->d.nu;
  const size_t nqp = (size_t)c->nqp;
  std::vector<double> h(nqp * 4 * nu);
  HIP_TRY(hipMemcpyAsync(h.data(), c->sc_limits, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  double* out[4] = {lo, up, rlo, rup};
  for (int k = 0; k < 4; ++k)
    if (out[k])
      for (size_t q = 0; q < nqp; ++q)
        std::memcpy(out[k] + q * nu, h.data() + (q * 4 + k) * nu, sizeof(double) * nu);
  return 0;
}

// Per-scenario boundary pressures (include/cmpc.h): B x [p_in, p_out].  The
// context's are the model's (the producer reads them at each launch), the
// simulator's the plant's (cmpc_sim_set_pressures, below).
static int pressures_check(const char* who, const double* p, size_t B) {
  for (size_t i = 0; i < 2 * B; ++i)
    if (!std::isfinite(p[i]) || !(p[i] > 0))
      return fail(std::string(who) + ": scenario " + std::to_string(i / 2) +
                  ": pressures must be finite and positive");
  return 0;
}

int cmpc_check_pressures(int B, const double* pressures) {
  if (!pressures || B < 1) return fail("cmpc_check_pressures: null array or empty batch");
  return pressures_check("cmpc_check_pressures", pressures, (size_t)B);
}

int cmpc_set_scenario_pressures(cmpc_ctx* c, const double* pressures) {
  if (!c) return fail("null context");
  if (!pressures) {
    c->sc_p = nullptr;
    return 0;
  }
  if (pressures_check("cmpc_set_scenario_pressures", pressures, (size_t)c->d.B)) return -1;
  if (scenario_upload(c, &c->own_sc_p, pressures, 2 * (size_t)c->d.B)) return -1;
  c->sc_p = c->own_sc_p;
  return 0;
}

int cmpc_bind_scenario_pressures(cmpc_ctx* c, const double* pressures_device) {
  if (!c) return fail("null context");
  if (pressures_device) {
    if (!device_ptr_ok(c, pressures_device, sizeof(double) * 2 * (size_t)c->d.B)) {
      (void)hipGetLastError();  // a failed pointer query is not a later launch's error
      return fail("cmpc_bind_scenario_pressures: not a device allocation of B * 2 doubles on the context's device");
    }
    if (reinterpret_cast<uintptr_t>(pressures_device) % 8)
      return fail("cmpc_bind_scenario_pressures: misaligned array");
  }
  c->sc_p = pressures_device;
  return 0;
}

int cmpc_get_scenario_pressures(cmpc_ctx* c, double* pressures) {
  if (!c || !pressures) return fail("null argument");
  if (!c->sc_p) return fail("cmpc_get_scenario_pressures: no per-scenario pressures are set");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(pressures, c->sc_p, sizeof(double) * 2 * (size_t)c->d.B, hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

static int fill_produce(cmpc_ctx* c, const char* who, int plant, double p_in, double p_out,
                        double Ts, const int32_t* input_order, const int32_t* out_idx,
                        ProduceParams* P, int* n_outputs) {
  const cmpc_dims& d = c->d;
  const cmpc_layout& L = c->L;
  int ns = 0, ni = 0, no = 0, nci = 0;
  if (cmpc_plant_dims(plant, &ns, &ni, &no, &nci)) return fail(std::string(who) + ": unknown plant");
  if (d.ns != ns || d.nu_tot != nci || d.ndist > no || d.ny > 4)
    return fail(std::string(who) + ": context dimensions do not match the plant");
  if (d.S > CMPC_MAX_S_PRODUCE) return fail(std::string(who) + ": too many sub-controllers");
  if (L.rec_len > 2 * 64 * CMPC_REC_CHUNKS)
    return fail(std::string(who) + ": lin record of " + std::to_string(L.rec_len) +
                " doubles exceeds the producer's " + std::to_string(2 * 64 * CMPC_REC_CHUNKS) +
                " (too many delay states)");
  std::memset(P, 0, sizeof *P);
  P->lin = c->lin;
  P->B = d.B;
  P->S = d.S;
  P->rec_len = L.rec_len;
  P->nu_tot = d.nu_tot;
  P->ny = d.ny;
  P->nobs = L.nobs;
  P->naug = L.naug;
  P->n_outputs = no;
  P->off_A = L.off_A; P->off_B = L.off_B; P->off_C = L.off_C;
  P->off_f = L.off_f; P->off_x = L.off_x; P->off_y = L.off_y;
  P->p_in = p_in;
  P->p_out = p_out;
  P->pressures = c->sc_p;  // in force: scenario b's pair in place of the two scalars
  P->Ts = Ts;
  for (int s = 0; s < d.S; ++s) {
    for (int k = 0; k < d.nu_tot; ++k) {
      const int v = input_order[s * d.nu_tot + k];
      if (v < 0 || v >= nci) return fail(std::string(who) + ": bad input_order");
      P->input_order[s][k] = v;
    }
    for (int o = 0; o < d.ny; ++o) {
      const int v = out_idx[s * d.ny + o];
      if (v < 0 || v >= no) return fail(std::string(who) + ": bad out_idx");
      P->out_idx[s][o] = v;
    }
  }
  if (n_outputs) *n_outputs = no;
  return 0;
}

int cmpc_produce_lin(cmpc_ctx* c, int plant, double p_in, double p_out, double Ts,
                     const int32_t* input_order, const int32_t* out_idx, const double* x,
                     const double* u_full, const double* dx_aug, const double* y) {
  if (!c) return fail("null context");
  if (!input_order || !out_idx || !x || !u_full || !y) return fail("cmpc_produce_lin: null argument");
  ProduceParams P;
  if (fill_produce(c, "cmpc_produce_lin", plant, p_in, p_out, Ts, input_order, out_idx, &P, nullptr))
    return -1;
  P.x = x;
  P.u_full = u_full;
  P.dx_aug = dx_aug;
  P.y = y;
  HIP_TRY(hipSetDevice(c->device));
  c->lin_bound = nullptr;  // the build reads the produced records
  c->pred_stale = "the records have changed since the build (cmpc_produce_lin)";
  TimedLaunch tl(c, CMPC_KERNEL_PRODUCE);
  if (tl.begin()) return -1;
  if (cmpc_launch_produce(P, plant, c->stream)) return fail("cmpc_produce_lin: launch failed");
  if (check_launch("produce kernel")) return -1;
  return tl.end();
}

// ---- observer ----
static void observer_params(cmpc_ctx* c, ObserverParams* P) {
  const cmpc_dims& d = c->d;
  const cmpc_layout& L = c->L;
  std::memset(P, 0, sizeof *P);
  P->obs = c->obs;
  P->M = c->d_obsM;
  P->lin = c->lin;
  P->du_old = c->du_old;
  P->u_old = c->u_old;
  P->nqp = c->nqp;
  P->S = d.S;
  P->ns = d.ns;
  P->ndist = d.ndist;
  P->nobs = L.nobs;
  P->ntot = L.ntot;
  P->n_out = c->obs_nout;
  P->obs_len = c->obs_len;
  P->nu = d.nu;
  P->nu_tot = d.nu_tot;
  P->nV = L.nV;
  P->rec_len = L.rec_len;
  P->off_B = L.off_B;
  P->off_f = L.off_f;
  int blk = L.nobs + L.nd;
  for (int i = 0; i < d.nu_tot; ++i) {
    P->delay[i] = d.delay[i];
    if (d.delay[i]) {
      P->dinput[P->nd] = i;
      P->blk[P->nd] = blk;
      P->rot[P->nd] = d.delay[i] > 1 ? (int)(c->obs_steps % (d.delay[i] - 1)) : 0;
      blk += d.delay[i] - 1;
      P->nd++;
    }
  }
}

static int observer_upload_M(cmpc_ctx* c) {
  for (int s = 0; s < c->d.S; ++s)
    if (!c->have_M[s]) return fail("observer gain of sub-controller " + std::to_string(s) + " not set");
  if (c->obsM_dirty) {
    HIP_TRY(hipMemcpyAsync(c->d_obsM, c->obsM.data(), sizeof(double) * c->obsM.size(),
                           hipMemcpyHostToDevice, c->stream));
    c->obsM_dirty = false;
  }
  return 0;
}

int cmpc_set_observer(cmpc_ctx* c, int s, int n_outputs, const double* M) {
  if (!c || !M) return fail("null argument");
  const cmpc_dims& d = c->d;
  if (s < 0 || s >= d.S) return fail("cmpc_set_observer: bad sub-controller index");
  if (n_outputs < 1 || n_outputs > 8 || n_outputs < d.ndist)
    return fail("cmpc_set_observer: n_outputs must be in [ndist, 8]");
  if (c->obs_nout && c->obs_nout != n_outputs)
    return fail("cmpc_set_observer: n_outputs differs between sub-controllers");
  if (c->L.nobs > 32) return fail("cmpc_set_observer: ns + ndist > 32");
  if (!cmpc_obs_supported(d.ns, n_outputs, d.ndist, c->L.ntot - c->L.nobs, c->L.nd, d.nu_tot))
    return fail("cmpc_set_observer: no observer kernel for these dimensions (instantiated: ns 10 or 11, "
                "4 outputs, 4 disturbance states, 4 inputs)");
  for (int i = 0; i < d.nu_tot; ++i)
    if (d.delay[i] == 1) return fail("cmpc_set_observer: a one-step input delay has no delay block");
  HIP_TRY(hipSetDevice(c->device));
  if (!c->obs) {
    c->obs_nout = n_outputs;
    // rows padded to 128 B (16 doubles): every row starts on a cache line, so
    // the observer kernels' field reads touch no line shared with a neighbour
    c->obs_len = (d.ns + c->L.ntot + n_outputs + n_outputs * d.ns + 15) / 16 * 16;
    c->obsM.assign((size_t)d.S * c->L.nobs * n_outputs, 0.0);
    c->have_M.assign(d.S, 0);
    HIP_TRY(hipMalloc(&c->d_obsM, sizeof(double) * c->obsM.size()));
    HIP_TRY(hipMalloc(&c->obs, sizeof(double) * (size_t)c->nqp * c->obs_len));
    HIP_TRY(hipMemsetAsync(c->obs, 0, sizeof(double) * (size_t)c->nqp * c->obs_len, c->stream));
  }
  std::memcpy(c->obsM.data() + (size_t)s * c->L.nobs * n_outputs, M,
              sizeof(double) * c->L.nobs * n_outputs);
  c->have_M[s] = 1;
  c->obsM_dirty = true;
  return 0;
}

int cmpc_observer_len(const cmpc_ctx* c) { return c ? c->obs_len : 0; }

// the producer's per-QP parameters: every QP slot linearised at its own
// x_hat (observer state), C stored; with_post: the a-posteriori update of
// each slot first, in the same kernel
static int observer_produce_params(cmpc_ctx* c, const double* u_full, const double* y, bool with_post,
                                   ProduceParams& P) {
  int no = 0;
  int io[CMPC_MAX_S_PRODUCE * CMPC_MAX_INPUTS], oi[CMPC_MAX_S_PRODUCE * 4];
  for (int s = 0; s < c->d.S; ++s) {
    for (int k = 0; k < c->d.nu_tot; ++k) io[s * c->d.nu_tot + k] = c->obs_io[s][k];
    for (int o = 0; o < c->d.ny; ++o) oi[s * c->d.ny + o] = c->obs_oi[s][o];
  }
  if (fill_produce(c, "observer", c->obs_plant, c->obs_pin, c->obs_pout, c->obs_Ts, io, oi, &P, &no))
    return -1;
  P.per_qp = 1;
  {  // the observer rows' delay blocks are rings (cmpc_obs_prior_kernel)
    ObserverParams O;
    observer_params(c, &O);
    P.nring = O.nd;
    for (int k = 0; k < O.nd && k < CMPC_ND_MAX; ++k) {
      P.rb[k] = O.blk[k] - c->d.ns;  // dx index -> dx_aug tail index
      P.rlen[k] = O.delay[O.dinput[k]] - 1;
      P.rot[k] = O.rot[k];
    }
  }
  P.x = c->obs;
  P.x_stride = c->obs_len;
  P.dx_aug = c->obs + c->d.ns + c->d.ns;  // dx_aug tail (aug states) of slot 0
  P.dx_stride = c->obs_len;
  P.c_out = c->obs + c->d.ns + c->L.ntot + c->obs_nout;
  P.c_stride = c->obs_len;
  P.u_full = u_full;
  P.y = y;
  if (with_post) {
    P.obs_M = c->d_obsM;
    P.obs = c->obs;
    P.obs_ntot = c->L.ntot;
  }
  return 0;
}

static int observer_produce(cmpc_ctx* c, const double* u_full, const double* y, bool with_post) {
  ProduceParams P;
  if (observer_produce_params(c, u_full, y, with_post, P)) return -1;
  c->lin_bound = nullptr;
  c->pred_stale = "the records have changed since the build (cmpc_observe_step / cmpc_observer_init)";
  TimedLaunch tl(c, CMPC_KERNEL_PRODUCE);
  if (tl.begin()) return -1;
  if (cmpc_launch_produce(P, c->obs_plant, c->stream)) return fail("observer: produce launch failed");
  if (check_launch("produce kernel (per QP)")) return -1;
  return tl.end();
}

int cmpc_observer_init(cmpc_ctx* c, int plant, double p_in, double p_out, double Ts,
                       const int32_t* input_order, const int32_t* out_idx, const double* x_init,
                       const double* u_full, const double* y_init, const double* dx_init) {
  if (!c) return fail("null context");
  if (!input_order || !out_idx || !x_init || !u_full || !y_init)
    return fail("cmpc_observer_init: null argument");
  if (!c->obs) return fail("cmpc_observer_init: set the observer gains first (cmpc_set_observer)");
  ProduceParams chk;
  int no = 0;
  if (fill_produce(c, "cmpc_observer_init", plant, p_in, p_out, Ts, input_order, out_idx, &chk, &no))
    return -1;
  if (no != c->obs_nout) return fail("cmpc_observer_init: plant outputs differ from the observer gains' n_outputs");
  c->obs_plant = plant;
  c->obs_pin = p_in;
  c->obs_pout = p_out;
  c->obs_Ts = Ts;
  for (int s = 0; s < c->d.S; ++s) {
    for (int k = 0; k < c->d.nu_tot; ++k) c->obs_io[s][k] = chk.input_order[s][k];
    for (int o = 0; o < c->d.ny; ++o) c->obs_oi[s][o] = chk.out_idx[s][o];
  }
  HIP_TRY(hipSetDevice(c->device));
  if (observer_upload_M(c)) return -1;
  c->obs_steps = 0;  // the rings start in logical order
  ObserverParams P;
  observer_params(c, &P);
  P.x_init = x_init;
  P.dx_init = dx_init;
  P.y = y_init;
  if (cmpc_launch_observer(P, CMPC_OBS_INIT, c->stream)) return fail("observer init launch failed");
  if (check_launch("observer init kernel")) return -1;
  return observer_produce(c, u_full, y_init, false);  // Initialize: Update(x_init, full_u_old)
}

int cmpc_observe_step(cmpc_ctx* c, const double* u_full, const double* y) {
  if (!c) return fail("null context");
  if (!u_full || !y) return fail("cmpc_observe_step: null argument");
  if (c->obs_plant < 0) return fail("cmpc_observe_step: call cmpc_observer_init first");
  HIP_TRY(hipSetDevice(c->device));
  if (observer_upload_M(c)) return -1;
  // ObserveAPosteriori + Update: one kernel (the producer runs the
  // a-posteriori update of its slot first, in or_observe_post's order)
  return observer_produce(c, u_full, y, true);
}

int cmpc_observe_apply(cmpc_ctx* c) {
  if (!c) return fail("null context");
  if (c->obs_plant < 0) return fail("cmpc_observe_apply: call cmpc_observer_init first");
  if (c->lin_bound) return fail("cmpc_observe_apply: records are bound externally");
  HIP_TRY(hipSetDevice(c->device));
  ObserverParams P;
  observer_params(c, &P);
  c->pred_stale = "u_old has moved since the build (cmpc_observe_apply applied the first move)";
  TimedLaunch tl(c, CMPC_KERNEL_OBSERVE_PRIOR);
  if (tl.begin()) return -1;
  if (cmpc_launch_observer(P, CMPC_OBS_PRIOR, c->stream))
    return fail("cmpc_observe_apply: no a-priori kernel instantiation for these dimensions");
  if (check_launch("observer a-priori kernel")) return -1;
  c->obs_steps++;  // the delay-block rings advance by one
  return tl.end();
}

// NerveCenter::GetNextInput on the device: cmpc_observe_step + cmpc_step(K,
// 0) + cmpc_observe_apply, as one kernel (cmpc_control_step_kernel) where
// the plan says so, else the three calls.
static int control_step(cmpc_ctx* c, const double* u_full, const double* y, int K, bool* flagged);

int cmpc_control_step(cmpc_ctx* c, const double* u_full, const double* y, int K) {
  return control_step(c, u_full, y, K, nullptr);
}

// flagged (optional): set when the launch stores c->done_seq into
// c->done_host once its results are in place
static int control_step(cmpc_ctx* c, const double* u_full, const double* y, int K, bool* flagged) {
  if (flagged) *flagged = false;
  if (!c) return fail("null context");
  if (!u_full || !y) return fail("cmpc_control_step: null argument");
  if (K < 0) return fail("K must be >= 0");
  if (c->obs_plant < 0) return fail("cmpc_control_step: call cmpc_observer_init first");
  HIP_TRY(hipSetDevice(c->device));
  if (observer_upload_M(c)) return -1;
  const cmpc_plan_t& pl = plan_of(c, K, false, false);
  if (!pl.control_fused) {
    if (cmpc_observe_step(c, u_full, y)) return -1;
    if (cmpc_step(c, K, 0)) return -1;
    return cmpc_observe_apply(c);
  }
  if (ensure_cfg(c)) return -1;
  ControlStepParams C;
  std::memset(&C, 0, sizeof C);
  if (observer_produce_params(c, u_full, y, true, C.pr)) return -1;
  c->lin_bound = nullptr;  // the build reads the produced records
  c->pred_stale = "the records and u_old have changed since the build (cmpc_control_step applied the first move)";
  if (build_params(c, C.b)) return -1;
  C.b.split = pl.control_build_kernel == CMPC_BUILD_SPLIT;
  C.b.grid = pl.control_grid;
  solve_params(c, &C.b.sv);
  C.b.sv.K = K;
  C.b.sv.flags = 0;  // u_old += du is the a-priori phase's
  observer_params(c, &C.ob);
  C.pr_off = cmpc_control_pr_off(C.pr.S, C.pr.rec_len, C.pr.naug);
  const bool flag = flagged && c->done_dev && pl.control_polled;
  C.done = flag ? c->done_dev : nullptr;
  C.seq = flag ? ++c->done_seq : 0u;
  TimedLaunch tl(c, CMPC_KERNEL_STEP);
  if (tl.begin()) return -1;
  if (cmpc_launch_control_step(C, c->d, c->stream)) return plan_mismatch("control step");
  if (check_launch("control step kernel")) return -1;
  c->last_build = pl.control_build_kernel;
  c->last_pair = false;
  c->last_solve = pl.control_solve_kernel;
  c->last_step_fused = 1;
  c->pred_built = true;  // (and stale at once: the a-priori phase has moved u_old)
  c->cert_plans = K > 0;
  c->obs_steps++;  // the delay-block rings advance by one (cmpc_observe_apply)
  if (flagged) *flagged = flag;
  return tl.end();
}

// copies host arrays (nullptr entries skipped) into the context's staging
// buffer on its stream; returns their device addresses
// host arrays of up to this many doubles are read by the kernels in place
static bool stage_in_place(size_t tot) { return tot <= 1024; }

static int stage_host(cmpc_ctx* c, const double* const* host, const size_t* n, int k,
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
static int stage_done(cmpc_ctx* c) {
  return c->pin_in.pending ? 0 : pinned_release(c->pin_in, c->stream);
}

int cmpc_observer_init_host(cmpc_ctx* c, int plant, double p_in, double p_out, double Ts,
                            const int32_t* input_order, const int32_t* out_idx,
                            const double* x_init, const double* u_full, const double* y_init,
                            const double* dx_init) {
  if (!c) return fail("null context");
  int ns = 0, ni = 0, no = 0, nci = 0;
  if (cmpc_plant_dims(plant, &ns, &ni, &no, &nci)) return fail("cmpc_observer_init_host: unknown plant");
  HIP_TRY(hipSetDevice(c->device));
  const size_t B = c->d.B;
  const double* h[4] = {x_init, u_full, y_init, dx_init};
  const size_t n[4] = {B * ns, B * ni, B * no, (size_t)c->nqp * c->L.ntot};
  const double* d[4];
  if (stage_host(c, h, n, 4, d)) return -1;
  const int rc = cmpc_observer_init(c, plant, p_in, p_out, Ts, input_order, out_idx, d[0], d[1], d[2], d[3]);
  return stage_done(c) ? -1 : rc;
}

int cmpc_observe_step_host(cmpc_ctx* c, const double* u_full, const double* y) {
  if (!c) return fail("null context");
  if (c->obs_plant < 0) return fail("cmpc_observe_step_host: call cmpc_observer_init first");
  int ns = 0, ni = 0, no = 0, nci = 0;
  if (cmpc_plant_dims(c->obs_plant, &ns, &ni, &no, &nci)) return fail("unknown plant");
  HIP_TRY(hipSetDevice(c->device));
  const size_t B = c->d.B;
  const double* h[2] = {u_full, y};
  const size_t n[2] = {B * ni, B * no};
  const double* d[2];
  if (stage_host(c, h, n, 2, d)) return -1;
  const int rc = cmpc_observe_step(c, d[0], d[1]);
  return stage_done(c) ? -1 : rc;
}

// cmpc_control_step_host + cmpc_download: a one-workgroup launch signals its
// completion word, which the host polls (the results are in page-locked host
// memory already) instead of a stream synchronisation; anything else, and a
// poll that has not seen the word after a second, synchronises the stream.
int cmpc_control_step_download(cmpc_ctx* c, const double* u_full, const double* y, int K, double* du,
                               int32_t* status, int32_t* nwsr) {
  if (!c) return fail("null context");
  if (c->obs_plant < 0) return fail("cmpc_control_step_download: call cmpc_observer_init first");
  int ns = 0, ni = 0, no = 0, nci = 0;
  if (cmpc_plant_dims(c->obs_plant, &ns, &ni, &no, &nci)) return fail("unknown plant");
  HIP_TRY(hipSetDevice(c->device));
  const size_t B = c->d.B;
  const double* h[2] = {u_full, y};
  const size_t n[2] = {B * ni, B * no};
  const double* d[2];
  if (stage_host(c, h, n, 2, d)) return -1;
  bool flagged = false;
  const int rc = control_step(c, d[0], d[1], K, &flagged);
  if (rc) {
    (void)stage_done(c);
    return -1;
  }
  // (after cmpc_download's stream synchronisation the kernels have read the
  // staged inputs too: no event is needed on that path either)
  auto synced = [&]() {
    if (cmpc_download(c, du, status, nwsr) == 0) return 0;
    (void)stage_done(c);
    return -1;
  };
  if (!flagged || !c->out_host) return synced();
  // polled: the kernel stores the done word after its last read of the
  // staged inputs, so once the word is seen the staging buffer is free and
  // no event need guard it (its record and the next call's wait on it cost
  // ~5 us per B = 1 call: profiles/r6q_b1_noevent_ab.txt)
  const volatile uint32_t* w = c->done_host;
  const uint32_t want = c->done_seq;
  const auto t0 = std::chrono::steady_clock::now();
  long spins = 0;
  while (__atomic_load_n(const_cast<const uint32_t*>(w), __ATOMIC_ACQUIRE) != want) {
    if ((++spins & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(1))
      return synced();  // (the stream synchronisation path)
  }
  const size_t nq = (size_t)c->nqp;
  if (du) std::memcpy(du, c->out_block, sizeof(double) * nq * c->L.nV);
  if (status) std::memcpy(status, c->out_block + c->out_st, sizeof(int32_t) * nq);
  if (nwsr) std::memcpy(nwsr, c->out_block + c->out_nw, sizeof(int32_t) * nq);
  return 0;
}

int cmpc_control_step_host(cmpc_ctx* c, const double* u_full, const double* y, int K) {
  if (!c) return fail("null context");
  if (c->obs_plant < 0) return fail("cmpc_control_step_host: call cmpc_observer_init first");
  int ns = 0, ni = 0, no = 0, nci = 0;
  if (cmpc_plant_dims(c->obs_plant, &ns, &ni, &no, &nci)) return fail("unknown plant");
  HIP_TRY(hipSetDevice(c->device));
  const size_t B = c->d.B;
  const double* h[2] = {u_full, y};
  const size_t n[2] = {B * ni, B * no};
  const double* d[2];
  if (stage_host(c, h, n, 2, d)) return -1;
  const int rc = cmpc_control_step(c, d[0], d[1], K);
  return stage_done(c) ? -1 : rc;
}

// ---- plant simulation ----
struct cmpc_sim {
  int plant = 0, B = 0, device = 0, ns = 0, ni = 0, no = 0, nc = 0, ring_len = 0;
  int cur[CMPC_MAX_INPUTS] = {};  // TimeDelay cursors (every scenario's are the same)
  double p_in = 1.0, p_out = 1.0;
  int delay[CMPC_MAX_INPUTS] = {}, cidx[CMPC_MAX_INPUTS] = {};
  hipStream_t stream = nullptr;
  bool own_stream = false;
  double *x = nullptr, *dt = nullptr, *u_full = nullptr, *u_offset = nullptr, *ring = nullptr,
         *scratch = nullptr, *stage = nullptr;  // stage: host-variant staging (B x max(ns, ni, no, nc))
  int32_t* status = nullptr;
  // per-scenario boundary pressures of the plant (B * 2, [p_in, p_out]) in
  // force, or null: p_in, p_out above.  The simulator's own copy
  // (cmpc_sim_set_pressures[_host], allocated on first use) or a bound array
  const double* pr = nullptr;
  double* own_pr = nullptr;
  // results of the last cmpc_sim_equilibrium (B each, allocated on first use)
  int32_t *eq_status = nullptr, *eq_iters = nullptr;
  double* eq_resid = nullptr;
  // results of the last cmpc_sim_target (status, iters B each, resid B * 2; allocated on first use)
  int32_t *tg_status = nullptr, *tg_iters = nullptr;
  double* tg_resid = nullptr;
  // results of the last cmpc_sim_gains (record B * CMPC_GAIN_LEN, status B; allocated on first use)
  double* gn_record = nullptr;
  int32_t* gn_status = nullptr;
  // results of the last cmpc_sim_modes (allocated on first use): wr, wi B * ns,
  // summary B * CMPC_MODES_NSUM, status and iters B
  double *md_wr = nullptr, *md_wi = nullptr, *md_summary = nullptr;
  int32_t *md_status = nullptr, *md_iters = nullptr;
  PinnedIO pin_in, pin_out;  // host-array calls: page-locked staging
};

int cmpc_sim_create(cmpc_sim** out, int plant, int B, int device, double p_in, double p_out,
                    int n_control, const int32_t* delays, const int32_t* control_index) {
  if (!out || !delays || !control_index) return fail("null argument");
  *out = nullptr;
  int ns = 0, ni = 0, no = 0, nci = 0;
  if (cmpc_plant_dims(plant, &ns, &ni, &no, &nci)) return fail("cmpc_sim_create: unknown plant");
  if (B < 1 || B > (1 << 28)) return fail("cmpc_sim_create: bad batch");
  if (n_control < 1 || n_control > CMPC_MAX_INPUTS) return fail("cmpc_sim_create: bad n_control");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail("no such HIP device");
  cmpc_sim* m = new cmpc_sim();
  m->plant = plant; m->B = B; m->device = device; m->ns = ns; m->ni = ni; m->no = no;
  m->nc = n_control; m->p_in = p_in; m->p_out = p_out;
  for (int i = 0; i < n_control; ++i) {
    if (delays[i] < 0 || control_index[i] < 0 || control_index[i] >= ni) {
      delete m;
      return fail("cmpc_sim_create: bad delay or control index");
    }
    m->delay[i] = delays[i];
    m->cidx[i] = control_index[i];
    m->ring_len += delays[i];
  }
  if (m->ring_len == 0) m->ring_len = 1;
  auto bail = [&](hipError_t e) {
    (void)e;
    void* bufs[] = {m->x, m->dt, m->u_full, m->u_offset, m->ring, m->scratch, m->stage, m->status};
    for (void* b : bufs)
      if (b) (void)hipFree(b);
    delete m;
    return fail("cmpc_sim_create: device allocation failed");
  };
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return bail(e);
  if ((e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking)) != hipSuccess) return bail(e);
  m->own_stream = true;
  const size_t Bz = (size_t)B;
  if ((e = hipMalloc(&m->x, sizeof(double) * Bz * ns)) != hipSuccess ||
      (e = hipMalloc(&m->dt, sizeof(double) * Bz)) != hipSuccess ||
      (e = hipMalloc(&m->u_full, sizeof(double) * Bz * ni)) != hipSuccess ||
      (e = hipMalloc(&m->u_offset, sizeof(double) * Bz * ni)) != hipSuccess ||
      (e = hipMalloc(&m->ring, sizeof(double) * Bz * m->ring_len)) != hipSuccess ||
      (e = hipMalloc(&m->scratch, sizeof(double) * Bz * (ni > n_control ? ni : n_control))) != hipSuccess ||
      (e = hipMalloc(&m->stage, sizeof(double) * Bz * 2 * std::max(std::max(ns, ni), std::max(no, n_control)))) !=
          hipSuccess ||
      (e = hipMalloc(&m->status, sizeof(int32_t) * Bz)) != hipSuccess ||
      (e = hipMemsetAsync(m->status, 0, sizeof(int32_t) * Bz, m->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(m->stream)) != hipSuccess)
    return bail(e);
  *out = m;
  return 0;
}

int cmpc_sim_destroy(cmpc_sim* m) {
  if (!m) return 0;
  (void)hipSetDevice(m->device);
  if (m->stream) (void)hipStreamSynchronize(m->stream);
  pinned_free(m->pin_in);
  pinned_free(m->pin_out);
  void* bufs[] = {m->x, m->dt, m->u_full, m->u_offset, m->ring, m->scratch, m->stage, m->status, m->own_pr,
                  m->eq_status, m->eq_iters, m->eq_resid, m->tg_status, m->tg_iters, m->tg_resid, m->gn_record, m->gn_status, m->md_wr, m->md_wi, m->md_summary, m->md_status,
                  m->md_iters};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  if (m->own_stream && m->stream) (void)hipStreamDestroy(m->stream);
  delete m;
  return 0;
}

int cmpc_sim_set_stream(cmpc_sim* m, void* stream) {
  if (!m) return fail("null simulator");
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (m->own_stream) (void)hipStreamDestroy(m->stream);
  m->stream = (hipStream_t)stream;
  m->own_stream = false;
  return 0;
}

static SimInputParams sim_input_params(cmpc_sim* m, const double* u_control, int use_delay) {
  SimInputParams P;
  std::memset(&P, 0, sizeof P);
  P.u_control = u_control;
  P.u_offset = m->u_offset;
  P.u_full = m->u_full;
  P.ring = m->ring;
  P.B = m->B;
  P.nc = m->nc;
  P.ni = m->ni;
  P.ring_len = m->ring_len;
  P.use_delay = use_delay;
  for (int i = 0; i < m->nc; ++i) {
    P.delay[i] = m->delay[i];
    P.cidx[i] = m->cidx[i];
    P.cur[i] = m->cur[i];
  }
  return P;
}

int cmpc_sim_reset(cmpc_sim* m, const double* x0, const double* u_offset, double dt0) {
  if (!m || !x0 || !u_offset) return fail("null argument");
  if (!(dt0 > 0)) return fail("cmpc_sim_reset: dt0 must be positive");
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B;
  HIP_TRY(hipMemcpyAsync(m->x, x0, sizeof(double) * Bz * m->ns, hipMemcpyDeviceToDevice, m->stream));
  HIP_TRY(hipMemcpyAsync(m->u_offset, u_offset, sizeof(double) * Bz * m->ni, hipMemcpyDeviceToDevice,
                         m->stream));
  std::vector<double> dts(Bz, dt0);
  HIP_TRY(hipMemcpyAsync(m->dt, dts.data(), sizeof(double) * Bz, hipMemcpyHostToDevice, m->stream));
  // TimeDelay(): zero memory, cursor of input i at the sum of the delays before it
  HIP_TRY(hipMemsetAsync(m->ring, 0, sizeof(double) * Bz * m->ring_len, m->stream));
  HIP_TRY(hipMemsetAsync(m->status, 0, sizeof(int32_t) * Bz, m->stream));  // failures are sticky until here
  for (int i = 0, sum = 0; i < m->nc; ++i) {
    m->cur[i] = sum;
    sum += m->delay[i];
  }
  // u_ = GetPlantInput(u_init = 0) = u_offset
  HIP_TRY(hipMemcpyAsync(m->u_full, u_offset, sizeof(double) * Bz * m->ni, hipMemcpyDeviceToDevice,
                         m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));  // (host staging buffers above)
  return 0;
}

int cmpc_sim_set_input(cmpc_sim* m, const double* u_control) {
  if (!m || !u_control) return fail("null argument");
  HIP_TRY(hipSetDevice(m->device));
  const SimInputParams P = sim_input_params(m, u_control, 1);
  if (cmpc_launch_sim_input(P, m->stream)) return fail("sim input launch failed");
  if (check_launch("sim input kernel")) return -1;
  // TimeDelay::GetDelayedInput's cursor step (time_delay.h:41-58), on the host
  for (int i = 0, end = 0; i < m->nc; ++i) {
    if (m->delay[i] == 0) continue;
    end += m->delay[i];
    if (++m->cur[i] == end) m->cur[i] -= m->delay[i];
  }
  return 0;
}

int cmpc_sim_set_offset(cmpc_sim* m, const double* u_offset) {
  if (!m || !u_offset) return fail("null argument");
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipMemcpyAsync(m->u_offset, u_offset, sizeof(double) * (size_t)m->B * m->ni,
                         hipMemcpyDeviceToDevice, m->stream));
  return 0;
}

int cmpc_sim_plant_input_offset(cmpc_sim* m, const double* u_control, const double* u_offset,
                                double* u_full_out) {
  if (!m || !u_control || !u_offset || !u_full_out) return fail("null argument");
  HIP_TRY(hipSetDevice(m->device));
  SimInputParams P = sim_input_params(m, u_control, 0);
  P.u_offset = u_offset;
  P.u_full = u_full_out;
  if (cmpc_launch_sim_input(P, m->stream)) return fail("sim input launch failed");
  return check_launch("sim input kernel");
}

int cmpc_sim_restart(cmpc_sim* m, double dt0) {
  if (!m) return fail("null simulator");
  if (!(dt0 > 0)) return fail("cmpc_sim_restart: dt0 must be positive");
  HIP_TRY(hipSetDevice(m->device));
  std::vector<double> dts((size_t)m->B, dt0);
  HIP_TRY(hipMemcpyAsync(m->dt, dts.data(), sizeof(double) * dts.size(), hipMemcpyHostToDevice, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));  // (host staging buffer)
  return 0;
}

int cmpc_sim_plant_input(cmpc_sim* m, const double* u_control, double* u_full_out) {
  if (!m || !u_control || !u_full_out) return fail("null argument");
  HIP_TRY(hipSetDevice(m->device));
  SimInputParams P = sim_input_params(m, u_control, 0);
  P.u_full = u_full_out;
  if (cmpc_launch_sim_input(P, m->stream)) return fail("sim input launch failed");
  return check_launch("sim input kernel");
}

int cmpc_sim_integrate(cmpc_sim* m, double t, double t_end, double eps_abs, double eps_rel) {
  if (!m) return fail("null simulator");
  if (!(t_end >= t)) return fail("cmpc_sim_integrate: t_end < t");
  HIP_TRY(hipSetDevice(m->device));
  SimParams P;
  std::memset(&P, 0, sizeof P);
  P.x = m->x;
  P.dt = m->dt;
  P.u_full = m->u_full;
  P.status = m->status;
  P.B = m->B;
  P.t = t;
  P.t_end = t_end;
  P.eps_abs = eps_abs;
  P.eps_rel = eps_rel;
  P.p_in = m->p_in;
  P.p_out = m->p_out;
  if (m->pr) {  // the per-scenario instance reads scenario b's pair at this launch
    SimParamsP Q;
    std::memset(&Q, 0, sizeof Q);
    static_cast<SimParams&>(Q) = P;
    Q.pressures = m->pr;
    if (cmpc_launch_sim_pressures(Q, m->plant, m->stream)) return fail("sim launch failed");
    return check_launch("sim kernel (per-scenario pressures)");
  }
  if (cmpc_launch_sim(P, m->plant, m->stream)) return fail("sim launch failed");
  return check_launch("sim kernel");
}

// Per-scenario boundary pressures of the plant (include/cmpc.h)
static int sim_own_pressures(cmpc_sim* m) {
  if (!m->own_pr) HIP_TRY(hipMalloc(&m->own_pr, sizeof(double) * 2 * (size_t)m->B));
  return 0;
}

int cmpc_sim_set_pressures(cmpc_sim* m, const double* pressures_device) {
  if (!m) return fail("null simulator");
  if (!pressures_device) {
    m->pr = nullptr;
    return 0;
  }
  HIP_TRY(hipSetDevice(m->device));
  if (sim_own_pressures(m)) return -1;
  HIP_TRY(hipMemcpyAsync(m->own_pr, pressures_device, sizeof(double) * 2 * (size_t)m->B, hipMemcpyDeviceToDevice,
                         m->stream));
  m->pr = m->own_pr;
  return 0;
}

int cmpc_sim_set_pressures_host(cmpc_sim* m, const double* pressures) {
  if (!m) return fail("null simulator");
  if (!pressures) {
    m->pr = nullptr;
    return 0;
  }
  if (pressures_check("cmpc_sim_set_pressures_host", pressures, (size_t)m->B)) return -1;
  HIP_TRY(hipSetDevice(m->device));
  if (sim_own_pressures(m)) return -1;
  HIP_TRY(hipMemcpyAsync(m->own_pr, pressures, sizeof(double) * 2 * (size_t)m->B, hipMemcpyHostToDevice,
                         m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));  // (the host array is free again)
  m->pr = m->own_pr;
  return 0;
}

int cmpc_sim_bind_pressures(cmpc_sim* m, const double* pressures_device) {
  if (!m) return fail("null simulator");
  if (pressures_device) {
    const size_t bytes = sizeof(double) * 2 * (size_t)m->B;
    hipPointerAttribute_t a;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipPointerGetAttributes(&a, pressures_device) != hipSuccess || a.type != hipMemoryTypeDevice ||
        a.device != m->device ||
        (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)pressures_device) == hipSuccess && base &&
         (uintptr_t)pressures_device + bytes > (uintptr_t)base + size)) {
      (void)hipGetLastError();  // a failed pointer query is not a later launch's error
      return fail("cmpc_sim_bind_pressures: not a device allocation of B * 2 doubles on the simulator's device");
    }
    // one 16-byte load per scenario
    if (reinterpret_cast<uintptr_t>(pressures_device) % 16)
      return fail("cmpc_sim_bind_pressures: the array must be 16-byte aligned");
  }
  m->pr = pressures_device;
  return 0;
}

int cmpc_sim_get_pressures(cmpc_sim* m, double* pressures) {
  if (!m || !pressures) return fail("null argument");
  HIP_TRY(hipSetDevice(m->device));
  if (!m->pr) {  // the scalars of cmpc_sim_create hold for every scenario
    for (int b = 0; b < m->B; ++b) {
      pressures[2 * b] = m->p_in;
      pressures[2 * b + 1] = m->p_out;
    }
    return 0;
  }
  HIP_TRY(hipMemcpyAsync(pressures, m->pr, sizeof(double) * 2 * (size_t)m->B, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return 0;
}

// Plant equilibrium (include/cmpc.h, equilibrium_body.h, equilibrium.hip)
static int equilibrium_check(const char* who, int max_iter, double tol) {
  if (max_iter < 0 || max_iter > CMPC_EQ_MAX_ITER)
    return fail(std::string(who) + ": max_iter must be in [0, " + std::to_string(CMPC_EQ_MAX_ITER) + "]");
  if (!std::isfinite(tol) || !(tol > 0)) return fail(std::string(who) + ": tol must be finite and positive");
  return 0;
}

int cmpc_plant_equilibrium_host(int plant, int B, const double* pressures, const double* u_full, double* x,
                                int max_iter, double tol, int32_t* status, int32_t* iters, double* resid) {
  int ns = 0, ni = 0, no = 0, nci = 0;
  if (cmpc_plant_dims(plant, &ns, &ni, &no, &nci)) return fail("cmpc_plant_equilibrium_host: unknown plant");
  if (B < 1) return fail("cmpc_plant_equilibrium_host: B must be >= 1");
  if (!pressures || !u_full || !x || !status || !iters || !resid)
    return fail("cmpc_plant_equilibrium_host: null argument");
  if (equilibrium_check("cmpc_plant_equilibrium_host", max_iter, tol)) return -1;
  for (size_t b = 0; b < (size_t)B; ++b) {
    const double p_in = pressures[2 * b], p_out = pressures[2 * b + 1];
    status[b] = plant == CMPC_PLANT_PARALLEL
                    ? cmpc_eq::eq_solve<CMPC_PLANT_PARALLEL>(p_in, p_out, u_full + b * ni, x + b * ns, max_iter, tol,
                                                             iters + b, resid + b)
                    : cmpc_eq::eq_solve<CMPC_PLANT_SERIAL>(p_in, p_out, u_full + b * ni, x + b * ns, max_iter, tol,
                                                           iters + b, resid + b);
  }
  return 0;
}

int cmpc_sim_equilibrium(cmpc_sim* m, int max_iter, double tol) {
  if (!m) return fail("cmpc_sim_equilibrium: null simulator");
  if (equilibrium_check("cmpc_sim_equilibrium", max_iter, tol)) return -1;
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B;
  if (!m->eq_status) HIP_TRY(hipMalloc(&m->eq_status, sizeof(int32_t) * Bz));
  if (!m->eq_iters) HIP_TRY(hipMalloc(&m->eq_iters, sizeof(int32_t) * Bz));
  if (!m->eq_resid) HIP_TRY(hipMalloc(&m->eq_resid, sizeof(double) * Bz));
  EquilibriumParams P;
  std::memset(&P, 0, sizeof P);
  P.x = m->x;
  P.u_full = m->u_full;
  P.sim_status = m->status;
  P.pressures = m->pr;  // the per-scenario instance reads scenario b's pair at this launch
  P.status = m->eq_status;
  P.iters = m->eq_iters;
  P.resid = m->eq_resid;
  P.B = m->B;
  P.max_iter = max_iter;
  P.tol = tol;
  P.p_in = m->p_in;
  P.p_out = m->p_out;
  if (cmpc_launch_equilibrium(P, m->plant, m->stream)) return fail("equilibrium launch failed");
  return check_launch("equilibrium kernel");
}

int cmpc_sim_equilibrium_download(cmpc_sim* m, int32_t* status, int32_t* iters, double* resid) {
  if (!m) return fail("cmpc_sim_equilibrium_download: null simulator");
  if (!m->eq_status) return fail("cmpc_sim_equilibrium_download: call cmpc_sim_equilibrium first");
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B, bi = sizeof(int32_t) * Bz, br = sizeof(double) * Bz;
  auto up = [](size_t v) { return (v + 15) / 16 * 16; };
  const size_t oi = up(br), os = oi + up(bi);
  if (pinned_acquire(m->pin_out, os + bi)) return -1;
  char* h = m->pin_out.buf;
  if (resid) HIP_TRY(hipMemcpyAsync(h, m->eq_resid, br, hipMemcpyDeviceToHost, m->stream));
  if (iters) HIP_TRY(hipMemcpyAsync(h + oi, m->eq_iters, bi, hipMemcpyDeviceToHost, m->stream));
  if (status) HIP_TRY(hipMemcpyAsync(h + os, m->eq_status, bi, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (resid) std::memcpy(resid, h, br);
  if (iters) std::memcpy(iters, h + oi, bi);
  if (status) std::memcpy(status, h + os, bi);
  return 0;
}

int32_t* cmpc_sim_equilibrium_status(cmpc_sim* m) { return m ? m->eq_status : nullptr; }
int32_t* cmpc_sim_equilibrium_iters(cmpc_sim* m) { return m ? m->eq_iters : nullptr; }
double* cmpc_sim_equilibrium_resid(cmpc_sim* m) { return m ? m->eq_resid : nullptr; }

// Steady-state target solve (include/cmpc.h, target_body.h, target.hip)
int cmpc_target_check(int plant, int nh, const int32_t* hold_idx, const int32_t* free_idx, int max_iter,
                      double tol_f, double tol_y) {
  int ns = 0, ni = 0, no = 0, nci = 0;
  if (cmpc_plant_dims(plant, &ns, &ni, &no, &nci)) return fail("cmpc_target_check: unknown plant");
  if (nh < 0 || nh > cmpc_tg::kMaxHold)
    return fail("cmpc_target_check: nh must be in [0, " + std::to_string(cmpc_tg::kMaxHold) + "]");
  if (nh > 0 && (!hold_idx || !free_idx)) return fail("cmpc_target_check: null index array");
  for (int j = 0; j < nh; ++j) {
    if (hold_idx[j] < 0 || hold_idx[j] >= 4)
      return fail("cmpc_target_check: hold_idx[" + std::to_string(j) + "] is not a plant output in [0, 4)");
    if (free_idx[j] < 0 || free_idx[j] >= 4)
      return fail("cmpc_target_check: free_idx[" + std::to_string(j) + "] is not a control input in [0, 4)");
    for (int i = 0; i < j; ++i) {
      if (hold_idx[i] == hold_idx[j])
        return fail("cmpc_target_check: hold_idx repeats output " + std::to_string(hold_idx[j]));
      if (free_idx[i] == free_idx[j])
        return fail("cmpc_target_check: free_idx repeats control input " + std::to_string(free_idx[j]));
    }
  }
  if (max_iter < 0 || max_iter > CMPC_EQ_MAX_ITER)
    return fail("cmpc_target_check: max_iter must be in [0, " + std::to_string(CMPC_EQ_MAX_ITER) + "]");
  if (!std::isfinite(tol_f) || !(tol_f > 0)) return fail("cmpc_target_check: tol_f must be finite and positive");
  if (!std::isfinite(tol_y) || !(tol_y > 0)) return fail("cmpc_target_check: tol_y must be finite and positive");
  return 0;
}

int cmpc_plant_target_host(int plant, int B, const double* pressures, int nh, const int32_t* hold_idx,
                           const int32_t* free_idx, const double* targets, double* u_full, double* x, int max_iter,
                           double tol_f, double tol_y, int32_t* status, int32_t* iters, double* resid) {
  if (cmpc_target_check(plant, nh, hold_idx, free_idx, max_iter, tol_f, tol_y)) return -1;
  int ns = 0, ni = 0, no = 0, nci = 0;
  (void)cmpc_plant_dims(plant, &ns, &ni, &no, &nci);
  if (B < 1) return fail("cmpc_plant_target_host: B must be >= 1");
  if (!pressures || !u_full || !x || !status || !iters || !resid || (nh > 0 && !targets))
    return fail("cmpc_plant_target_host: null argument");
  for (size_t b = 0; b < (size_t)B; ++b) {
    const double p_in = pressures[2 * b], p_out = pressures[2 * b + 1];
    const double* t = nh > 0 ? targets + b * nh : nullptr;
    status[b] = plant == CMPC_PLANT_PARALLEL
                    ? cmpc_tg::tg_solve<CMPC_PLANT_PARALLEL>(p_in, p_out, nh, hold_idx, free_idx, t, u_full + b * ni,
                                                             x + b * ns, max_iter, tol_f, tol_y, iters + b,
                                                             resid + 2 * b)
                    : cmpc_tg::tg_solve<CMPC_PLANT_SERIAL>(p_in, p_out, nh, hold_idx, free_idx, t, u_full + b * ni,
                                                           x + b * ns, max_iter, tol_f, tol_y, iters + b,
                                                           resid + 2 * b);
  }
  return 0;
}

int cmpc_sim_target(cmpc_sim* m, int nh, const int32_t* hold_idx, const int32_t* free_idx,
                    const double* targets_device, int max_iter, double tol_f, double tol_y) {
  if (!m) return fail("cmpc_sim_target: null simulator");
  if (cmpc_target_check(m->plant, nh, hold_idx, free_idx, max_iter, tol_f, tol_y)) return -1;
  if (nh > 0 && !targets_device) return fail("cmpc_sim_target: null targets");
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B;
  if (!m->tg_status) HIP_TRY(hipMalloc(&m->tg_status, sizeof(int32_t) * Bz));
  if (!m->tg_iters) HIP_TRY(hipMalloc(&m->tg_iters, sizeof(int32_t) * Bz));
  if (!m->tg_resid) HIP_TRY(hipMalloc(&m->tg_resid, sizeof(double) * 2 * Bz));
  TargetParams P;
  std::memset(&P, 0, sizeof P);
  P.x = m->x;
  P.u_full = m->u_full;
  P.u_offset = m->u_offset;
  P.targets = nh > 0 ? targets_device : nullptr;
  P.sim_status = m->status;
  P.pressures = m->pr;  // the per-scenario instance reads scenario b's pair at this launch
  P.status = m->tg_status;
  P.iters = m->tg_iters;
  P.resid = m->tg_resid;
  P.B = m->B;
  P.max_iter = max_iter;
  P.nh = nh;
  for (int j = 0; j < nh; ++j) {
    P.hold[j] = hold_idx[j];
    P.fre[j] = free_idx[j];
  }
  P.tol_f = tol_f;
  P.tol_y = tol_y;
  P.p_in = m->p_in;
  P.p_out = m->p_out;
  if (cmpc_launch_target(P, m->plant, m->stream)) return fail("target launch failed");
  return check_launch("target kernel");
}

int cmpc_sim_target_host(cmpc_sim* m, int nh, const int32_t* hold_idx, const int32_t* free_idx,
                         const double* targets, int max_iter, double tol_f, double tol_y) {
  if (!m) return fail("cmpc_sim_target_host: null simulator");
  if (cmpc_target_check(m->plant, nh, hold_idx, free_idx, max_iter, tol_f, tol_y)) return -1;
  if (nh > 0 && !targets) return fail("cmpc_sim_target_host: null targets");
  HIP_TRY(hipSetDevice(m->device));
  // the staging buffer holds 2 * max(ns, ni, no, nc) >= nh doubles per scenario
  if (nh > 0)
    HIP_TRY(hipMemcpyAsync(m->stage, targets, sizeof(double) * (size_t)m->B * nh, hipMemcpyHostToDevice, m->stream));
  const int rc = cmpc_sim_target(m, nh, hold_idx, free_idx, m->stage, max_iter, tol_f, tol_y);
  HIP_TRY(hipStreamSynchronize(m->stream));  // (the host array is free again)
  return rc;
}

int cmpc_sim_target_download(cmpc_sim* m, int32_t* status, int32_t* iters, double* resid) {
  if (!m) return fail("cmpc_sim_target_download: null simulator");
  if (!m->tg_status) return fail("cmpc_sim_target_download: call cmpc_sim_target first");
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B, bi = sizeof(int32_t) * Bz, br = sizeof(double) * 2 * Bz;
  auto up = [](size_t v) { return (v + 15) / 16 * 16; };
  const size_t oi = up(br), os = oi + up(bi);
  if (pinned_acquire(m->pin_out, os + bi)) return -1;
  char* h = m->pin_out.buf;
  if (resid) HIP_TRY(hipMemcpyAsync(h, m->tg_resid, br, hipMemcpyDeviceToHost, m->stream));
  if (iters) HIP_TRY(hipMemcpyAsync(h + oi, m->tg_iters, bi, hipMemcpyDeviceToHost, m->stream));
  if (status) HIP_TRY(hipMemcpyAsync(h + os, m->tg_status, bi, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (resid) std::memcpy(resid, h, br);
  if (iters) std::memcpy(iters, h + oi, bi);
  if (status) std::memcpy(status, h + os, bi);
  return 0;
}

int32_t* cmpc_sim_target_status(cmpc_sim* m) { return m ? m->tg_status : nullptr; }
int32_t* cmpc_sim_target_iters(cmpc_sim* m) { return m ? m->tg_iters : nullptr; }
double* cmpc_sim_target_resid(cmpc_sim* m) { return m ? m->tg_resid : nullptr; }

// Steady-state gains, RGA and pressure feed-forward (include/cmpc.h, gains_body.h, gains.hip)
int cmpc_gain_check(int plant, int ny, const int32_t* out_idx, int nu, const int32_t* in_idx) {
  int ns = 0, ni = 0, no = 0, nci = 0;
  if (cmpc_plant_dims(plant, &ns, &ni, &no, &nci)) return fail("cmpc_gain_check: unknown plant");
  if (ny < 1 || ny > cmpc_gn::kMaxSel)
    return fail("cmpc_gain_check: ny must be in [1, " + std::to_string(cmpc_gn::kMaxSel) + "]");
  if (nu < 1 || nu > cmpc_gn::kMaxSel)
    return fail("cmpc_gain_check: nu must be in [1, " + std::to_string(cmpc_gn::kMaxSel) + "]");
  if (!out_idx || !in_idx) return fail("cmpc_gain_check: null index array");
  for (int j = 0; j < ny; ++j) {
    if (out_idx[j] < 0 || out_idx[j] >= 4)
      return fail("cmpc_gain_check: out_idx[" + std::to_string(j) + "] is not a plant output in [0, 4)");
    for (int i = 0; i < j; ++i)
      if (out_idx[i] == out_idx[j])
        return fail("cmpc_gain_check: out_idx repeats output " + std::to_string(out_idx[j]));
  }
  for (int j = 0; j < nu; ++j) {
    if (in_idx[j] < 0 || in_idx[j] >= 4)
      return fail("cmpc_gain_check: in_idx[" + std::to_string(j) + "] is not a control input in [0, 4)");
    for (int i = 0; i < j; ++i)
      if (in_idx[i] == in_idx[j])
        return fail("cmpc_gain_check: in_idx repeats control input " + std::to_string(in_idx[j]));
  }
  return 0;
}

int cmpc_plant_gains_host(int plant, int B, const double* pressures, const double* u_full, const double* x, int ny,
                          const int32_t* out_idx, int nu, const int32_t* in_idx, double* record, int32_t* status) {
  if (cmpc_gain_check(plant, ny, out_idx, nu, in_idx)) return -1;
  int ns = 0, ni = 0, no = 0, nci = 0;
  (void)cmpc_plant_dims(plant, &ns, &ni, &no, &nci);
  if (B < 1) return fail("cmpc_plant_gains_host: B must be >= 1");
  if (!pressures || !u_full || !x || !record || !status) return fail("cmpc_plant_gains_host: null argument");
  for (size_t b = 0; b < (size_t)B; ++b) {
    const double p_in = pressures[2 * b], p_out = pressures[2 * b + 1];
    double* rec = record + b * CMPC_GAIN_LEN;
    status[b] = plant == CMPC_PLANT_PARALLEL
                    ? cmpc_gn::gn_solve<CMPC_PLANT_PARALLEL>(p_in, p_out, ny, out_idx, nu, in_idx, u_full + b * ni,
                                                             x + b * ns, rec)
                    : cmpc_gn::gn_solve<CMPC_PLANT_SERIAL>(p_in, p_out, ny, out_idx, nu, in_idx, u_full + b * ni,
                                                           x + b * ns, rec);
  }
  return 0;
}

int cmpc_sim_gains(cmpc_sim* m, int ny, const int32_t* out_idx, int nu, const int32_t* in_idx) {
  if (!m) return fail("cmpc_sim_gains: null simulator");
  if (cmpc_gain_check(m->plant, ny, out_idx, nu, in_idx)) return -1;
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B;
  if (!m->gn_record) HIP_TRY(hipMalloc(&m->gn_record, sizeof(double) * CMPC_GAIN_LEN * Bz));
  if (!m->gn_status) HIP_TRY(hipMalloc(&m->gn_status, sizeof(int32_t) * Bz));
  GainsParams P;
  std::memset(&P, 0, sizeof P);
  P.x = m->x;
  P.u_full = m->u_full;
  P.sim_status = m->status;
  P.pressures = m->pr;  // the per-scenario instance reads scenario b's pair at this launch
  P.record = m->gn_record;
  P.status = m->gn_status;
  P.B = m->B;
  P.ny = ny;
  P.nu = nu;
  for (int j = 0; j < ny; ++j) P.out[j] = out_idx[j];
  for (int j = 0; j < nu; ++j) P.in[j] = in_idx[j];
  P.p_in = m->p_in;
  P.p_out = m->p_out;
  if (cmpc_launch_gains(P, m->plant, m->stream)) return fail("gains launch failed");
  return check_launch("gains kernel");
}

int cmpc_sim_gains_download(cmpc_sim* m, double* record, int32_t* status) {
  if (!m) return fail("cmpc_sim_gains_download: null simulator");
  if (!m->gn_status) return fail("cmpc_sim_gains_download: call cmpc_sim_gains first");
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B, br = sizeof(double) * CMPC_GAIN_LEN * Bz, bi = sizeof(int32_t) * Bz;
  auto up = [](size_t v) { return (v + 15) / 16 * 16; };
  const size_t os = up(br);
  if (pinned_acquire(m->pin_out, os + bi)) return -1;
  char* h = m->pin_out.buf;
  if (record) HIP_TRY(hipMemcpyAsync(h, m->gn_record, br, hipMemcpyDeviceToHost, m->stream));
  if (status) HIP_TRY(hipMemcpyAsync(h + os, m->gn_status, bi, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (record) std::memcpy(record, h, br);
  if (status) std::memcpy(status, h + os, bi);
  return 0;
}

double* cmpc_sim_gains_record(cmpc_sim* m) { return m ? m->gn_record : nullptr; }
int32_t* cmpc_sim_gains_status(cmpc_sim* m) { return m ? m->gn_status : nullptr; }

// Eigenvalues and plant modes (include/cmpc.h, eig_body.h, eig.hip)
static int eig_check(const char* who, int max_iter) {
  if (max_iter < 1 || max_iter > CMPC_EIG_MAX_ITER)
    return fail(std::string(who) + ": max_iter must be in [1, " + std::to_string(CMPC_EIG_MAX_ITER) + "]");
  return 0;
}

int cmpc_eig_host(int n, int B, const double* A, int max_iter, double* wr, double* wi, int32_t* status,
                  int32_t* iters) {
  if (n < 1 || n > CMPC_EIG_MAX_N)
    return fail("cmpc_eig_host: n must be in [1, " + std::to_string(CMPC_EIG_MAX_N) + "]");
  if (B < 1) return fail("cmpc_eig_host: B must be >= 1");
  if (!A || !wr || !wi || !status || !iters) return fail("cmpc_eig_host: null argument");
  if (eig_check("cmpc_eig_host", max_iter)) return -1;
  const size_t nz = (size_t)n;
  for (size_t b = 0; b < (size_t)B; ++b)
    status[b] = cmpc_eig::eig_host(n, A + b * nz * nz, max_iter, wr + b * nz, wi + b * nz, iters + b, nullptr);
  return 0;
}

int cmpc_eig_device(int n, int B, const double* A, int max_iter, double* wr, double* wi, int32_t* status,
                    int32_t* iters, void* stream) {
  if (n != 10 && n != 11) return fail("cmpc_eig_device: n must be 10 or 11");
  if (B < 1) return fail("cmpc_eig_device: B must be >= 1");
  if (!A || !wr || !wi || !status || !iters) return fail("cmpc_eig_device: null argument");
  if (eig_check("cmpc_eig_device", max_iter)) return -1;
  EigParams P;
  std::memset(&P, 0, sizeof P);
  P.A = A;
  P.wr = wr;
  P.wi = wi;
  P.status = status;
  P.iters = iters;
  P.B = B;
  P.max_iter = max_iter;
  if (cmpc_launch_eig(P, n, stream)) return fail("cmpc_eig_device: launch failed");
  return check_launch("eig kernel");
}

int cmpc_modes_summary_host(int n, int B, const double* wr, const double* wi, const int32_t* status,
                            double* summary) {
  if (n < 1 || n > CMPC_EIG_MAX_N)
    return fail("cmpc_modes_summary_host: n must be in [1, " + std::to_string(CMPC_EIG_MAX_N) + "]");
  if (B < 1) return fail("cmpc_modes_summary_host: B must be >= 1");
  if (!wr || !wi || !status || !summary) return fail("cmpc_modes_summary_host: null argument");
  for (size_t b = 0; b < (size_t)B; ++b)
    cmpc_eig::eig_summary(n, wr + b * n, wi + b * n, status[b] == CMPC_EIG_OK, summary + b * CMPC_MODES_NSUM);
  return 0;
}

extern "C++" {
template <int PLANT>
static int plant_modes_one(double p_in, double p_out, const double* u, const double* x, int max_iter, double* wr,
                           double* wi, double* summary, int32_t* iters) {
  constexpr int ns = cmpc_eq::Dims<PLANT>::ns;
  double A[ns * ns], Bm[ns * 4], C[4 * ns], f[ns];
  cmpc_eq::eq_linearize<PLANT>(p_in, p_out, x, u, A, Bm, C, f);
  return cmpc_eig::eig_host_one<ns>(A, max_iter, wr, wi, iters, summary);
}
}  // extern "C++"

int cmpc_plant_modes_host(int plant, int B, const double* pressures, const double* u_full, const double* x,
                          int max_iter, double* wr, double* wi, double* summary, int32_t* status, int32_t* iters) {
  int ns = 0, ni = 0, no = 0, nci = 0;
  if (cmpc_plant_dims(plant, &ns, &ni, &no, &nci)) return fail("cmpc_plant_modes_host: unknown plant");
  if (B < 1) return fail("cmpc_plant_modes_host: B must be >= 1");
  if (!pressures || !u_full || !x || !wr || !wi || !summary || !status || !iters)
    return fail("cmpc_plant_modes_host: null argument");
  if (eig_check("cmpc_plant_modes_host", max_iter)) return -1;
  for (size_t b = 0; b < (size_t)B; ++b) {
    const double p_in = pressures[2 * b], p_out = pressures[2 * b + 1];
    double *r = wr + b * ns, *i = wi + b * ns, *s = summary + b * CMPC_MODES_NSUM;
    status[b] = plant == CMPC_PLANT_PARALLEL
                    ? plant_modes_one<CMPC_PLANT_PARALLEL>(p_in, p_out, u_full + b * ni, x + b * ns, max_iter, r, i, s,
                                                           iters + b)
                    : plant_modes_one<CMPC_PLANT_SERIAL>(p_in, p_out, u_full + b * ni, x + b * ns, max_iter, r, i, s,
                                                         iters + b);
  }
  return 0;
}

int cmpc_sim_modes(cmpc_sim* m, int max_iter) {
  if (!m) return fail("cmpc_sim_modes: null simulator");
  if (eig_check("cmpc_sim_modes", max_iter)) return -1;
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B;
  if (!m->md_wr) HIP_TRY(hipMalloc(&m->md_wr, sizeof(double) * Bz * m->ns));
  if (!m->md_wi) HIP_TRY(hipMalloc(&m->md_wi, sizeof(double) * Bz * m->ns));
  if (!m->md_summary) HIP_TRY(hipMalloc(&m->md_summary, sizeof(double) * Bz * CMPC_MODES_NSUM));
  if (!m->md_status) HIP_TRY(hipMalloc(&m->md_status, sizeof(int32_t) * Bz));
  if (!m->md_iters) HIP_TRY(hipMalloc(&m->md_iters, sizeof(int32_t) * Bz));
  ModesParams P;
  std::memset(&P, 0, sizeof P);
  P.x = m->x;
  P.u_full = m->u_full;
  P.sim_status = m->status;
  P.pressures = m->pr;  // the per-scenario instance reads scenario b's pair at this launch
  P.wr = m->md_wr;
  P.wi = m->md_wi;
  P.summary = m->md_summary;
  P.status = m->md_status;
  P.iters = m->md_iters;
  P.B = m->B;
  P.max_iter = max_iter;
  P.p_in = m->p_in;
  P.p_out = m->p_out;
  if (cmpc_launch_modes(P, m->plant, m->stream)) return fail("modes launch failed");
  return check_launch("modes kernel");
}

int cmpc_sim_modes_download(cmpc_sim* m, double* wr, double* wi, double* summary, int32_t* status,
                            int32_t* iters) {
  if (!m) return fail("cmpc_sim_modes_download: null simulator");
  if (!m->md_status) return fail("cmpc_sim_modes_download: call cmpc_sim_modes first");
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B, bw = sizeof(double) * Bz * m->ns, bs = sizeof(double) * Bz * CMPC_MODES_NSUM,
               bi = sizeof(int32_t) * Bz;
  auto up = [](size_t v) { return (v + 15) / 16 * 16; };
  const size_t o_wi = up(bw), o_sm = o_wi + up(bw), o_st = o_sm + up(bs), o_it = o_st + up(bi);
  if (pinned_acquire(m->pin_out, o_it + bi)) return -1;
  char* h = m->pin_out.buf;
  if (wr) HIP_TRY(hipMemcpyAsync(h, m->md_wr, bw, hipMemcpyDeviceToHost, m->stream));
  if (wi) HIP_TRY(hipMemcpyAsync(h + o_wi, m->md_wi, bw, hipMemcpyDeviceToHost, m->stream));
  if (summary) HIP_TRY(hipMemcpyAsync(h + o_sm, m->md_summary, bs, hipMemcpyDeviceToHost, m->stream));
  if (status) HIP_TRY(hipMemcpyAsync(h + o_st, m->md_status, bi, hipMemcpyDeviceToHost, m->stream));
  if (iters) HIP_TRY(hipMemcpyAsync(h + o_it, m->md_iters, bi, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (wr) std::memcpy(wr, h, bw);
  if (wi) std::memcpy(wi, h + o_wi, bw);
  if (summary) std::memcpy(summary, h + o_sm, bs);
  if (status) std::memcpy(status, h + o_st, bi);
  if (iters) std::memcpy(iters, h + o_it, bi);
  return 0;
}

double* cmpc_sim_modes_wr(cmpc_sim* m) { return m ? m->md_wr : nullptr; }
double* cmpc_sim_modes_wi(cmpc_sim* m) { return m ? m->md_wi : nullptr; }
double* cmpc_sim_modes_summary(cmpc_sim* m) { return m ? m->md_summary : nullptr; }
int32_t* cmpc_sim_modes_status(cmpc_sim* m) { return m ? m->md_status : nullptr; }
int32_t* cmpc_sim_modes_iters(cmpc_sim* m) { return m ? m->md_iters : nullptr; }

int cmpc_sim_output(cmpc_sim* m, double* y) {
  if (!m || !y) return fail("null argument");
  HIP_TRY(hipSetDevice(m->device));
  if (cmpc_launch_sim_output(m->plant, m->x, y, m->B, m->stream)) return fail("sim output launch failed");
  return check_launch("sim output kernel");
}

int cmpc_sim_download(cmpc_sim* m, double* x, double* u_full, double* dt, int32_t* status) {
  if (!m) return fail("null simulator");
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B;
  const size_t bx = sizeof(double) * Bz * m->ns, bu = sizeof(double) * Bz * m->ni, bd = sizeof(double) * Bz,
               bs = sizeof(int32_t) * Bz;
  auto up = [](size_t v) { return (v + 15) / 16 * 16; };
  const size_t ou = up(bx), od = ou + up(bu), os = od + up(bd);
  // device -> page-locked buffer (DMA), then host copies after one sync
  if (pinned_acquire(m->pin_out, os + bs)) return -1;
  char* h = m->pin_out.buf;
  if (x) HIP_TRY(hipMemcpyAsync(h, m->x, bx, hipMemcpyDeviceToHost, m->stream));
  if (u_full) HIP_TRY(hipMemcpyAsync(h + ou, m->u_full, bu, hipMemcpyDeviceToHost, m->stream));
  if (dt) HIP_TRY(hipMemcpyAsync(h + od, m->dt, bd, hipMemcpyDeviceToHost, m->stream));
  if (status) HIP_TRY(hipMemcpyAsync(h + os, m->status, bs, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (x) std::memcpy(x, h, bx);
  if (u_full) std::memcpy(u_full, h + ou, bu);
  if (dt) std::memcpy(dt, h + od, bd);
  if (status) std::memcpy(status, h + os, bs);
  return 0;
}

// Host-array variants: stage through the simulator's device buffer; each
// returns once the call's work is done (the host arrays are free again).
static int sim_stage(cmpc_sim* m, const double* h0, size_t n0, const double* h1, size_t n1) {
  HIP_TRY(hipSetDevice(m->device));
  const size_t half = (size_t)m->B * std::max(std::max(m->ns, m->ni), std::max(m->no, m->nc));
  // one DMA from page-locked memory: h0 at stage, h1 at stage + half
  const size_t tot = n1 ? half + n1 : n0;
  if (pinned_acquire(m->pin_in, sizeof(double) * std::max<size_t>(tot, 1))) return -1;
  double* h = reinterpret_cast<double*>(m->pin_in.buf);
  if (n0) std::memcpy(h, h0, sizeof(double) * n0);
  if (n1) std::memcpy(h + half, h1, sizeof(double) * n1);
  if (tot) HIP_TRY(hipMemcpyAsync(m->stage, h, sizeof(double) * tot, hipMemcpyHostToDevice, m->stream));
  return pinned_release(m->pin_in, m->stream);
}

int cmpc_sim_reset_host(cmpc_sim* m, const double* x0, const double* u_offset, double dt0) {
  if (!m || !x0 || !u_offset) return fail("null argument");
  const size_t half = (size_t)m->B * std::max(std::max(m->ns, m->ni), std::max(m->no, m->nc));
  if (sim_stage(m, x0, (size_t)m->B * m->ns, u_offset, (size_t)m->B * m->ni)) return -1;
  return cmpc_sim_reset(m, m->stage, m->stage + half, dt0);  // (synchronises)
}

int cmpc_sim_set_input_host(cmpc_sim* m, const double* u_control) {
  if (!m || !u_control) return fail("null argument");
  if (sim_stage(m, u_control, (size_t)m->B * m->nc, nullptr, 0)) return -1;
  if (cmpc_sim_set_input(m, m->stage)) return -1;
  return cmpc_sim_synchronize(m);
}

int cmpc_sim_set_offset_host(cmpc_sim* m, const double* u_offset) {
  if (!m || !u_offset) return fail("null argument");
  if (sim_stage(m, u_offset, (size_t)m->B * m->ni, nullptr, 0)) return -1;
  if (cmpc_sim_set_offset(m, m->stage)) return -1;
  return cmpc_sim_synchronize(m);
}

int cmpc_sim_output_host(cmpc_sim* m, double* y) {
  if (!m || !y) return fail("null argument");
  HIP_TRY(hipSetDevice(m->device));
  const size_t by = sizeof(double) * (size_t)m->B * m->no;
  if (pinned_acquire(m->pin_out, by)) return -1;
  if (cmpc_sim_output(m, m->stage)) return -1;
  HIP_TRY(hipMemcpyAsync(m->pin_out.buf, m->stage, by, hipMemcpyDeviceToHost, m->stream));
  if (cmpc_sim_synchronize(m)) return -1;
  std::memcpy(y, m->pin_out.buf, by);
  return 0;
}

double* cmpc_sim_state(cmpc_sim* m) { return m ? m->x : nullptr; }
double* cmpc_sim_input(cmpc_sim* m) { return m ? m->u_full : nullptr; }
double* cmpc_sim_step_size(cmpc_sim* m) { return m ? m->dt : nullptr; }
int32_t* cmpc_sim_status(cmpc_sim* m) { return m ? m->status : nullptr; }
int cmpc_sim_delay_len(cmpc_sim* m) { return m ? m->ring_len : -1; }

int cmpc_sim_download_inputs(cmpc_sim* m, double* u_offset, double* delay_line) {
  if (!m) return fail("null simulator");
  HIP_TRY(hipSetDevice(m->device));
  const size_t Bz = (size_t)m->B;
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (u_offset) HIP_TRY(hipMemcpy(u_offset, m->u_offset, sizeof(double) * Bz * m->ni, hipMemcpyDeviceToHost));
  if (delay_line) HIP_TRY(hipMemcpy(delay_line, m->ring, sizeof(double) * Bz * m->ring_len, hipMemcpyDeviceToHost));
  return 0;
}

int cmpc_sim_synchronize(cmpc_sim* m) {
  if (!m) return fail("null simulator");
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return 0;
}

// NerveCenter::UpdateUOld at the nerve level (nerve_center.h:313-319): the
// control input u_old_ (B x nu_tot, plant control order) += every
// sub-controller's first move of its own inputs (ControlInputIndices order)
int cmpc_accumulate_moves(cmpc_ctx* c, const int32_t* input_order, double* u_control) {
  if (!c || !input_order || !u_control) return fail("null argument");
  const cmpc_dims& d = c->d;
  if (d.S > CMPC_MAX_S_PRODUCE) return fail("cmpc_accumulate_moves: too many sub-controllers");
  AccumParams P;
  std::memset(&P, 0, sizeof P);
  P.du = c->du_old;
  P.u_control = u_control;
  P.B = d.B;
  P.S = d.S;
  P.nu = d.nu;
  P.nu_tot = d.nu_tot;
  P.nV = c->L.nV;
  for (int s = 0; s < d.S; ++s)
    for (int k = 0; k < d.nu; ++k) {
      const int v = input_order[s * d.nu_tot + k];
      if (v < 0 || v >= d.nu_tot) return fail("cmpc_accumulate_moves: bad input_order");
      P.order[s][k] = v;
    }
  HIP_TRY(hipSetDevice(c->device));
  if (cmpc_launch_accumulate(P, c->stream)) return fail("accumulate launch failed");
  return check_launch("accumulate kernel");
}

// Rows between the device layout (delay blocks as rings, rotated by the
// a-priori step count, cmpc_obs_prior_kernel) and the logical layout of the
// ABI (observer.h's AugmentedState order).  to_logical: device -> logical.
static void observer_rows_rotate(cmpc_ctx* c, const double* in, double* out, bool to_logical) {
  ObserverParams O;
  observer_params(c, &O);
  const size_t n = (size_t)c->nqp, len = c->obs_len;
  std::memcpy(out, in, sizeof(double) * n * len);
  for (int k = 0; k < O.nd; ++k) {
    const int L = O.delay[O.dinput[k]] - 1, r = O.rot[k];
    if (L < 2 || r == 0) continue;
    const size_t b0 = (size_t)c->d.ns + O.blk[k];  // row offset of the block (after x_hat)
    for (size_t q = 0; q < n; ++q)
      for (int i = 0; i < L; ++i) {
        const size_t phys = b0 + (i + r) % L, logi = b0 + i;
        if (to_logical) out[q * len + logi] = in[q * len + phys];
        else out[q * len + phys] = in[q * len + logi];
      }
  }
}

int cmpc_get_observer_state(cmpc_ctx* c, double* host) {
  if (!c || !host) return fail("null argument");
  if (!c->obs) return fail("no observer state (cmpc_set_observer)");
  HIP_TRY(hipSetDevice(c->device));
  std::vector<double> dev((size_t)c->nqp * c->obs_len);
  HIP_TRY(hipMemcpyAsync(dev.data(), c->obs, sizeof(double) * dev.size(), hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  observer_rows_rotate(c, dev.data(), host, true);
  return 0;
}

int cmpc_set_observer_state(cmpc_ctx* c, const double* host) {
  if (!c || !host) return fail("null argument");
  if (!c->obs) return fail("no observer state (cmpc_set_observer)");
  HIP_TRY(hipSetDevice(c->device));
  std::vector<double> dev((size_t)c->nqp * c->obs_len);
  observer_rows_rotate(c, host, dev.data(), false);
  HIP_TRY(hipMemcpyAsync(c->obs, dev.data(), sizeof(double) * dev.size(), hipMemcpyHostToDevice,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
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

// whether this cmpc_build runs the shared form of the row build; <0: an error
static int build_uses_pairing(cmpc_ctx* c, const BuildParams& P, const cmpc_plan_t& pl) {
  if (c->pairing == CMPC_PAIRING_OFF || pl.build_kernel != CMPC_BUILD_ROWS) return 0;
  const double* lw0 = c->h_cfg.data() + c->co.lwt;
  const double* lw1 = c->d.S > 1 ? lw0 + c->co.len : lw0;
  const char* e = cmpc_pairing_error(c->d, P, lw0, lw1);
  if (c->pairing == CMPC_PAIRING_ON) return e ? fail(std::string("cmpc_build (CMPC_PAIRING_ON): ") + e) : 1;
  return !e && cmpc_pairing_auto(c->d.B) ? 1 : 0;
}

int cmpc_build(cmpc_ctx* c) {
  if (!c) return fail("null context");
  if (ensure_cfg(c)) return -1;
  if (c->sc_w && ensure_yref(c)) return -1;
  HIP_TRY(hipSetDevice(c->device));
  BuildParams P;
  if (build_params(c, P)) return -1;
  const cmpc_plan_t& pl = plan_of(c, 0, false, false);
  if (pl.build_error) return fail(cmpc_plan_error_string(pl.build_error));
  const int pair = build_uses_pairing(c, P, pl);
  if (pair < 0) return -1;
  if (pair) {
    if (!c->pair_cnt) {
      HIP_TRY(hipMalloc(&c->pair_cnt, 2 * sizeof(uint32_t)));
      HIP_TRY(hipMemsetAsync(c->pair_cnt, 0, 2 * sizeof(uint32_t), c->stream));
    }
    P.use_pair = 1;
    P.pair_cnt = c->pair_cnt + (c->pair_seq & 1u);
    P.pair_cnt_next = c->pair_cnt + ((c->pair_seq + 1) & 1u);
  }
  TimedLaunch tl(c, CMPC_KERNEL_BUILD);
  if (tl.begin()) return -1;
  P.split = pl.build_kernel == CMPC_BUILD_SPLIT;
  if (c->sc_w) {  // per-slot weights: the one-QP-per-wave kernel's instances that load them
    BuildParamsW W;
    cmpc_dispatch_params_weights(c->d, P, &W);
    W.sc_w = c->sc_w;
    W.yref = c->d_yref;
    if (pl.build_kernel != CMPC_BUILD_WAVE || cmpc_launch_build_weights(W, c->d, c->stream))
      return plan_mismatch("build with per-scenario weights");
  } else if (pl.build_kernel == CMPC_BUILD_ROWS ? cmpc_launch_build_rows(P, c->d, c->stream)
                                                : cmpc_launch_build(P, c->d, c->stream))
    return plan_mismatch("build");
  if (check_launch("build kernel")) return -1;
  if (pair) ++c->pair_seq;
  c->last_pair = pair != 0;
  c->last_build = pl.build_kernel;
  if (tl.end()) return -1;
  if (c->sc_dref) {  // f -= Su' ywt dref, in place (untimed: no CMPC_KERNEL_* slot of its own)
    RefshiftParams R;
    std::memset(&R, 0, sizeof R);
    R.lin = P.lin;
    R.cfg = P.cfg;
    R.dref = c->sc_dref;
    R.sc_w = c->sc_w;
    R.qp = P.qp;
    R.nqp = P.nqp;
    R.S = P.S;
    R.p = P.p;
    R.rec_len = P.rec_len;
    R.nobs = P.nobs;
    R.qp_len = P.qp_len;
    R.off_A = P.off_A; R.off_B = P.off_B; R.off_C = P.off_C;
    R.co = P.co;
    for (int i = 0; i < c->d.nu_tot; ++i) R.delay[i] = c->d.delay[i];
    if (cmpc_launch_refshift(R, c->d, c->stream)) return plan_mismatch("reference profile");
    if (check_launch("reference-profile kernel")) return -1;
  }
  c->pred_built = true;
  c->pred_stale = nullptr;
  c->cert_plans = false;
  return 0;
}

// working-set trace buffers for K iterations of every QP (CMPC_TRACE)
static int trace_buffers(cmpc_ctx* c, int K) {
  const size_t need = (size_t)c->nqp * K * 16;
  if (need > c->trace_cap) {
    if (c->trace) HIP_TRY(hipFree(c->trace));
    if (c->ntrace) HIP_TRY(hipFree(c->ntrace));
    c->trace = nullptr;
    c->ntrace = nullptr;
    HIP_TRY(hipMalloc(&c->trace, need));
    HIP_TRY(hipMalloc(&c->ntrace, sizeof(int32_t) * (size_t)c->nqp * K));
    c->trace_cap = need;
  }
  c->trace_K = K;
  return 0;
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

// the solve kernel of the plan for this call, or its error; launch_solve
// launches it (after TimedLaunch::begin, so nothing there may fail over)
static int solve_kernel_of(cmpc_ctx* c, const SolveParams& P, const char* who, int* kernel) {
  const cmpc_plan_t& pl = plan_of(c, P.K, P.trace != nullptr, P.du_other != nullptr);
  if (pl.solve_error) return fail(std::string(who) + ": " + cmpc_plan_error_string(pl.solve_error));
  *kernel = pl.solve_kernel;
  return 0;
}

static int launch_solve(cmpc_ctx* c, const SolveParams& P, int kernel) {
  const int nV = c->L.nV, nu = c->d.nu, nVo = c->L.nVo;
  if (kernel == CMPC_SOLVE_ROWS ? cmpc_launch_solve_rows(P, nV, nu, nVo, c->stream)
                                : cmpc_launch_solve(P, nV, nu, nVo, c->stream))
    return plan_mismatch("solve");
  c->last_solve = kernel;
  return 0;
}

int cmpc_init_warmstart(cmpc_ctx* c) {
  if (!c) return fail("null context");
  if (ensure_cfg(c)) return -1;
  HIP_TRY(hipSetDevice(c->device));
  SolveParams P;
  solve_params(c, &P);
  P.init = 1;
  int kernel = 0;
  if (solve_kernel_of(c, P, "cmpc_init_warmstart", &kernel)) return -1;
  if (launch_solve(c, P, kernel)) return -1;
  return check_launch("init kernel");
}

int cmpc_iterate(cmpc_ctx* c, int K, uint32_t flags) {
  if (!c) return fail("null context");
  if (K < 0) return fail("K must be >= 0");
  if (c->L.nuo != (c->d.S - 1) * c->d.nu)
    return fail("cmpc_iterate: the other controllers' plans are not in this context (S = 1, nu < nu_tot): "
                "use cmpc_get_input");
  if (ensure_cfg(c)) return -1;
  HIP_TRY(hipSetDevice(c->device));
  SolveParams P;
  solve_params(c, &P);
  P.K = K;
  P.flags = flags;
  if ((flags & CMPC_TRACE) && K > 0) {
    if (trace_buffers(c, K)) return -1;
    P.trace = c->trace;
    P.ntrace = c->ntrace;
  }
  int kernel = 0;
  if (solve_kernel_of(c, P, "cmpc_iterate", &kernel)) return -1;
  TimedLaunch tl(c, CMPC_KERNEL_ITERATE);
  if (tl.begin()) return -1;
  if (flags & CMPC_APPLY_MOVE) c->pred_stale = kStaleMove;
  if (launch_solve(c, P, kernel)) return -1;
  if (check_launch("iterate kernel")) return -1;
  if (K > 0) c->cert_plans = true;
  return tl.end();
}

// DistributedController::GetInput (include/distributed_controller.h:206-226):
// one warm-started solve per slot with the other controllers' plans given.
int cmpc_get_input(cmpc_ctx* c, const double* du_last, uint32_t flags) {
  if (!c) return fail("null context");
  if (flags & CMPC_TRACE) return fail("cmpc_get_input: no trace");
  if (ensure_cfg(c)) return -1;
  if (c->L.nVo > 0 && !du_last) return fail("cmpc_get_input: du_last is needed (nu < nu_tot)");
  if (c->L.nVo == 0) return cmpc_iterate(c, 1, flags);  // full controller: SolveQP(qp_, u_old_)
  HIP_TRY(hipSetDevice(c->device));
  SolveParams P;
  solve_params(c, &P);
  P.K = 1;
  P.flags = flags;
  P.du_other = du_last;
  int kernel = 0;
  if (solve_kernel_of(c, P, "cmpc_get_input", &kernel)) return -1;
  TimedLaunch tl(c, CMPC_KERNEL_ITERATE);
  if (tl.begin()) return -1;
  if (flags & CMPC_APPLY_MOVE) c->pred_stale = kStaleMove;
  if (launch_solve(c, P, kernel)) return -1;
  if (check_launch("get-input kernel")) return -1;
  c->cert_plans = true;
  return tl.end();
}

int cmpc_get_input_host(cmpc_ctx* c, const double* du_last, uint32_t flags) {
  if (!c) return fail("null context");
  if (c->L.nVo == 0 || !du_last) return cmpc_get_input(c, nullptr, flags);
  HIP_TRY(hipSetDevice(c->device));
  const double* h[1] = {du_last};
  const size_t n[1] = {(size_t)c->nqp * c->L.nVo};
  const double* d[1];
  if (stage_host(c, h, n, 1, d)) return -1;
  const int rc = cmpc_get_input(c, d[0], flags);
  return stage_done(c) ? -1 : rc;
}

// DistributedController::UpdateU(du) (include/distributed_controller.h:145-152)
// with the caller's full input change: ObserveAPriori(du, u_old_), u_old_ += du.
int cmpc_update_u(cmpc_ctx* c, const double* du_full) {
  if (!c || !du_full) return fail("null argument");
  if (c->obs_plant < 0) return fail("cmpc_update_u: call cmpc_observer_init first");
  if (c->lin_bound) return fail("cmpc_update_u: records are bound externally");
  HIP_TRY(hipSetDevice(c->device));
  ObserverParams P;
  observer_params(c, &P);
  P.du_full = du_full;
  c->pred_stale = "u_old has moved since the build (cmpc_update_u)";
  TimedLaunch tl(c, CMPC_KERNEL_OBSERVE_PRIOR);
  if (tl.begin()) return -1;
  if (cmpc_launch_observer(P, CMPC_OBS_PRIOR, c->stream))
    return fail("cmpc_update_u: no a-priori kernel instantiation for these dimensions");
  if (check_launch("observer a-priori kernel")) return -1;
  c->obs_steps++;  // the delay-block rings advance by one
  return tl.end();
}

int cmpc_update_u_host(cmpc_ctx* c, const double* du_full) {
  if (!c || !du_full) return fail("null argument");
  HIP_TRY(hipSetDevice(c->device));
  const double* h[1] = {du_full};
  const size_t n[1] = {(size_t)c->nqp * c->d.nu_tot};
  const double* d[1];
  if (stage_host(c, h, n, 1, d)) return -1;
  const int rc = cmpc_update_u(c, d[0]);
  return stage_done(c) ? -1 : rc;
}

int cmpc_coupled_validate(const cmpc_dims* d, int S_total, int S_local, int s_offset, size_t G_ext_len,
                          size_t du_all_len) {
  if (!d) return fail("cmpc_coupled_validate: null dims");
  cmpc_layout L;
  if (layout_of(d, &L)) return -1;
  const long long nqp_ll = (long long)d->B * d->S;
  if (S_local < 1 || nqp_ll % S_local || S_local % d->S)
    return fail("cmpc_coupled_iterate: S_local must divide B*S and be a multiple of S");
  if (S_total < S_local || S_total % S_local || s_offset < 0 || s_offset % S_local ||
      s_offset + S_local > S_total)
    return fail("cmpc_coupled_iterate: bad S_total / s_offset");
  // every read of the kernel must fall inside the caller's buffers: G_ext
  // holds nV x (S_total-1) nV per local QP, du_all the plans of all S_total
  // sub-controllers of the B scenarios (rank-major, S_total / S_local ranks)
  const size_t nV = (size_t)L.nV, nqp = (size_t)nqp_ll, B = nqp / (size_t)S_local;
  const size_t need_g = nV * (size_t)(S_total - 1) * nV * nqp;
  const size_t need_d = (size_t)S_total * B * nV;
  if (G_ext_len < need_g)
    return fail("cmpc_coupled_iterate: G_ext holds " + std::to_string(G_ext_len) + " doubles, the kernel reads " +
                std::to_string(need_g) + " (nV*(S_total-1)*nV per local QP)");
  if (du_all_len < need_d)
    return fail("cmpc_coupled_iterate: du_all holds " + std::to_string(du_all_len) + " doubles, the kernel reads " +
                std::to_string(need_d) + " (S_total x B x nV: every rank's plans; does S_local x world cover "
                "S_total?)");
  return 0;
}

int cmpc_coupled_iterate(cmpc_ctx* c, int S_total, int S_local, int s_offset, const double* G_ext,
                         size_t G_ext_len, const double* du_all, size_t du_all_len, double* du_out,
                         uint32_t flags) {
  if (!c) return fail("null context");
  if (!G_ext || !du_all) return fail("cmpc_coupled_iterate: null argument");
  if (cmpc_coupled_validate(&c->d, S_total, S_local, s_offset, G_ext_len, du_all_len)) return -1;
  if (ensure_cfg(c)) return -1;
  HIP_TRY(hipSetDevice(c->device));
  CoupledParams P;
  std::memset(&P, 0, sizeof P);
  P.qp = c->qp;
  P.cfg = c->cfg;
  P.limits = c->sc_limits;
  P.co = c->co;
  P.u_old = c->u_old;
  P.du_old = c->du_old;
  P.ws = c->ws;
  P.du = c->du;
  P.du_out = du_out;
  P.status = c->status;
  P.nwsr = c->nwsr;
  P.G_ext = G_ext;
  P.du_all = du_all;
  P.nqp = c->nqp;
  P.qp_len = c->qp_len;
  P.nu_tot = c->d.nu_tot;
  P.S_cfg = c->d.S;
  P.S_total = S_total;
  P.S_local = S_local;
  P.s_offset = s_offset;
  P.B = c->nqp / S_local;
  P.flags = flags;
  if (flags & CMPC_APPLY_MOVE) c->pred_stale = kStaleMove;
  TimedLaunch tl(c, CMPC_KERNEL_ITERATE);
  if (tl.begin()) return -1;
  if (cmpc_launch_coupled(P, c->L.nV, c->d.nu, c->stream))
    return fail("coupled kernel not instantiated for these dimensions (nV = 4, nu = 2)");
  if (check_launch("coupled kernel")) return -1;
  return tl.end();
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

// GetNextInputWithTiming's device part: the build, then K Jacobi iterations.
// One fused launch where the plan says so (the build kernel solves its own
// QPs: no launch gap, no HBM round trip of H, f, G); else cmpc_build +
// cmpc_iterate.
int cmpc_step(cmpc_ctx* c, int K, uint32_t flags) {
  if (!c) return fail("null context");
  if (K < 0) return fail("K must be >= 0");
  const bool trace = (flags & CMPC_TRACE) != 0;
  const cmpc_plan_t& pl = plan_of(c, K, trace, false);
  if (!pl.step_fused && !pl.step_error) {
    c->last_step_fused = 0;
    if (cmpc_build(c)) return -1;
    return cmpc_iterate(c, K, flags);
  }
  if (ensure_cfg(c)) return -1;
  HIP_TRY(hipSetDevice(c->device));
  BuildParams P;
  if (build_params(c, P)) return -1;
  if (pl.step_error) return fail(cmpc_plan_error_string(pl.step_error));
  solve_params(c, &P.sv);
  P.sv.K = K;
  P.sv.flags = flags;
  if (trace) {
    if (trace_buffers(c, K)) return -1;
    P.sv.trace = c->trace;
    P.sv.ntrace = c->ntrace;
  }
  TimedLaunch tl(c, CMPC_KERNEL_STEP);
  if (tl.begin()) return -1;
  if (pl.step_build_kernel == CMPC_BUILD_ROWS ? cmpc_launch_step_rows(P, c->d, pl.step_solve_kernel, c->stream)
                                              : cmpc_launch_step_wave(P, c->d, c->stream))
    return plan_mismatch("fused step");
  if (check_launch("fused step kernel")) return -1;
  c->last_build = pl.step_build_kernel;
  c->last_pair = false;
  c->last_solve = pl.step_solve_kernel;
  c->last_step_fused = 1;
  c->pred_built = true;
  c->pred_stale = (flags & CMPC_APPLY_MOVE) ? kStaleMove : nullptr;
  c->cert_plans = K > 0;
  return tl.end();
}

int cmpc_synchronize(cmpc_ctx* c) {
  if (!c) return fail("null context");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int cmpc_download(cmpc_ctx* c, double* du, int32_t* status, int32_t* nwsr) {
  if (!c) return fail("null context");
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)c->nqp;
  const size_t b_du = sizeof(double) * n * c->L.nV, b_i = sizeof(int32_t) * n;
  const size_t o_st = c->out_st, o_nw = c->out_nw;
  if (c->out_host) {  // the kernels wrote the block in place
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (du) std::memcpy(du, c->out_block, b_du);
    if (status) std::memcpy(status, c->out_block + o_st, b_i);
    if (nwsr) std::memcpy(nwsr, c->out_block + o_nw, b_i);
    return 0;
  }
  // device -> page-locked buffer (DMA; one copy of the du | status | nwsr
  // block when all are asked for), then host copies after one sync
  if (pinned_acquire(c->pin_out, c->out_len)) return -1;
  char* h = c->pin_out.buf;
  if (du && status && nwsr) {
    HIP_TRY(hipMemcpyAsync(h, c->out_block, c->out_len, hipMemcpyDeviceToHost, c->stream));
  } else {
    if (du) HIP_TRY(hipMemcpyAsync(h, c->du, b_du, hipMemcpyDeviceToHost, c->stream));
    if (status) HIP_TRY(hipMemcpyAsync(h + o_st, c->status, b_i, hipMemcpyDeviceToHost, c->stream));
    if (nwsr) HIP_TRY(hipMemcpyAsync(h + o_nw, c->nwsr, b_i, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (du) std::memcpy(du, h, b_du);
  if (status) std::memcpy(status, h + o_st, b_i);
  if (nwsr) std::memcpy(nwsr, h + o_nw, b_i);
  return 0;
}

int cmpc_download_qp(cmpc_ctx* c, double* H, double* f, double* G) {
  if (!c) return fail("null context");
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)c->nqp;
  const int nV = c->L.nV, nVo = c->L.nVo;
  std::vector<double> buf(n * c->qp_len);
  HIP_TRY(hipMemcpyAsync(buf.data(), c->qp, sizeof(double) * buf.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t q = 0; q < n; ++q) {
    const double* r = buf.data() + q * c->qp_len;
    if (H) std::memcpy(H + q * nV * nV, r, sizeof(double) * nV * nV);
    if (f) std::memcpy(f + q * nV, r + nV * nV, sizeof(double) * nV);
    if (G && nVo) std::memcpy(G + q * nV * nVo, r + nV * nV + nV, sizeof(double) * nV * nVo);
  }
  return 0;
}

int cmpc_download_trace(cmpc_ctx* c, uint8_t* trace, int32_t* ntrace) {
  if (!c) return fail("null context");
  if (!c->trace) return fail("no traced iterate (pass CMPC_TRACE to cmpc_iterate)");
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)c->nqp * c->trace_K;
  if (trace) HIP_TRY(hipMemcpyAsync(trace, c->trace, n * 16, hipMemcpyDeviceToHost, c->stream));
  if (ntrace) HIP_TRY(hipMemcpyAsync(ntrace, c->ntrace, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// Predicted outputs and objective values of every QP slot (predict.hip).
int cmpc_predict(cmpc_ctx* c, const double* du, const double* du_other, uint32_t flags) {
  if (!c) return fail("null context");
  if (flags) return fail("cmpc_predict: flags must be 0 (reserved)");
  if (!cmpc_predict_instance(c->d, c->L))
    return fail("cmpc_predict: predict kernel not instantiated for these dimensions (ns, ny, nu, m)");
  if (!c->pred_built) return fail("cmpc_predict: no build has run (cmpc_build, cmpc_step or cmpc_control_step)");
  if (c->pred_stale) return fail(std::string("cmpc_predict: ") + c->pred_stale);
  if (c->L.nVo == 0) du_other = nullptr;
  if (c->L.nVo > 0 && !du_other && c->L.nuo != (c->d.S - 1) * c->d.nu)
    return fail("cmpc_predict: the other controllers' plans are not in this context (S = 1, nu < nu_tot): "
                "give du_other");
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)c->nqp;
  if (!c->pred_y) HIP_TRY(hipMalloc(&c->pred_y, sizeof(double) * n * c->d.p * c->d.ny));
  if (!c->pred_cost) HIP_TRY(hipMalloc(&c->pred_cost, sizeof(double) * n * 2));
  if (c->sc_w && ensure_yref(c)) return -1;
  PredictParams P;
  std::memset(&P, 0, sizeof P);
  P.lin = c->lin_bound ? c->lin_bound : c->lin;
  P.cfg = c->cfg;
  P.u_old = c->u_old;
  P.dy_ref = c->sc_dy;
  P.dref = c->sc_dref;
  P.sc_w = c->sc_w;
  P.yref = c->d_yref;  // (uploaded by the build that made the prediction current)
  P.du = du ? du : c->du;  // (page-locked host memory up to CMPC_HOST_OUT_MAX_QP slots: its device address)
  P.d = du_other;
  P.y_pred = c->pred_y;
  P.cost = c->pred_cost;
  P.nqp = c->nqp;
  P.S = c->d.S;
  P.p = c->d.p;
  P.ndist = c->d.ndist;
  P.rec_len = c->L.rec_len;
  P.nobs = c->L.nobs;
  P.off_A = c->L.off_A; P.off_B = c->L.off_B; P.off_C = c->L.off_C;
  P.off_f = c->L.off_f; P.off_x = c->L.off_x; P.off_y = c->L.off_y;
  P.co = c->co;
  int kd = 0, blk = c->d.ndist + c->L.nd;
  for (int i = 0; i < c->d.nu_tot; ++i) {
    P.delay[i] = c->d.delay[i];
    if (c->d.delay[i] > 0) {
      P.dslot[i] = c->d.ndist + kd++;
      P.dblk[i] = blk;
      blk += c->d.delay[i] - 1;
    }
  }
  if (cmpc_launch_predict(P, c->d, c->stream)) return plan_mismatch("predict");
  if (check_launch("predict kernel")) return -1;
  c->pred_done = true;
  return 0;
}

int cmpc_predict_host(cmpc_ctx* c, const double* du, const double* du_other, uint32_t flags) {
  if (!c) return fail("null context");
  if (!du && !(du_other && c->L.nVo)) return cmpc_predict(c, nullptr, nullptr, flags);
  HIP_TRY(hipSetDevice(c->device));
  const double* h[2] = {du, c->L.nVo ? du_other : nullptr};
  const size_t n[2] = {(size_t)c->nqp * c->L.nV, (size_t)c->nqp * c->L.nVo};
  const double* d[2];
  if (stage_host(c, h, n, 2, d)) return -1;
  const int rc = cmpc_predict(c, d[0], d[1], flags);
  return stage_done(c) ? -1 : rc;
}

double* cmpc_prediction_device(cmpc_ctx* c) { return c && c->pred_done ? c->pred_y : nullptr; }
double* cmpc_prediction_cost_device(cmpc_ctx* c) { return c && c->pred_done ? c->pred_cost : nullptr; }

int cmpc_download_prediction(cmpc_ctx* c, double* y_pred, double* cost) {
  if (!c) return fail("null context");
  if (!c->pred_done) return fail("cmpc_download_prediction: nothing has been predicted (cmpc_predict)");
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)c->nqp;
  if (y_pred)
    HIP_TRY(hipMemcpyAsync(y_pred, c->pred_y, sizeof(double) * n * c->d.p * c->d.ny, hipMemcpyDeviceToHost,
                           c->stream));
  if (cost) HIP_TRY(hipMemcpyAsync(cost, c->pred_cost, sizeof(double) * n * 2, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// Multipliers and KKT certificate of every QP slot (include/cmpc.h, certify.hip).
static const struct {
  const char* name;
  int CertifyFields::*row;
} kCertifyFields[] = {
    {"lam", &CertifyFields::lam},           {"r_stat", &CertifyFields::r_stat},
    {"r_prim", &CertifyFields::r_prim},     {"r_dual", &CertifyFields::r_dual},
    {"r_comp", &CertifyFields::r_comp},     {"obj", &CertifyFields::obj},
    {"scale", &CertifyFields::scale},       {"n_active", &CertifyFields::n_active},
    {"status", &CertifyFields::status},     {"rank_def", &CertifyFields::rank_def},
};

int cmpc_certify_len(const cmpc_dims* dims) {
  cmpc_layout L;
  if (!dims) return fail("null argument");
  if (layout_of(dims, &L)) return -1;
  return cmpc_certify_fields(L.nV).len;
}

int cmpc_certify_field(const cmpc_dims* dims, const char* name, int* offset, int* count) {
  cmpc_layout L;
  if (!dims || !name) return fail("null argument");
  if (layout_of(dims, &L)) return -1;
  const CertifyFields F = cmpc_certify_fields(L.nV);
  for (const auto& f : kCertifyFields)
    if (!std::strcmp(name, f.name)) {
      if (offset) *offset = F.*(f.row);
      if (count) *count = f.row == &CertifyFields::lam ? 2 * L.nV : 1;
      return 0;
    }
  return fail(std::string("cmpc_certify_field: no field named '") + name + "'");
}

int cmpc_certify_available(const cmpc_dims* dims) {
  cmpc_layout L;
  if (!dims || cmpc_layout_error(dims, &L) || cmpc_context_dims_error(*dims, L)) return 0;
  return cmpc_certify_instance(L.nV, dims->nu, L.nVo) ? 1 : 0;
}

int cmpc_certify(cmpc_ctx* c, const double* du_other, uint32_t flags) {
  if (!c) return fail("null context");
  if (flags) return fail("cmpc_certify: flags must be 0 (reserved)");
  if (!cmpc_certify_instance(c->L.nV, c->d.nu, c->L.nVo))
    return fail("cmpc_certify: certify kernel not instantiated for these dimensions (nV, nu, nVo)");
  if (!c->pred_built) return fail("cmpc_certify: no build has run (cmpc_build, cmpc_step or cmpc_control_step)");
  if (c->pred_stale) return fail(std::string("cmpc_certify: ") + c->pred_stale);
  if (!c->cert_plans)
    return fail("cmpc_certify: no solve has written plans for the last build (cmpc_iterate or cmpc_step with "
                "K > 0, cmpc_get_input)");
  if (c->L.nVo == 0) du_other = nullptr;
  if (c->L.nVo > 0 && !du_other && c->d.nu_tot != c->d.S * c->d.nu)
    return fail("cmpc_certify: the other controllers' plans are not in this context (nu_tot != S * nu): "
                "give du_other");
  if (ensure_cfg(c)) return -1;
  HIP_TRY(hipSetDevice(c->device));
  const CertifyFields F = cmpc_certify_fields(c->L.nV);
  if (!c->cert_rec) HIP_TRY(hipMalloc(&c->cert_rec, sizeof(double) * (size_t)F.len * c->nqp));
  if (!c->cert_work) HIP_TRY(hipMalloc(&c->cert_work, cmpc_certify_summary_bytes()));
  CertifyParams P;
  std::memset(&P, 0, sizeof P);
  P.rec = c->cert_rec;
  P.qp = c->qp;
  P.cfg = c->cfg;
  P.limits = c->sc_limits;
  P.u_old = c->u_old;
  P.du = c->du;  // (page-locked host memory up to CMPC_HOST_OUT_MAX_QP slots: its device address)
  P.d = du_other;
  P.ws = c->ws;
  P.status = c->status;
  P.nqp = c->nqp;
  P.S = c->d.S;
  P.nu_tot = c->d.nu_tot;
  P.qp_len = c->qp_len;
  P.co = c->co;
  if (cmpc_launch_certify(P, c->L.nV, c->d.nu, c->L.nVo, c->stream)) return plan_mismatch("certify");
  if (check_launch("certify kernel")) return -1;
  c->cert_done = true;
  return 0;
}

int cmpc_certify_host(cmpc_ctx* c, const double* du_other, uint32_t flags) {
  if (!c) return fail("null context");
  if (!du_other || !c->L.nVo) return cmpc_certify(c, nullptr, flags);
  HIP_TRY(hipSetDevice(c->device));
  const double* h[1] = {du_other};
  const size_t n[1] = {(size_t)c->nqp * c->L.nVo};
  const double* d[1];
  if (stage_host(c, h, n, 1, d)) return -1;
  const int rc = cmpc_certify(c, d[0], flags);
  return stage_done(c) ? -1 : rc;
}

double* cmpc_certify_device(cmpc_ctx* c) { return c && c->cert_done ? c->cert_rec : nullptr; }

int cmpc_certify_download(cmpc_ctx* c, double* record) {
  if (!c || !record) return fail("null argument");
  if (!c->cert_done) return fail("cmpc_certify_download: nothing has been certified (cmpc_certify)");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(record, c->cert_rec,
                         sizeof(double) * (size_t)cmpc_certify_fields(c->L.nV).len * c->nqp,
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int cmpc_certify_summary(cmpc_ctx* c, double tol, cmpc_certify_summary_t* out) {
  if (!c || !out) return fail("null argument");
  if (!c->cert_done) return fail("cmpc_certify_summary: nothing has been certified (cmpc_certify)");
  if (!(tol >= 0)) return fail("cmpc_certify_summary: tol must be >= 0");
  HIP_TRY(hipSetDevice(c->device));
  if (cmpc_launch_certify_summary(c->cert_rec, c->nqp, c->L.nV, tol, c->cert_work, c->stream))
    return plan_mismatch("certify summary");
  if (check_launch("certify summary kernels")) return -1;
  alignas(8) unsigned char head[kCertifySummaryHead];
  HIP_TRY(hipMemcpyAsync(head, c->cert_work, sizeof head, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  cmpc_certify_summary_unpack(head, out);
  return 0;
}

// Closed-loop performance indices (include/cmpc.h, score.hip).
static const struct {
  const char* name;
  int ScoreFields::*row;
  int per;  // rows: 0 one, 1 ny, 2 nu
} kScoreFields[] = {
    {"n", &ScoreFields::n, 0},           {"ise", &ScoreFields::ise, 1},
    {"iae", &ScoreFields::iae, 1},       {"peak", &ScoreFields::peak, 1},
    {"last_out", &ScoreFields::last_out, 1}, {"j_track", &ScoreFields::j_track, 0},
    {"j_move", &ScoreFields::j_move, 0}, {"tv", &ScoreFields::tv, 2},
    {"sat_bound", &ScoreFields::sat_bound, 2}, {"sat_rate", &ScoreFields::sat_rate, 2},
    {"n_fail", &ScoreFields::n_fail, 0}, {"nwsr_sum", &ScoreFields::nwsr_sum, 0},
    {"plant_fail_step", &ScoreFields::plant_fail_step, 0},
};

int cmpc_score_len(const cmpc_dims* dims) {
  cmpc_layout L;
  if (!dims) return fail("null argument");
  if (layout_of(dims, &L)) return -1;
  return cmpc_score_fields(dims->ny, dims->nu).len;
}

int cmpc_score_field(const cmpc_dims* dims, const char* name, int* offset, int* count) {
  cmpc_layout L;
  if (!dims || !name) return fail("null argument");
  if (layout_of(dims, &L)) return -1;
  const ScoreFields F = cmpc_score_fields(dims->ny, dims->nu);
  for (const auto& f : kScoreFields)
    if (!std::strcmp(name, f.name)) {
      if (offset) *offset = F.*(f.row);
      if (count) *count = f.per == 0 ? 1 : f.per == 1 ? dims->ny : dims->nu;
      return 0;
    }
  return fail(std::string("cmpc_score_field: no field named '") + name + "'");
}

int cmpc_score_check(const cmpc_dims* dims, int n_outputs, const int32_t* out_idx, double Ts, const double* band) {
  cmpc_layout L;
  if (!dims || !out_idx) return fail("cmpc_score_enable: null argument");
  if (layout_of(dims, &L)) return -1;
  if (!cmpc_score_instance(dims->ny, dims->nu))
    return fail("cmpc_score_enable: score kernel not instantiated for these dimensions (ny, nu)");
  if (n_outputs < 1) return fail("cmpc_score_enable: n_outputs must be >= 1");
  if (!std::isfinite(Ts) || Ts < 0) return fail("cmpc_score_enable: Ts must be finite and >= 0");
  for (int i = 0; i < dims->S * dims->ny; ++i) {
    if (out_idx[i] < 0 || out_idx[i] >= n_outputs)
      return fail("cmpc_score_enable: sub-controller " + std::to_string(i / dims->ny) +
                  ": out_idx outside [0, n_outputs)");
    if (band && (!std::isfinite(band[i]) || band[i] < 0))
      return fail("cmpc_score_enable: sub-controller " + std::to_string(i / dims->ny) +
                  ": band must be finite and >= 0");
  }
  return 0;
}

int cmpc_score_capture_check(const cmpc_dims* dims, int n_sel, const int32_t* scenarios, int t_cap) {
  cmpc_layout L;
  if (!dims) return fail("cmpc_score_capture: null argument");
  if (layout_of(dims, &L)) return -1;
  if (n_sel < 0) return fail("cmpc_score_capture: n_sel must be >= 0");
  if (n_sel == 0) return 0;
  if (!scenarios) return fail("cmpc_score_capture: null scenario list");
  if (t_cap < 1) return fail("cmpc_score_capture: t_cap must be >= 1");
  if (n_sel > dims->B) return fail("cmpc_score_capture: more scenarios than the batch holds");
  for (int i = 0; i < n_sel; ++i) {
    if (scenarios[i] < 0 || scenarios[i] >= dims->B)
      return fail("cmpc_score_capture: scenario " + std::to_string(scenarios[i]) + " outside [0, B)");
    for (int j = 0; j < i; ++j)
      if (scenarios[j] == scenarios[i])
        return fail("cmpc_score_capture: scenario " + std::to_string(scenarios[i]) + " given twice");
  }
  return 0;
}

static int score_cap_width(const cmpc_ctx* c) { return c->score_nout + c->d.nu_tot + c->d.ns; }

static void score_capture_free(cmpc_ctx* c) {
  if (c->score_map) (void)hipFree(c->score_map);
  if (c->score_cap_own) (void)hipFree(c->score_cap_own);
  c->score_map = nullptr;
  c->score_cap_own = c->score_cap = nullptr;
  c->score_nsel = c->score_tcap = 0;
}

int cmpc_score_reset(cmpc_ctx* c) {
  if (!c) return fail("null context");
  if (!c->score_on) return fail("cmpc_score_reset: scoring is not enabled (cmpc_score_enable)");
  HIP_TRY(hipSetDevice(c->device));
  if (cmpc_launch_score_reset(c->score_rec, c->nqp, c->d.ny, c->d.nu, c->stream))
    return fail("cmpc_score_reset: launch failed");
  if (check_launch("score reset kernel")) return -1;
  if (c->score_cap_own && c->score_cap == c->score_cap_own)
    HIP_TRY(hipMemsetAsync(c->score_cap_own, 0,
                           sizeof(double) * (size_t)c->score_tcap * c->score_nsel * score_cap_width(c), c->stream));
  c->score_k = 0;
  return 0;
}

int cmpc_score_enable(cmpc_ctx* c, int n_outputs, const int32_t* out_idx, double Ts, const double* band) {
  if (!c) return fail("null context");
  if (cmpc_score_check(&c->d, n_outputs, out_idx, Ts, band)) return -1;
  HIP_TRY(hipSetDevice(c->device));
  const size_t m = (size_t)c->d.S * c->d.ny;
  if (c->score_on && n_outputs != c->score_nout) score_capture_free(c);  // (its row width has changed)
  if (!c->score_band) HIP_TRY(hipMalloc(&c->score_band, sizeof(double) * m));
  if (!c->score_oi) HIP_TRY(hipMalloc(&c->score_oi, sizeof(int32_t) * m));
  if (!c->score_own)
    HIP_TRY(hipMalloc(&c->score_own, sizeof(double) * (size_t)cmpc_score_fields(c->d.ny, c->d.nu).len * c->nqp));
  if (ensure_yref(c)) return -1;
  std::vector<double> hb(m, 0.0);
  if (band) std::copy(band, band + m, hb.begin());
  HIP_TRY(hipMemcpyAsync(c->score_band, hb.data(), sizeof(double) * m, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->score_oi, out_idx, sizeof(int32_t) * m, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (!c->score_rec) c->score_rec = c->score_own;
  c->score_nout = n_outputs;
  c->score_Ts = Ts;
  c->score_on = true;
  return cmpc_score_reset(c);
}

int cmpc_score_bind(cmpc_ctx* c, double* scores_device) {
  if (!c) return fail("null context");
  if (!c->score_on) return fail("cmpc_score_bind: scoring is not enabled (cmpc_score_enable)");
  if (scores_device) {
    const size_t bytes = sizeof(double) * (size_t)cmpc_score_fields(c->d.ny, c->d.nu).len * c->nqp;
    if (!device_ptr_ok(c, scores_device, bytes)) {
      (void)hipGetLastError();  // a failed pointer query is not a later launch's error
      return fail("cmpc_score_bind: not a device allocation of len * nqp doubles on the context's device");
    }
    if (reinterpret_cast<uintptr_t>(scores_device) % 8) return fail("cmpc_score_bind: misaligned array");
  }
  c->score_rec = scores_device ? scores_device : c->score_own;
  return 0;
}

int cmpc_score_capture(cmpc_ctx* c, int n_sel, const int32_t* scenarios, int t_cap) {
  if (!c) return fail("null context");
  if (!c->score_on) return fail("cmpc_score_capture: scoring is not enabled (cmpc_score_enable)");
  if (cmpc_score_capture_check(&c->d, n_sel, scenarios, t_cap)) return -1;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  score_capture_free(c);
  if (n_sel == 0) return 0;
  std::vector<int32_t> map((size_t)c->d.B, -1);
  for (int i = 0; i < n_sel; ++i) map[scenarios[i]] = i;
  const size_t rows = sizeof(double) * (size_t)t_cap * n_sel * score_cap_width(c);
  HIP_TRY(hipMalloc(&c->score_map, sizeof(int32_t) * map.size()));
  HIP_TRY(hipMalloc(&c->score_cap_own, rows));
  HIP_TRY(hipMemcpyAsync(c->score_map, map.data(), sizeof(int32_t) * map.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(c->score_cap_own, 0, rows, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->score_cap = c->score_cap_own;
  c->score_nsel = n_sel;
  c->score_tcap = t_cap;
  return 0;
}

int cmpc_score_bind_capture(cmpc_ctx* c, double* rows_device) {
  if (!c) return fail("null context");
  if (!c->score_on || !c->score_nsel)
    return fail("cmpc_score_bind_capture: no capture is enabled (cmpc_score_capture)");
  if (rows_device) {
    const size_t bytes = sizeof(double) * (size_t)c->score_tcap * c->score_nsel * score_cap_width(c);
    if (!device_ptr_ok(c, rows_device, bytes)) {
      (void)hipGetLastError();  // a failed pointer query is not a later launch's error
      return fail("cmpc_score_bind_capture: not a device allocation of t_cap * n_sel * width doubles on the "
                  "context's device");
    }
    if (reinterpret_cast<uintptr_t>(rows_device) % 8) return fail("cmpc_score_bind_capture: misaligned array");
  }
  c->score_cap = rows_device ? rows_device : c->score_cap_own;
  return 0;
}

int cmpc_score_step(cmpc_ctx* c, const double* y, const double* target, const int32_t* plant_status,
                    const double* u_control, const double* x) {
  if (!c) return fail("null context");
  if (!c->score_on) return fail("cmpc_score_step: scoring is not enabled (cmpc_score_enable)");
  if (!y) return fail("cmpc_score_step: null y");
  if (!c->last_solve) return fail("cmpc_score_step: no solve has run (cmpc_iterate, cmpc_step, cmpc_control_step)");
  if (c->score_k >= INT32_MAX) return fail("cmpc_score_step: step count overflow (cmpc_score_reset)");
  if (ensure_cfg(c)) return -1;
  HIP_TRY(hipSetDevice(c->device));
  if (!target && ensure_yref(c)) return -1;  // (allocated by cmpc_score_enable; a copy when the references changed)
  ScoreParams P;
  std::memset(&P, 0, sizeof P);
  P.rec = c->score_rec;
  P.y = y;
  P.target = target;
  P.cfg = c->cfg;
  P.yref = c->d_yref;
  P.dy_ref = c->sc_dy;
  P.sc_w = c->sc_w;
  P.du = c->du;  // (page-locked host memory up to CMPC_HOST_OUT_MAX_QP slots: its device address)
  P.status = c->status;
  P.nwsr = c->nwsr;
  P.ws = c->ws;
  P.plant_status = plant_status;
  P.out_idx = c->score_oi;
  P.band = c->score_band;
  if (c->score_nsel) {
    P.cap_map = c->score_map;
    P.cap = c->score_cap;
    P.u_control = u_control;
    P.x = x;
    P.n_sel = c->score_nsel;
    P.t_cap = c->score_tcap;
    P.cap_w = score_cap_width(c);
  }
  P.n_out = c->score_nout;
  P.nu_tot = c->d.nu_tot;
  P.ns = c->d.ns;
  P.nqp = c->nqp;
  P.S = c->d.S;
  P.p = c->d.p;
  P.nV = c->L.nV;
  P.k = (int)c->score_k;
  P.Ts = c->score_Ts;
  P.co = c->co;
  if (cmpc_launch_score(P, c->d.ny, c->d.nu, c->stream)) return plan_mismatch("score");
  if (check_launch("score kernel")) return -1;
  c->score_k++;
  return 0;
}

int cmpc_score_download(cmpc_ctx* c, double* scores) {
  if (!c || !scores) return fail("null argument");
  if (!c->score_on) return fail("cmpc_score_download: scoring is not enabled (cmpc_score_enable)");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(scores, c->score_rec,
                         sizeof(double) * (size_t)cmpc_score_fields(c->d.ny, c->d.nu).len * c->nqp,
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int cmpc_score_download_capture(cmpc_ctx* c, double* rows, int32_t* n_rows) {
  if (!c) return fail("null context");
  if (!c->score_on || !c->score_nsel)
    return fail("cmpc_score_download_capture: no capture is enabled (cmpc_score_capture)");
  HIP_TRY(hipSetDevice(c->device));
  if (rows)
    HIP_TRY(hipMemcpyAsync(rows, c->score_cap,
                           sizeof(double) * (size_t)c->score_tcap * c->score_nsel * score_cap_width(c),
                           hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (n_rows) *n_rows = (int32_t)std::min<int64_t>(c->score_k, c->score_tcap);
  return 0;
}

int cmpc_score_disable(cmpc_ctx* c) {
  if (!c) return fail("null context");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  score_capture_free(c);
  if (c->score_band) (void)hipFree(c->score_band);
  if (c->score_oi) (void)hipFree(c->score_oi);
  if (c->score_own) (void)hipFree(c->score_own);
  c->score_band = nullptr;
  c->score_oi = nullptr;
  c->score_own = c->score_rec = nullptr;
  c->score_on = false;
  c->score_k = 0;
  return 0;
}

// Ensemble statistics of the score record (include/cmpc.h, score_ensemble.hip).
int cmpc_score_ensemble(cmpc_ctx* c, const double* thresholds, double* out) {
  if (!c || !out) return fail("cmpc_score_ensemble: null argument");
  if (!c->score_on) return fail("cmpc_score_ensemble: scoring is not enabled (cmpc_score_enable)");
  const int len = cmpc_score_fields(c->d.ny, c->d.nu).len, S = c->d.S;
  if (thresholds)
    for (int f = 0; f < len; ++f)
      if (std::isnan(thresholds[f]))
        return fail("cmpc_score_ensemble: threshold of row " + std::to_string(f) + " is not a number");
  HIP_TRY(hipSetDevice(c->device));
  if (!c->score_ens_work.p) HIP_TRY(hipMalloc(&c->score_ens_work.p, cmpc_score_ensemble_bytes(len, S)));
  void* work = c->score_ens_work.p;
  if (thresholds)
    HIP_TRY(hipMemcpyAsync(cmpc_score_ensemble_thresholds(work, len, S), thresholds, sizeof(double) * len,
                           hipMemcpyHostToDevice, c->stream));
  if (cmpc_launch_score_ensemble(c->score_rec, len, c->d.B, S, thresholds != nullptr, work, c->stream))
    return plan_mismatch("score ensemble");
  if (check_launch("score ensemble kernels")) return -1;
  HIP_TRY(hipMemcpyAsync(out, work, sizeof(double) * (size_t)len * S * kScoreEnsembleStats, hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// Exact ensemble quantiles and the envelope (include/cmpc.h, ensemble_select.h,
// ensemble_quantiles.hip).
static int quantile_levels_check(const char* who, int n_levels, int n_min, const double* levels) {
  if (n_levels < n_min || n_levels > CMPC_QUANTILE_MAX_LEVELS)
    return fail(std::string(who) + ": n_levels must be inside [" + std::to_string(n_min) + ", " +
                std::to_string(CMPC_QUANTILE_MAX_LEVELS) + "]");
  if (n_levels > 0 && !levels) return fail(std::string(who) + ": null levels");
  for (int l = 0; l < n_levels; ++l)
    if (!(levels[l] >= 0.0 && levels[l] <= 1.0))
      return fail(std::string(who) + ": level " + std::to_string(l) + " must be inside [0, 1]");
  return 0;
}

static QuantileRanks quantile_ranks(int B, int n_levels, const double* levels, double* g) {
  QuantileRanks R{};
  R.n = n_levels;
  for (int l = 0; l < n_levels; ++l) {
    double gl;
    cmpc_select_rank(B, levels[l], &R.k_lo[l], &R.k_hi[l], &gl);
    if (g) g[l] = gl;
  }
  return R;
}

int cmpc_quantile_check(int B, int n_levels, const double* levels) {
  if (B < 1) return fail("cmpc_quantile: B must be >= 1");
  return quantile_levels_check("cmpc_quantile", n_levels, 1, levels);
}

int cmpc_quantile_rank(int B, double level, int32_t* k_lo, int32_t* k_hi, double* g) {
  if (!k_lo || !k_hi || !g) return fail("cmpc_quantile_rank: null argument");
  if (cmpc_quantile_check(B, 1, &level)) return -1;
  uint32_t lo, hi;
  cmpc_select_rank(B, level, &lo, &hi, g);
  *k_lo = (int32_t)lo;
  *k_hi = (int32_t)hi;
  return 0;
}

double cmpc_quantile_value(double x_lo, double x_hi, double g) { return cmpc_select_interpolate(x_lo, x_hi, g); }

int cmpc_quantiles_host(const double* x, int len, int B, int S, int n_levels, const double* levels, double* out) {
  if (!x || !out) return fail("cmpc_quantiles_host: null argument");
  if (cmpc_quantile_check(B, n_levels, levels)) return -1;
  if (len < 1 || S < 1) return fail("cmpc_quantiles_host: len and S must be >= 1");
  const QuantileRanks R = quantile_ranks(B, n_levels, levels, nullptr);
  for (int f = 0; f < len; ++f)
    for (int s = 0; s < S; ++s)
      cmpc_select_row_host(x + (size_t)f * B * S + s, (size_t)S, B, n_levels, R.k_lo, R.k_hi,
                           out + ((size_t)f * S + s) * n_levels * 3);
  return 0;
}

int cmpc_score_quantiles(cmpc_ctx* c, int n_levels, const double* levels, double* out) {
  if (!c || !out) return fail("cmpc_score_quantiles: null argument");
  if (!c->score_on) return fail("cmpc_score_quantiles: scoring is not enabled (cmpc_score_enable)");
  if (cmpc_quantile_check(c->d.B, n_levels, levels)) return -1;
  const int len = cmpc_score_fields(c->d.ny, c->d.nu).len, S = c->d.S, B = c->d.B;
  if ((size_t)len * S > 65535) return fail("cmpc_score_quantiles: more rows than one launch covers");
  const int rows = len * S;
  HIP_TRY(hipSetDevice(c->device));
  if (!c->quant_work.p)
    HIP_TRY(hipMalloc(&c->quant_work.p, cmpc_quantile_work_bytes(rows, B, CMPC_QUANTILE_MAX_LEVELS)));
  void* work = c->quant_work.p;
  EnsRowMap M{};
  M.p0 = c->score_rec;
  M.fstride0 = (int64_t)B * S;
  M.rows0 = rows;
  M.S0 = S;
  const QuantileRanks R = quantile_ranks(B, n_levels, levels, nullptr);
  const QuantileOut O{static_cast<double*>(work), (int64_t)n_levels * 3, 3};
  if (cmpc_launch_quantiles(M, B, R, O, work, c->stream)) return plan_mismatch("score quantiles");
  if (check_launch("quantile kernels")) return -1;
  HIP_TRY(hipMemcpyAsync(out, O.out, sizeof(double) * (size_t)rows * n_levels * 3, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

static int envelope_width(int n_levels) { return kScoreEnsembleStats + 2 * n_levels; }

int cmpc_envelope_check(const cmpc_dims* dims, int n_outputs, int t_cap, int n_levels, const double* levels,
                        const double* thresholds) {
  cmpc_layout L;
  if (!dims) return fail("cmpc_envelope_enable: null argument");
  if (layout_of(dims, &L)) return -1;
  if (n_outputs < 1) return fail("cmpc_envelope_enable: n_outputs must be >= 1");
  if (t_cap < 1) return fail("cmpc_envelope_enable: t_cap must be >= 1");
  if (quantile_levels_check("cmpc_envelope_enable", n_levels, 0, levels)) return -1;
  if ((int64_t)n_outputs + dims->nu_tot > 65535)
    return fail("cmpc_envelope_enable: more channels than one launch covers");
  for (int ch = 0; thresholds && ch < n_outputs + dims->nu_tot; ++ch)
    if (std::isnan(thresholds[ch]))
      return fail("cmpc_envelope_enable: threshold of channel " + std::to_string(ch) + " is not a number");
  return 0;
}

int cmpc_envelope_len(const cmpc_dims* dims, int n_outputs, int n_levels) {
  cmpc_layout L;
  if (!dims) return fail("cmpc_envelope_len: null argument");
  if (layout_of(dims, &L)) return -1;
  if (n_outputs < 1 || n_levels < 0 || n_levels > CMPC_QUANTILE_MAX_LEVELS ||
      (int64_t)n_outputs + dims->nu_tot > 65535)
    return fail("cmpc_envelope_len: n_outputs or n_levels outside the limits");
  return (n_outputs + dims->nu_tot) * envelope_width(n_levels);
}

static size_t envelope_row_len(const cmpc_ctx* c) {
  return (size_t)(c->env_nout + c->d.nu_tot) * envelope_width(c->env_ranks.n);
}

static void envelope_free(cmpc_ctx* c) {
  for (auto* b : {&c->env_thr, &c->env_mom_work, &c->env_quant_work, &c->env_own}) {
    if (b->p) (void)hipFree(b->p);
    b->p = nullptr;
  }
  c->env_rows = nullptr;
  c->env_on = false;
  c->env_k = 0;
}

int cmpc_envelope_disable(cmpc_ctx* c) {
  if (!c) return fail("null context");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  envelope_free(c);
  return 0;
}

int cmpc_envelope_enable(cmpc_ctx* c, int n_outputs, int t_cap, int n_levels, const double* levels,
                         const double* thresholds) {
  if (!c) return fail("null context");
  if (cmpc_envelope_check(&c->d, n_outputs, t_cap, n_levels, levels, thresholds)) return -1;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  envelope_free(c);
  const int chans = n_outputs + c->d.nu_tot, B = c->d.B;
  c->env_nout = n_outputs;
  c->env_tcap = t_cap;
  c->env_ranks = quantile_ranks(B, n_levels, levels, nullptr);
  const size_t rows = sizeof(double) * (size_t)t_cap * envelope_row_len(c);
  HIP_TRY(hipMalloc(&c->env_own.p, rows));
  HIP_TRY(hipMemsetAsync(c->env_own.p, 0, rows, c->stream));
  HIP_TRY(hipMalloc(&c->env_mom_work.p, cmpc_envelope_moments_bytes(chans)));
  if (thresholds) {
    HIP_TRY(hipMalloc(&c->env_thr.p, sizeof(double) * chans));
    HIP_TRY(hipMemcpyAsync(c->env_thr.p, thresholds, sizeof(double) * chans, hipMemcpyHostToDevice, c->stream));
  }
  if (n_levels > 0) {
    // (a step without u_control covers n_outputs rows, with its own block count)
    const size_t bytes = std::max(cmpc_quantile_work_bytes(chans, B, n_levels),
                                  cmpc_quantile_work_bytes(n_outputs, B, n_levels));
    HIP_TRY(hipMalloc(&c->env_quant_work.p, bytes));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->env_rows = static_cast<double*>(c->env_own.p);
  c->env_k = 0;
  c->env_on = true;
  return 0;
}

int cmpc_envelope_reset(cmpc_ctx* c) {
  if (!c) return fail("null context");
  if (!c->env_on) return fail("cmpc_envelope_reset: no envelope is enabled (cmpc_envelope_enable)");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemsetAsync(c->env_own.p, 0, sizeof(double) * (size_t)c->env_tcap * envelope_row_len(c), c->stream));
  c->env_k = 0;
  return 0;
}

int cmpc_envelope_bind(cmpc_ctx* c, double* rows_device) {
  if (!c) return fail("null context");
  if (!c->env_on) return fail("cmpc_envelope_bind: no envelope is enabled (cmpc_envelope_enable)");
  if (rows_device) {
    const size_t bytes = sizeof(double) * (size_t)c->env_tcap * envelope_row_len(c);
    if (!device_ptr_ok(c, rows_device, bytes)) {
      (void)hipGetLastError();  // a failed pointer query is not a later launch's error
      return fail("cmpc_envelope_bind: not a device allocation of t_cap * cmpc_envelope_len doubles on the "
                  "context's device");
    }
    if (reinterpret_cast<uintptr_t>(rows_device) % 8) return fail("cmpc_envelope_bind: misaligned array");
  }
  c->env_rows = rows_device ? rows_device : static_cast<double*>(c->env_own.p);
  return 0;
}

int cmpc_envelope_step(cmpc_ctx* c, const double* y, const double* u_control) {
  if (!c) return fail("null context");
  if (!c->env_on) return fail("cmpc_envelope_step: no envelope is enabled (cmpc_envelope_enable)");
  if (!y) return fail("cmpc_envelope_step: null y");
  if (c->env_k >= c->env_tcap) {  // dropped, as the capture drops its steps
    if (c->env_k < INT32_MAX) c->env_k++;
    return 0;
  }
  HIP_TRY(hipSetDevice(c->device));
  const int W = envelope_width(c->env_ranks.n);
  EnsRowMap M{};
  M.p0 = y;
  M.rows0 = M.S0 = c->env_nout;
  M.fstride0 = 0;
  if (u_control) {
    M.p1 = u_control;
    M.rows1 = M.S1 = c->d.nu_tot;
  }
  double* row = c->env_rows + (size_t)c->env_k * envelope_row_len(c);
  if (cmpc_launch_envelope_moments(M, c->d.B, static_cast<const double*>(c->env_thr.p), row, W, c->env_mom_work.p,
                                   c->stream))
    return plan_mismatch("envelope statistics");
  if (c->env_ranks.n > 0) {
    const QuantileOut O{row + kScoreEnsembleStats, W, 2};
    if (cmpc_launch_quantiles(M, c->d.B, c->env_ranks, O, c->env_quant_work.p, c->stream))
      return plan_mismatch("envelope quantiles");
  }
  if (check_launch("envelope kernels")) return -1;
  c->env_k++;
  return 0;
}

int cmpc_envelope_download(cmpc_ctx* c, double* rows, int32_t* n_rows) {
  if (!c) return fail("null context");
  if (!c->env_on) return fail("cmpc_envelope_download: no envelope is enabled (cmpc_envelope_enable)");
  HIP_TRY(hipSetDevice(c->device));
  if (rows)
    HIP_TRY(hipMemcpyAsync(rows, c->env_rows, sizeof(double) * (size_t)c->env_tcap * envelope_row_len(c),
                           hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (n_rows) *n_rows = (int32_t)std::min<int64_t>(c->env_k, c->env_tcap);
  return 0;
}

// Seeded per-scenario noise (include/cmpc.h, noise_body.h, noise.hip).
int cmpc_noise_check(const cmpc_noise_key* key, uint64_t step, int B, int n) {
  if (!key) return fail("cmpc_noise: null key");
  if (B < 1) return fail("cmpc_noise: B must be >= 1");
  if (n < 1) return fail("cmpc_noise: n must be >= 1");
  if (step >> 32) return fail("cmpc_noise: step must be below 2^32 (the counter's word)");
  if ((uint64_t)key->scenario0 + (uint64_t)B > (1ull << 32))
    return fail("cmpc_noise: scenario0 + B must be at most 2^32 (the counter's word)");
  if (((uint64_t)B * (uint64_t)((n + 1) / 2) + 63) / 64 > 0x7fffffffull)
    return fail("cmpc_noise: B * ceil(n / 2) is more than one launch covers");
  return 0;
}

int cmpc_noise_check_params(int B, int n, const double* sigma, const double* rho) {
  if (B < 1 || n < 1) return fail("cmpc_noise_check_params: B and n must be >= 1");
  const size_t m = (size_t)B * n;
  for (size_t e = 0; sigma && e < m; ++e)
    if (!std::isfinite(sigma[e]) || sigma[e] < 0)
      return fail("cmpc_noise_check_params: scenario " + std::to_string(e / n) + ", channel " + std::to_string(e % n) +
                  ": sigma must be finite and >= 0");
  for (size_t e = 0; rho && e < m; ++e)
    if (!(rho[e] >= -1.0 && rho[e] <= 1.0))
      return fail("cmpc_noise_check_params: scenario " + std::to_string(e / n) + ", channel " + std::to_string(e % n) +
                  ": rho must be inside [-1, 1]");
  return 0;
}

static NoiseKeyWords noise_words(const cmpc_noise_key* key) {
  return NoiseKeyWords{(uint32_t)key->seed, (uint32_t)(key->seed >> 32), key->stream, key->scenario0};
}

int cmpc_noise_uniforms_host(const cmpc_noise_key* key, uint64_t step, int B, int n, double* u) {
  if (cmpc_noise_check(key, step, B, n)) return -1;
  if (!u) return fail("cmpc_noise_uniforms_host: null u");
  const NoiseKeyWords k = noise_words(key);
  const int np = (n + 1) / 2;
  for (int b = 0; b < B; ++b)
    for (int j = 0; j < np; ++j) {
      double* o = u + ((size_t)b * np + j) * 2;
      cmpc_noise_uniforms(k, key->scenario0 + (uint32_t)b, (uint32_t)step, (uint32_t)j, o, o + 1);
    }
  return 0;
}

int cmpc_noise_step_host(const cmpc_noise_key* key, uint64_t step, int B, int n, const double* sigma,
                         const double* rho, double* w, const double* base, double* out) {
  if (cmpc_noise_check(key, step, B, n)) return -1;
  if (!out) return fail("cmpc_noise_step_host: null out");
  if (rho && !w) return fail("cmpc_noise_step_host: rho needs the AR(1) state w");
  const NoiseKeyWords k = noise_words(key);
  const int np = (n + 1) / 2;
  for (int b = 0; b < B; ++b)
    for (int j = 0; j < np; ++j) {
      double u1, u2, z0, z1;
      cmpc_noise_uniforms(k, key->scenario0 + (uint32_t)b, (uint32_t)step, (uint32_t)j, &u1, &u2);
      cmpc_noise_normals(u1, u2, &z0, &z1);
      const size_t e = (size_t)b * n + 2 * (size_t)j;
      cmpc_noise_element(z0, e, sigma, rho, w, base, out);
      if (2 * j + 1 < n) cmpc_noise_element(z1, e + 1, sigma, rho, w, base, out);
    }
  return 0;
}

// cmpc_bind_state's check of a device pointer (device_ptr_ok) without a
// context: a device allocation on `device` that holds `bytes` from p on,
// 8-byte aligned.  The last pointers that passed are remembered per host
// thread, as a context remembers its own: the queries cost host time per call.
static bool noise_ptr_ok(int device, const void* p, size_t bytes) {
  struct Entry {
    int dev;
    const void* p;
    size_t bytes;
  };
  static thread_local Entry cache[16];
  static thread_local int n = 0;
  if (reinterpret_cast<uintptr_t>(p) % 8) return false;
  for (int i = 0; i < n && i < 16; ++i)
    if (cache[i].dev == device && cache[i].p == p && cache[i].bytes >= bytes) return true;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeDevice || a.device != device) {
    (void)hipGetLastError();  // a failed pointer query is not a later launch's error
    return false;
  }
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) == hipSuccess && base &&
      (uintptr_t)p + bytes > (uintptr_t)base + size)
    return false;
  cache[n % 16] = Entry{device, p, bytes};
  ++n;
  return true;
}

static int noise_device(int device) {
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail("cmpc_noise: no such HIP device");
  HIP_TRY(hipSetDevice(device));
  return 0;
}

int cmpc_noise_uniforms(int device, void* stream, const cmpc_noise_key* key, uint64_t step, int B, int n,
                        double* u_dev) {
  if (cmpc_noise_check(key, step, B, n)) return -1;
  if (!u_dev) return fail("cmpc_noise_uniforms: null u");
  if (noise_device(device)) return -1;
  const int np = (n + 1) / 2;
  if (!noise_ptr_ok(device, u_dev, sizeof(double) * (size_t)B * np * 2))
    return fail("cmpc_noise_uniforms: u is not an 8-byte aligned device allocation of B * ceil(n / 2) * 2 doubles "
                "on the device");
  NoiseParams P{};
  const NoiseKeyWords k = noise_words(key);
  P.k0 = k.k0, P.k1 = k.k1, P.stream = k.stream, P.scenario0 = k.scenario0;
  P.step = (uint32_t)step;
  P.B = B, P.n = n, P.np = np;
  P.u = u_dev;
  if (cmpc_launch_noise_uniforms(P, stream)) return plan_mismatch("noise uniforms");
  return check_launch("noise uniforms kernel");
}

int cmpc_noise_step(int device, void* stream, const cmpc_noise_key* key, uint64_t step, int B, int n,
                    const double* sigma_dev, const double* rho_dev, double* w_dev, const double* base_dev,
                    double* out_dev) {
  if (cmpc_noise_check(key, step, B, n)) return -1;
  if (!out_dev) return fail("cmpc_noise_step: null out");
  if (rho_dev && !w_dev) return fail("cmpc_noise_step: rho needs the AR(1) state w");
  if (noise_device(device)) return -1;
  const size_t bytes = sizeof(double) * (size_t)B * n;
  const struct {
    const void* p;
    const char* name;
  } ptrs[] = {{sigma_dev, "sigma"}, {rho_dev, "rho"}, {rho_dev ? w_dev : nullptr, "w"}, {base_dev, "base"},
              {out_dev, "out"}};
  for (const auto& a : ptrs)
    if (a.p && !noise_ptr_ok(device, a.p, bytes))
      return fail(std::string("cmpc_noise_step: ") + a.name +
                  " is not an 8-byte aligned device allocation of B * n doubles on the device");
  NoiseParams P{};
  const NoiseKeyWords k = noise_words(key);
  P.k0 = k.k0, P.k1 = k.k1, P.stream = k.stream, P.scenario0 = k.scenario0;
  P.step = (uint32_t)step;
  P.B = B, P.n = n, P.np = (n + 1) / 2;
  P.sigma = sigma_dev;
  P.rho = rho_dev;
  P.w = rho_dev ? w_dev : nullptr;
  P.base = base_dev;
  P.out = out_dev;
  if (cmpc_launch_noise_step(P, stream)) return plan_mismatch("noise step");
  return check_launch("noise kernel");
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

int cmpc_qp_solve_batch(int device, int n, int nu, int nqp, const double* H, const double* g,
                        const double* lb, const double* ub, const double* lbA, const double* ubA,
                        const uint32_t* ws_in, int max_chg, double* x, int32_t* status,
                        int32_t* nchg, uint32_t* ws_out, uint8_t* trace, int32_t* ntrace) {
  return cmpc_qp_solve_batch_map(device, n, nu, 0, nqp, H, g, nullptr, nullptr, lb, ub, lbA, ubA, ws_in, max_chg, x,
                                 status, nchg, ws_out, trace, ntrace);
}

// cmpc_qp_solve_batch(_map): host arrays in, host arrays out.  The dimensions
// are checked against the kernel instances before anything is allocated, the
// device buffers are released on every exit path, and only the stream of the
// launch is waited for.
int cmpc_qp_solve_batch_map(int device, int n, int nu, int nvo, int nqp, const double* H, const double* f,
                            const double* G, const double* d, const double* lb, const double* ub,
                            const double* lbA, const double* ubA, const uint32_t* ws_in, int max_chg, double* x,
                            int32_t* status, int32_t* nchg, uint32_t* ws_out, uint8_t* trace, int32_t* ntrace) {
  if (nvo < 0) return fail("cmpc_qp_solve_batch_map: nvo < 0");
  if (nvo > 0 && (!G || !d)) return fail("cmpc_qp_solve_batch_map: G and d required for nvo > 0");
  if (nvo > 0 ? !cmpc_qp_batch_map_supported(n, nu, nvo) : !cmpc_qp_batch_supported(n, nu))
    return fail(nvo > 0 ? "map-form qp batch kernel not instantiated for (n, nu, nvo) = (" + std::to_string(n) +
                              ", " + std::to_string(nu) + ", " + std::to_string(nvo) + ")"
                        : "qp batch kernel not instantiated for (n, nu) = (" + std::to_string(n) + ", " +
                              std::to_string(nu) + ")");
  if (nqp <= 0) return 0;
  HIP_TRY(hipSetDevice(device));
  const size_t q = (size_t)nqp;
  struct Bufs {  // scope guard: every buffer allocated below is freed on return
    std::vector<void*> p;
    ~Bufs() {
      for (void* b : p) (void)hipFree(b);
    }
  } bufs;
  auto alloc = [&](auto** ptr, size_t bytes) -> hipError_t {
    void* v = nullptr;
    const hipError_t e = hipMalloc(&v, bytes ? bytes : 8);
    if (e == hipSuccess) bufs.p.push_back(v);
    *ptr = static_cast<std::remove_pointer_t<decltype(ptr)>>(v);
    return e;
  };
  double *dH, *dg, *dG = nullptr, *dd = nullptr, *dlb, *dub, *dlbA, *dubA, *dx;
  uint32_t *dws, *dwo;
  int32_t *dst, *dnc, *dnt;
  uint8_t* dtr;
  HIP_TRY(alloc(&dH, sizeof(double) * q * n * n));
  HIP_TRY(alloc(&dg, sizeof(double) * q * n));
  if (nvo > 0) {
    HIP_TRY(alloc(&dG, sizeof(double) * q * n * nvo));
    HIP_TRY(alloc(&dd, sizeof(double) * q * nvo));
  }
  HIP_TRY(alloc(&dlb, sizeof(double) * q * n));
  HIP_TRY(alloc(&dub, sizeof(double) * q * n));
  HIP_TRY(alloc(&dlbA, sizeof(double) * q * n));
  HIP_TRY(alloc(&dubA, sizeof(double) * q * n));
  HIP_TRY(alloc(&dx, sizeof(double) * q * n));
  HIP_TRY(alloc(&dws, sizeof(uint32_t) * q));
  HIP_TRY(alloc(&dwo, sizeof(uint32_t) * q));
  HIP_TRY(alloc(&dst, sizeof(int32_t) * q));
  HIP_TRY(alloc(&dnc, sizeof(int32_t) * q));
  HIP_TRY(alloc(&dnt, sizeof(int32_t) * q));
  HIP_TRY(alloc(&dtr, 16 * q));
  HIP_TRY(hipMemcpy(dH, H, sizeof(double) * q * n * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dg, f, sizeof(double) * q * n, hipMemcpyHostToDevice));
  if (nvo > 0) {
    HIP_TRY(hipMemcpy(dG, G, sizeof(double) * q * n * nvo, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dd, d, sizeof(double) * q * nvo, hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy(dlb, lb, sizeof(double) * q * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dub, ub, sizeof(double) * q * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dlbA, lbA, sizeof(double) * q * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dubA, ubA, sizeof(double) * q * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dws, ws_in, sizeof(uint32_t) * q, hipMemcpyHostToDevice));
  QpBatchParams P{dH, dg, dlb, dub, dlbA, dubA, dws, dx, dst, dnc, dnt, dwo, dtr, nqp, max_chg, dG, dd, nvo};
  const int lr = nvo > 0 ? cmpc_launch_qp_batch_map(P, n, nu, nvo, nullptr) : cmpc_launch_qp_batch(P, n, nu, nullptr);
  if (lr) return fail("qp batch kernel not instantiated");
  if (check_launch("qp batch kernel")) return -1;
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipMemcpy(x, dx, sizeof(double) * q * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(status, dst, sizeof(int32_t) * q, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(nchg, dnc, sizeof(int32_t) * q, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(ws_out, dwo, sizeof(uint32_t) * q, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(trace, dtr, 16 * q, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(ntrace, dnt, sizeof(int32_t) * q, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
