// The step of the C ABI (include/cmpc.h): build, solve, fused step, coupled
// iterate, downloads, prediction and the KKT certificate.
#include "abi_ctx.h"

using namespace cmpc_abi;

extern "C" {

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
  const double* h[1] = {du_last};
  const size_t n[1] = {(size_t)c->nqp * c->L.nVo};
  return with_staged(c, h, n, 1, [&](const double* const* d) { return cmpc_get_input(c, d[0], flags); });
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
  if (direct_download(c->stream, {{c->qp, buf.data(), sizeof(double) * buf.size()}})) return -1;
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
  return direct_download(c->stream, {{c->trace, trace, n * 16}, {c->ntrace, ntrace, sizeof(int32_t) * n}});
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
  const double* h[2] = {du, c->L.nVo ? du_other : nullptr};
  const size_t n[2] = {(size_t)c->nqp * c->L.nV, (size_t)c->nqp * c->L.nVo};
  return with_staged(c, h, n, 2, [&](const double* const* d) { return cmpc_predict(c, d[0], d[1], flags); });
}

double* cmpc_prediction_device(cmpc_ctx* c) { return c && c->pred_done ? c->pred_y : nullptr; }
double* cmpc_prediction_cost_device(cmpc_ctx* c) { return c && c->pred_done ? c->pred_cost : nullptr; }

int cmpc_download_prediction(cmpc_ctx* c, double* y_pred, double* cost) {
  if (!c) return fail("null context");
  if (!c->pred_done) return fail("cmpc_download_prediction: nothing has been predicted (cmpc_predict)");
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)c->nqp;
  return direct_download(c->stream, {{c->pred_y, y_pred, sizeof(double) * n * c->d.p * c->d.ny},
                                     {c->pred_cost, cost, sizeof(double) * n * 2}});
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
  const double* h[1] = {du_other};
  const size_t n[1] = {(size_t)c->nqp * c->L.nVo};
  return with_staged(c, h, n, 1, [&](const double* const* d) { return cmpc_certify(c, d[0], flags); });
}

double* cmpc_certify_device(cmpc_ctx* c) { return c && c->cert_done ? c->cert_rec : nullptr; }

int cmpc_certify_download(cmpc_ctx* c, double* record) {
  if (!c || !record) return fail("null argument");
  if (!c->cert_done) return fail("cmpc_certify_download: nothing has been certified (cmpc_certify)");
  HIP_TRY(hipSetDevice(c->device));
  return direct_download(c->stream,
                         {{c->cert_rec, record, sizeof(double) * (size_t)cmpc_certify_fields(c->L.nV).len * c->nqp}});
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
  if (direct_download(c->stream, {{c->cert_work, head, sizeof head}})) return -1;
  cmpc_certify_summary_unpack(head, out);
  return 0;
}

}  // extern "C"
