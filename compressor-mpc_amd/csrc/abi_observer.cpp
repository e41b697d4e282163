// Record producer, observer and control step of the C ABI (include/cmpc.h),
// with their host-array variants.
#include "abi_ctx.h"

#include <chrono>

using namespace cmpc_abi;

extern "C" {

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

// the a-priori step: ObserveAPriori(du, u_old_), u_old_ += du, with the
// solver's first move (du_full null) or the caller's full input change
static int observe_prior(cmpc_ctx* c, const char* who, const double* du_full, const char* stale) {
  if (c->obs_plant < 0) return fail(std::string(who) + ": call cmpc_observer_init first");
  if (c->lin_bound) return fail(std::string(who) + ": records are bound externally");
  HIP_TRY(hipSetDevice(c->device));
  ObserverParams P;
  observer_params(c, &P);
  P.du_full = du_full;
  c->pred_stale = stale;
  TimedLaunch tl(c, CMPC_KERNEL_OBSERVE_PRIOR);
  if (tl.begin()) return -1;
  if (cmpc_launch_observer(P, CMPC_OBS_PRIOR, c->stream))
    return fail(std::string(who) + ": no a-priori kernel instantiation for these dimensions");
  if (check_launch("observer a-priori kernel")) return -1;
  c->obs_steps++;  // the delay-block rings advance by one
  return tl.end();
}

int cmpc_observe_apply(cmpc_ctx* c) {
  if (!c) return fail("null context");
  return observe_prior(c, "cmpc_observe_apply", nullptr,
                       "u_old has moved since the build (cmpc_observe_apply applied the first move)");
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

int cmpc_observer_init_host(cmpc_ctx* c, int plant, double p_in, double p_out, double Ts,
                            const int32_t* input_order, const int32_t* out_idx,
                            const double* x_init, const double* u_full, const double* y_init,
                            const double* dx_init) {
  if (!c) return fail("null context");
  int ns = 0, ni = 0, no = 0, nci = 0;
  if (cmpc_plant_dims(plant, &ns, &ni, &no, &nci)) return fail("cmpc_observer_init_host: unknown plant");
  const size_t B = c->d.B;
  const double* h[4] = {x_init, u_full, y_init, dx_init};
  const size_t n[4] = {B * ns, B * ni, B * no, (size_t)c->nqp * c->L.ntot};
  return with_staged(c, h, n, 4, [&](const double* const* d) {
    return cmpc_observer_init(c, plant, p_in, p_out, Ts, input_order, out_idx, d[0], d[1], d[2], d[3]);
  });
}

int cmpc_observe_step_host(cmpc_ctx* c, const double* u_full, const double* y) {
  if (!c) return fail("null context");
  if (c->obs_plant < 0) return fail("cmpc_observe_step_host: call cmpc_observer_init first");
  int ns = 0, ni = 0, no = 0, nci = 0;
  if (cmpc_plant_dims(c->obs_plant, &ns, &ni, &no, &nci)) return fail("unknown plant");
  const size_t B = c->d.B;
  const double* h[2] = {u_full, y};
  const size_t n[2] = {B * ni, B * no};
  return with_staged(c, h, n, 2, [&](const double* const* d) { return cmpc_observe_step(c, d[0], d[1]); });
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

// DistributedController::UpdateU(du) (include/distributed_controller.h:145-152)
// with the caller's full input change: ObserveAPriori(du, u_old_), u_old_ += du.
int cmpc_update_u(cmpc_ctx* c, const double* du_full) {
  if (!c || !du_full) return fail("null argument");
  return observe_prior(c, "cmpc_update_u", du_full, "u_old has moved since the build (cmpc_update_u)");
}

int cmpc_update_u_host(cmpc_ctx* c, const double* du_full) {
  if (!c || !du_full) return fail("null argument");
  const double* h[1] = {du_full};
  const size_t n[1] = {(size_t)c->nqp * c->d.nu_tot};
  return with_staged(c, h, n, 1, [&](const double* const* d) { return cmpc_update_u(c, d[0]); });
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
  if (direct_download(c->stream, {{c->obs, dev.data(), sizeof(double) * dev.size()}})) return -1;
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

}  // extern "C"
