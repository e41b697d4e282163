/*
 * cmpc.h — C ABI of the MI355X-native condensed-QP hot path of
 * katie-jones/compressor-mpc (cooperative / non-cooperative / centralized
 * linear-time-varying MPC).
 *
 * Plain C, POD arguments only, int status returns (0 = ok, <0 = error; the
 * message is in cmpc_last_error()).  One context per (device, stream, host
 * thread); a context is not thread-safe.  All batched device buffers are
 * owned by the library; host arrays are owned by the caller.
 *
 * What each entry point replaces in the reference (paths relative to the
 * reference root):
 *
 *   cmpc_create            MpcQpSolver ctor  libs/mpc_qp_solver.cc:3-14,
 *                          DistributedController ctor libs/distributed_controller.cc:6-22,
 *                          NerveCenter ctor include/nerve_center.h:89-95
 *   cmpc_set_weights       MpcQpSolver::SetWeights include/mpc_qp_solver.h:62-80,
 *                          NerveCenter::SetWeights include/nerve_center.h:107-116
 *   cmpc_set_constraints   InputConstraints include/input_constraints.h:12-26
 *   cmpc_set_reference     MpcQpSolver::SetOutputReference include/mpc_qp_solver.h:94,
 *                          NerveCenter::SetOutputReference include/nerve_center.h:119-122
 *   cmpc_set_state         DistributedController::Initialize (u_old_) libs/distributed_controller.cc:27-67,
 *                          NerveCenter du_old_ include/nerve_center.h:73,94
 *   cmpc_upload_lin        AugmentedLinearizedSystem::Update result (A,B,C,f)
 *                          libs/aug_lin_sys.cc:145-177 + Observer state estimate
 *   cmpc_build             GenerateInitialQP libs/distributed_controller.cc:72-108 =
 *                          AdjustAllDelayedStates include/aug_lin_sys.h:141-154
 *                          + GeneratePrediction libs/aug_lin_sys.cc:260-334
 *                          + GenerateDistributedQP include/distributed_solver.h:83-94
 *                          + GenerateQP libs/mpc_qp_solver.cc:16-40
 *   cmpc_init_warmstart    MpcQpSolver::InitializeQPProblem libs/mpc_qp_solver.cc:77-101
 *   cmpc_iterate           Jacobi loop include/nerve_center.h:146-172 (SolveQPHelper :276-296,
 *                          DistributedController::GetInput include/distributed_controller.h:206-226,
 *                          ApplyOtherInput include/distributed_solver.h:98-103,
 *                          SolveQP libs/mpc_qp_solver.cc:42-75, UpdateUOld/SendUHelper
 *                          include/nerve_center.h:313-328)
 *   cmpc_step              cmpc_build + cmpc_iterate = NerveCenter::GetNextInputWithTiming
 *                          include/nerve_center.h:134-182
 *   cmpc_control_step      the same with the observer (ObserveAPosteriori, Update,
 *                          UpdateU: libs/observer.cc:8-44, libs/distributed_controller.cc:72-108,
 *                          include/distributed_controller.h:145-152) = GetNextInput
 *
 * The QP solver is this library's own warm-started dual active-set method
 * (qpOASES 3.2.0 SQProblem::hotstart is not vendored in the reference); it
 * keeps the reference's n_wsr_max = 10 cap (include/mpc_qp_solver.h:24) and
 * the zero-move fallback on any non-success (libs/mpc_qp_solver.cc:66-69).
 */
#ifndef CMPC_H
#define CMPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMPC_MAX_INPUTS 8   /* nu_tot */
#define CMPC_MAX_NV 8       /* m * nu */
#define CMPC_MAX_NS 15      /* plant states (+ inputs <= 16 lanes) */
#define CMPC_NWSR_MAX 10    /* include/mpc_qp_solver.h:24 */

/* QP status words (per QP slot, last solve of the step) */
#define CMPC_QP_OK 0          /* qpOASES::SUCCESSFUL_RETURN */
#define CMPC_QP_MAX_NWSR 1    /* > n_wsr_max working-set changes -> zero move */
#define CMPC_QP_INFEASIBLE 2  /* -> zero move */
#define CMPC_QP_NOT_PD 3      /* Hessian not positive definite -> zero move */
#define CMPC_QP_NONFINITE 4   /* non-finite plan (NaN / infinite gradient) -> zero move */

/* cmpc_iterate / cmpc_step flags */
#define CMPC_APPLY_MOVE 1u    /* u_old += first move (UpdateUOld/SendUHelper) */
#define CMPC_TRACE 2u         /* record working-set change sequences */

/* Problem dimensions.  All sub-controllers of a context share them
 * (coop: every sub-controller has nu own inputs, nu_tot - nu other inputs). */
typedef struct cmpc_dims {
  int32_t ns;      /* plant states                   AugmentedLinearizedSystem::n_states */
  int32_t ndist;   /* disturbance/integrator states  n_disturbance_states */
  int32_t nu_tot;  /* plant control inputs           n_control_inputs */
  int32_t nu;      /* own inputs per sub-controller  n_sub_control_inputs */
  int32_t ny;      /* controlled outputs             ControlledOutputIndices::size */
  int32_t p;       /* prediction horizon */
  int32_t m;       /* move horizon */
  int32_t delay[CMPC_MAX_INPUTS]; /* Delays, per sub-controller-ordered input */
  int32_t S;       /* sub-controllers per scenario (NerveCenter pack size) */
  int32_t B;       /* independent scenarios in the batch */
} cmpc_dims;

/* Derived sizes and the packed per-QP input record ("lin record").
 * One record per QP slot q = b * S + s (scenario-major), doubles, row-major:
 *   [off_A ] Aorig   ns x ns        discrete A       (AComposite::Aorig)
 *   [off_B ] Bin     ns x nu_tot    column c = input c of this sub-controller's
 *                                   ordering: Borig column if delay[c]==0,
 *                                   Adelay column otherwise (BComposite/AComposite)
 *   [off_C ] Csel    ny x nobs      controlled rows of C = [Cplant | I_dist]
 *   [off_f ] fd      ns             discrete affine term (GetDerivative())
 *   [off_x ] dxaug   naug           observer augmented state tail: ndist
 *                                   disturbance, nd delayed-input slots, then
 *                                   per delayed input delay-1 shift states
 *                                   (raw: AdjustAllDelayedStates is applied here)
 *   [off_y ] yprev   ny             controlled part of the measured output
 * stride = rec_len (multiple of 8 doubles). */
typedef struct cmpc_layout {
  int32_t nd, n_delay_states, naug, nobs, ntot, nV, nuo, nVo;
  int32_t off_A, off_B, off_C, off_f, off_x, off_y, rec_len;
} cmpc_layout;

/* Fill *L from *d.  Returns 0, or <0 if the dimensions are unsupported. */
int cmpc_layout_of(const cmpc_dims* d, cmpc_layout* L);

typedef struct cmpc_ctx cmpc_ctx;

/* Context on HIP device `device`, all work on a private non-blocking stream
 * unless cmpc_set_stream() is called. */
int cmpc_create(cmpc_ctx** ctx, const cmpc_dims* dims, int device);
int cmpc_destroy(cmpc_ctx* ctx);
int cmpc_set_stream(cmpc_ctx* ctx, void* hip_stream);
const char* cmpc_last_error(void);
int cmpc_get_layout(const cmpc_ctx* ctx, cmpc_layout* L);

/* Per sub-controller configuration (s = 0..S-1), shared by all scenarios. */
int cmpc_set_weights(cmpc_ctx* ctx, int s, const double* uwt /* nu x nu */,
                     const double* ywt /* ny x ny */);
int cmpc_set_constraints(cmpc_ctx* ctx, int s, const double* lower,
                         const double* upper, const double* rate_lower,
                         const double* rate_upper); /* each nu */
int cmpc_set_reference(cmpc_ctx* ctx, int s, const double* y_ref /* p x ny */);

/* Mutable per-slot state.  Any pointer may be NULL (left unchanged).
 * u_old  : B*S*nu_tot  sub-controller's u_old_ in its own input ordering
 * du_old : B*S*nV      previous step's move plans (NerveCenter::du_old_)
 * ws     : B*S         warm-start working-set words */
int cmpc_set_state(cmpc_ctx* ctx, const double* u_old, const double* du_old,
                   const uint32_t* ws);
int cmpc_get_state(cmpc_ctx* ctx, double* u_old, double* du_old, uint32_t* ws);
/* Bind external device-resident state arrays (shapes as above, on the ctx
 * device, 8-byte aligned): every later call reads and updates them in place
 * of the context's own state, as if they were the context's.  All three
 * pointers, or all NULL to re-bind the context's own buffers.  Lets one
 * context serve several sets of B scenarios in rotation (cmpc_bind_lin for
 * their records), each set warm-started from its own previous step, as each
 * reference controller hot-starts its own QProblem (libs/mpc_qp_solver.cc:42-75). */
int cmpc_bind_state(cmpc_ctx* ctx, double* u_old_device, double* du_old_device,
                    uint32_t* ws_device);

/* Inputs: B*S lin records from host memory (H2D copy on the ctx stream), or
 * written in place by a device-side producer through cmpc_lin_device(). */
int cmpc_upload_lin(cmpc_ctx* ctx, const double* lin_host);
void* cmpc_lin_device(cmpc_ctx* ctx);
/* Copy the context's own record buffer to the host (B*S*rec_len doubles),
 * e.g. to inspect what cmpc_produce_lin wrote. */
int cmpc_download_lin(cmpc_ctx* ctx, double* lin_host);
/* Bind an external device-resident record array (B*S*rec_len doubles on the
 * ctx device, 16-byte aligned, e.g. the output of a device-side producer);
 * NULL re-binds the context's own buffer.  Takes effect for the next
 * cmpc_build.  cmpc_bind_lin and cmpc_bind_state check that each pointer is
 * device memory of the context's device inside an allocation of the
 * required size, once per (pointer, size) and context: re-binding a buffer
 * freed and re-allocated at the same address is not re-checked. */
int cmpc_bind_lin(cmpc_ctx* ctx, const double* lin_device);

/* Per-scenario setpoints and input limits (slot order q = b*S + s).
 *
 * Per slot: a constant setpoint offset dy_ref[q] (ny values) and the four
 * limit vectors (nu values each).  Slot q then tracks y_ref[s][r] + dy_ref[q]
 * at every horizon row r, inside its own lower/upper/rate limits.  Shared by
 * the batch as before: the weights (cmpc_set_weights) and the reference's
 * base shape over the horizon (cmpc_set_reference).  A reference that differs
 * between scenarios in more than a constant is a reference profile (below).
 *
 * The offset is applied in the build kernels as y_prev - dy_ref: the reference
 * enters the free response only as kappa - L_W' y_ref with kappa = C_dist
 * x_dist + L_W' y_prev, so a build with the offset computes, bit for bit, what
 * a build without it computes from records whose y_prev is y_prev - dy_ref
 * (one FP64 subtraction).  H and G do not depend on it.  The limits replace
 * the sub-controller's cmpc_set_constraints block in every solve
 * (cmpc_iterate, cmpc_step, cmpc_control_step, cmpc_init_warmstart,
 * cmpc_get_input, cmpc_coupled_iterate); lb/ub still subtract the slot's
 * u_old.  cmpc_qp_solve_batch[_map] take their own per-QP bounds and ignore
 * both.  With nothing set (the default, and the state after a clear) every
 * call computes exactly what it did without these arrays.
 *
 * cmpc_set_scenario_*: host arrays, validated (finite, lower <= upper,
 * rate_lower <= rate_upper; the message names the first bad slot) and copied
 * on the ctx stream into buffers the context owns.  All four limit arrays or
 * all NULL (clear); a NULL dy_ref clears.
 * cmpc_bind_scenario_*: device arrays read in place by every later call
 * (checked as cmpc_bind_state checks: device memory of the ctx device inside
 * an allocation of the required size, 8-byte aligned); NULL clears.  The
 * bound limits are one array of B*S*4*nu doubles, per slot
 * [lower | upper | rate_lower | rate_upper], and are not validated.
 * cmpc_get_scenario_*: host copies of what is in force (set or bound); -1 if
 * nothing is.  NULL limit outputs are skipped. */
int cmpc_set_scenario_reference(cmpc_ctx* ctx, const double* dy_ref /* B*S*ny */);
int cmpc_bind_scenario_reference(cmpc_ctx* ctx, const double* dy_ref_device /* B*S*ny */);
int cmpc_set_scenario_constraints(cmpc_ctx* ctx, const double* lower, const double* upper,
                                  const double* rate_lower, const double* rate_upper); /* each B*S*nu */
int cmpc_bind_scenario_constraints(cmpc_ctx* ctx, const double* limits_device /* B*S*4*nu */);
int cmpc_get_scenario_reference(cmpc_ctx* ctx, double* dy_ref);
int cmpc_get_scenario_constraints(cmpc_ctx* ctx, double* lower, double* upper, double* rate_lower,
                                  double* rate_upper);

/* Per-scenario reference profiles over the horizon (slot order q = b*S + s).
 *
 * dref[q][r][o], B*S*p*ny doubles (slot, then horizon row, then output: the
 * layout of cmpc_predict's y_pred, so one run's prediction can be another's
 * target).  With a profile in force slot q tracks
 *   y_ref[s][r] + dy_ref[q] + dref[q][r]
 * at horizon row r: the profile adds to the constant offset of
 * cmpc_set_scenario_reference, it does not replace it.  Setpoint steps or
 * ramps scheduled at different times in different scenarios, and changes the
 * controller sees coming inside its horizon (preview), are profiles.
 *
 * H and G do not depend on the reference and f is affine in it: the profile
 * changes the QP only by f <- f - Su' w, w[r] = ywt[s] dref[q][r] (ywt[q]
 * where per-slot weights are in force, below).  cmpc_build
 * launches a correction kernel (refshift.hip) right after its build kernel,
 * on the same stream: a backward sweep over the slot's record that never
 * forms Su, and one FP64 subtraction per entry of f in place; H and G are
 * neither read nor written.  cmpc_download_qp, cmpc_iterate,
 * cmpc_init_warmstart, cmpc_get_input and cmpc_coupled_iterate therefore see
 * the corrected f.  Like dy_ref it takes effect at the next build.  The
 * correction has no timing slot: cmpc_kernel_time(CMPC_KERNEL_BUILD) stays
 * the build kernel's own time.
 *
 * The fused paths keep f in registers and cannot take the correction.  With
 * a profile in force cmpc_step runs as cmpc_build + cmpc_iterate (the same
 * results bit for bit; cmpc_last_step_fused() == 0), CMPC_STEP_FUSED forced
 * fails (CMPC_PLAN_PROFILE_NEEDS_SPLIT), and cmpc_control_step* runs as its
 * three calls.  cmpc_plan answers for this case under CMPC_PLAN_REF_PROFILE.
 * cmpc_predict honours the profile (e[r] below), so its identity keeps
 * holding.  With nothing set (the default, and the state after a clear) every
 * call computes exactly what it did without a profile.
 *
 * set / bind / get as for cmpc_*_scenario_reference: set validates (every
 * value finite; the message names the first bad slot) and copies on the ctx
 * stream into a buffer allocated on first use, NULL clears; bind is checked
 * as cmpc_bind_state checks its pointers, for B*S*p*ny doubles, 8-byte
 * aligned, NULL clears; get returns -1 if nothing is in force.  set and bind
 * fail with a message where the dimensions have no kernel instance
 * (cmpc_reference_profile_available: host only, 1 for every dimension set
 * with a one-QP-per-wave build instance, 0 elsewhere). */
int cmpc_set_scenario_reference_profile(cmpc_ctx* ctx, const double* dref /* B*S*p*ny */);
int cmpc_bind_scenario_reference_profile(cmpc_ctx* ctx, const double* dref_device /* B*S*p*ny */);
int cmpc_get_scenario_reference_profile(cmpc_ctx* ctx, double* dref);
int cmpc_reference_profile_available(const cmpc_dims* dims);

/* Per-scenario weights (slot order q = b*S + s).
 *
 * With per-slot weights in force slot q is built with its own ywt[q] (ny x ny,
 * symmetric positive semi-definite) and uwt[q] (nu x nu, symmetric) in place
 * of cmpc_set_weights(s): a sweep of the output and move weights over a grid
 * or a random design, on the same plant and the same disturbances, is one
 * batch.  The shared weights must still be set; they stay in force for
 * anything per-slot weights do not cover, and come back after a clear.
 *
 * Weights change H and G, so unlike a reference profile they cannot be a
 * correction after the build: the one-QP-per-wave build kernel has instances
 * that load the slot's block [L_W'[q] | uwt[q]] (ywt[q] = L_W[q] L_W'[q]) into
 * a per-wave table and form yhat[q] = L_W'[q] y_ref[s] there.  A slot whose
 * block equals sub-controller s's shared one bit for bit gets the
 * bit-identical H, f and G of CMPC_BUILD_WAVE.  Only that kernel takes them:
 * the build is CMPC_BUILD_WAVE at every batch size under CMPC_BUILD_AUTO
 * (cmpc_last_build_kernel reports it), CMPC_BUILD_ROWS or CMPC_BUILD_SPLIT
 * forced fails (CMPC_PLAN_WEIGHTS_NEED_WAVE), and nothing is fused: cmpc_step
 * runs as cmpc_build + cmpc_iterate (cmpc_last_step_fused() == 0),
 * CMPC_STEP_FUSED forced fails (CMPC_PLAN_WEIGHTS_NEED_SPLIT) and
 * cmpc_control_step* runs as its three calls.  cmpc_plan answers for this
 * case under CMPC_PLAN_SCENARIO_WEIGHTS.  Build pairing applies to the row
 * build only and needs nothing.  cmpc_predict and a reference profile's
 * correction read the slot's block too (ywt[q], uwt[q] in their formulae).
 * With nothing set (the default, and the state after a clear) every call
 * computes exactly what it did without per-slot weights.
 *
 * cmpc_weight_factor (host only): lwt = L_W' (upper triangular, ny x ny
 * row-major) with ywt = L_W L_W', the Cholesky factorisation the library uses
 * for the shared weights as well, so a slot whose ywt equals the shared one
 * bit for bit gets a bit-identical L_W'.  It tests symmetry and allows zero
 * pivots for positive semi-definite weights; -1 with a message otherwise.
 * cmpc_set_scenario_weights: host arrays, every slot validated (finite values,
 * ywt symmetric positive semi-definite as above, uwt symmetric; the message
 * names the first bad slot), factored on the host and copied on the ctx stream
 * into a buffer allocated on first use, one block per slot
 * [L_W' (ny*ny) | uwt (nu*nu)].  Both pointers NULL clears; exactly one NULL is
 * an error.
 * cmpc_bind_scenario_weights: the same packed per-slot blocks in device
 * memory, already factored (cmpc_weight_factor), read in place by every later
 * call; checked as cmpc_bind_state checks its pointers, for
 * B*S*(ny*ny + nu*nu) doubles, 8-byte aligned; not validated.  NULL clears.
 * cmpc_get_scenario_weights: host copies of what is in force, uwt and the
 * factor L_W' (either pointer may be NULL); -1 if nothing is.
 * set and bind take effect at the next build, and fail with a message where
 * cmpc_scenario_weights_available is 0 (host only: 1 for every dimension set
 * with a one-QP-per-wave build instance whose LDS still fits with the
 * per-wave tables, 0 elsewhere). */
int cmpc_set_scenario_weights(cmpc_ctx* ctx, const double* uwt /* B*S*nu*nu */, const double* ywt /* B*S*ny*ny */);
int cmpc_bind_scenario_weights(cmpc_ctx* ctx, const double* weights_device /* B*S*(ny*ny + nu*nu) */);
int cmpc_get_scenario_weights(cmpc_ctx* ctx, double* uwt, double* ywt_factor /* L_W', B*S*ny*ny */);
int cmpc_scenario_weights_available(const cmpc_dims* dims);
int cmpc_weight_factor(int ny, const double* ywt, double* lwt);

/* Per-scenario boundary pressures of the controller's model:
 * B x 2 doubles, [p_in, p_out] of scenario b, the plant's suction and discharge
 * pressures that cmpc_produce_lin and cmpc_observer_init otherwise take as two
 * scalars for the whole batch.  Per scenario, not per slot: the sub-controllers
 * of a scenario model one plant.  While an array is in force
 *   - cmpc_produce_lin and cmpc_observer_init IGNORE their scalar p_in / p_out
 *     arguments and linearise scenario b at its own pair;
 *   - cmpc_observe_step and cmpc_control_step* (the one-launch kernel, its
 *     role-split pairs and polled completion, and the three-call form alike)
 *     do the same in place of the scalars cmpc_observer_init kept.
 * Only the record producer reads it: kernel selection (cmpc_plan), the build,
 * the solves and cmpc_predict are what they were, and a scenario whose pair
 * equals the scalars gets bit-identical records.
 * cmpc_set_scenario_pressures: a host array, every value checked finite and
 * > 0 (the message names the first bad scenario), copied on the ctx stream into
 * a buffer the context owns, allocated on first use.  NULL clears: back to the
 * scalars.
 * cmpc_bind_scenario_pressures: a device array read in place at each later
 * launch, so the caller may rewrite it between steps (on the ctx stream, or
 * ordered with it); checked as cmpc_bind_state checks its pointers, for B*2
 * doubles, 8-byte aligned; the contents are not checked.  NULL clears.
 * cmpc_get_scenario_pressures: a host copy of what is in force; -1 if
 * nothing is.
 * cmpc_check_pressures (host only): the check of the host setters here and of
 * cmpc_sim_set_pressures_host on B pairs; -1 with their message. */
int cmpc_check_pressures(int B, const double* pressures /* B*2, host */);
int cmpc_set_scenario_pressures(cmpc_ctx* ctx, const double* pressures /* B*2, host */);
int cmpc_bind_scenario_pressures(cmpc_ctx* ctx, const double* pressures_device /* B*2 */);
int cmpc_get_scenario_pressures(cmpc_ctx* ctx, double* pressures /* B*2, host */);

/* Hot path. */
int cmpc_build(cmpc_ctx* ctx);
/* Kernel selection.  Which kernel an entry point launches is decided by one
 * host function, cmpc_dispatch_plan (compressor-mpc_amd/csrc/dispatch.cpp),
 * from the dimensions, the batch, the device's CU count and the three
 * variants below; its thresholds and the measurements behind them are
 * beside it and in DESIGN.md §3.0.  cmpc_plan() further down answers the
 * same question without a device.  With cus = compute units, nqp = B * S:
 *
 * Build (cmpc_build; the same H, f, G within rounding):
 *   CMPC_BUILD_ROWS   four QPs per wave, one per 16-lane DPP row (m <= 2, an
 *                     LDS layout exists); an error where it is not available
 *   CMPC_BUILD_WAVE   one QP per wave (every instantiated dimension set)
 *   CMPC_BUILD_SPLIT  one QP per two waves, the DPP chain in one and the
 *                     gather in the other (every ny, the ny = 4 simulation
 *                     pre-pass included)
 *   CMPC_BUILD_AUTO   (default) rows where available and ceil(nqp / 4) >=
 *                     4 cus (a row group per SIMD); else split up to
 *                     nqp <= 4 cus (one QP per SIMD); else wave
 * WAVE and SPLIT give the same QP bit for bit; ROWS sums in another order
 * (agreement within rounding, 1e-11 relative). */
#define CMPC_BUILD_AUTO 0
#define CMPC_BUILD_WAVE 1
#define CMPC_BUILD_ROWS 2
#define CMPC_BUILD_SPLIT 3
int cmpc_set_build_variant(cmpc_ctx* ctx, int variant);
/* The build kernel the last cmpc_build, cmpc_step or cmpc_control_step
 * launched (CMPC_BUILD_WAVE, CMPC_BUILD_ROWS or CMPC_BUILD_SPLIT), 0 before the
 * first build, <0 on a null context. */
int cmpc_last_build_kernel(cmpc_ctx* ctx);
/* Build pairing: a mode of the row build (CMPC_BUILD_ROWS, chosen or forced as
 * above; cmpc_plan and cmpc_last_build_kernel report ROWS either way).  The
 * two sub-controllers of a cooperative scenario linearise the same plant at
 * the same point: their records' A, C and f are equal and slot 1's B is slot
 * 0's with the columns rotated by nu.  The shared form builds one scenario per
 * 16-lane row and computes the Markov chain once for both QPs; the QP buffer
 * is bit-identical to the unpaired row build's.  Per scenario the kernel
 * compares the two records' A, B, C and f as 64-bit integers; a group of four
 * scenarios with any difference is built the long way (same results, about
 * the unpaired cost), so records need not satisfy the assumption.
 *   CMPC_PAIRING_AUTO  (default) the shared form where the configuration is
 *                      eligible and the batch is large enough to gain
 *   CMPC_PAIRING_OFF   never
 *   CMPC_PAIRING_ON    whenever the row build runs a cmpc_build; an error
 *                      naming the failed condition where the configuration is
 *                      not eligible: from cmpc_set_build_pairing for the
 *                      dimensions, from cmpc_build / cmpc_step for the weights
 * Eligible: S = 2, nu_tot = 2 nu, delay[c] == delay[(c + nu) % nu_tot], the
 * sub-controllers' L_W' (ywt's Cholesky factor) bitwise equal, a shared-form
 * instance for (ns, ny, nu, m) (the parallel plant's cooperative set), plain
 * hand-off lines (no ring) and LDS for two workgroups per CU.  The fused steps
 * and the one-launch control step keep the unpaired kernels. */
#define CMPC_PAIRING_AUTO 0
#define CMPC_PAIRING_OFF 1
#define CMPC_PAIRING_ON 2
int cmpc_set_build_pairing(cmpc_ctx* ctx, int mode);
/* The eligibility above, without a device (the batch size aside): 1 or 0.
 * lwt_s0 / lwt_s1: the two sub-controllers' L_W' tables (ny x ny, row-major),
 * or null to leave the weights out.  cmpc_build_pairing_reason: "" when
 * eligible, else the failed condition. */
int cmpc_build_pairing_available(const cmpc_dims* dims, const double* lwt_s0, const double* lwt_s1);
const char* cmpc_build_pairing_reason(const cmpc_dims* dims, const double* lwt_s0, const double* lwt_s1);
/* Scenarios the last cmpc_build (or unfused cmpc_step) built in the shared
 * form; the rest of the batch was built the long way.  -1 if that build was
 * not the shared form, < -1 on error.  Synchronises the context's stream. */
int cmpc_last_build_shared_scenarios(cmpc_ctx* ctx);
/* Solve (cmpc_iterate / cmpc_init_warmstart / cmpc_get_input; the same
 * results bit for bit):
 *   CMPC_SOLVE_LANE  one QP per lane
 *   CMPC_SOLVE_ROWS  one QP per 16-lane DPP row, its H^-1 and matrix-vector
 *                    products spread over the row (needs S | 4; an error
 *                    where it is not available)
 *   CMPC_SOLVE_AUTO  (default) rows, where available, for nV >= 6 below
 *                    16 384 QPs and for smaller nV up to nqp <= 16 cus
 *                    (four QPs per SIMD); else lane */
#define CMPC_SOLVE_AUTO 0
#define CMPC_SOLVE_LANE 1
#define CMPC_SOLVE_ROWS 2
int cmpc_set_solve_variant(cmpc_ctx* ctx, int variant);
/* The solve kernel the last iterate / init / get-input launched. */
int cmpc_last_solve_kernel(cmpc_ctx* ctx);
/* Step (cmpc_step).  One launch: the build kernel runs the K Jacobi
 * iterations of the QPs it built, H, f, G handed over in registers (the same
 * results bit for bit as cmpc_build + cmpc_iterate on the same build kernel).
 *   CMPC_STEP_SPLIT  two launches
 *   CMPC_STEP_FUSED  one launch (K > 0): the one-QP-per-wave kernel below a
 *                    row group per SIMD, else the row kernel; an error where
 *                    neither has a fused instance for the dimensions
 *   CMPC_STEP_AUTO   (default) one launch when the build and solve variants
 *                    are AUTO too, nV >= 6, p >= 50 and cus < nqp <= 4 cus;
 *                    two launches otherwise (nV <= 4 at every size) */
#define CMPC_STEP_AUTO 0
#define CMPC_STEP_SPLIT 1
#define CMPC_STEP_FUSED 2
int cmpc_set_step_variant(cmpc_ctx* ctx, int variant);
/* 1 if the last cmpc_step ran fused, 0 if split, <0 on a null context. */
int cmpc_last_step_fused(cmpc_ctx* ctx);

/* What the entry points will launch, answered on the host (no device, no
 * context): the plan of cmpc_dispatch_plan for a batch of dims->B scenarios
 * on a device of `cus` compute units under the three variants, for calls
 * with K iterations and `flags` (CMPC_TRACE; CMPC_PLAN_DU_OTHER: the solve is
 * a cmpc_get_input with the other controllers' plans given;
 * CMPC_PLAN_REF_PROFILE: a reference profile is in force, so no path is
 * fused: step_fused, control_fused, control_grid and control_polled are 0 and
 * the step's kernels are those of CMPC_STEP_SPLIT;
 * CMPC_PLAN_SCENARIO_WEIGHTS: per-slot weights are in force, so the build is
 * CMPC_BUILD_WAVE at every batch size under CMPC_BUILD_AUTO, ROWS or SPLIT
 * forced is a build error, and no path is fused, as under
 * CMPC_PLAN_REF_PROFILE).  A context takes the same plan with its device's CU
 * count. */
#define CMPC_PLAN_DU_OTHER 0x100u
#define CMPC_PLAN_REF_PROFILE 0x200u
#define CMPC_PLAN_SCENARIO_WEIGHTS 0x400u
/* plan errors: what a call fails with (cmpc_plan_error_string) */
#define CMPC_PLAN_OK 0
#define CMPC_PLAN_NO_ROWS_BUILD 1  /* CMPC_BUILD_ROWS forced, not available */
#define CMPC_PLAN_NO_BUILD 2       /* no build kernel instance for (ns, ny, nu, m) */
#define CMPC_PLAN_NO_ROWS_SOLVE 3  /* CMPC_SOLVE_ROWS forced, not available */
#define CMPC_PLAN_NO_SOLVE 4       /* no solve kernel instance for (nV, nu, nVo) */
#define CMPC_PLAN_NO_FUSED_STEP 5  /* CMPC_STEP_FUSED forced, not available */
#define CMPC_PLAN_PROFILE_NEEDS_SPLIT 6  /* CMPC_STEP_FUSED forced with a reference profile in force */
#define CMPC_PLAN_WEIGHTS_NEED_WAVE 7    /* CMPC_BUILD_ROWS or CMPC_BUILD_SPLIT forced with per-slot weights in force */
#define CMPC_PLAN_WEIGHTS_NEED_SPLIT 8   /* CMPC_STEP_FUSED forced with per-slot weights in force */
#define CMPC_PLAN_NO_WEIGHTS_BUILD 9     /* per-slot weights: no build instance, or its LDS does not fit */
typedef struct cmpc_plan_t {
  /* cmpc_build */
  int32_t build_kernel;        /* CMPC_BUILD_WAVE / ROWS / SPLIT; 0 with build_error */
  int32_t build_error;
  /* cmpc_iterate / cmpc_init_warmstart / cmpc_get_input */
  int32_t solve_kernel;        /* CMPC_SOLVE_LANE / ROWS; 0 with solve_error */
  int32_t solve_error;         /* (the message follows "<entry point>: ") */
  /* cmpc_step: one launch, or cmpc_build + cmpc_iterate as above; the two
   * kernels are what cmpc_last_build_kernel / cmpc_last_solve_kernel report
   * after it */
  int32_t step_fused;
  int32_t step_build_kernel, step_solve_kernel;
  int32_t step_error;          /* CMPC_PLAN_NO_FUSED_STEP, CMPC_PLAN_PROFILE_NEEDS_SPLIT,
                                  CMPC_PLAN_WEIGHTS_NEED_SPLIT or 0 */
  /* cmpc_control_step: one launch, or the three calls with cmpc_step as above */
  int32_t control_fused;
  int32_t control_build_kernel, control_solve_kernel;
  int32_t control_grid;        /* workgroups of the one launch (0: three calls) */
  int32_t control_polled;      /* cmpc_control_step_download polls its completion */
} cmpc_plan_t;
int cmpc_plan(const cmpc_dims* dims, int cus, int build_variant, int solve_variant, int step_variant,
              int K, uint32_t flags, cmpc_plan_t* plan);
/* the text cmpc_last_error() holds after a call that failed with this plan error */
const char* cmpc_plan_error_string(int plan_error);
/* Diagnostic (no GPU needed): the row kernel's LDS layout for *dims as
 * cmpc_build chooses it.  Writes the bank-conflict model's extra LDS cycles
 * per wave-step of the horizon loop (wave 0) for the packed layout (regions
 * back to back) and for the chosen one, and the chosen layout's LDS bytes per
 * workgroup.  Returns 0, or -1 if the row kernel cannot run these dims. */
int cmpc_rows_lds_model(const cmpc_dims* dims, double* packed_cycles, double* chosen_cycles,
                        int32_t* lds_bytes);
int cmpc_init_warmstart(cmpc_ctx* ctx);
int cmpc_iterate(cmpc_ctx* ctx, int K, uint32_t flags);
int cmpc_step(cmpc_ctx* ctx, int K, uint32_t flags);
int cmpc_synchronize(cmpc_ctx* ctx);

/* Results of the last cmpc_iterate (any pointer may be NULL).
 * du: B*S*nV move plans; status/nwsr: B*S of the last solve. */
int cmpc_download(cmpc_ctx* ctx, double* du, int32_t* status, int32_t* nwsr);
/* The condensed QPs of the last cmpc_build (parity/debug):
 * H: B*S*nV*nV (row-major), f: B*S*nV, G: B*S*nV*nVo (G = Su' W Su_other). */
int cmpc_download_qp(cmpc_ctx* ctx, double* H, double* f, double* G);
/* Working-set change sequences of the last traced cmpc_iterate:
 * trace: B*S*K*16 bytes (bit7 add, bit6 upper side, bits0-5 constraint j;
 * 0xFF terminates), ntrace: B*S*K counts. */
int cmpc_download_trace(cmpc_ctx* ctx, uint8_t* trace, int32_t* ntrace);

/* Prediction: what the controller expects plans to do (the reference hands
 * out Prediction{Su, Sx, Sf, Su_other}, include/prediction.h,
 * AugmentedLinearizedSystem::GeneratePrediction, and leaves the products to
 * the caller).  For QP slot q = b*S + s, its record and u_old as the last
 * build read them, a plan du (nV) and the other controllers' plans d (nVo, in
 * the Jacobi iteration's order d[mv*nuo + rank*nu + c], rank = index among the
 * scenario's other sub-controllers):
 *   y_pred[r] = y_prev + (Su du + Su_other d + Sf fd + Sx xa)[r],  r = 0..p-1
 *   e[r]      = y_pred[r] - (y_ref[s][r] + dy_ref[q] + dref[q][r])
 *   J_track   = 1/2 sum_r e[r]' ywt[s] e[r]
 *   J_move    = 1/2 sum_mv du_mv' uwt[s] du_mv
 * with xa the record's dx_aug after AdjustAllDelayedStates (u_old); ywt[q] and
 * uwt[q] in place of ywt[s] and uwt[s] where per-slot weights are in force
 * (cmpc_set/bind_scenario_weights).  Then
 *   J_track + J_move - J_track(du = 0) = 1/2 du' H du + (f + G d)' du,
 * the objective of the QP the step solved.  Limits do not enter.
 *
 * cmpc_predict: asynchronous on the ctx stream.  du_device NULL: the
 * context's current plans (what cmpc_download returns).  du_other_device
 * NULL: gathered from the other slots of the same scenario, out of the same
 * array as du (needs nu_tot = S * nu); ignored for nVo = 0.  flags must be 0.
 * cmpc_predict_host: the same two arrays from host memory (staged as the
 * other _host calls stage theirs).
 * Results: y_pred, B*S*p*ny doubles (slot, then horizon row, then output),
 * and cost, B*S*2 doubles [J_track, J_move]; the two buffers are allocated by
 * the first cmpc_predict (the pointers are NULL before), so a context that
 * never predicts allocates nothing for it.  cmpc_download_prediction makes
 * host copies (either pointer may be NULL); -1 before the first prediction.
 *
 * The prediction reads what the build read (records, u_old, weights and
 * references, dy_ref).  cmpc_predict is refused (-1, the message names the
 * cause) before a build has run (cmpc_build, or the build inside cmpc_step /
 * cmpc_control_step) and after any call that changed one of them since:
 * CMPC_APPLY_MOVE in any call, cmpc_observe_apply, cmpc_update_u[_host],
 * cmpc_control_step*, cmpc_set_state with u_old, cmpc_bind_state,
 * cmpc_upload_lin, cmpc_bind_lin, cmpc_produce_lin, cmpc_observe_step*,
 * cmpc_observer_init*, cmpc_set_weights, cmpc_set_reference,
 * cmpc_set/bind_scenario_reference, cmpc_set/bind_scenario_reference_profile,
 * cmpc_set/bind_scenario_weights.
 * The flag lives on the host: writes the
 * library does not see (a producer writing through cmpc_lin_device(), bound
 * state or offsets changed by the caller's kernels) are the caller's to order.
 *
 * cmpc_predict_available: host only, 1 where a predict kernel instance
 * exists (every dimension set that has a one-QP-per-wave build instance), 0
 * elsewhere; cmpc_predict fails with a message for other dimensions. */
int cmpc_predict(cmpc_ctx* ctx, const double* du_device, const double* du_other_device, uint32_t flags);
int cmpc_predict_host(cmpc_ctx* ctx, const double* du, const double* du_other, uint32_t flags);
double* cmpc_prediction_device(cmpc_ctx* ctx);
double* cmpc_prediction_cost_device(cmpc_ctx* ctx);
int cmpc_download_prediction(cmpc_ctx* ctx, double* y_pred, double* cost);
int cmpc_predict_available(const cmpc_dims* dims);

/* Closed-loop performance indices per QP slot (score.hip).
 *
 * How well each scenario of a batch did, kept on the device: one small launch
 * per sampling instant (cmpc_score_step) reads the step's results where the
 * context holds them and updates a running record per QP slot q = b*S + s.
 * With e[o] = y[b][out_idx[s][o]] - r[q][o], r = target[q] where a target is
 * given and y_ref[s][0] + dy_ref[q] otherwise (row 0 of cmpc_set_reference,
 * dy_ref of cmpc_set/bind_scenario_reference where one is in force), du the
 * slot's first move of its own inputs, and k the step index (0 after a reset,
 * counted on the host):
 *
 *   field            rows  update at step k
 *   n                1     += 1
 *   ise[o]           ny    += (e e) Ts
 *   iae[o]           ny    += |e| Ts
 *   peak[o]          ny    max(peak, |e|)
 *   last_out[o]      ny    k if |e| > band[s][o]; starts at -1: the settling
 *                          time is (last_out + 1) Ts
 *   j_track          1     += 1/2 |L_W' e|^2, the realised stage cost in the
 *                          controller's own weights (the slot's ywt[q] where
 *                          per-slot weights are in force)
 *   j_move           1     += 1/2 du' uwt du (uwt[q] likewise)
 *   tv[c]            nu    += |du[c]|
 *   sat_bound[c]     nu    += 1 when status == CMPC_QP_OK and the slot's
 *                          working-set word holds the first move's bound of own
 *                          input c (bit c, either side)
 *   sat_rate[c]      nu    the same for its rate row (bit nV + c)
 *   n_fail           1     += 1 when status != CMPC_QP_OK
 *   nwsr_sum         1     += nwsr
 *   plant_fail_step  1     the first k with a non-zero plant status; -1 until then
 *
 * All fields are doubles (the counters are exact far beyond any run length),
 * in this order, cmpc_score_len(dims) = 4 ny + 3 nu + 6 rows in all.  Storage
 * is field-major: row f of slot q at f*B*S + q.  cmpc_score_field gives a
 * field's first row and row count by name (-1 for an unknown name); callers
 * take offsets from it.  The sums are plain FP64 multiplies and adds in the
 * order written, so a float64 host model reproduces every field but j_track
 * and j_move (any fixed order) bit for bit.
 *
 * cmpc_score_enable: out_idx (host, S*ny) names the plant output of each
 *   controlled output in y (B x n_outputs), as cmpc_produce_lin's; band (host,
 *   S*ny, or NULL for 0) the settling bands; Ts the sampling time.  Allocates
 *   the context's own record and resets it.  Refused: out_idx outside
 *   [0, n_outputs), a negative or non-finite band or Ts, dimensions without a
 *   kernel instance.  cmpc_score_check is the same check without a context
 *   (host only).  A context that never enables scoring allocates and launches
 *   nothing for it.
 * cmpc_score_bind: keep the record in a caller's device buffer (len*B*S
 *   doubles, checked as cmpc_bind_state checks its pointers, 8-byte aligned);
 *   NULL: the context's own again.  The buffer is taken as it is: follow with
 *   cmpc_score_reset.
 * cmpc_score_capture: also record the trajectories of n_sel chosen scenarios
 *   (host list), one row [y (n_outputs) | u_control (nu_tot) | x (ns)] per
 *   step k < t_cap into a t_cap x n_sel x width buffer, in the same launch;
 *   later steps are dropped, not wrapped.  n_sel = 0 turns it off.  Refused:
 *   t_cap < 1, an index outside [0, B) or given twice
 *   (cmpc_score_capture_check: the same, host only).  The buffer is allocated
 *   here and zeroed; cmpc_score_bind_capture puts the rows into a caller's
 *   device buffer instead (checked as above; NULL: the own one).
 * cmpc_score_reset: every field to 0, last_out and plant_fail_step to -1,
 *   k = 0, the context's own capture buffer to 0.
 * cmpc_score_step: device pointers, asynchronous on the ctx stream.  y: B x
 *   n_outputs; target: B*S x ny or NULL; plant_status: B int32 (the
 *   simulator's status words) or NULL; u_control (B x nu_tot) and x (B x ns)
 *   feed the capture only and may be NULL (their columns stay zero).  Valid
 *   once a solve has run (cmpc_iterate, cmpc_step, any cmpc_control_step*,
 *   cmpc_get_input, cmpc_init_warmstart); it scores that solve's results as
 *   they stand in the context, so call it after the step's solves and before
 *   the next build.  Refused: not enabled, NULL y, no solve yet.
 * cmpc_score_download: len*B*S doubles of the record in force.
 * cmpc_score_download_capture: the t_cap*n_sel*width rows and the number of
 *   steps recorded, min(k, t_cap) (either pointer may be NULL).
 * cmpc_score_disable: frees what enable and capture allocated; later score
 *   calls are refused until the next enable. */
int cmpc_score_len(const cmpc_dims* dims);
int cmpc_score_field(const cmpc_dims* dims, const char* name, int* offset, int* count);
int cmpc_score_check(const cmpc_dims* dims, int n_outputs, const int32_t* out_idx, double Ts, const double* band);
int cmpc_score_capture_check(const cmpc_dims* dims, int n_sel, const int32_t* scenarios, int t_cap);
int cmpc_score_enable(cmpc_ctx* ctx, int n_outputs, const int32_t* out_idx /* S*ny, host */, double Ts,
                      const double* band /* S*ny, host, or NULL: 0 */);
int cmpc_score_bind(cmpc_ctx* ctx, double* scores_device /* len*B*S, or NULL: own buffer */);
int cmpc_score_capture(cmpc_ctx* ctx, int n_sel, const int32_t* scenarios /* host */, int t_cap);
int cmpc_score_bind_capture(cmpc_ctx* ctx, double* rows_device /* t_cap*n_sel*width, or NULL: own buffer */);
int cmpc_score_reset(cmpc_ctx* ctx);
int cmpc_score_step(cmpc_ctx* ctx, const double* y, const double* target, const int32_t* plant_status,
                    const double* u_control, const double* x);
int cmpc_score_download(cmpc_ctx* ctx, double* scores);
int cmpc_score_download_capture(cmpc_ctx* ctx, double* rows, int32_t* n_rows);
int cmpc_score_disable(cmpc_ctx* ctx);

/* Lagrange multipliers and a KKT certificate per QP slot (certify.hip,
 * DESIGN.md §3.16): qpOASES's getDualSolution for the library's own solver,
 * and evidence on the device that a slot's "OK" is an optimum.
 *
 * For QP slot q = b*S + s, n = nV: x the slot's plan (what cmpc_download
 * returns as du); H, f, G of the last build (f corrected where a reference
 * profile is in force); d (nVo) the other controllers' plans in cmpc_predict's
 * order d[mv*nuo + rank*nu + c].  The 2n constraint rows are C = [I; A], A = I
 * with A[i][i-nu] = -1 for i >= nu, with the solver's limits (c = j mod nu):
 *   lo[j]   = lower[c] - u_old[q][c],  hi[j]   = upper[c] - u_old[q][c]   j < n
 *   lo[n+j] = rate_lower[c],           hi[n+j] = rate_upper[c]
 * (the slot's own limits where cmpc_set/bind_scenario_constraints is in
 * force).  The working set W is the slot's working-set word in the state in
 * force (bound state included): bit j, row j is active; bit 16+j, on its upper
 * side.  W is taken as empty where status != CMPC_QP_OK (such slots hold the
 * zero move).  With g = H x + f + G d, cx = C x and t[j] the active side's
 * limit, the record of a slot is
 *
 *   field      rows  value
 *   lam        2n    on W the least-squares solution of C_W' lam_W = g, 0 off
 *                    W; qpOASES's sign: >= 0 on an active lower side, <= 0 on
 *                    an active upper side.  Rows 0..n-1 the bounds, n..2n-1
 *                    the rate rows
 *   r_stat     1     max_i |g - C' lam|_i
 *   r_prim     1     max_j max(lo[j] - cx[j], cx[j] - hi[j], 0), all 2n rows
 *   r_dual     1     the largest wrong-signed |lam[j]| over W; 0 if none
 *   r_comp     1     max over W of |lam[j]| |cx[j] - t[j]|
 *   obj        1     1/2 x'Hx + (f + G d)'x
 *   scale      1     max|H| max(1, max|x|) + max_i |f + G d|_i + 1
 *   n_active   1     rows in W
 *   status     1     the slot's status word
 *   rank_def   1     1 where the normals of W are dependent (the solver's own
 *                    dependency test should exclude it for an OK slot): lam = 0
 *
 * All rows are doubles, in this order, cmpc_certify_len(dims) = 2 nV + 9 rows.
 * Storage is field-major: row r of slot q at r*B*S + q.  cmpc_certify_field
 * gives a field's first row and row count by name (-1 for an unknown name);
 * callers take offsets from it.
 *
 * Two readings.  With d what the slot's last solve saw (nVo = 0; the du_last
 * of cmpc_get_input; after cmpc_iterate(1) the du_old in force before it), an
 * OK slot's residuals certify the solver: all four are rounding-sized against
 * scale.  With d NULL after K iterations, d is gathered from the scenario's
 * other slots' final plans and r_stat is the scenario's Jacobi gap: zero
 * exactly at a fixed point of the iteration.
 *
 * cmpc_certify: asynchronous on the ctx stream; du_other_device NULL gathers
 *   d as cmpc_predict does (needs nu_tot = S * nu); ignored for nVo = 0.
 *   flags must be 0.  It changes nothing the solve wrote.  Refused (-1, the
 *   message names the cause): dimensions without an instance, before a build,
 *   before a solve has written plans for that build (cmpc_iterate with K > 0,
 *   cmpc_step with K > 0, cmpc_get_input), and after any call on the list that
 *   invalidates cmpc_predict (above): lo and hi depend on u_old.
 * cmpc_certify_host: d from host memory (staged as the other _host calls).
 * cmpc_certify_device: the record's device address; NULL before the first
 *   cmpc_certify, which allocates it: a context that never certifies allocates
 *   and launches nothing for it.
 * cmpc_certify_download: len*B*S doubles of the last record.
 * cmpc_certify_summary: a small two-pass reduction on the device over the
 *   slots with status == CMPC_QP_OK: the largest r_stat/scale, r_prim,
 *   r_dual/scale and r_comp/scale, each with its slot (the lowest on ties; 0
 *   and -1 without an OK slot), n_above the OK slots with any of the four
 *   above tol, n_not_ok the other slots.  Maxima and counts are exact in any
 *   order: the result equals the same reduction of the downloaded record bit
 *   for bit.  Synchronises the stream.
 * cmpc_certify_available: host only, 1 where an instance exists (every
 *   (nV, nu, nVo) the iterate kernels are instantiated for), 0 elsewhere.
 * cmpc_certify_len, cmpc_certify_field: host only. */
typedef struct cmpc_certify_summary_t {
  double r_stat, r_prim, r_dual, r_comp;
  int32_t slot_stat, slot_prim, slot_dual, slot_comp;
  int32_t n_above, n_not_ok;
} cmpc_certify_summary_t;
int cmpc_certify_len(const cmpc_dims* dims);
int cmpc_certify_field(const cmpc_dims* dims, const char* name, int* offset, int* count);
int cmpc_certify_available(const cmpc_dims* dims);
int cmpc_certify(cmpc_ctx* ctx, const double* du_other_device, uint32_t flags);
int cmpc_certify_host(cmpc_ctx* ctx, const double* du_other, uint32_t flags);
double* cmpc_certify_device(cmpc_ctx* ctx);
int cmpc_certify_download(cmpc_ctx* ctx, double* record);
int cmpc_certify_summary(cmpc_ctx* ctx, double tol, cmpc_certify_summary_t* out);

/* Ensemble statistics of the score record (score_ensemble.hip, DESIGN.md
 * §3.17): what a Monte Carlo run reads in place of the len*B*S record.
 *
 * cmpc_score_ensemble: for every row f of the record in force (own or bound,
 *   cmpc_score_bind) and every sub-controller s, over the B scenarios' values
 *   x_b = record[f*B*S + b*S + s], six doubles at out[(f*S + s)*6]:
 *     0 mean    sum x_b / B
 *     1 std     sqrt(sum (x_b - mean)^2 / B): the population value about that
 *               mean, from a second pass over the record
 *     2 min     3 max
 *     4 argmax  the scenario of the maximum, the lowest on a tie
 *     5 count   scenarios with x_b > thresholds[f]; 0 with thresholds NULL
 *   thresholds: len host doubles or NULL; out: len*S*6 host doubles.  Three
 *   small launches (partials per block by wave shuffles and LDS, a wave per
 *   row over the partials, no floating-point atomics), one copy, and a stream
 *   synchronisation.  min, max, argmax and count equal the same reduction of
 *   the downloaded record exactly; mean and std are sums in a fixed order for
 *   a given B.  It reads the record and changes nothing but its own work
 *   buffer, allocated by the first call.  Refused before cmpc_score_enable
 *   and for a threshold that is not a number. */
int cmpc_score_ensemble(cmpc_ctx* ctx, const double* thresholds, double* out);

/* Exact ensemble quantiles and per-step envelopes (ensemble_select.h,
 * ensemble_quantiles.hip): the median, P95, P99 of a score
 * row, and per sampling instant the spread of every output and input over the
 * ensemble (a fan chart), without the per-scenario data leaving the device.
 *
 *   order   values are ordered as  -inf < negatives < -0 < +0 < positives <
 *           +inf < NaN  (a double's bits u as the key u | 2^63 with the sign
 *           clear, ~u with it set; every NaN the largest key, returned as the
 *           one quiet NaN 0x7ff8000000000000): np.sort's order
 *   rank    for B values and a level q in [0, 1]: h = q (double)(B - 1) (one
 *           product), k_lo = floor(h), g = h - k_lo (exact), k_hi = k_lo + 1
 *           where g > 0, else k_lo
 *   result  per (row, level) three doubles: x_lo and x_hi, the values at
 *           sorted positions k_lo and k_hi, and arg, the lowest scenario b
 *           whose key is x_lo's (the scenario to replay as "the P95 scenario")
 *   value   cmpc_quantile_value(x_lo, x_hi, g) = x_lo where x_lo == x_hi; else
 *           with d = x_hi - x_lo: x_lo + d g for g < 0.5, x_hi - d (1 - g)
 *           otherwise (products and sums separate).  On finite data this is
 *           numpy's quantile (linear method) bit for bit; between a finite
 *           value and an infinity it is the infinity where numpy gives NaN
 * x_lo, x_hi and arg equal a sort's bit for bit and do not depend on the
 * launch shape: the selection is integer counting (an MSB-first radix
 * selection with 8-bit digits), with no floating-point atomics.
 *
 * Host only (no device is touched); refused (-1, cmpc_last_error names the
 * cause): B < 1, n_levels outside [1, CMPC_QUANTILE_MAX_LEVELS], a level
 * outside [0, 1] or not a number, a NULL pointer.
 * cmpc_quantile_check: the argument check of the others.
 * cmpc_quantile_rank: the rank rule for one level.
 * cmpc_quantile_value: the value rule (no refusals).
 * cmpc_quantiles_host: the same selection on host memory.  x is a (len, B, S)
 *   array, row (f, s) holding x_b = x[f*B*S + b*S + s] (a scenario-major
 *   (B x C) array is len = 1, S = C); out holds len*S*n_levels*3 doubles, row
 *   (f, s), level l at ((f*S + s)*n_levels + l)*3.
 *
 * cmpc_score_quantiles: the same for every row of the score record in force
 *   (own or bound, cmpc_score_bind), len = cmpc_score_len, on the device: 18
 *   launches whatever the arguments (two per digit, two for the last pass),
 *   one copy and one stream synchronisation.  levels: n_levels host doubles; out:
 *   len*S*n_levels*3 host doubles in cmpc_quantiles_host's layout.  It reads
 *   the record and changes nothing but its own work buffer, allocated by the
 *   first call and released with the context.  Refused before
 *   cmpc_score_enable and as cmpc_quantile_check refuses.
 *
 * The envelope: per sampling instant k and channel c (the n_outputs plant
 * outputs, then the nu_tot control inputs), over the B scenarios, W = 6 +
 * 2 n_levels doubles at rows[(k*C + c)*W], C = n_outputs + nu_tot:
 *   0..5  cmpc_score_ensemble's six statistics in its order, the count
 *         against thresholds[c] (0 with thresholds NULL)
 *   6 + 2l, 7 + 2l   x_lo, x_hi of level l
 * cmpc_envelope_check: host only, the argument check of cmpc_envelope_enable.
 *   Refused: n_outputs < 1, t_cap < 1, n_levels outside [0,
 *   CMPC_QUANTILE_MAX_LEVELS] (0: the statistics only), a level outside [0, 1]
 *   or not a number, NULL levels with n_levels > 0, a threshold that is not a
 *   number, more than 65535 channels.
 * cmpc_envelope_len: host only, C*W, the doubles per step row.
 * cmpc_envelope_enable: allocates the rows (t_cap of them, zero) and the work
 *   buffers, uploads the thresholds (n_outputs + nu_tot host doubles or NULL)
 *   and starts at k = 0.  A context that never calls it allocates and launches
 *   nothing for the envelope.
 * cmpc_envelope_step: y_device (B x n_outputs) and u_control_device (B x
 *   nu_tot, or NULL: its channels stay zero) are scenario-major device arrays.
 *   Launches only, on the context's stream (3 for the statistics, 18 more with
 *   n_levels > 0): no copy, no synchronisation; row k of the rows in force is
 *   written directly.  Steps k >= t_cap are dropped, not wrapped.  Refused
 *   before cmpc_envelope_enable and for a NULL y.
 * cmpc_envelope_reset: k = 0 (own rows are zeroed; bound ones are the caller's).
 * cmpc_envelope_bind: keep the rows in a device buffer of t_cap *
 *   cmpc_envelope_len doubles (NULL: the context's own).
 * cmpc_envelope_download: t_cap * cmpc_envelope_len doubles (rows may be NULL)
 *   and the number of rows recorded, min(k, t_cap); synchronises the stream.
 * cmpc_envelope_disable: releases everything the envelope allocated. */
#define CMPC_QUANTILE_MAX_LEVELS 8
int cmpc_quantile_check(int B, int n_levels, const double* levels);
int cmpc_quantile_rank(int B, double level, int32_t* k_lo, int32_t* k_hi, double* g);
double cmpc_quantile_value(double x_lo, double x_hi, double g);
int cmpc_quantiles_host(const double* x, int len, int B, int S, int n_levels, const double* levels, double* out);
int cmpc_score_quantiles(cmpc_ctx* ctx, int n_levels, const double* levels, double* out);
int cmpc_envelope_check(const cmpc_dims* dims, int n_outputs, int t_cap, int n_levels, const double* levels,
                        const double* thresholds);
int cmpc_envelope_len(const cmpc_dims* dims, int n_outputs, int n_levels);
int cmpc_envelope_enable(cmpc_ctx* ctx, int n_outputs, int t_cap, int n_levels, const double* levels,
                         const double* thresholds);
int cmpc_envelope_step(cmpc_ctx* ctx, const double* y_device, const double* u_control_device);
int cmpc_envelope_reset(cmpc_ctx* ctx);
int cmpc_envelope_bind(cmpc_ctx* ctx, double* rows_device);
int cmpc_envelope_download(cmpc_ctx* ctx, double* rows, int32_t* n_rows);
int cmpc_envelope_disable(cmpc_ctx* ctx);

/* Seeded per-scenario noise and disturbances (noise_body.h, noise.hip,
 * DESIGN.md §3.17): normal draws that are a pure function of (seed, stream,
 * global scenario, step, channel), so a run is reproducible from its seed and
 * the same however the scenarios are cut into batches or shards: batch b of a
 * shard that starts at global scenario scenario0 draws what scenario
 * scenario0 + b of the whole ensemble draws.  There is no generator state.
 *
 *   bits      Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants
 *             0x9E3779B9, 0xBB67AE85), key (seed low 32, seed high 32), counter
 *             (scenario0 + b, step, pair j = c / 2, stream)
 *   uniforms  k1 = (x0 >> 5) 2^26 + (x1 >> 6), k2 likewise from x2 and x3;
 *             u1 = (k1 + 1) 2^-53 in (0, 1], u2 = k2 2^-53 in [0, 1)
 *   normals   r = sqrt(-2 log u1); channel 2j draws z = r cospi(2 u2), channel
 *             2j + 1 z = r sinpi(2 u2); with n odd the last sine is dropped
 *   element   e = b*n + c, s = sigma ? sigma[e] : 1
 *             rho given:  g = sqrt(1 - rho[e] rho[e]) s
 *                         w[e] = rho[e] w[e] + g z;  d = w[e]
 *                         (an AR(1) of stationary standard deviation s; the
 *                         state w is the caller's and starts where the caller
 *                         puts it)
 *             rho NULL:   d = s z
 *             out[e] = d == 0 ? base[e] : base[e] + d   (a NULL base counts as
 *             0): a zero sigma reproduces base bit for bit
 * Products and sums are separate operations in that order, so given z a
 * float64 host model reproduces w and out bit for bit.
 *
 * Streams: CMPC_NOISE_STREAM_MEASUREMENT (0) and CMPC_NOISE_STREAM_INPUT (1)
 * are the closed loop's (cmpc.driver.ClosedLoop.set_noise); the others are the
 * caller's.  All arrays are B*n doubles, row b the scenario's n channels; u is
 * B*ceil(n/2)*2 doubles, [u1, u2] of pair j of scenario b at (b*ceil(n/2) + j)*2.
 *
 * cmpc_noise_check: host only, the argument check of every entry point.
 *   Refused (-1, cmpc_last_error names the cause): NULL key, B < 1, n < 1,
 *   step >= 2^32, scenario0 + B > 2^32 (each is one word of the counter).
 * cmpc_noise_check_params: host only, over host arrays (either may be NULL):
 *   sigma finite and >= 0, rho inside [-1, 1].  The step entry points do not
 *   read the values to check them: that is the caller's, with this function.
 * cmpc_noise_uniforms_host, cmpc_noise_step_host: the same arithmetic on host
 *   arrays; no device is touched.
 * cmpc_noise_uniforms, cmpc_noise_step: one launch on `stream` of `device`,
 *   asynchronous; every pointer is checked as cmpc_bind_state checks its own
 *   (a device allocation of the array's size on that device, 8-byte aligned).
 *   Also refused: NULL out (or u), rho without w.  sigma, rho, base may be
 *   NULL; w is read only with rho.  out may be base (in place). */
#define CMPC_NOISE_STREAM_MEASUREMENT 0u
#define CMPC_NOISE_STREAM_INPUT 1u
typedef struct cmpc_noise_key {
  uint64_t seed;
  uint32_t stream;
  uint32_t scenario0;
} cmpc_noise_key;
int cmpc_noise_check(const cmpc_noise_key* key, uint64_t step, int B, int n);
int cmpc_noise_check_params(int B, int n, const double* sigma, const double* rho);
int cmpc_noise_uniforms_host(const cmpc_noise_key* key, uint64_t step, int B, int n, double* u);
int cmpc_noise_step_host(const cmpc_noise_key* key, uint64_t step, int B, int n, const double* sigma,
                         const double* rho, double* w, const double* base, double* out);
int cmpc_noise_uniforms(int device, void* stream, const cmpc_noise_key* key, uint64_t step, int B, int n,
                        double* u_dev);
int cmpc_noise_step(int device, void* stream, const cmpc_noise_key* key, uint64_t step, int B, int n,
                    const double* sigma_dev, const double* rho_dev, double* w_dev, const double* base_dev,
                    double* out_dev);

/* Per-kernel device time (HIP events stamped by the kernel's own dispatch,
 * opt-in).  enable: 0 off, 1 every kernel, or an OR of CMPC_TIME_ONLY(k)
 * to time only those kernels (the others launch without events). */
#define CMPC_KERNEL_BUILD 0
#define CMPC_KERNEL_ITERATE 1         /* cmpc_iterate, cmpc_coupled_iterate */
#define CMPC_KERNEL_PRODUCE 2         /* cmpc_produce_lin; cmpc_observe_step (a posteriori + per-QP producer, one kernel) */
#define CMPC_KERNEL_OBSERVE_POST 3    /* no launches since the a posteriori update runs in the producer (kept for the numbering) */
#define CMPC_KERNEL_OBSERVE_PRIOR 4   /* cmpc_observe_apply */
#define CMPC_KERNEL_STEP 5            /* cmpc_step as one fused build + K-iteration launch */
#define CMPC_KERNEL_COUNT 6
#define CMPC_TIME_ONLY(kernel) (2 << (kernel))
int cmpc_enable_timing(cmpc_ctx* ctx, int enable);
int cmpc_kernel_time(cmpc_ctx* ctx, int kernel, double* total_ms,
                     int64_t* launches);
/* Time only every stride-th launch of each timed kernel (1, the default:
 * every launch).  An event-stamped launch costs the stream a few us after
 * the kernel; sampling keeps the mean launch time while the untimed launches
 * run as in production.  Counted from the last cmpc_enable_timing. */
int cmpc_set_timing_stride(cmpc_ctx* ctx, int stride);

/* The batched QP solver alone, on device `device`, for host arrays of nqp
 * QPs of size n (nu inputs per move): H nqp*n*n, g/lb/ub/lbA/ubA nqp*n,
 * ws_in nqp; outputs x nqp*n, status/nchg nqp, ws_out nqp, trace nqp*16,
 * ntrace nqp.  (Parity and known-answer tests of the solver.) */
int cmpc_qp_solve_batch(int device, int n, int nu, int nqp, const double* H,
                        const double* g, const double* lb, const double* ub,
                        const double* lbA, const double* ubA,
                        const uint32_t* ws_in, int max_chg, double* x,
                        int32_t* status, int32_t* nchg, uint32_t* ws_out,
                        uint8_t* trace, int32_t* ntrace);
/* The same for one Jacobi-iteration solve (the map form of DESIGN.md §4):
 * g = f + G d with G nqp*n*nvo (row-major per QP, columns in the order of the
 * other sub-controllers' plans d, nqp*nvo: controller-major within each move,
 * include/nerve_center.h:283-285).  Replaces ApplyOtherInput + SolveQP of
 * DistributedSolver::UpdateAndSolveQP (include/distributed_solver.h:69-80,
 * 98-103; libs/mpc_qp_solver.cc:42-75); bit-identical to the solves inside
 * cmpc_iterate / cmpc_get_input.  nvo = 0: cmpc_qp_solve_batch. */
int cmpc_qp_solve_batch_map(int device, int n, int nu, int nvo, int nqp,
                            const double* H, const double* f, const double* G,
                            const double* d, const double* lb, const double* ub,
                            const double* lbA, const double* ubA,
                            const uint32_t* ws_in, int max_chg, double* x,
                            int32_t* status, int32_t* nchg, uint32_t* ws_out,
                            uint8_t* trace, int32_t* ntrace);

/* Upstream producer (host, untimed): AugmentedLinearizedSystem::Update for the
 * reference plants — linearise the plant at (x, u_full), discretise
 * (Taylor-4, libs/aug_lin_sys.cc:232-255), reorder the inputs by input_order
 * (ControlInputIndices) and fill off_A..off_f of one lin record for the
 * controlled outputs out_idx[0..ny-1].  plant: 0 parallel, 1 serial. */
#define CMPC_PLANT_PARALLEL 0
#define CMPC_PLANT_SERIAL 1
int cmpc_plant_dims(int plant, int* ns, int* n_inputs, int* n_outputs,
                    int* n_control_inputs);
int cmpc_plant_default(int plant, double* x, double* u_full);
int cmpc_plant_output(int plant, const double* x, double* y);
int cmpc_plant_lin_record(int plant, double p_in, double p_out, double Ts,
                          const double* x, const double* u_full,
                          const int32_t* input_order, const int32_t* out_idx,
                          const cmpc_dims* dims, double* record);

/* One stand-alone sub-controller per QP slot (the reference's per-object
 * DistributedController API; the NerveCenter path is cmpc_iterate /
 * cmpc_observe_apply):
 *   cmpc_get_input  DistributedController::GetInput(&du, du_last)
 *                   (include/distributed_controller.h:206-226): f_k = f + G du_last
 *                   (ApplyOtherInput, distributed_solver.h:98-103) and one
 *                   warm-started SolveQP; du_last: device, B*S*nVo doubles per
 *                   slot, the other controllers' plans controller-major, then
 *                   move, then input (nerve_center.h:283-285); NULL for a full
 *                   (centralized, nVo = 0) controller: SolveQP(qp_, u_old_).
 *                   Results through cmpc_download (du, status, nwsr); flags as
 *                   cmpc_iterate (CMPC_APPLY_MOVE: u_old += first move)
 *   cmpc_update_u   DistributedController::UpdateU(du) (:145-152): ObserveAPriori
 *                   (du, u_old_) and u_old_ += du with the caller's full input
 *                   change du (device, B*S*nu_tot, the slot's input order);
 *                   NerveCenter passes only the own inputs, the others zero
 *                   (nerve_center.h:323-328; cmpc_observe_apply does that)
 * The _host variants take host arrays (staged on the context's stream). */
int cmpc_get_input(cmpc_ctx* ctx, const double* du_last, uint32_t flags);
int cmpc_get_input_host(cmpc_ctx* ctx, const double* du_last, uint32_t flags);
int cmpc_update_u(cmpc_ctx* ctx, const double* du_full);
int cmpc_update_u_host(cmpc_ctx* ctx, const double* du_full);

/* Sub-controller-sharded cooperative iteration.
 * S_total sub-controllers per scenario are spread over the ranks, S_local of
 * them on this context (QP slot q = scenario * S_local + local index; global
 * index s_offset + local index); the context's H, f come from cmpc_build.
 * One Jacobi iteration (nerve_center.h:146-172 with ApplyOtherInput
 * distributed_solver.h:98-103):
 *   f_k = f + G_ext du_other,   du = SolveQP(H, f_k) warm-started
 * G_ext: device, [nV * (S_total-1) * nV][B*S_local] (element-major),
 *        column block j = the j-th other sub-controller in global order.
 * du_all: device, all-gathered plans [world][B][S_local][nV] (rank-major),
 *        world = S_total / S_local: the kernel reads all of it.
 * G_ext_len, du_all_len: the element counts (doubles) of the caller's two
 *        buffers.  The call is refused (-1, cmpc_last_error) unless
 *        G_ext_len >= nV*(S_total-1)*nV * B*S_local and
 *        du_all_len >= S_total * B * nV, i.e. unless every read of the
 *        kernel falls inside them (a rank layout that does not cover
 *        S_total would otherwise read past the gathered plans).
 * du_out: device [B*S_local][nV] or NULL: this rank's new plans (the next
 *        all-gather's input).  CMPC_APPLY_MOVE on the last iteration of a
 *        step applies the first move (UpdateUOld) and stores du_old.
 * The caller all-gathers between calls (RCCL; cmpc/coupled.py). */
/* The checks cmpc_coupled_iterate makes before any launch, for a context of
 * these dims (B scenarios x S = B*S local QPs): 0, or -1 with
 * cmpc_last_error().  Host only, no device needed. */
int cmpc_coupled_validate(const cmpc_dims* dims, int S_total, int S_local, int s_offset,
                          size_t G_ext_len, size_t du_all_len);
int cmpc_coupled_iterate(cmpc_ctx* ctx, int S_total, int S_local, int s_offset,
                         const double* G_ext, size_t G_ext_len, const double* du_all,
                         size_t du_all_len, double* du_out, uint32_t flags);

/* Observer and receding-horizon update on the device (SURVEY.md §8(f)
 * row 2).  Each QP slot keeps the state of its sub-controller's
 * DistributedController (observer.h:53-56, distributed_controller.h:104-111)
 * in HBM, a row of cmpc_observer_len() doubles:
 *   [x_hat ns][dx_aug ntot][y_old n_outputs][C n_outputs x ns][padding]
 * (rows padded to a multiple of 16 doubles, one 128-byte line;
 * ntot = ns + ndist + delay states, the full AugmentedState; C = the plant
 * output matrix of the last linearisation).  A closed-loop control step is
 *   cmpc_observe_step(u_full, y)   ObserveAPosteriori + x_ += (observer.cc:27-44,
 *                                  distributed_controller.cc:80), then
 *                                  Update(x_, u_full) per QP slot: the lin
 *                                  records (GenerateInitialQP, :75-110)
 *   cmpc_build, cmpc_iterate(K, 0) the QP and the Jacobi iterations (no
 *                                  CMPC_APPLY_MOVE: the update below applies it)
 *   cmpc_observe_apply()           UpdateU (distributed_controller.h:145-152):
 *                                  ObserveAPriori (observer.cc:8-22) with the own
 *                                  first move (other inputs zero,
 *                                  nerve_center.h:323-328), then u_old += du
 * All device pointers; asynchronous on the context's stream.
 * Not graph-capturable: the delay blocks' ring phase (a-priori steps since
 * cmpc_observer_init) is host state that reaches the kernels as a launch
 * argument and advances per cmpc_observe_apply call, so a replayed capture
 * would reuse the phase it was captured with.  The same holds for
 * cmpc_sim_set_input (the TimeDelay cursors).  cmpc_build, cmpc_iterate and
 * cmpc_step carry no such host state. */
/* ObserverMatrix M of sub-controller s ((ns + ndist) x n_outputs, row-major;
 * the DistributedController constructor argument, distributed_controller.cc:14).
 * n_outputs (the plant's outputs, ObserverOutputIndices) must agree for all s. */
int cmpc_set_observer(cmpc_ctx* ctx, int s, int n_outputs, const double* M);
int cmpc_observer_len(const cmpc_ctx* ctx);
/* DistributedController::Initialize (distributed_controller.cc:30-43):
 * x_hat = x_init[b] (B x ns), y_old = y_init[b] (B x n_outputs), dx_aug =
 * dx_init (B*S x ntot, or NULL for zero), then the records at x_init (as
 * cmpc_produce_lin, input_order / out_idx as there).  Follow with cmpc_build
 * and cmpc_init_warmstart (InitializeQPProblem).  p_in, p_out are kept for the
 * later cmpc_observe_step / cmpc_control_step calls; both are ignored while
 * per-scenario pressures are in force (cmpc_set/bind_scenario_pressures). */
int cmpc_observer_init(cmpc_ctx* ctx, int plant, double p_in, double p_out, double Ts,
                       const int32_t* input_order, const int32_t* out_idx,
                       const double* x_init, const double* u_full, const double* y_init,
                       const double* dx_init);
/* u_full: B x n_inputs plant input at the linearisation (NerveCenter
 * u_old_ + u_offset, nerve_center.h:139); y: B x n_outputs measured outputs. */
int cmpc_observe_step(cmpc_ctx* ctx, const double* u_full, const double* y);
int cmpc_observe_apply(cmpc_ctx* ctx);
/* The same two calls with HOST arrays (staged to the device on the
 * context's stream), for host-side harnesses such as the C++ adapter. */
int cmpc_observer_init_host(cmpc_ctx* ctx, int plant, double p_in, double p_out, double Ts,
                            const int32_t* input_order, const int32_t* out_idx,
                            const double* x_init, const double* u_full, const double* y_init,
                            const double* dx_init);
int cmpc_observe_step_host(cmpc_ctx* ctx, const double* u_full, const double* y);
/* NerveCenter::GetNextInput (include/nerve_center.h:134-182) on the device:
 * cmpc_observe_step(u_full, y) + cmpc_step(K, 0) + cmpc_observe_apply() with
 * the same results bit for bit.  ONE kernel launch (observer a posteriori +
 * linearisation, the QP build, K Jacobi iterations and the a-priori update,
 * one workgroup per four QP slots) when K > 0, the step variant is not
 * CMPC_STEP_SPLIT, the build and solve variants are AUTO, nqp <= 4 cus and
 * the dimensions have a control-step instance; up to nqp <= cus its build
 * runs as role-split pairs, two QP slots per workgroup.  Elsewhere the three
 * calls (cmpc_dispatch_plan, dispatch.cpp; cmpc_plan's control_* fields).
 * Plans, statuses and nWSR through cmpc_download; u_old has moved by the own
 * first moves. */
int cmpc_control_step(cmpc_ctx* ctx, const double* u_full, const double* y, int K);
int cmpc_control_step_host(cmpc_ctx* ctx, const double* u_full, const double* y, int K);
/* cmpc_control_step_host + cmpc_download (host arrays in and out; any output
 * pointer may be NULL), the C++ NerveCenter::GetNextInput path: a one-
 * workgroup launch (up to four QP slots) marks its completion in page-locked
 * host memory, which the call polls instead of synchronising the stream. */
int cmpc_control_step_download(cmpc_ctx* ctx, const double* u_full, const double* y, int K,
                               double* du, int32_t* status, int32_t* nwsr);
/* Host copies of the observer state rows (B*S x cmpc_observer_len()). */
int cmpc_get_observer_state(cmpc_ctx* ctx, double* host);
int cmpc_set_observer_state(cmpc_ctx* ctx, const double* host);

/* Batched plant simulation: the harness's
 * SimulationSystem for B scenarios on the GPU, one lane per scenario.
 *   cmpc_sim_reset      SimulationSystem(p_sys, u_offset, x_in) + TimeDelay()
 *                       (simulation_system.h:50-56, time_delay.h:26-38):
 *                       x0 (B x ns), u_offset (B x n_inputs), device; dt0 =
 *                       the integrate_const step (the sampling time)
 *   cmpc_sim_set_input  SetInput(u) (simulation_system.h:67-70): u_control
 *                       (B x n_control, device) through the input delay line
 *                       (time_delay.h:41-58) onto u_offset (GetPlantInput)
 *   cmpc_sim_integrate  one observation interval [t, t_end] of Integrate
 *                       (simulation_system.h:108-116): controlled
 *                       Dormand-Prince with Boost odeint's semantics and the
 *                       reference's 2-norm error (:121-133); the step size
 *                       carries over between intervals as in integrate_const
 *   cmpc_sim_set_offset SetOffset(u_offset) (simulation_system.h:64): the
 *                       plant-input offset (B x n_inputs, device) that the next
 *                       cmpc_sim_set_input adds the control inputs to; the
 *                       current plant input is unchanged until then (the
 *                       setup files' `simulation` segments, a step of an
 *                       unmeasured input such as the discharge valve)
 *   cmpc_sim_restart    a new Integrate call (simulation_system.h:108-116):
 *                       integrate_const's controlled stepper starts again from
 *                       the step size dt0 (the harness integrates each setup
 *                       segment with its own call)
 *   cmpc_sim_output     GetOutput() (B x n_outputs, device)
 *   cmpc_sim_plant_input GetPlantInput(u_control) without the delay line (the
 *                       controller's linearisation input, nerve_center.h:139)
 *   cmpc_sim_plant_input_offset  the same over a given offset (B x n_inputs,
 *                       device): the controller's own u_offset_, which keeps
 *                       its Initialize value when the plant's steps
 * Device arrays: cmpc_sim_state (x), cmpc_sim_input (plant input u_),
 * cmpc_sim_step_size (dt), cmpc_sim_status (1 = step-size control failed:
 * 500 rejected tries of one step; 2 = more than 500 steps in one interval,
 * odeint's max_step_checker; 3 = non-finite error norm or state). A status
 * is sticky: the scenario's state stays where it stopped and later
 * cmpc_sim_integrate calls skip it (the reference's odeint throws and ends
 * the run) until cmpc_sim_reset clears it, so one read after a run counts
 * every scenario that failed in any interval. */
typedef struct cmpc_sim cmpc_sim;
int cmpc_sim_create(cmpc_sim** sim, int plant, int B, int device, double p_in, double p_out,
                    int n_control, const int32_t* delays /* n_control, control order */,
                    const int32_t* control_index /* ControlInputIndex: plant input of each */);
int cmpc_sim_destroy(cmpc_sim* sim);
int cmpc_sim_set_stream(cmpc_sim* sim, void* hip_stream);
int cmpc_sim_reset(cmpc_sim* sim, const double* x0, const double* u_offset, double dt0);
int cmpc_sim_set_input(cmpc_sim* sim, const double* u_control);
int cmpc_sim_set_offset(cmpc_sim* sim, const double* u_offset);
int cmpc_sim_restart(cmpc_sim* sim, double dt0);
int cmpc_sim_plant_input(cmpc_sim* sim, const double* u_control, double* u_full_out);
int cmpc_sim_plant_input_offset(cmpc_sim* sim, const double* u_control, const double* u_offset,
                                double* u_full_out);
int cmpc_sim_integrate(cmpc_sim* sim, double t, double t_end, double eps_abs, double eps_rel);
int cmpc_sim_output(cmpc_sim* sim, double* y);
int cmpc_sim_synchronize(cmpc_sim* sim);
/* Host-array variants of reset / set_input / set_offset / output (staged
 * through the simulator's own device buffer; each returns once done). */
int cmpc_sim_reset_host(cmpc_sim* sim, const double* x0, const double* u_offset, double dt0);
int cmpc_sim_set_input_host(cmpc_sim* sim, const double* u_control);
int cmpc_sim_set_offset_host(cmpc_sim* sim, const double* u_offset);
int cmpc_sim_output_host(cmpc_sim* sim, double* y);
/* Host copies (any pointer may be NULL): x B x ns, plant input B x n_inputs,
 * step size B, status B. */
int cmpc_sim_download(cmpc_sim* sim, double* x, double* u_full, double* dt, int32_t* status);
double* cmpc_sim_state(cmpc_sim* sim);
double* cmpc_sim_input(cmpc_sim* sim);
double* cmpc_sim_step_size(cmpc_sim* sim);
int32_t* cmpc_sim_status(cmpc_sim* sim);
/* Per-scenario boundary pressures of the plant: B x 2
 * doubles, [p_in, p_out] of scenario b, in place of the two scalars given to
 * cmpc_sim_create.  Each cmpc_sim_integrate reads the array in force at its
 * launch (one 16-byte load per scenario, in the kernel's per-scenario
 * instance), so the pressures may change between intervals; a scenario whose
 * pair equals the scalars integrates bit for bit as it does without.
 *   cmpc_sim_set_pressures       a device array, copied on the simulator's
 *                                stream into its own buffer (allocated on
 *                                first use); not checked
 *   cmpc_sim_set_pressures_host  a host array, every value checked finite and
 *                                > 0 (the message names the first bad
 *                                scenario), then copied
 *   cmpc_sim_bind_pressures      a device array read in place (16-byte
 *                                aligned, on the simulator's device); the
 *                                caller may rewrite it between intervals; not
 *                                checked
 *   cmpc_sim_get_pressures       a host copy of what is in force (the scalars,
 *                                repeated, when no array is)
 * NULL restores the scalars of cmpc_sim_create in all three. */
int cmpc_sim_set_pressures(cmpc_sim* sim, const double* pressures_device /* B*2 */);
int cmpc_sim_set_pressures_host(cmpc_sim* sim, const double* pressures /* B*2, host */);
int cmpc_sim_bind_pressures(cmpc_sim* sim, const double* pressures_device /* B*2 */);
int cmpc_sim_get_pressures(cmpc_sim* sim, double* pressures /* B*2, host */);
/* Plant equilibrium: for each scenario the state x with
 * f(x, u, p) = 0 at its plant input and boundary pressures, by Newton's method
 * from the x given.  Each iteration linearises the plant (A and f as
 * cmpc_plant_lin_record does before it discretises), takes r = max|f_i| and
 * solves A d = -f by Gaussian elimination with partial pivoting; host and
 * device run the same arithmetic (csrc/equilibrium_body.h) and agree bit for
 * bit.  Per scenario: a status, the iteration that returned and the last r.
 *   CMPC_EQ_OK              r <= tol; x is the equilibrium
 *   CMPC_EQ_NO_CONVERGENCE  r > tol after max_iter Newton steps
 *   CMPC_EQ_NONFINITE       f or A had a non-finite entry (no forward-flow
 *                           equilibrium at these pressures, as a rule)
 *   CMPC_EQ_SINGULAR        a zero or non-finite pivot
 *   CMPC_EQ_SKIPPED         the simulator's status of the scenario was nonzero
 *                           (a failed integration): not touched
 * Every status but CMPC_EQ_OK leaves the scenario's x as it was on entry, and
 * none of them is an error of the call.  max_iter in [0, 64] (0: only test the
 * x given), tol finite and > 0; 20 and 1e-12 are the defaults of the Python
 * layer (plain Newton from cmpc_plant_default needs at most 5 steps to 1e-12
 * for pressures within 5 % of 1 and input offsets within 0.02).
 *   cmpc_plant_derivative        dx = f(x, u_full) of one state (host); -1: a
 *                                null pointer or an unknown plant
 *   cmpc_plant_equilibrium_host  B scenarios on the host, no device: pressures
 *                                B x 2, u_full B x n_inputs, x B x ns in and out
 *   cmpc_sim_equilibrium         the simulator's scenarios on its stream, one
 *                                launch: from its current x, at its current
 *                                plant input and the pressures in force (the
 *                                scalars, or the array set or bound); x is
 *                                written in place; the step sizes and the
 *                                delay lines stay as they are
 *   cmpc_sim_equilibrium_download  host copies of the last solve's results
 *                                (any pointer may be NULL); synchronises
 *   cmpc_sim_equilibrium_status, _iters, _resid  the device arrays (B each;
 *                                NULL before the first cmpc_sim_equilibrium) */
#define CMPC_EQ_OK 0
#define CMPC_EQ_NO_CONVERGENCE 1
#define CMPC_EQ_NONFINITE 2
#define CMPC_EQ_SINGULAR 3
#define CMPC_EQ_SKIPPED 4
#define CMPC_EQ_MAX_ITER 64
int cmpc_plant_derivative(int plant, double p_in, double p_out, const double* x, const double* u_full,
                          double* dx);
int cmpc_plant_equilibrium_host(int plant, int B, const double* pressures /* B*2 */,
                                const double* u_full /* B*n_inputs */, double* x /* B*ns, in/out */,
                                int max_iter, double tol, int32_t* status, int32_t* iters, double* resid);
int cmpc_sim_equilibrium(cmpc_sim* sim, int max_iter, double tol);
int cmpc_sim_equilibrium_download(cmpc_sim* sim, int32_t* status, int32_t* iters, double* resid);
int32_t* cmpc_sim_equilibrium_status(cmpc_sim* sim);
int32_t* cmpc_sim_equilibrium_iters(cmpc_sim* sim);
double* cmpc_sim_equilibrium_resid(cmpc_sim* sim);
/* Steady-state targets: for each scenario the state x and
 * nh <= 4 free control inputs with f(x, u, p) = 0 and y_h(x) = t_h for nh held
 * plant outputs, by Newton's method from the x and u given; the inputs that
 * are not free stay.  hold_idx[nh]: distinct plant outputs in [0, 4).
 * free_idx[nh]: distinct control inputs in [0, 4), the columns of the
 * continuous B in plant order (plant inputs 0, 3, 4, 7 of both plants: 0 and 2
 * are the torques, 1 and 3 the recycle valves).  targets: B x nh, in plant-
 * output units.  Each iteration linearises the plant (A, B, C and f as
 * cmpc_plant_lin_record does before it discretises), takes r_f = max|f_i| and
 * r_y = max|y_h - t_h| and solves
 *   [[A, B_free], [C_hold, 0]] d = [-f; t - y]
 * by the equilibrium solve's elimination on ns + 4 rows, an unused border row
 * and column being the unit ones; host and device run the same arithmetic
 * (csrc/target_body.h) and agree bit for bit, and nh = 0 is the equilibrium
 * solve bit for bit.  The torque columns of B and C are exact derivatives, and
 * so is a recycle column from u_rec >= 2e-2; below that the plant's recycle
 * flow jumps (at 1e-2) and the column is an approximation, so a scenario with
 * a free recycle valve below 2e-2, on entry or after a Newton step, stops:
 *   CMPC_EQ_DEADZONE        a free recycle valve below 2e-2: not iterated
 * The other statuses are the equilibrium solve's (OK: r_f <= tol_f and r_y <=
 * tol_y; NONFINITE: an entry of the bordered system; SKIPPED: the simulator's
 * status was nonzero).  Every status but CMPC_EQ_OK leaves x, the plant input
 * and the offset as they were; iters is the iteration that returned, resid
 * the pair (r_f, r_y) of its last test (B x 2).  max_iter in [0, 64], both
 * tolerances finite and > 0; 20, 1e-12 and 1e-10 are the Python layer's.
 *   cmpc_target_check       -1 with a message for an unknown plant, nh outside
 *                           [0, 4], a repeated or out-of-range index, max_iter
 *                           outside [0, 64] or a bad tolerance (host only)
 *   cmpc_plant_target_host  B scenarios on the host, no device: u_full
 *                           B x n_inputs and x B x ns in and out
 *   cmpc_sim_target         the simulator's scenarios on its stream, one
 *                           launch, from its current x and plant input at the
 *                           pressures in force; targets a device array.  Where
 *                           the status is CMPC_EQ_OK it writes x, the free
 *                           entries v of the plant input, and the same entries
 *                           of the input offset as v - (u_full - u_offset) of
 *                           before: exactly v when no control input is in the
 *                           delay line.  The step sizes and the delay lines
 *                           stay as they are
 *   cmpc_sim_target_host    the same with targets on the host; synchronises
 *   cmpc_sim_target_download  host copies of the last solve's results (any
 *                           pointer may be NULL; resid B x 2); synchronises
 *   cmpc_sim_target_status, _iters, _resid  the device arrays (NULL before the
 *                           first cmpc_sim_target); buffers of their own:
 *                           cmpc_sim_equilibrium_download keeps its meaning
 *   cmpc_sim_download_inputs  host copies of the simulator's input offset
 *                           (B x n_inputs) and of its delay line
 *                           (cmpc_sim_delay_len slots of B doubles); either
 *                           pointer may be NULL; synchronises */
#define CMPC_EQ_DEADZONE 5
int cmpc_target_check(int plant, int nh, const int32_t* hold_idx, const int32_t* free_idx, int max_iter,
                      double tol_f, double tol_y);
int cmpc_plant_target_host(int plant, int B, const double* pressures /* B*2 */, int nh, const int32_t* hold_idx,
                           const int32_t* free_idx, const double* targets /* B*nh */,
                           double* u_full /* B*n_inputs, in/out */, double* x /* B*ns, in/out */, int max_iter,
                           double tol_f, double tol_y, int32_t* status, int32_t* iters, double* resid /* B*2 */);
int cmpc_sim_target(cmpc_sim* sim, int nh, const int32_t* hold_idx, const int32_t* free_idx,
                    const double* targets_device /* B*nh */, int max_iter, double tol_f, double tol_y);
int cmpc_sim_target_host(cmpc_sim* sim, int nh, const int32_t* hold_idx, const int32_t* free_idx,
                         const double* targets /* B*nh, host */, int max_iter, double tol_f, double tol_y);
int cmpc_sim_target_download(cmpc_sim* sim, int32_t* status, int32_t* iters, double* resid /* B*2 */);
int32_t* cmpc_sim_target_status(cmpc_sim* sim);
int32_t* cmpc_sim_target_iters(cmpc_sim* sim);
double* cmpc_sim_target_resid(cmpc_sim* sim);
int cmpc_sim_delay_len(cmpc_sim* sim);
int cmpc_sim_download_inputs(cmpc_sim* sim, double* u_offset /* B*n_inputs */, double* delay_line);
/* Steady-state gains, relative gain array and pressure feed-forward (DESIGN.md
 * §3.22): for each scenario the steady-state map of its linearisation at
 * (x, u, p), from nu <= 4 control inputs and from the two boundary pressures
 * to ny <= 4 plant outputs.  out_idx[ny]: distinct plant outputs in [0, 4),
 * ny >= 1.  in_idx[nu]: distinct control inputs in [0, 4), nu >= 1, the
 * columns of the continuous B as cmpc_sim_target's free_idx (0 and 2 are the
 * torques, 1 and 3 the recycle valves).  With A, B, C, f of the continuous
 * linearisation and E = df/dp (ns x 2) by a central difference of the plant's
 * derivative in p_in and in p_out, step 2^-21:
 *   G   = -C_sel A^-1 B_sel   ny x nu   d y / d u at rest
 *   Gp  = -C_sel A^-1 E       ny x 2    d y / d (p_in, p_out) at rest
 * through one adjoint solve A^T Z = C_sel^T by the equilibrium solve's
 * elimination on ns rows and ns + 4 columns, and for ny == nu = n
 *   RGA  = G .* (G^-1)^T      n x n     the relative gain array
 *   K_ff = -G^-1 Gp           n x 2     d u / d p that holds the outputs
 * by the same elimination on 4 rows, rows and columns from n on being the unit
 * ones.  Host and device run the same arithmetic (csrc/gains_body.h) and agree
 * bit for bit.  r_f = max|f_i| is reported and not tested: any state gives
 * the gains of its linearisation, and they are steady-state gains where
 * r_f ~ 0 (after cmpc_sim_equilibrium or cmpc_sim_target).
 * The record, CMPC_GAIN_LEN = 49 doubles per scenario: G 4 x 4 row-major in
 * the order of out_idx x in_idx, Gp 4 x 2, RGA 4 x 4, K_ff 4 x 2, r_f.  An
 * entry outside ny / nu is the quiet NaN 0x7ff8000000000000.  Statuses:
 *   CMPC_EQ_OK              with ny != nu, RGA and K_ff are that NaN
 *   CMPC_GAIN_SINGULAR_G    ny == nu and a zero or non-finite pivot of G: G,
 *                           Gp and r_f stand, RGA and K_ff are that NaN
 *   CMPC_EQ_DEADZONE        a selected recycle valve below 2e-2, where its B
 *                           column is an approximation (an unselected valve
 *                           may stand anywhere)
 *   CMPC_EQ_NONFINITE       an entry of A, of the selected part of B or C, of
 *                           f or of E is not finite
 *   CMPC_EQ_SINGULAR        a zero or non-finite pivot of A
 *   CMPC_EQ_SKIPPED         the simulator's status was nonzero
 * and for the last four all 49 entries are that NaN.  No status is an error
 * of the call.
 *   cmpc_gain_check         -1 with a message for an unknown plant, ny or nu
 *                           outside [1, 4], a null index array, or a repeated
 *                           or out-of-range index (host only)
 *   cmpc_plant_gains_host   B scenarios on the host, no device: record
 *                           B x 49, status B
 *   cmpc_sim_gains          the simulator's scenarios on its stream, one
 *                           launch, at its current x and plant input and the
 *                           pressures in force (scalar, set or bound).  Nothing
 *                           of the simulator is written: x, inputs, offset,
 *                           step sizes and delay lines stay bit for bit
 *   cmpc_sim_gains_download host copies of the last call's results (either
 *                           pointer may be NULL); synchronises
 *   cmpc_sim_gains_record, _status  the device arrays (NULL before the first
 *                           cmpc_sim_gains); buffers of their own */
#define CMPC_GAIN_SINGULAR_G 6
#define CMPC_GAIN_LEN 49
int cmpc_gain_check(int plant, int ny, const int32_t* out_idx, int nu, const int32_t* in_idx);
int cmpc_plant_gains_host(int plant, int B, const double* pressures /* B*2 */, const double* u_full /* B*n_inputs */,
                          const double* x /* B*ns */, int ny, const int32_t* out_idx, int nu, const int32_t* in_idx,
                          double* record /* B*49 */, int32_t* status /* B */);
int cmpc_sim_gains(cmpc_sim* sim, int ny, const int32_t* out_idx, int nu, const int32_t* in_idx);
int cmpc_sim_gains_download(cmpc_sim* sim, double* record /* B*49 */, int32_t* status /* B */);
double* cmpc_sim_gains_record(cmpc_sim* sim);
int32_t* cmpc_sim_gains_status(cmpc_sim* sim);
/* Plant frequency responses: for each scenario the map of its
 * linearisation at (x, u, p) away from rest, from nu <= 4 control inputs and
 * from the two boundary pressures to ny <= 4 plant outputs, at nw frequencies
 * shared by all scenarios.  out_idx, in_idx, A, B, C, f and E = df/dp as for
 * the gains above; omega[nw]: rad/s, each finite and >= 0, in any order,
 * repeats allowed, 1 <= nw <= CMPC_FREQ_MAX_NW.  Per scenario A is balanced
 * once by a diagonal similarity of powers of two (Parlett-Reinsch scaling
 * without permutation, the rule of the modes' balancing; A <- D^-1 A D,
 * B <- D^-1 B, E <- D^-1 E, C <- C D, all exact), which keeps partial
 * pivoting from comparing states of different units against j omega.  Then
 * per frequency
 *   G (j w) = C_sel (j w I - A)^-1 B_sel   ny x nu, complex
 *   Gp(j w) = C_sel (j w I - A)^-1 E       ny x 2,  complex
 * through one complex adjoint solve (A - j w I)^T Z = C_sel^T on ns rows and
 * ns + 4 columns (pivot: the first largest |re| + |im|; quotients by Smith's
 * formula).  Host and device run the same arithmetic (csrc/freq_body.h) and
 * agree bit for bit.  r_f = max|f_i| is reported and not tested.
 * The record, CMPC_FREQ_LEN = 48 doubles per scenario and frequency (B x nw x
 * 48 in all): G 4 x 4 row-major in the order of out_idx x in_idx as (re, im)
 * pairs, then Gp 4 x 2 as pairs.  The summary, CMPC_FREQ_NSUM = 49 doubles per
 * scenario: the largest re^2 + im^2 over the list of each of the 16 + 8
 * entries, then the index k into omega of each of these peaks as a double (the
 * first of equal ones), then r_f.  An entry outside ny / nu is the quiet NaN
 * 0x7ff8000000000000.  Statuses, one per scenario:
 *   CMPC_EQ_OK
 *   CMPC_EQ_DEADZONE        a selected recycle valve below 2e-2
 *   CMPC_EQ_NONFINITE       an entry of A, of the selected part of B or C, of
 *                           f or of E is not finite, before or after scaling
 *   CMPC_EQ_SINGULAR        a zero or non-finite pivot at any frequency (j w
 *                           an eigenvalue of A in this arithmetic)
 *   CMPC_EQ_SKIPPED         the simulator's status was nonzero
 * and for every status but CMPC_EQ_OK all of the scenario's record and summary
 * is that NaN.  No status is an error of the call.
 *   cmpc_freq_check         -1 with a message for everything cmpc_gain_check
 *                           refuses, nw outside [1, 64], a null omega, or a
 *                           negative or non-finite frequency (host only)
 *   cmpc_plant_freq_host    B scenarios on the host, no device: record
 *                           B x nw x 48, summary B x 49, status B
 *   cmpc_freq_host          the same arithmetic from the balancing on for B
 *                           sets of matrices given, 1 <= n <= CMPC_FREQ_MAX_N:
 *                           A B x n x n, Bm B x n x 4, C B x 4 x n, E B x n x 2,
 *                           outputs and inputs the first ny rows of C and nu
 *                           columns of Bm (the others are not read); r_f of
 *                           the summary is 0.  Host only
 *   cmpc_sim_freq           the simulator's scenarios on its stream, one
 *                           launch, at its current x and plant input and the
 *                           pressures in force; omega a host array, uploaded.
 *                           The result buffers are allocated on first use and
 *                           grow when B x nw exceeds what they hold.  Nothing
 *                           of the simulator is written
 *   cmpc_sim_freq_download  host copies of the last call's results (any
 *                           pointer may be NULL; record B x nw x 48 with the
 *                           last call's nw); synchronises
 *   cmpc_sim_freq_record, _summary, _status  the device arrays (NULL before
 *                           the first cmpc_sim_freq); a later call with more
 *                           frequencies may move the record */
#define CMPC_FREQ_MAX_NW 64
#define CMPC_FREQ_MAX_N 12
#define CMPC_FREQ_LEN 48
#define CMPC_FREQ_NSUM 49
int cmpc_freq_check(int plant, int ny, const int32_t* out_idx, int nu, const int32_t* in_idx, int nw,
                    const double* omega);
int cmpc_plant_freq_host(int plant, int B, const double* pressures /* B*2 */, const double* u_full /* B*n_inputs */,
                         const double* x /* B*ns */, int ny, const int32_t* out_idx, int nu, const int32_t* in_idx,
                         int nw, const double* omega /* nw */, double* record /* B*nw*48 */,
                         double* summary /* B*49 */, int32_t* status /* B */);
int cmpc_freq_host(int n, int B, const double* A /* B*n*n */, const double* Bm /* B*n*4 */,
                   const double* C /* B*4*n */, const double* E /* B*n*2 */, int ny, int nu, int nw,
                   const double* omega /* nw */, double* record /* B*nw*48 */, double* summary /* B*49 */,
                   int32_t* status /* B */);
int cmpc_sim_freq(cmpc_sim* sim, int ny, const int32_t* out_idx, int nu, const int32_t* in_idx, int nw,
                  const double* omega_host /* nw */);
int cmpc_sim_freq_download(cmpc_sim* sim, double* record /* B*nw*48 */, double* summary /* B*49 */,
                           int32_t* status /* B */);
double* cmpc_sim_freq_record(cmpc_sim* sim);
double* cmpc_sim_freq_summary(cmpc_sim* sim);
int32_t* cmpc_sim_freq_status(cmpc_sim* sim);
/* Plant modes: the eigenvalues of small real nonsymmetric
 * matrices in batches, and on top of them the modes of the plant, that is the
 * eigenvalues of the continuous Jacobian A = df/dx at each scenario's state
 * (an equilibrium after cmpc_sim_equilibrium, but any state gives a valid A).
 * Per matrix: scaling by powers of two (Parlett-Reinsch), Householder
 * reduction to Hessenberg form, Francis double-shift QR with deflation; no
 * eigenvectors.  Host and device run the same arithmetic (csrc/eig_body.h) and
 * agree bit for bit.  Per matrix: wr and wi (n each), a status, and iters, the
 * QR sweeps used (<= max_iter).
 *   CMPC_EIG_OK              all n eigenvalues found
 *   CMPC_EIG_NO_CONVERGENCE  more than max_iter QR sweeps would be needed (or
 *                            an eigenvalue overflowed)
 *   CMPC_EIG_NONFINITE       an entry of the matrix was not finite
 *   CMPC_EIG_SKIPPED         the simulator's status of the scenario was nonzero
 * None of them is an error of the call.  The eigenvalues are ordered by real
 * part descending, then imaginary part descending: a conjugate pair sits
 * together, the member with wi > 0 first, the real parts equal bit for bit and
 * wi[k + 1] == -wi[k].  For every status but CMPC_EIG_OK wr, wi and the summary
 * are the quiet NaN 0x7ff8000000000000.  max_iter in [1, CMPC_EIG_MAX_ITER];
 * the Python layer's default is 30 n.
 * The summary, CMPC_MODES_NSUM doubles per matrix, from the ordered values:
 *   [0] spectral abscissa, max Re
 *   [1] the number of eigenvalues with Re > 0
 *   [2] the least damping ratio zeta = -Re / |lambda| over the eigenvalues with
 *       Im > 0 (the first in the order on a tie); 1 when there is none
 *   [3] that eigenvalue's damped frequency Im (0 when none)
 *   [4] its natural frequency |lambda| = sqrt(Re Re + Im Im) (0 when none)
 *   [5] min Re, the fastest mode
 *   cmpc_eig_host            B matrices (row-major n x n blocks, 1 <= n <= 12)
 *                            on the host, no device
 *   cmpc_eig_device          the same on the current device, n = 10 or 11 (a
 *                            smaller matrix is embedded block-diagonally); all
 *                            arrays device pointers; asynchronous on stream
 *   cmpc_modes_summary_host  the summary of eigenvalues given (B x n, ordered),
 *                            NaN where status is not CMPC_EIG_OK
 *   cmpc_plant_modes_host    B scenarios of the plant on the host: pressures
 *                            B x 2, u_full B x n_inputs, x B x ns; wr, wi B x ns,
 *                            summary B x 6
 *   cmpc_sim_modes           the simulator's scenarios on its stream, one
 *                            launch: at its current x and plant input and the
 *                            pressures in force; x is not written
 *   cmpc_sim_modes_download  host copies of the last analysis (any pointer may
 *                            be NULL); synchronises
 *   cmpc_sim_modes_wr, _wi, _summary, _status, _iters  the device arrays (NULL
 *                            before the first cmpc_sim_modes) */
#define CMPC_EIG_OK 0
#define CMPC_EIG_NO_CONVERGENCE 1
#define CMPC_EIG_NONFINITE 2
#define CMPC_EIG_SKIPPED 3
#define CMPC_EIG_MAX_N 12
#define CMPC_EIG_MAX_ITER 360 /* 30 * CMPC_EIG_MAX_N */
#define CMPC_MODES_NSUM 6
int cmpc_eig_host(int n, int B, const double* A /* B*n*n */, int max_iter, double* wr /* B*n */,
                  double* wi /* B*n */, int32_t* status, int32_t* iters);
int cmpc_eig_device(int n, int B, const double* A_device, int max_iter, double* wr_device, double* wi_device,
                    int32_t* status_device, int32_t* iters_device, void* stream);
int cmpc_modes_summary_host(int n, int B, const double* wr, const double* wi, const int32_t* status,
                            double* summary /* B*6 */);
int cmpc_plant_modes_host(int plant, int B, const double* pressures /* B*2 */,
                          const double* u_full /* B*n_inputs */, const double* x /* B*ns */, int max_iter,
                          double* wr, double* wi, double* summary /* B*6 */, int32_t* status, int32_t* iters);
int cmpc_sim_modes(cmpc_sim* sim, int max_iter);
int cmpc_sim_modes_download(cmpc_sim* sim, double* wr, double* wi, double* summary, int32_t* status,
                            int32_t* iters);
double* cmpc_sim_modes_wr(cmpc_sim* sim);
double* cmpc_sim_modes_wi(cmpc_sim* sim);
double* cmpc_sim_modes_summary(cmpc_sim* sim);
int32_t* cmpc_sim_modes_status(cmpc_sim* sim);
int32_t* cmpc_sim_modes_iters(cmpc_sim* sim);
/* NerveCenter::UpdateUOld (nerve_center.h:313-319): u_control (device,
 * B x nu_tot, plant control order) += each sub-controller's first move of its
 * own inputs (du_old after cmpc_iterate; input_order as cmpc_produce_lin). */
int cmpc_accumulate_moves(cmpc_ctx* ctx, const int32_t* input_order, double* u_control);

/* Device producer: AugmentedLinearizedSystem::Update
 * (libs/aug_lin_sys.cc:145-177, DiscretizeRK4 :232-255) for every scenario b
 * of the context's batch, on the GPU.  Linearises the plant at (x[b],
 * u_full[b]), discretises with sampling time Ts and writes the S lin records
 * of b into the context's own record buffer (replacing any cmpc_bind_lin
 * binding): input columns in input_order[s] order (host, S x nu_tot),
 * controlled rows out_idx[s] (host, S x ny), the observer tail dx_aug
 * (B*S x naug, or NULL for zeros) and y_prev = y[b][out_idx[s]].
 * x (B x ns), u_full (B x n_inputs), dx_aug and y (B x n_outputs) are DEVICE
 * pointers; the call is asynchronous on the context's stream.  p_in, p_out:
 * the plant's boundary pressures for the whole batch, ignored while
 * per-scenario pressures are in force (cmpc_set/bind_scenario_pressures). */
int cmpc_produce_lin(cmpc_ctx* ctx, int plant, double p_in, double p_out, double Ts,
                     const int32_t* input_order, const int32_t* out_idx, const double* x,
                     const double* u_full, const double* dx_aug, const double* y);

#ifdef __cplusplus
}
#endif
#endif /* CMPC_H */
