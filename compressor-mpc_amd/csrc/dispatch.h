// Kernel selection on the host (dispatch.cpp): which kernels can run a
// batch (availability predicates over kernel_dims.h) and which ones do
// (cmpc_dispatch_plan).  No HIP call: the file links into a stand-alone
// program (tests/cpp/dispatch_asan.cpp).
#pragma once
#include "cmpc_internal.h"

// CU count assumed when the device attribute query fails
constexpr int kCusFallback = 256;
constexpr size_t kLdsLimitBytes = 160 * 1024;  // LDS of a CU (gfx950)
// doubles of LDS per scenario row of the record producer (cmpc_prod::kScnLds)
constexpr int kProduceRowLds = 251;

// Dimension checks: nullptr, or the error text.  cmpc_layout_error fills *L
// (cmpc_layout_of); cmpc_context_dims_error adds what a context needs.
const char* cmpc_layout_error(const cmpc_dims* d, cmpc_layout* L);
const char* cmpc_context_dims_error(const cmpc_dims& d, const cmpc_layout& L);

// lwt = L_W' (upper triangular, ny x ny row-major) with ywt = L_W L_W': nullptr,
// or why ywt is refused (not symmetric, not positive semi-definite)
const char* cmpc_weight_factor_error(int ny, const double* ywt, double* lwt);

inline int cmpc_qp_len(const cmpc_layout& L) { return (L.nV * L.nV + L.nV + L.nV * L.nVo + 1) / 2 * 2; }
// LDS offset (doubles, 16-byte aligned) of the control step's producer rows
inline int cmpc_control_pr_off(int S, int rec_len, int naug) { return ((S * rec_len + naug + 3) / 4) * 2; }

// Every BuildParams field that follows from the dimensions, the batch and the
// CU count (the LDS layouts of both build kernels, the grid): all but the
// device pointers, co and sv.  Returns nullptr, or the error text when no
// build kernel can take the dimensions (record or LDS too long).
const char* cmpc_dispatch_params(const cmpc_dims& d, const cmpc_layout& L, int nqp, int cus, BuildParams* P);

// --- availability: everything a launcher needs to be true ------------------
// a delayed input's line of the row layout is a ring (the RING instantiations)
inline bool rows_has_ring(const RowsLayout& R) {
  for (int c = 0; c < CMPC_MAX_INPUTS; ++c)
    if (R.ring[c] > 0) return true;
  return false;
}
bool cmpc_build_wave_available(const cmpc_dims& d, const BuildParams& P);  // the role-split form too
// the row build's waves per workgroup (4 or 2), 0 when it cannot run
int cmpc_build_rows_waves(const cmpc_dims& d, const BuildParams& P);
inline bool cmpc_build_rows_available(const cmpc_dims& d, const BuildParams& P) {
  return cmpc_build_rows_waves(d, P) != 0;
}
// Per-slot weights (cmpc_set/bind_scenario_weights, BuildParamsW): the SCW
// instances of the one-QP-per-wave kernel keep a private yhat_q table
// (yl_stride) and the slot's [L_W' | uwt] block per wave; the wave region grows
// by this many doubles (even, so the 16-byte record chunks stay aligned)
inline int cmpc_scenario_weights_region(const cmpc_dims& d, const BuildParams& P) {
  return P.yl_stride + (d.ny * d.ny + d.nu * d.nu + 1) / 2 * 2;
}
// P: cmpc_dispatch_params.  An SCW instance exists (the WAVE column) and the
// workgroup's LDS still fits with the grown wave regions.
bool cmpc_build_weights_available(const cmpc_dims& d, const BuildParams& P);
// cmpc_dispatch_params for the SCW instances: P with lds_per_wave grown and
// tab_off set; the two pointers are left null
void cmpc_dispatch_params_weights(const cmpc_dims& d, const BuildParams& P, BuildParamsW* W);
// the launcher's check: W's wave region is the grown one and it fits
bool cmpc_build_weights_launchable(const cmpc_dims& d, const BuildParamsW& W);
// Shared form of the row build (cmpc_set_build_pairing): nullptr, or why the
// configuration cannot use it.  lwt0 / lwt1: the two sub-controllers' L_W'
// tables (ny x ny), compared bit for bit; null: not compared.
const char* cmpc_pairing_error(const cmpc_dims& d, const BuildParams& P, const double* lwt0, const double* lwt1);
// CMPC_PAIRING_AUTO uses the shared form for a batch of this many scenarios
bool cmpc_pairing_auto(int scenarios);
// fused steps and the one-launch control step: the solver the kernel runs
// (CMPC_SOLVE_ROWS / CMPC_SOLVE_LANE), 0 when it cannot run
int cmpc_step_wave_solver(const cmpc_dims& d, const BuildParams& P);
int cmpc_step_rows_solver(const cmpc_dims& d, const BuildParams& P);
// split: the build as role-split pairs on `grid` workgroups of two QP slots
int cmpc_control_solver(const cmpc_dims& d, const BuildParams& P, bool split, int grid, bool trace, int pr_off);
bool cmpc_solve_lane_available(int nV, int nu, int nVo, int qp_len, bool trace, bool du_other);
bool cmpc_solve_rows_available(int nV, int nu, int nVo, int S, int qp_len, bool trace, bool du_other);
// the predict kernel (predict.hip) has an instance: every dimension set with a
// one-QP-per-wave build instance (cmpc_predict_available, cmpc.h, adds the
// context's dimension checks)
bool cmpc_predict_instance(const cmpc_dims& d, const cmpc_layout& L);
// the reference-profile correction (refshift.hip) has an instance: the same
// column (cmpc_reference_profile_available, cmpc.h, adds the context's
// dimension checks)
bool cmpc_refshift_instance(const cmpc_dims& d, const cmpc_layout& L);

// --- the policy ------------------------------------------------------------
// P: cmpc_dispatch_params of the batch (nqp, cus and the layouts).  K, trace
// and du_other describe the call (cmpc.h, cmpc_plan).  ref_profile: a
// per-slot reference profile is in force (CMPC_PLAN_REF_PROFILE): the fused
// paths keep f in registers and cannot take its correction, so the step is
// two launches and the control step its three calls.  scenario_weights:
// per-slot weights are in force (CMPC_PLAN_SCENARIO_WEIGHTS): only the
// one-QP-per-wave kernel's SCW instances take them, so the build is
// CMPC_BUILD_WAVE at every batch size, ROWS or SPLIT forced is an error, and
// nothing is fused (FUSED forced is an error).
cmpc_plan_t cmpc_dispatch_plan(const cmpc_dims& d, const cmpc_layout& L, const BuildParams& P, int build_variant,
                               int solve_variant, int step_variant, int K, bool trace, bool du_other,
                               bool ref_profile = false, bool scenario_weights = false);
// cmpc_plan (cmpc.h) without the error slot: nullptr, or the error text
const char* cmpc_plan_or_error(const cmpc_dims* dims, int cus, int build_variant, int solve_variant,
                               int step_variant, int K, uint32_t flags, cmpc_plan_t* plan);
