// The plant simulator of the C ABI (include/cmpc.h):
// abi_sim.cpp runs it, abi_analysis.cpp analyses its scenarios.
#pragma once
#include "abi_common.h"

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
  // results of the last cmpc_sim_freq (allocated on first use): the frequencies uploaded (CMPC_FREQ_MAX_NW),
  // record B * fq_nw * CMPC_FREQ_LEN (room for B * fq_cap frequencies), summary B * CMPC_FREQ_NSUM, status B
  double *fq_omega = nullptr, *fq_record = nullptr, *fq_summary = nullptr;
  int32_t* fq_status = nullptr;
  int fq_nw = 0, fq_cap = 0;
  // results of the last cmpc_sim_modes (allocated on first use): wr, wi B * ns,
  // summary B * CMPC_MODES_NSUM, status and iters B
  double *md_wr = nullptr, *md_wi = nullptr, *md_summary = nullptr;
  int32_t *md_status = nullptr, *md_iters = nullptr;
  cmpc_abi::PinnedIO pin_in, pin_out;  // host-array calls: page-locked staging
};
