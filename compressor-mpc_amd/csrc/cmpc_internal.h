// Internal launch parameters shared by cmpc_abi.cpp (host) and
// cmpc_kernels.hip (device).  Not part of the public ABI.
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cmpc.h"
#include "kernel_dims.h"

// Kernel timing (cmpc_enable_timing).  cmpc_abi.cpp sets these events around
// a timed launch (null otherwise); the launchers hand them to
// hipExtLaunchKernelGGL, which stamps the kernel's own start and end into
// them from its dispatch packet.  hipEventRecord markers before and after
// each kernel cost ~7 us per bench step (tools/time_step_gaps.py).  One
// context per host thread (cmpc.h), hence thread_local.
struct LaunchEvents {
  hipEvent_t start = nullptr, stop = nullptr;
};
extern thread_local LaunchEvents cmpc_launch_events;
template <typename F, typename... A>
inline void cmpc_launch(F kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, A... args) {
  if (cmpc_launch_events.start || cmpc_launch_events.stop)
    hipExtLaunchKernelGGL(kernel, grid, block, (std::uint32_t)lds, stream, cmpc_launch_events.start,
                          cmpc_launch_events.stop, 0u, args...);
  else  // the plain launch path: ~8 us of host time per hipExtLaunchKernel
        // call in the B = 1 step's --hip-trace (profiles/r4e_b1_hip_api_stats.csv)
    hipLaunchKernelGGL(kernel, grid, block, (std::uint32_t)lds, stream, args...);
}

// Resident workgroups per CU of `kernel` at `threads` x `lds` bytes, from the
// occupancy query, cached per (kernel, threads, lds): the query costs ~9 us of
// host time per call (B = 1 step --hip-trace), once per launch before.
// 0 when the query fails.  One context per host thread, hence thread_local.
template <typename F>
inline int cmpc_blocks_per_cu(F kernel, int threads, size_t lds) {
  struct Entry {
    const void* k;
    int threads;
    size_t lds;
    int blocks;
  };
  static thread_local Entry cache[32];
  static thread_local int n = 0;
  const void* key = reinterpret_cast<const void*>(kernel);
  for (int i = 0; i < n && i < 32; ++i)
    if (cache[i].k == key && cache[i].threads == threads && cache[i].lds == lds) return cache[i].blocks;
  int v = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, kernel, threads, lds) != hipSuccess) v = 0;
  cache[n % 32] = Entry{key, threads, lds, v};
  ++n;
  return v;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (device, kernel,
// size): a launcher that set it on every launch paid its host time per step
// (a config-5 step: 57 us of wall time per 41 us kernel).  The attribute
// belongs to the function object of the current device, so a host thread
// that drives contexts on two devices sets it on each.
inline void cmpc_allow_lds(const void* kernel, size_t bytes) {
  struct Entry {
    int dev;
    const void* k;
    size_t bytes;
  };
  static thread_local Entry cache[32];
  static thread_local int n = 0;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) dev = -1;
  for (int i = 0; i < n && i < 32; ++i)
    if (cache[i].dev == dev && cache[i].k == kernel && cache[i].bytes >= bytes) return;
  (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  cache[n % 32] = Entry{dev, kernel, bytes};
  ++n;
}

#define CMPC_ND_MAX 4            // delayed inputs supported by the build kernel
#define CMPC_BUILD_WAVES 4       // waves per build workgroup (one QP per wave at a time)
#ifndef CMPC_ROWS_U
#define CMPC_ROWS_U 5            // horizon unroll of the row build kernel (4 or 5; 5: p = 50 in whole blocks, +0.7%)
#endif
#ifndef CMPC_ROWS_U2
#define CMPC_ROWS_U2 10          // ... for ny = 2 (config 3: 211 -> 205 us; profiles/r6f_stride_u10_ab/)
#endif
// the row build kernel's horizon unroll for ny outputs (the kernel and its
// LDS layout, rows_layout.cpp, take it from here)
__host__ __device__ constexpr int cmpc_rows_unroll(int ny) { return ny == 2 ? CMPC_ROWS_U2 : CMPC_ROWS_U; }
#define CMPC_ROWS_NSEG 16        // loop segment bounds of the row build kernel
#define CMPC_REC_CHUNKS 3        // 16-byte lin-record chunks per lane (rec_len <= 384)
// QPs (= lanes) per solve workgroup: one wave, so a batch of fewer waves than
// CUs spreads one wave per CU (the CU's scalar unit and instruction fetch
// are shared by its waves): config 2 iterate (K = 9, 128 waves) 11.6 -> 9.8 us
// against 256; level at the bench size (profiles/r5h_solve_wg_ab.txt)
#ifndef CMPC_SOLVE_THREADS
#define CMPC_SOLVE_THREADS 64
#endif
#define CMPC_HOST_OUT_MAX_QP 64  // up to this many QPs: du/status/nWSR live in page-locked host memory
#ifndef CMPC_SOLVE_ROWS_MAX_QP
#define CMPC_SOLVE_ROWS_MAX_QP 16384  // CMPC_SOLVE_AUTO: the row solve kernel below this many QPs
#endif

// Per sub-controller configuration block in device memory (doubles):
//   [lwt  : ny*ny ]  L_W' with ywt = L_W L_W' (upper triangular)
//   [yhat : p*ny  ]  L_W' y_ref_r
//   [uwt  : nu*nu ]  input weight block of R = blkdiag_m(uwt)
//   [lower, upper, rate_lower, rate_upper : nu each]  contiguous, in this order:
//     the solve bodies read them from one base pointer, co.lower or a slot's
//     own block of SolveParams::limits
struct CfgOffsets {
  int lwt, yhat, uwt, lower, upper, rlower, rupper, len;
};

// LDS layout of the row-layout build kernel (build_rows.hip), doubles.
// Block region: [zeros 16][yhat S x NY x yls (output-major)][lwt][uwt].
// Wave region : [hand-off 4 x LQ][C_hat 4 x NY x 16][w 4 x ND x WL].
// Hand-off area of one QP, in entries of NY doubles ([entry][output]): per
// input c at lo[c] a ring of U + 1 entries (undelayed) or m - 1 zero entries
// + max(0, p - D_c) values (delayed); then a dump area, the free-response z
// entries and a zero area (U entries each).
// A delayed input's line is a ring of D + m entries when its p - D values
// would need more (p > 2 D + 1): the writer and the two gather readers step
// back by ring[c] entries at each of their wrap steps (every ring[c] steps),
// which are loop segment bounds too (at most CMPC_ROWS_NSEG of them).  The C_hat rows overlay the hand-off areas: they are read in the
// prologue only, before the zero areas are written.
struct RowsLayout {
  int ok;                        // the row kernel can run these dimensions
  int lds_block, per_wave;
  int yl_off, yls, lw_off, uw_off;
  int LQ, lo[CMPC_MAX_INPUTS], dump_off, z_off, zr_off;
  int ring[CMPC_MAX_INPUTS];      // entries of a wrapping delayed line, 0: a plain line
  int ch_off, w_off, WL;
  int nseg, seg[CMPC_ROWS_NSEG];  // ascending distinct D, p - D and wrap steps inside (0, p)
  int U;                          // the kernel's horizon unroll (cmpc_rows_unroll)
};

// Shared-form row build (build_pair_kernel.h): one cooperative scenario per
// row.  Its wave region keeps RowsLayout's hand-off areas and C_hat rows and
// adds: [z of slot 1: 4 x U x NY at z1_off][w: 4 x 2 x ND x WL at w_off].  The
// group's staging, 4 x (rec_len + rec_len - tail0) doubles, overlays the
// region up to w_off: the w tables are filled while the records are read.
#define CMPC_PAIR_CMP 4          // 64-entry blocks of a record's head (A, B, C, f) compared per lane
struct PairLayout {
  int ok;                        // the shared form can run these dimensions
  int z1_off, w_off, WL, per_wave;
  int tail0;                     // first entry (even) of the other slot's staged tail: off_x rounded down
};

struct SolveParams {
  const double* qp;
  const double* cfg;
  double* u_old;      // nqp * nu_tot
  double* du_old;     // nqp * nV
  uint32_t* ws;       // nqp
  double* du;         // nqp * nV
  int32_t* status;    // nqp
  int32_t* nwsr;      // nqp
  uint8_t* trace;     // nqp * K * 16 or null
  int32_t* ntrace;    // nqp * K or null
  int nqp, S, K, nu_tot, qp_len;
  CfgOffsets co;
  uint32_t flags;
  int init;           // 1: InitializeQPProblem (cold, f only, ws only)
  const double* du_other;  // nqp * nVo other controllers' plans (cmpc_get_input), or null:
                           // the in-scenario exchange of cmpc_iterate
  const double* limits;    // nqp * 4 nu per-slot [lower | upper | rate_lower | rate_upper]
                           // (cmpc_set_scenario_constraints), or null: the cfg block's
};

struct BuildParams {
  const double* lin;     // nqp * rec_len
  const double* cfg;     // S * cfg.len
  const double* u_old;   // nqp * nu_tot
  double* qp;            // nqp * qp_len   [H nV*nV | f nV | G nV*nVo]
  const double* dy_ref;  // nqp * ny per-slot setpoint offsets, applied as y_prev - dy_ref
                         // (cmpc_set_scenario_reference), or null
  int nqp, S, p, nu_tot, ndist, nd, dmax, rec_len, qp_len;
  int off_A, off_B, off_C, off_f, off_x, off_y, nobs;
  CfgOffsets co;
  int delay[CMPC_MAX_INPUTS];    // per input
  int dindex[CMPC_MAX_INPUTS];   // per input: delayed index kd or -1
  int dinput[CMPC_ND_MAX];       // per delayed index: input c
  int dlen[CMPC_ND_MAX];         // per delayed index: delay D
  int boff[CMPC_ND_MAX];         // per delayed index: offset of its shift block in dx_aug
  // LDS layout (doubles), computed on the host by build_lds_layout() so that
  // the per-step hand-off reads/writes are free of bank conflicts
  int lds_block;                 // block-shared: yhat (S x yl_stride), lwt, uwt, zeros
  int yl_stride;                 // per sub-controller yhat stride (multiple of 32)
  int lds_per_wave;              // per-wave region (multiple of 32)
  int line_off[CMPC_MAX_INPUTS]; // delay line of input c inside a row
  int line_rs;                   // delay-line row stride (one row per output)
  int w_off;                     // w table
  int zs_off;                    // free-response hand-off slots (NY x 4), or the
                                 // ny = 4 pre-pass z lines (NY x zl_stride)
  int zl_stride;
  int nbound;                    // distinct delays 0 < D < p, ascending (loop segments)
  int bound[CMPC_MAX_INPUTS];
  int grid;                      // workgroups needed (one QP per wave); launcher caps it
  int split;                     // cmpc_launch_build: the role-split kernel (every ny)
  int cus;                       // compute units of the device
  RowsLayout rows;               // row-layout kernel (four QPs per wave)
  // shared form of the row build (cmpc_set_build_pairing): its layout, whether
  // this launch uses it, and the coverage counters (scenarios built shared):
  // this launch's and the one it clears for the next launch
  PairLayout pair;
  int use_pair;
  uint32_t* pair_cnt;
  uint32_t* pair_cnt_next;
  // fused step (cmpc_step on small batches): the K Jacobi iterations run in
  // the build kernel on the QPs it just built (solve_rows.h), with these
  // parameters (sv.qp unused: H, f, G stay in registers)
  SolveParams sv;
};

// Per-slot weights (cmpc_set/bind_scenario_weights): the
// one-QP-per-wave build kernel's SCW instances take BuildParams and these.
// lds_per_wave is then the grown region: the wave's private tables
// [yhat_q yl_stride][L_W' ny*ny | uwt nu*nu] sit at tab_off, after the plain
// region; lds_block is the zero slots alone (no block-shared tables).  Its own
// struct, so that the kernel arguments of every other instance stay what they
// are.
struct BuildParamsW : BuildParams {
  const double* sc_w;   // nqp * (ny*ny + nu*nu): per slot [L_W' | uwt]
  const double* yref;   // S * p * ny raw references y_ref[s][r] (cfg holds L_W' y_ref only)
  int tab_off;          // the private tables inside the wave region (doubles, even)
};


// Prediction (predict.hip, cmpc_predict): the predicted controlled outputs of
// every QP slot over the horizon for given plans, and the two parts of the
// objective.  Reads what the build read (records, u_old, cfg, dy_ref).
struct PredictParams {
  const double* lin;     // nqp * rec_len
  const double* cfg;     // S * co.len
  const double* u_old;   // nqp * nu_tot
  const double* dy_ref;  // nqp * ny per-slot setpoint offsets, or null
  const double* dref;    // nqp * p * ny per-slot reference profiles (RefshiftParams), or null
  const double* sc_w;    // nqp * (ny*ny + nu*nu) per-slot [L_W' | uwt] (BuildParamsW), or null: the cfg block's
  const double* yref;    // S * p * ny raw references, read with sc_w (yhat[q] = L_W'[q] y_ref[s])
  const double* du;      // nqp * nV own plans
  const double* d;       // nqp * nVo other controllers' plans (the Jacobi iteration's order), or
                         // null: gathered from du of the scenario's other slots
  double* y_pred;        // nqp * p * ny
  double* cost;          // nqp * 2: [J_track, J_move]
  int nqp, S, p, ndist, rec_len, nobs;
  int off_A, off_B, off_C, off_f, off_x, off_y;
  CfgOffsets co;
  int delay[CMPC_MAX_INPUTS];  // per input
  int dslot[CMPC_MAX_INPUTS];  // per delayed input: dx_aug index of its delayed-input state
  int dblk[CMPC_MAX_INPUTS];   // per delayed input: dx_aug index of its shift block's first entry
};
// one QP per 16-lane row, four per one-wave workgroup; -1: no instance
int cmpc_launch_predict(const PredictParams& P, const cmpc_dims& d, void* stream);

// Reference-profile correction (refshift.hip): f -= Su' w of
// every QP slot, w[r] = ywt[s] dref[q][r] (ywt[q] with per-slot weights), in
// place in the QP buffer right after the build.  Reads the records the build
// read.
struct RefshiftParams {
  const double* lin;     // nqp * rec_len
  const double* cfg;     // S * co.len
  const double* dref;    // nqp * p * ny, [slot][horizon row][output]
  const double* sc_w;    // nqp * (ny*ny + nu*nu) per-slot [L_W' | uwt] (BuildParamsW), or null: the cfg block's
  double* qp;            // nqp * qp_len; only f (nV doubles at nV * nV) is read and written
  int nqp, S, p, rec_len, nobs, qp_len;
  int off_A, off_B, off_C;
  CfgOffsets co;
  int delay[CMPC_MAX_INPUTS];  // per input
};
// one QP per 16-lane row, four per one-wave workgroup; -1: no instance
int cmpc_launch_refshift(const RefshiftParams& P, const cmpc_dims& d, void* stream);

// Closed-loop performance indices (score.hip, cmpc_score_*):
// one running record per QP slot, field-major (field row f of slot q at
// f * nqp + q), all doubles.  The rows of each field, in the record's order;
// the kernel, the host functions and cmpc_score_field take them from here.
struct ScoreFields {
  int n, ise, iae, peak, last_out, j_track, j_move, tv, sat_bound, sat_rate, n_fail, nwsr_sum,
      plant_fail_step, len;
};
__host__ __device__ constexpr ScoreFields cmpc_score_fields(int ny, int nu) {
  ScoreFields F{};
  int o = 0;
  F.n = o; o += 1;
  F.ise = o; o += ny;
  F.iae = o; o += ny;
  F.peak = o; o += ny;
  F.last_out = o; o += ny;
  F.j_track = o; o += 1;
  F.j_move = o; o += 1;
  F.tv = o; o += nu;
  F.sat_bound = o; o += nu;
  F.sat_rate = o; o += nu;
  F.n_fail = o; o += 1;
  F.nwsr_sum = o; o += 1;
  F.plant_fail_step = o; o += 1;
  F.len = o;
  return F;
}
struct ScoreParams {
  double* rec;                  // len * nqp running records, field-major
  const double* y;              // B * n_out measured plant outputs
  const double* target;         // nqp * ny, or null: y_ref[s][0] + dy_ref[q]
  const double* cfg;            // S * co.len
  const double* yref;           // S * p * ny raw references (row 0 is read), with target null
  const double* dy_ref;         // nqp * ny per-slot setpoint offsets, or null
  const double* sc_w;           // nqp * (ny*ny + nu*nu) per-slot [L_W' | uwt], or null: the cfg block's
  const double* du;             // nqp * nV plans (the own first move is read)
  const int32_t* status;        // nqp
  const int32_t* nwsr;          // nqp
  const uint32_t* ws;           // nqp working-set words of the state in force
  const int32_t* plant_status;  // B simulator status words, or null
  const int32_t* out_idx;       // S * ny: plant output of each controlled output
  const double* band;           // S * ny settling bands
  // trajectory capture: row [y n_out | u_control nu_tot | x ns] of the chosen
  // scenarios at step k < t_cap, written by the lane of slot s == 0
  const int32_t* cap_map;       // B: capture column of scenario b or -1; null: capture off
  double* cap;                  // t_cap * n_sel * cap_w
  const double* u_control;      // B * nu_tot or null (columns left as they are)
  const double* x;              // B * ns or null
  int n_sel, t_cap, cap_w, n_out, nu_tot, ns;
  int nqp, S, p, nV, k;
  double Ts;
  CfgOffsets co;
};
bool cmpc_score_instance(int ny, int nu);
// one lane per QP slot, 64-lane workgroups; -1: no instance for (ny, nu)
int cmpc_launch_score(const ScoreParams& P, int ny, int nu, void* stream);
// every field of every slot to 0, last_out and plant_fail_step to -1
int cmpc_launch_score_reset(double* rec, int nqp, int ny, int nu, void* stream);

// Multipliers and KKT certificate (certify.hip, cmpc_certify*, DESIGN.md
// §3.16): one record per QP slot, field-major (row r of slot q at
// r * nqp + q), all doubles.  The rows of each field, in the record's order;
// the kernels, the host functions and cmpc_certify_field take them from here.
struct CertifyFields {
  int lam, r_stat, r_prim, r_dual, r_comp, obj, scale, n_active, status, rank_def, len;
};
__host__ __device__ constexpr CertifyFields cmpc_certify_fields(int nV) {
  CertifyFields F{};
  int o = 0;
  F.lam = o; o += 2 * nV;
  F.r_stat = o; o += 1;
  F.r_prim = o; o += 1;
  F.r_dual = o; o += 1;
  F.r_comp = o; o += 1;
  F.obj = o; o += 1;
  F.scale = o; o += 1;
  F.n_active = o; o += 1;
  F.status = o; o += 1;
  F.rank_def = o; o += 1;
  F.len = o;
  return F;
}
struct CertifyParams {
  double* rec;             // len * nqp records, field-major
  const double* qp;        // nqp * qp_len   [H nV*nV | f nV | G nV*nVo]
  const double* cfg;       // S * co.len
  const double* limits;    // nqp * 4 nu per-slot limits (SolveParams::limits), or null: the cfg block's
  const double* u_old;     // nqp * nu_tot
  const double* du;        // nqp * nV plans
  const double* d;         // nqp * nVo other controllers' plans (cmpc_predict's order), or null:
                           // gathered from du of the scenario's other slots
  const uint32_t* ws;      // nqp working-set words of the state in force
  const int32_t* status;   // nqp
  int nqp, S, nu_tot, qp_len;
  CfgOffsets co;
};
bool cmpc_certify_instance(int nV, int nu, int nVo);
// one lane per QP slot, 64-lane workgroups; -1: no instance for (nV, nu, nVo)
int cmpc_launch_certify(const CertifyParams& P, int nV, int nu, int nVo, void* stream);
// The summary: two launches over the record's residual rows; `work` holds
// cmpc_certify_summary_bytes() bytes, its head the result once both have run
// (cmpc_certify_summary_unpack turns a host copy of the head into the ABI's struct).
size_t cmpc_certify_summary_bytes();
int cmpc_launch_certify_summary(const double* rec, int nqp, int nV, double tol, void* work, void* stream);
void cmpc_certify_summary_unpack(const void* work_head, cmpc_certify_summary_t* out);
constexpr size_t kCertifySummaryHead = 64;  // bytes of the head (>= the partial's size)

// Seeded per-scenario noise (noise.hip, cmpc_noise_*): the
// draw's arithmetic is noise_body.h's, shared with the host entry points.
struct NoiseParams {
  uint32_t k0, k1, stream, scenario0;  // seed low and high words, stream, first global scenario
  uint32_t step;
  int B, n, np;          // np = ceil(n / 2) Box-Muller pairs per scenario
  const double* sigma;   // B * n, or null: 1
  const double* rho;     // B * n, or null: white
  double* w;             // B * n AR(1) state (with rho)
  const double* base;    // B * n, or null: 0
  double* out;           // B * n
  double* u;             // B * np * 2 uniforms (cmpc_launch_noise_uniforms)
};
// one lane per (scenario, pair), 64-lane workgroups; -1: more workgroups than a grid holds
int cmpc_launch_noise_step(const NoiseParams& P, void* stream);
int cmpc_launch_noise_uniforms(const NoiseParams& P, void* stream);

// Ensemble statistics of the score record (score_ensemble.hip,
// cmpc_score_ensemble): per record row f and sub-controller s over the B
// scenarios, kScoreEnsembleStats doubles [mean, std, min, max, argmax, count]
// at head[(f * S + s) * kScoreEnsembleStats].  `work` holds
// cmpc_score_ensemble_bytes(len, S) bytes: the head (what the host copies),
// then the thresholds (len doubles, read where has_thr), then the partials.
constexpr int kScoreEnsembleStats = 6;
size_t cmpc_score_ensemble_bytes(int len, int S);
// the device address of the thresholds inside `work`
double* cmpc_score_ensemble_thresholds(void* work, int len, int S);
// three launches: partials per block, centred squares per block, a wave per row over both
int cmpc_launch_score_ensemble(const double* rec, int len, int B, int S, bool has_thr, void* work, void* stream);

// Exact ensemble quantiles and the per-step envelope (ensemble_quantiles.hip,
// cmpc_score_quantiles, cmpc_envelope_step); the selection
// arithmetic is ensemble_select.h's, shared with the host entry points.
// The rows reduced over the B scenarios, in two segments: row r < rows0 is
// (f, s) = (r / S0, r mod S0) of a (len, B, S0) array, x_b = p0[f * fstride0 +
// b * S0 + s] (the score record: fstride0 = B * S0; a scenario-major (B x C)
// array: rows0 = S0 = C); row rows0 + c is column c of the scenario-major
// (B x S1) array p1.
struct EnsRowMap {
  const double *p0, *p1;
  int64_t fstride0;
  int rows0, S0, rows1, S1;
};
// the ranks of a call's levels, computed on the host (cmpc_select_rank)
struct QuantileRanks {
  uint32_t k_lo[CMPC_QUANTILE_MAX_LEVELS], k_hi[CMPC_QUANTILE_MAX_LEVELS];
  int n;
};
// where the results go: row r's at out + r * row_stride; level l's x_lo, x_hi
// (and, with lvl_stride 3, arg) at + l * lvl_stride
struct QuantileOut {
  double* out;
  int64_t row_stride;
  int lvl_stride;
};
// blocks per row a call launches: a function of (rows, B) alone
int cmpc_quantile_blocks(int rows, int B);
// bytes of the work buffer for up to n_levels levels.  Its head is room for
// rows * n_levels * 3 doubles, for a caller that wants the results there.
size_t cmpc_quantile_work_bytes(int rows, int B, int n_levels);
// 18 launches (two per digit, two for the last pass), nothing else; -1: an
// argument outside the limits
int cmpc_launch_quantiles(const EnsRowMap& M, int B, const QuantileRanks& R, const QuantileOut& O, void* work,
                          void* stream);
// The six statistics of cmpc_score_ensemble over an EnsRowMap's rows, row r's
// at out + r * row_stride, the count against thr[r] (device, one per row, or
// null: 0).  Three launches; `work` holds cmpc_envelope_moments_bytes(rows).
size_t cmpc_envelope_moments_bytes(int rows);
int cmpc_launch_envelope_moments(const EnsRowMap& M, int B, const double* thr, double* out, int64_t row_stride,
                                 void* work, void* stream);

// Standalone batched solver (parity / KKT tests).  G (nqp * n * nvo) and d
// (nqp * nvo) non-null: the Jacobi iteration's map-form solve with g = f + G d
// (cmpc_qp_solve_batch_map); g is f then.
struct QpBatchParams {
  const double *H, *g, *lb, *ub, *lbA, *ubA;
  const uint32_t* ws_in;
  double* x;
  int32_t *status, *nchg, *ntrace;
  uint32_t* ws_out;
  uint8_t* trace;
  int nqp, max_chg;
  const double *G = nullptr, *d = nullptr;
  int nvo = 0;
};

// Device record producer (produce.hip): one scenario's plant linearisation
// -> its S lin records.
#define CMPC_MAX_S_PRODUCE 8
struct ProduceParams {
  double* lin;                  // B*S*rec_len, written
  const double* x;              // B*ns
  const double* u_full;         // B*n_inputs
  const double* dx_aug;         // B*S*naug or null (zeros)
  const double* y;              // B*n_outputs
  int B, S, rec_len, nu_tot, ny, nobs, naug, n_outputs;
  int off_A, off_B, off_C, off_f, off_x, off_y;
  double p_in, p_out, Ts;
  int input_order[CMPC_MAX_S_PRODUCE][CMPC_MAX_INPUTS];
  int out_idx[CMPC_MAX_S_PRODUCE][4];
  // per-QP mode (the observer's closed loop): one linearisation per QP slot
  // q at x + q * x_stride, dx_aug row stride dx_stride, and the plant's full
  // output matrix (n_outputs x ns) stored to c_out + q * c_stride
  int per_qp, x_stride, dx_stride, c_stride;
  double* c_out;
  // per-QP mode: dx_aug's delay blocks are rings (observer.hip): block k
  // spans dx_aug entries [rb[k], rb[k] + rlen[k]), logical entry i stored at
  // rb[k] + (i + rot[k]) mod rlen[k]
  int nring, rb[CMPC_ND_MAX], rlen[CMPC_ND_MAX], rot[CMPC_ND_MAX];
  // per-QP mode, cmpc_observe_step: the observer's a-posteriori update of the
  // slot (ObserveAPosteriori, in or_observe_post's arithmetic order) runs first in
  // the same kernel, x = the observer rows (x_hat, then dx of obs_ntot
  // entries, y_old, C): obs_M = S x nobs x n_outputs gains, or null
  const double* obs_M;
  double* obs;  // the observer rows (x above, writable)
  int obs_ntot;
  // per-scenario boundary pressures (cmpc_set/bind_scenario_pressures): B x
  // [p_in, p_out], scenario b's pair in place of p_in, p_out above, or null
  const double* pressures;
};

// Observer kernels (observer.hip)
#define CMPC_OBS_INIT 0
#define CMPC_OBS_PRIOR 2
struct ObserverParams {
  double* obs;              // nqp * obs_len state rows
  const double* M;          // S * nobs * n_out observer gains
  const double* y;          // B * n_out plant outputs (init / post)
  const double* x_init;     // B * ns (init)
  const double* dx_init;    // nqp * ntot or null (init)
  const double* lin;        // step records (prior: B, f)
  const double* du_old;     // nqp * nV plans (prior)
  double* u_old;            // nqp * nu_tot (prior)
  const double* du_full;    // nqp * nu_tot applied input change (cmpc_update_u), or null:
                            // the own first move of du_old (cmpc_observe_apply)
  int nqp, S, ns, ndist, nobs, ntot, n_out, obs_len;
  int nu, nu_tot, nV, nd, rec_len, off_B, off_f;
  int delay[CMPC_MAX_INPUTS];   // per input (sub-controller order)
  int dinput[CMPC_MAX_INPUTS];  // k-th delayed input -> input index
  int blk[CMPC_MAX_INPUTS];     // first dx index of delay block k
  int rot[CMPC_MAX_INPUTS];     // ring position of block k's first state (step count mod D - 1)
};

// One-launch control step (cmpc_control_step, cmpc_kernels.hip): the
// producer (per-QP mode with the a-posteriori update), the fused build + K
// iterations and the observer's a-priori update of a small batch.  pr_off:
// the producer rows' LDS offset (doubles) after its element table.
struct ControlStepParams {
  BuildParams b;
  ProduceParams pr;
  ObserverParams ob;
  int pr_off;
  // one-workgroup launches: after the last phase, seq is stored to *done
  // (page-locked host memory) with a system-scope release, so the host can
  // wait for the results by polling instead of a stream synchronisation
  uint32_t* done;
  uint32_t seq;
};
int cmpc_launch_control_step(const ControlStepParams& C, const cmpc_dims& d, void* stream);

// One Jacobi iteration of the sub-controller-sharded cooperative loop
// (coupled.hip).
struct CoupledParams {
  const double* qp;       // nqp * qp_len (H, f from cmpc_build)
  const double* cfg;
  const double* limits;   // nqp * 4 nu per-slot limits or null (SolveParams::limits)
  CfgOffsets co;
  double* u_old;          // nqp * nu_tot
  double* du_old;         // nqp * nV
  uint32_t* ws;
  double* du;             // nqp * nV (context buffer)
  double* du_out;         // nqp * nV caller buffer (the next all-gather's input) or null
  int32_t *status, *nwsr;
  const double* G_ext;    // [nV * (S_total-1) * nV][nqp], element-major
  const double* du_all;   // [world][B][S_local][nV], all-gathered plans
  int nqp, qp_len, nu_tot, S_cfg, S_total, S_local, s_offset, B;
  uint32_t flags;
};

// Kernel launchers.  Which one runs is decided before the call
// (cmpc_dispatch_plan, dispatch.h); a launcher only launches.  Each checks its
// availability predicate once more and returns -1 where it is false: the plan
// and the launcher disagree, an internal error and never a fallback.
int cmpc_launch_build(const BuildParams& P, const cmpc_dims& d, void* stream);  // P.split: the role-split kernel
// the one-QP-per-wave kernel's per-slot-weights instances (BuildParamsW)
int cmpc_launch_build_weights(const BuildParamsW& P, const cmpc_dims& d, void* stream);
// Row-layout build kernel (build_rows.hip)
int cmpc_launch_build_rows(const BuildParams& P, const cmpc_dims& d, void* stream);
// Fused step (step_rows.hip): the row build kernel running the K Jacobi
// iterations of its QPs itself (P.sv) with `solver` (cmpc_step_rows_solver)
int cmpc_launch_step_rows(const BuildParams& P, const cmpc_dims& d, int solver, void* stream);
// the same on the one-QP-per-wave build kernel (cmpc_kernels.hip)
int cmpc_launch_step_wave(const BuildParams& P, const cmpc_dims& d, void* stream);
// Waves per workgroup the row kernel launches with for layout R (4, 2 or 1;
// 0: does not fit) (build_rows.hip).
int cmpc_rows_waves_per_group(const RowsLayout& R);
// workgroups of w waves per CU that the layout's LDS lets run at once
int cmpc_rows_resident_groups(const RowsLayout& R, int w);
// LDS layout of the row kernel, chosen by a bank-conflict model of its
// horizon loop (rows_layout.cpp); cached per dimension set, thread-safe.
void cmpc_rows_layout(const cmpc_dims& d, int nd, int nobs, int rec_len, RowsLayout* out);
// the shared form's wave region on top of the row layout (rows_layout.cpp)
void cmpc_pair_layout(const cmpc_dims& d, const RowsLayout& R, int nd, int rec_len, int off_x, PairLayout* out);
// Shared form of the row build (build_pair.hip), launched by
// cmpc_launch_build_rows when P.use_pair is set; -1: no instance
int cmpc_launch_build_pair(const BuildParams& P, const cmpc_dims& d, void* stream);
// modelled extra LDS cycles per wave-step of the horizon loop for one wave
double cmpc_rows_layout_conflicts(const cmpc_dims& d, int nd, const RowsLayout& R, int wave);
int cmpc_launch_solve(const SolveParams& P, int nV, int nu, int nVo,
                      void* stream);
// Row-layout iterate kernel (solve_rows.hip): one QP per 16-lane row
int cmpc_launch_solve_rows(const SolveParams& P, int nV, int nu, int nVo, void* stream);
int cmpc_launch_qp_batch(const QpBatchParams& P, int n, int nu, void* stream);
int cmpc_launch_qp_batch_map(const QpBatchParams& P, int n, int nu, int nvo, void* stream);
// the (n, nu[, nvo]) the two launchers above have instances for
bool cmpc_qp_batch_supported(int n, int nu);
bool cmpc_qp_batch_map_supported(int n, int nu, int nvo);
// Plant simulation (sim.hip)
struct SimParams {
  double* x;              // B * ns
  double* dt;             // B (controlled stepper's step, carried between intervals)
  const double* u_full;   // B * n_inputs
  int32_t* status;        // B or null (1: step-size control failed)
  int B;
  double t, t_end, eps_abs, eps_rel, p_in, p_out;
};
// Per-scenario boundary pressures (cmpc_sim_set/bind_pressures, DESIGN.md
// §3.14): the sim kernel's per-scenario instances take SimParams and the
// array.  Its own struct, so that the scalar instances' arguments stay what
// they are.
struct SimParamsP : SimParams {
  const double* pressures;  // B * 2, [p_in, p_out] per scenario, 16-byte aligned
};
struct SimInputParams {
  const double* u_control;  // B * nc
  const double* u_offset;   // B * ni
  double* u_full;           // B * ni
  double* ring;             // ring_len * B, slot-major: slot k of every scenario is contiguous
  int B, nc, ni, ring_len, use_delay;
  int delay[CMPC_MAX_INPUTS];
  int cidx[CMPC_MAX_INPUTS];
  int cur[CMPC_MAX_INPUTS];  // ring slot of each delayed input (the same for every scenario)
};
struct AccumParams {
  const double* du;   // nqp * nV
  double* u_control;  // B * nu_tot
  int B, S, nu, nu_tot, nV;
  int order[CMPC_MAX_S_PRODUCE][CMPC_MAX_INPUTS];
};
int cmpc_launch_accumulate(const AccumParams& P, void* stream);
int cmpc_launch_sim(const SimParams& P, int plant, void* stream);
int cmpc_launch_sim_pressures(const SimParamsP& P, int plant, void* stream);  // -1 without the array
int cmpc_launch_sim_input(const SimInputParams& P, void* stream);
int cmpc_launch_sim_output(int plant, const double* x, double* y, int B, void* stream);
// Plant equilibrium (equilibrium.hip, cmpc_sim_equilibrium)
struct EquilibriumParams {
  double* x;                  // B * ns, in and out (written where the status is CMPC_EQ_OK)
  const double* u_full;       // B * n_inputs
  const int32_t* sim_status;  // B or null: nonzero leaves the scenario alone (CMPC_EQ_SKIPPED)
  const double* pressures;    // B * 2, [p_in, p_out] per scenario, 16-byte aligned; null: p_in, p_out
  int32_t* status;            // B: CMPC_EQ_*
  int32_t* iters;             // B
  double* resid;              // B
  int B, max_iter;
  double tol, p_in, p_out;
};
// four scenarios per wave; -1: unknown plant, max_iter outside [0, 64] or a null array
int cmpc_launch_equilibrium(const EquilibriumParams& P, int plant, void* stream);
// Steady-state target solve (target.hip, cmpc_sim_target)
struct TargetParams {
  double* x;                  // B * ns, in and out (written where the status is CMPC_EQ_OK)
  double* u_full;             // B * n_inputs: the free entries written where the status is CMPC_EQ_OK
  double* u_offset;           // B * n_inputs: likewise, moved by the same amount
  const double* targets;      // B * nh (null when nh = 0)
  const int32_t* sim_status;  // B or null: nonzero leaves the scenario alone (CMPC_EQ_SKIPPED)
  const double* pressures;    // B * 2, [p_in, p_out] per scenario, 16-byte aligned; null: p_in, p_out
  int32_t* status;            // B: CMPC_EQ_*
  int32_t* iters;             // B
  double* resid;              // B * 2: (r_f, r_y)
  int B, max_iter, nh;
  int32_t hold[4], fre[4];    // held plant outputs, free control inputs (the first nh of each)
  double tol_f, tol_y, p_in, p_out;
};
// four scenarios per wave; -1: unknown plant, max_iter outside [0, 64], nh
// outside [0, 4], an index outside [0, 4) or a null array
int cmpc_launch_target(const TargetParams& P, int plant, void* stream);
// Steady-state gains, RGA and pressure feed-forward (gains.hip, cmpc_sim_gains)
struct GainsParams {
  const double* x;            // B * ns, read only
  const double* u_full;       // B * n_inputs, read only
  const int32_t* sim_status;  // B or null: nonzero gives CMPC_EQ_SKIPPED
  const double* pressures;    // B * 2, [p_in, p_out] per scenario, 16-byte aligned; null: p_in, p_out
  double* record;             // B * CMPC_GAIN_LEN
  int32_t* status;            // B: CMPC_EQ_* or CMPC_GAIN_SINGULAR_G
  int B, ny, nu;
  int32_t out[4], in[4];      // selected plant outputs and control inputs (the first ny and nu)
  double p_in, p_out;
};
// four scenarios per wave; -1: unknown plant, ny or nu outside [1, 4], an index
// outside [0, 4) or a null array
int cmpc_launch_gains(const GainsParams& P, int plant, void* stream);
// Plant frequency responses (freq.hip, cmpc_sim_freq)
struct FreqParams {
  const double* x;            // B * ns, read only
  const double* u_full;       // B * n_inputs, read only
  const int32_t* sim_status;  // B or null: nonzero gives CMPC_EQ_SKIPPED
  const double* pressures;    // B * 2, [p_in, p_out] per scenario, 16-byte aligned; null: p_in, p_out
  const double* omega;        // nw frequencies (device), the same for every scenario
  double* record;             // B * nw * CMPC_FREQ_LEN
  double* summary;            // B * CMPC_FREQ_NSUM
  int32_t* status;            // B: CMPC_EQ_*
  int B, ny, nu, nw;
  int32_t out[4], in[4];      // selected plant outputs and control inputs (the first ny and nu)
  double p_in, p_out;
};
// four scenarios per wave; -1: unknown plant, ny or nu outside [1, 4], nw
// outside [1, CMPC_FREQ_MAX_NW], an index outside [0, 4) or a null array
int cmpc_launch_freq(const FreqParams& P, int plant, void* stream);
// Eigenvalues and plant modes (eig.hip, cmpc_eig_device, cmpc_sim_modes)
struct EigParams {
  const double* A;   // B * n * n, row-major blocks
  double *wr, *wi;   // B * n
  int32_t* status;   // B: CMPC_EIG_*
  int32_t* iters;    // B
  int B, max_iter;
};
struct ModesParams {
  const double* x;            // B * ns, read only
  const double* u_full;       // B * n_inputs
  const int32_t* sim_status;  // B or null: nonzero gives CMPC_EIG_SKIPPED
  const double* pressures;    // B * 2, [p_in, p_out] per scenario, 16-byte aligned; null: p_in, p_out
  double *wr, *wi;            // B * ns
  double* summary;            // B * CMPC_MODES_NSUM
  int32_t* status;            // B: CMPC_EIG_*
  int32_t* iters;             // B
  int B, max_iter;
  double p_in, p_out;
};
// four matrices per wave; -1: n not 10 or 11, an unknown plant, max_iter outside
// [1, CMPC_EIG_MAX_ITER] or a null array
int cmpc_launch_eig(const EigParams& P, int n, void* stream);
int cmpc_launch_modes(const ModesParams& P, int plant, void* stream);

int cmpc_launch_produce(const ProduceParams& P, int plant, void* stream);
int cmpc_obs_prior_shape(int n_aug, int nd, int nu_tot);
bool cmpc_obs_supported(int ns, int n_out, int ndist, int n_aug, int nd, int nu_tot);
int cmpc_launch_observer(const ObserverParams& P, int mode, void* stream);
int cmpc_launch_coupled(const CoupledParams& P, int n, int nu, void* stream);
