// Kernel selection (host only, no HIP call): the dimension checks, the
// launch parameters that follow from the dimensions, the availability of
// every kernel family and the policy that picks among them.  cmpc_abi.cpp
// takes a plan from here and launches what it names; cmpc_plan() answers
// the same question without a device.
#include "dispatch.h"

#include <algorithm>
#include <cmath>
#include <cstring>

// ---------------------------------------------------------------------------
// dimensions
// ---------------------------------------------------------------------------
const char* cmpc_layout_error(const cmpc_dims* d, cmpc_layout* L) {
  if (!d || !L) return "null argument";
  if (d->ns < 1 || d->ns > CMPC_MAX_NS || d->nu_tot < 1 || d->nu_tot > CMPC_MAX_INPUTS ||
      d->nu < 1 || d->nu > d->nu_tot || d->ny < 1 || d->p < 1 || d->m < 1 || d->m > d->p ||
      d->m * d->nu > CMPC_MAX_NV || d->ndist < 0 || d->S < 1 || d->B < 1)
    return "invalid dimensions";
  std::memset(L, 0, sizeof *L);
  for (int i = 0; i < d->nu_tot; ++i) {
    if (d->delay[i] < 0) return "negative delay";
    if (d->delay[i]) L->nd++;
    L->n_delay_states += d->delay[i];
  }
  L->naug = d->ndist + L->n_delay_states;
  L->nobs = d->ns + d->ndist;
  L->ntot = L->nobs + L->n_delay_states;
  L->nV = d->m * d->nu;
  L->nuo = d->nu_tot - d->nu;
  L->nVo = d->m * L->nuo;
  L->off_A = 0;
  L->off_B = d->ns * d->ns;
  L->off_C = L->off_B + d->ns * d->nu_tot;
  L->off_f = L->off_C + d->ny * L->nobs;
  L->off_x = L->off_f + d->ns;
  L->off_y = L->off_x + L->naug;
  L->rec_len = ((L->off_y + d->ny) + 7) / 8 * 8;
  return nullptr;
}

const char* cmpc_context_dims_error(const cmpc_dims& d, const cmpc_layout& L) {
  if (64 % d.S != 0) return "S must divide the wavefront size (64)";
  // S sub-controllers share the inputs (nu_tot = S nu), or S = 1 with
  // nu < nu_tot: one stand-alone sub-controller whose other controllers'
  // plans come with every cmpc_get_input (DistributedController::GetInput)
  if (L.nuo != (d.S - 1) * d.nu && d.S != 1)
    return "nu_tot must equal S * nu (each sub-controller owns nu inputs), or S = 1";
  if (L.nd > CMPC_ND_MAX) return "more than 4 delayed inputs";
  // A one-step delay with several delayed inputs: the reference's BComposite
  // (libs/aug_lin_sys.cc:189-197) places such an input at index
  // n_delayed_inputs + (sum of the earlier blocks' D - 1) - 1 of the
  // augmented state, which is another input's delay state (only a single
  // delayed input gets its own slot).  That mapping is not reproduced.
  for (int i = 0; i < d.nu_tot; ++i)
    if (d.delay[i] == 1 && L.nd > 1)
      return "a delay of one step with several delayed inputs: the reference's BComposite "
             "maps it onto another input's delay state (aug_lin_sys.cc:189-197); not supported";
  if (d.ns + d.nu_tot > 15) return "ns + nu_tot must be <= 15 (16-lane DPP rows)";
  if (d.m * d.nu_tot + 1 > 16) return "m * nu_tot + 1 must be <= 16 (gather lanes of a DPP row)";
  if (d.ny > 4) return "ny > 4 is not instantiated in the build kernel (one DPP row per output)";
  if (d.ns + d.ny + L.nd > 16) return "ns + ny + (delayed inputs) must be <= 16 (free-response DPP row)";
  if ((long long)d.B * d.S > (1LL << 30)) return "batch too large";
  return nullptr;
}

// ---------------------------------------------------------------------------
// the output weight's factor
// ---------------------------------------------------------------------------
// ywt = L_W L_W' (Cholesky; zero pivots allowed for PSD weights), stored as
// lwt = L_W' (upper triangular, row-major).  The one place it is computed: the
// shared weights (rebuild_cfg) and the per-slot ones (cmpc_set_scenario_weights)
// go through it, so equal ywt give bitwise equal lwt.
const char* cmpc_weight_factor_error(int ny, const double* W, double* lwt) {
  if (ny < 1 || ny > 4 || !W || !lwt) return "weight factor: ny must be 1..4 and the arrays non-null";
  double Lw[16] = {0};
  double scale = 0;
  for (int i = 0; i < ny * ny; ++i) scale = std::max(scale, std::fabs(W[i]));
  for (int i = 0; i < ny; ++i)
    for (int j = 0; j < ny; ++j)
      if (std::fabs(W[i * ny + j] - W[j * ny + i]) > 1e-12 * (1 + scale)) return "ywt must be symmetric";
  for (int j = 0; j < ny; ++j) {
    double dd = W[j * ny + j];
    for (int k = 0; k < j; ++k) dd -= Lw[j * ny + k] * Lw[j * ny + k];
    if (dd < -1e-12 * (1 + scale)) return "ywt must be positive semi-definite";
    if (dd <= 1e-14 * (1 + scale)) continue;  // zero column
    const double ljj = std::sqrt(dd);
    Lw[j * ny + j] = ljj;
    for (int i = j + 1; i < ny; ++i) {
      double v = W[i * ny + j];
      for (int k = 0; k < j; ++k) v -= Lw[i * ny + k] * Lw[j * ny + k];
      Lw[i * ny + j] = v / ljj;
    }
  }
  for (int o = 0; o < ny; ++o)
    for (int o2 = 0; o2 < ny; ++o2) lwt[o * ny + o2] = Lw[o2 * ny + o];
  return nullptr;
}

// ---------------------------------------------------------------------------
// launch parameters that follow from the dimensions
// ---------------------------------------------------------------------------
// LDS layout of the build kernel (doubles; must match cmpc_kernels.hip).
// Bank model (MI355X_MICROARCH.md §LDS): ds_read_b64 is serviced per 32-lane
// group with 32 double-wide banks, ds_write_b64 per 16-lane group with 16.
// Per step the gather lanes of rows 0/1 (one read group) read lines at
// line_off[c] + (m-1-k) + r - D_c and row o's Markov lanes write at
// line_off[c] + m - 1 + r.  Lines (length m - 1 + p) are placed so that input
// c's read window sits at residues [m*pi(c), m*pi(c) + m) mod 32 and the
// write residues are distinct mod 16; rows are 16 mod 32 apart so row 1's
// window is disjoint from row 0's.  All addresses advance together, so a
// layout that is conflict-free at one step is conflict-free at every step.
static void build_lds_layout(const cmpc_dims& d, const cmpc_layout& L, BuildParams* P) {
  const int nut = d.nu_tot, M = d.m, ng = M * nut + 1;
  auto up = [](int v, int a) { return (v + a - 1) / a * a; };
  auto place = [&](const int* perm, int* off) {  // returns total length
    int cur = 0;
    for (int c = 0; c < nut; ++c) {
      const int want = (((M * perm[c] + d.delay[c]) % 32) + 32) % 32;
      int o = cur;
      while (((o % 32) + 32) % 32 != want) ++o;
      off[c] = o;
      cur = o + M - 1 + d.p;
    }
    return cur;
  };
  int perm[CMPC_MAX_INPUTS], best[CMPC_MAX_INPUTS], off[CMPC_MAX_INPUTS];
  for (int c = 0; c < nut; ++c) perm[c] = best[c] = c;
  int best_len = -1;
  do {  // permutations of the read windows: first one whose writes are conflict-free
    const int len = place(perm, off);
    bool ok = true;
    for (int a = 0; a < nut && ok; ++a)
      for (int b = a + 1; b < nut && ok; ++b)
        ok = (off[a] - off[b]) % 16 != 0;
    if (ok && (best_len < 0 || len < best_len)) {
      best_len = len;
      for (int c = 0; c < nut; ++c) best[c] = perm[c];
    }
  } while (std::next_permutation(perm, perm + nut));
  const int len = place(best, off);
  for (int c = 0; c < nut; ++c) P->line_off[c] = off[c];
  int rs = up(len, 2);
  while (rs % 32 != 16) rs += 2;
  P->line_rs = rs;
  const int head = L.rec_len + 8 + d.ny * L.nobs + 4;  // record, u_old, C_hat, kappa
  int o = std::max(std::max(d.ny * rs, (d.ny - 1) * ng * L.nV), head);
  o = up(o, 32) + 16;                                   // w table at 16 mod 32
  P->w_off = o;
  o += up((d.p + 3) * d.ny, 2);
  while (o % 32 != (M * nut) % 32) o += 2;               // z slots next to row 0's window
  P->zs_off = o;
  if (d.ny == 4) {
    // pre-pass z lines: stride = 1 mod 32, so row o's z read sits at residue
    // m*nu_tot + o (between the line windows of rows o and o+1 at 0 / 16 mod 32)
    // and the four writes of a step hit distinct banks
    int zst = d.p;
    while (zst % 32 != 1) ++zst;
    P->zl_stride = zst;
    o += d.ny * zst;
  } else {
    P->zl_stride = 4;
    o += d.ny * 4;
  }
  P->lds_per_wave = up(o, 32);
  P->yl_stride = up((d.p + 1) * d.ny, 32);
  P->lds_block = up(d.S * P->yl_stride + d.S * d.ny * d.ny + d.S * d.nu * d.nu + 16, 32);
  // loop segments: the distinct delays inside the horizon, ascending
  P->nbound = 0;
  for (int c = 0; c < nut; ++c) {
    const int D = d.delay[c];
    if (D <= 0 || D >= d.p) continue;
    bool seen = false;
    for (int i = 0; i < P->nbound; ++i) seen = seen || P->bound[i] == D;
    if (!seen) P->bound[P->nbound++] = D;
  }
  std::sort(P->bound, P->bound + P->nbound);
}

const char* cmpc_dispatch_params(const cmpc_dims& d, const cmpc_layout& L, int nqp, int cus, BuildParams* Pp) {
  BuildParams& P = *Pp;
  std::memset(&P, 0, sizeof P);
  P.nqp = nqp;
  // workgroups needed at one QP per wave; the persistent build caps it at the
  // resident workgroups (occupancy x CUs), so no workgroup waits for a second round
  P.cus = cus;
  P.grid = std::max(1, (nqp + CMPC_BUILD_WAVES - 1) / CMPC_BUILD_WAVES);
  P.S = d.S;
  P.p = d.p;
  P.nu_tot = d.nu_tot;
  P.ndist = d.ndist;
  P.nd = L.nd;
  P.rec_len = L.rec_len;
  P.qp_len = cmpc_qp_len(L);
  P.off_A = L.off_A; P.off_B = L.off_B; P.off_C = L.off_C;
  P.off_f = L.off_f; P.off_x = L.off_x; P.off_y = L.off_y;
  P.nobs = L.nobs;
  int kd = 0, boff = d.ndist + L.nd, dmax = 1;
  for (int i = 0; i < d.nu_tot; ++i) {
    P.delay[i] = d.delay[i];
    P.dindex[i] = -1;
    if (d.delay[i] > 0 && kd < CMPC_ND_MAX) {
      P.dindex[i] = kd;
      P.dinput[kd] = i;
      P.dlen[kd] = d.delay[i];
      P.boff[kd] = boff;
      boff += d.delay[i] - 1;
      dmax = std::max(dmax, d.delay[i]);
      ++kd;
    }
  }
  P.dmax = dmax;
  build_lds_layout(d, L, &P);
  if (L.rec_len > 2 * 64 * CMPC_REC_CHUNKS) return "lin record too long for the build kernel";
  if (sizeof(double) * ((size_t)P.lds_block + (size_t)P.lds_per_wave * CMPC_BUILD_WAVES) > kLdsLimitBytes)
    return "horizon/delays too long for the build kernel's LDS";
  cmpc_rows_layout(d, L.nd, L.nobs, L.rec_len, &P.rows);  // cached per dimension set
  cmpc_pair_layout(d, P.rows, L.nd, L.rec_len, L.off_x, &P.pair);
  return nullptr;
}

// ---------------------------------------------------------------------------
// availability
// ---------------------------------------------------------------------------
namespace {

#define CMPC_DIMS_ARE(NS_, NY_, NU_, M_) if (d.ns == NS_ && d.ny == NY_ && d.nu == NU_ && d.m == M_) return true;
#define CMPC_DIMS_IN(name, LIST)                                            \
  bool name(const cmpc_dims& d, const BuildParams& P) {                     \
    if (P.nd != CMPC_DIMS_ND || P.nu_tot != CMPC_DIMS_NUT) return false;    \
    LIST(CMPC_DIMS_ARE)                                                     \
    return false;                                                           \
  }
CMPC_DIMS_IN(in_build_wave, CMPC_FOR_BUILD_WAVE)
CMPC_DIMS_IN(in_build_rows, CMPC_FOR_BUILD_ROWS)
CMPC_DIMS_IN(in_step_wave_row, CMPC_FOR_STEP_WAVE_ROW)
CMPC_DIMS_IN(in_step_wave_lane, CMPC_FOR_STEP_WAVE_LANE)
CMPC_DIMS_IN(in_step_rows_row, CMPC_FOR_STEP_ROWS_ROW)
CMPC_DIMS_IN(in_step_rows_lane, CMPC_FOR_STEP_ROWS_LANE)
CMPC_DIMS_IN(in_control_cent, CMPC_FOR_CONTROL_CENT)
CMPC_DIMS_IN(in_control_dist, CMPC_FOR_CONTROL_DIST)
#undef CMPC_DIMS_IN
#undef CMPC_DIMS_ARE

bool in_solve(int nV, int nu, int nVo) {
#define CMPC_SOLVE_IS(N_, NU_, NVO_) if (nV == N_ && nu == NU_ && nVo == NVO_) return true;
  CMPC_FOR_SOLVE(CMPC_SOLVE_IS)
#undef CMPC_SOLVE_IS
  return false;
}

// a layout exists and the row kernel has an instance for its segments: the
// plain (no ring) kernels unroll over the two delays' bounds
bool rows_layout_usable(const RowsLayout& R) { return R.ok && (rows_has_ring(R) || R.nseg <= 2 * CMPC_DIMS_ND); }

bool rows_lds_fits(const RowsLayout& R, int wpg) {
  return sizeof(double) * ((size_t)R.lds_block + (size_t)R.per_wave * wpg) <= kLdsLimitBytes;
}

// the fused wave-kernel row solver's factor areas beside the build's lines
bool wave_row_solver_fits(const cmpc_dims& d, const BuildParams& P) {
  const int nV = d.nu * d.m;
  return P.lds_per_wave >= d.ny * (d.m * 4 + 1) * nV + 4 * nV * nV;
}

}  // namespace

bool cmpc_build_wave_available(const cmpc_dims& d, const BuildParams& P) { return in_build_wave(d, P); }

// per-slot weights: the SCW instances have no block-shared tables (yhat, L_W'
// and uwt are per wave), their block region is the zero slots alone
constexpr int kWeightsLdsBlock = 32;
static bool weights_lds_fits(int per_wave) {
  return sizeof(double) * ((size_t)kWeightsLdsBlock + (size_t)per_wave * CMPC_BUILD_WAVES) <= kLdsLimitBytes;
}

bool cmpc_build_weights_available(const cmpc_dims& d, const BuildParams& P) {
  return in_build_wave(d, P) && weights_lds_fits(P.lds_per_wave + cmpc_scenario_weights_region(d, P));
}

void cmpc_dispatch_params_weights(const cmpc_dims& d, const BuildParams& P, BuildParamsW* W) {
  static_cast<BuildParams&>(*W) = P;
  W->sc_w = nullptr;
  W->yref = nullptr;
  W->lds_block = kWeightsLdsBlock;
  W->tab_off = P.lds_per_wave;  // (a multiple of 32)
  W->lds_per_wave = P.lds_per_wave + cmpc_scenario_weights_region(d, P);
}

bool cmpc_build_weights_launchable(const cmpc_dims& d, const BuildParamsW& W) {
  return in_build_wave(d, W) && !W.split && W.lds_block == kWeightsLdsBlock && W.tab_off > 0 && W.tab_off % 2 == 0 &&
         W.lds_per_wave == W.tab_off + cmpc_scenario_weights_region(d, W) && weights_lds_fits(W.lds_per_wave);
}

extern "C" int cmpc_scenario_weights_available(const cmpc_dims* dims) {
  cmpc_layout L;
  if (!dims || cmpc_layout_error(dims, &L) || cmpc_context_dims_error(*dims, L)) return 0;
  BuildParams P;
  if (cmpc_dispatch_params(*dims, L, dims->B * dims->S, kCusFallback, &P)) return 0;
  return cmpc_build_weights_available(*dims, P) ? 1 : 0;
}

int cmpc_build_rows_waves(const cmpc_dims& d, const BuildParams& P) {
  if (!rows_layout_usable(P.rows) || !in_build_rows(d, P)) return 0;
  const int w = cmpc_rows_waves_per_group(P.rows);
  return (w == 4 || w == 2) && rows_lds_fits(P.rows, w) ? w : 0;
}

// CMPC_PAIRING_AUTO: the shared form from this many scenarios on.  It runs
// half the waves of the unpaired row build at two per SIMD instead of three,
// so it needs several groups per wave to gain (par-coop, row build forced,
// unpaired vs shared, three alternating rounds of 30 builds,
// profiles/pair_build_ab/sizes.txt): 4 096 scenarios (config 2's size) p = 50
// 25.0-26.1 vs 35.7-36.7 us and p = 20 14.8-15.3 vs 26.8-27.2 us, a loss: one
// group per SIMD; 16 384 scenarios 77.0-84.2 vs 76.7-80.0 us, level; 32 768
// scenarios 140-157 vs 128-138 us, the shared form ahead in every round;
// 65 536 (the headline) 268-315 vs 233-270 us, 0.87x in every round (in the
// bench's step loop 248 vs 224 us, profiles/pair_build_ab/README.md).
constexpr int kPairAutoScenarios = 32768;

// Shared form of the row build (build_pair_kernel.h): the two QPs of a
// cooperative scenario share one P chain.  What must hold per configuration;
// per scenario the kernel compares the two records' plants bit for bit and
// builds a group that differs the long way.
const char* cmpc_pairing_error(const cmpc_dims& d, const BuildParams& P, const double* lwt0, const double* lwt1) {
  if (d.S != 2 || d.nu_tot != 2 * d.nu)
    return "build pairing needs two sub-controllers that own half of the inputs each (S = 2, nu_tot = 2 nu)";
  for (int c = 0; c < d.nu_tot; ++c)
    if (d.delay[c] != d.delay[(c + d.nu) % d.nu_tot])
      return "build pairing: the input delays are not invariant under the rotation by nu (the sub-controllers' "
             "column orders)";
  if (lwt0 && lwt1 && std::memcmp(lwt0, lwt1, sizeof(double) * d.ny * d.ny) != 0)
    return "build pairing: the sub-controllers' output weights (lwt) are not bitwise equal";
  bool inst = false;
#define CMPC_PAIR_IS(NS_, NY_, NU_, M_) inst = inst || (d.ns == NS_ && d.ny == NY_ && d.nu == NU_ && d.m == M_);
  CMPC_FOR_BUILD_PAIR(CMPC_PAIR_IS)
#undef CMPC_PAIR_IS
  if (!inst || P.nd != CMPC_DIMS_ND || P.nu_tot != CMPC_DIMS_NUT)
    return "build pairing: no shared-form instance for these dimensions (ns, ny, nu, m; parallel coop only)";
  if (!cmpc_build_rows_available(d, P)) return "build pairing: the row build cannot run these dimensions";
  if (rows_has_ring(P.rows)) return "build pairing: the horizon needs ring hand-off lines (no ring instance)";
  if (!P.pair.ok)
    return "build pairing: the shared form's LDS region does not fit two workgroups per CU for this horizon";
  return nullptr;
}

bool cmpc_pairing_auto(int scenarios) { return scenarios >= kPairAutoScenarios; }

static const char* pairing_reason(const cmpc_dims* dims, const double* lwt0, const double* lwt1) {
  if (!dims) return "null argument";
  cmpc_layout L;
  if (const char* e = cmpc_layout_error(dims, &L)) return e;
  if (const char* e = cmpc_context_dims_error(*dims, L)) return e;
  BuildParams P;
  if (const char* e = cmpc_dispatch_params(*dims, L, dims->B * dims->S, kCusFallback, &P)) return e;
  return cmpc_pairing_error(*dims, P, lwt0, lwt1);
}

extern "C" const char* cmpc_build_pairing_reason(const cmpc_dims* dims, const double* lwt_s0, const double* lwt_s1) {
  const char* e = pairing_reason(dims, lwt_s0, lwt_s1);
  return e ? e : "";
}

extern "C" int cmpc_build_pairing_available(const cmpc_dims* dims, const double* lwt_s0, const double* lwt_s1) {
  return pairing_reason(dims, lwt_s0, lwt_s1) ? 0 : 1;
}

int cmpc_step_wave_solver(const cmpc_dims& d, const BuildParams& P) {
  if (P.grid * CMPC_BUILD_WAVES < P.nqp) return 0;  // one workgroup per four QPs, no persistent loop
  if (P.S == 1) return in_step_wave_row(d, P) && wave_row_solver_fits(d, P) ? CMPC_SOLVE_ROWS : 0;
  // the scenario's sub-controllers in adjacent waves of one workgroup
  return CMPC_BUILD_WAVES % P.S == 0 && in_step_wave_lane(d, P) ? CMPC_SOLVE_LANE : 0;
}

int cmpc_step_rows_solver(const cmpc_dims& d, const BuildParams& P) {
  const RowsLayout& R = P.rows;
  if (!rows_layout_usable(R) || P.S < 1 || 4 % P.S) return 0;
  // four-wave workgroups only (the solvers' state on top of the build's registers)
  if (cmpc_rows_waves_per_group(R) != 4 || !rows_lds_fits(R, 4)) return 0;
  const int nV = d.nu * d.m;
  if (in_step_rows_lane(d, P)) {
    // one QP per lane after the wave's groups: G / U columns in the wave's LDS
    // region, at most 16 groups per wave of the launch's two (WPE 2)
    // four-wave workgroups per CU, fewer if the LDS layout allows fewer; no
    // ring instances
    if (rows_has_ring(R) || R.per_wave < nV * nV * 64) return 0;
    if ((P.nqp + 3) / 4 > 16 * 4 * P.cus * std::min(2, cmpc_rows_resident_groups(R, 4))) return 0;
    return CMPC_SOLVE_LANE;
  }
  return in_step_rows_row(d, P) && R.per_wave >= 4 * nV * nV ? CMPC_SOLVE_ROWS : 0;
}

int cmpc_control_solver(const cmpc_dims& d, const BuildParams& P, bool split, int grid, bool trace, int pr_off) {
  const int slots = split ? CMPC_BUILD_WAVES / 2 : CMPC_BUILD_WAVES;  // QP slots per workgroup
  if (grid * slots < P.nqp || trace) return 0;
  const size_t lds = sizeof(double) * std::max((size_t)P.lds_block + (size_t)P.lds_per_wave * CMPC_BUILD_WAVES,
                                               (size_t)pr_off + 4 * kProduceRowLds);
  if (lds > kLdsLimitBytes) return 0;
  if (P.S == 1) return in_control_cent(d, P) && wave_row_solver_fits(d, P) ? CMPC_SOLVE_ROWS : 0;
  if (slots % P.S || !in_control_dist(d, P)) return 0;
  return split ? CMPC_SOLVE_ROWS : CMPC_SOLVE_LANE;  // pairs: the coop row solver, faster there
}

bool cmpc_solve_lane_available(int nV, int nu, int nVo, int qp_len, bool trace, bool du_other) {
  if (!in_solve(nV, nu, nVo) || qp_len != nV * nV + nV + nV * nVo) return false;
  return !du_other || (nVo != 0 && !trace);  // the other controllers' plans given: no trace instance
}

bool cmpc_solve_rows_available(int nV, int nu, int nVo, int S, int qp_len, bool trace, bool du_other) {
  // the plan exchange stays inside a wave's four rows
  return S >= 1 && 4 % S == 0 && cmpc_solve_lane_available(nV, nu, nVo, qp_len, trace, du_other);
}

bool cmpc_predict_instance(const cmpc_dims& d, const cmpc_layout& L) {
  if (L.nd != CMPC_DIMS_ND || d.nu_tot != CMPC_DIMS_NUT) return false;
#define CMPC_PREDICT_IS(NS_, NY_, NU_, M_) \
  if (d.ns == NS_ && d.ny == NY_ && d.nu == NU_ && d.m == M_) return true;
  CMPC_FOR_BUILD_WAVE(CMPC_PREDICT_IS)
#undef CMPC_PREDICT_IS
  return false;
}

extern "C" int cmpc_predict_available(const cmpc_dims* dims) {
  cmpc_layout L;
  if (cmpc_layout_error(dims, &L) || cmpc_context_dims_error(*dims, L)) return 0;
  return cmpc_predict_instance(*dims, L) ? 1 : 0;
}

bool cmpc_refshift_instance(const cmpc_dims& d, const cmpc_layout& L) {
  if (L.nd != CMPC_DIMS_ND || d.nu_tot != CMPC_DIMS_NUT) return false;
#define CMPC_REFSHIFT_IS(NS_, NY_, NU_, M_) \
  if (d.ns == NS_ && d.ny == NY_ && d.nu == NU_ && d.m == M_) return true;
  CMPC_FOR_BUILD_WAVE(CMPC_REFSHIFT_IS)
#undef CMPC_REFSHIFT_IS
  return false;
}

extern "C" int cmpc_reference_profile_available(const cmpc_dims* dims) {
  cmpc_layout L;
  if (cmpc_layout_error(dims, &L) || cmpc_context_dims_error(*dims, L)) return 0;
  return cmpc_refshift_instance(*dims, L) ? 1 : 0;
}

// ---------------------------------------------------------------------------
// the policy
// ---------------------------------------------------------------------------
namespace {

// Row build: from one row group (four QPs) per SIMD, ceil(nqp / 4) >= 4 cus.
// It is as fast or faster than the one-QP-per-wave kernel for every
// plant/controller type at p = 20, 50, 100, 200 once the batch gives it a wave
// per SIMD (tools/gpu_build_table.sh); below, the wave kernel
// has four times the waves (cent p = 200, 1 024 QPs: 0.026 vs 0.057 ms).
constexpr int kRowsFillGroupsPerCu = 4;
// Role-split build: up to one QP per SIMD, nqp <= 4 cus: two waves per QP
// (config 5: 28.1 -> 22.6 us, profiles/r5g_build_split_ab.txt).
constexpr int kSplitQpPerCu = 4;
// Row solve, nV >= 6: below CMPC_SOLVE_ROWS_MAX_QP QPs at any CU count (the
// lane kernel's nV = 8 solve is one long dependency chain per lane, 17 us for
// one solve of 1 024 QPs against 9 us in rows, tools/time_small.py).
// Row solve, nV < 6: up to four QPs per SIMD, nqp <= 16 cus (K = 9: 7.7-7.8 vs
// 9.7-9.9 us from 2 to 1 024 QPs, profiles/r5k_small_batch.txt; in the
// bench's step loop with the move applied 9.6-10.2 vs 11.6-12.1 us at 2 048
// and 4 096 QPs, p = 20, profiles/r6r_solver_variant_sweep.txt); the lane
// kernel above (8 192 QPs: 11.9 vs 17.5 us).
constexpr int kSolveRowsNvLong = 6;
constexpr int kSolveRowsSmallQpPerCu = 16;
// Fused step under AUTO: nV >= 6 steps above one and up to four QPs per CU,
// at p >= 50.  Below one per CU the role-split build and the iterate kernel
// are faster (cent-ser B = 1 21.8 vs 24.4 us); in the range fused wins by
// 2-3 % (config 5: 37.3 vs 38.1 us with the move; ser-cent p = 100 512 QPs
// 37.6 vs 38.4 us) but loses at p = 20 (15.0 vs 13.9 us), and above it the two
// launches win: 2 048 QPs 17.1 vs 28.3 us (par-cent p = 20) and 60.1 vs 73.0 us
// (ser-cent p = 100), 8 192 QPs 112 vs 135 us (par-cent p = 200)
// (tools/step_variant_ab.py, profiles/r6r_step_variant_sweep.txt; it costs
// 3 % at 4 096 QPs for p = 50 and 200).  nV = 4 steps are two launches at
// every size (coop-par 1 024 QPs 17.8 vs 18.6 us, config 2 26.4 vs 54.1 us;
// profiles/r5j_split_step_ab.txt, profiles/r5k_small_batch.txt).
constexpr int kFuseNvMin = 6;
constexpr int kFuseAboveQpPerCu = 1;
constexpr int kFuseUpToQpPerCu = 4;
constexpr int kFuseHorizonMin = 50;
// A fused step on the row kernel with the lane solver (nV <= 4) is left to
// the two launches unless FUSED is forced: measured faster (config 2:
// 32.0-32.2 vs 33.7-33.9 us back to back, profiles/r4i_small_batch.txt).
constexpr int kRowsLaneStepNvMax = 4;
// One-launch control step: up to four QPs per CU.  It wins there (config 5's
// cent-par p = 200 at 1 024 QPs 50.7 vs 58.6 us, coop-par p = 50 at 512 QPs
// 48.5 vs 49.5 us) and loses above (2 048 QPs: 75.2 vs 72.7 and 102.0 vs
// 73.0 us; tools/control_step_ab.py, profiles/r6r_control_step_ab.txt).
constexpr int kControlQpPerCu = 4;
// ... with its build as role-split pairs, two QP slots per workgroup, up to
// one QP per CU (cent-ser B = 1 build 17.7 -> 15.7 us).
constexpr int kControlSplitQpPerCu = 1;

}  // namespace

cmpc_plan_t cmpc_dispatch_plan(const cmpc_dims& d, const cmpc_layout& L, const BuildParams& P, int build_variant,
                               int solve_variant, int step_variant, int K, bool trace, bool du_other,
                               bool ref_profile, bool scenario_weights) {
  const int nqp = P.nqp, cus = P.cus;
  cmpc_plan_t pl;
  std::memset(&pl, 0, sizeof pl);

  // build
  const bool rows_fill = (nqp + 3) / 4 >= kRowsFillGroupsPerCu * cus;
  const bool want_rows_build = build_variant == CMPC_BUILD_ROWS || (build_variant == CMPC_BUILD_AUTO && rows_fill);
  if (scenario_weights) {
    // only the one-QP-per-wave kernel's SCW instances take per-slot weights
    if (build_variant == CMPC_BUILD_ROWS || build_variant == CMPC_BUILD_SPLIT)
      pl.build_error = CMPC_PLAN_WEIGHTS_NEED_WAVE;
    else if (!cmpc_build_weights_available(d, P))
      pl.build_error = CMPC_PLAN_NO_WEIGHTS_BUILD;
    else
      pl.build_kernel = CMPC_BUILD_WAVE;
  } else if (want_rows_build && cmpc_build_rows_available(d, P))
    pl.build_kernel = CMPC_BUILD_ROWS;
  else if (build_variant == CMPC_BUILD_ROWS)
    pl.build_error = CMPC_PLAN_NO_ROWS_BUILD;
  else if (!cmpc_build_wave_available(d, P))
    pl.build_error = CMPC_PLAN_NO_BUILD;
  else if (build_variant == CMPC_BUILD_SPLIT || (build_variant == CMPC_BUILD_AUTO && nqp <= kSplitQpPerCu * cus))
    pl.build_kernel = CMPC_BUILD_SPLIT;
  else
    pl.build_kernel = CMPC_BUILD_WAVE;

  // solve (a trace is recorded by iterations only)
  const bool solve_trace = trace && K > 0;
  const bool rows_small =
      L.nV >= kSolveRowsNvLong ? nqp < CMPC_SOLVE_ROWS_MAX_QP : nqp <= kSolveRowsSmallQpPerCu * cus;
  const bool want_rows_solve = solve_variant == CMPC_SOLVE_ROWS || (solve_variant == CMPC_SOLVE_AUTO && rows_small);
  if (want_rows_solve && cmpc_solve_rows_available(L.nV, d.nu, L.nVo, d.S, P.qp_len, solve_trace, du_other))
    pl.solve_kernel = CMPC_SOLVE_ROWS;
  else if (solve_variant == CMPC_SOLVE_ROWS)
    pl.solve_error = CMPC_PLAN_NO_ROWS_SOLVE;
  else if (!cmpc_solve_lane_available(L.nV, d.nu, L.nVo, P.qp_len, solve_trace, du_other))
    pl.solve_error = CMPC_PLAN_NO_SOLVE;
  else
    pl.solve_kernel = CMPC_SOLVE_LANE;

  // step: fused on the build kernel AUTO would pick (one QP per wave below a
  // row group per SIMD, else the row kernel), else the two launches above.
  // A fused kernel exchanges plans inside the scenario: every controller's
  // inputs must be in the context.
  const bool all_auto = step_variant == CMPC_STEP_AUTO && build_variant == CMPC_BUILD_AUTO &&
                        solve_variant == CMPC_SOLVE_AUTO;
  const bool own_plans = L.nuo == (d.S - 1) * d.nu;
  const bool auto_fuse = all_auto && L.nV >= kFuseNvMin && nqp > kFuseAboveQpPerCu * cus &&
                         nqp <= kFuseUpToQpPerCu * cus && d.p >= kFuseHorizonMin;
  pl.step_build_kernel = pl.build_kernel;
  pl.step_solve_kernel = pl.solve_kernel;
  if (ref_profile) {
    // the correction of f runs between the build and the solve
    if (step_variant == CMPC_STEP_FUSED) pl.step_error = CMPC_PLAN_PROFILE_NEEDS_SPLIT;
  } else if (scenario_weights) {
    // no fused instance takes per-slot weights
    if (step_variant == CMPC_STEP_FUSED) pl.step_error = CMPC_PLAN_WEIGHTS_NEED_SPLIT;
  } else if ((step_variant == CMPC_STEP_FUSED || auto_fuse) && K > 0 && own_plans) {
    const bool leave_rows_lane = rows_fill && L.nV <= kRowsLaneStepNvMax && step_variant == CMPC_STEP_AUTO;
    int kind = 0, solver = 0;
    if (!rows_fill && (solver = cmpc_step_wave_solver(d, P)))
      kind = CMPC_BUILD_WAVE;
    else if (!leave_rows_lane && (solver = cmpc_step_rows_solver(d, P)))
      kind = CMPC_BUILD_ROWS;
    if (kind) {
      pl.step_fused = 1;
      pl.step_build_kernel = kind;
      pl.step_solve_kernel = solver;
    } else if (step_variant == CMPC_STEP_FUSED) {
      pl.step_error = CMPC_PLAN_NO_FUSED_STEP;
    }
  }

  // control step: one launch (never traced), else the three calls
  pl.control_build_kernel = pl.step_build_kernel;
  pl.control_solve_kernel = pl.step_solve_kernel;
  if (K > 0 && !ref_profile && !scenario_weights && step_variant != CMPC_STEP_SPLIT && build_variant == CMPC_BUILD_AUTO &&
      solve_variant == CMPC_SOLVE_AUTO && nqp <= kControlQpPerCu * cus && own_plans) {
    const bool split = nqp <= kControlSplitQpPerCu * cus;
    const int grid = split ? std::max(1, (nqp + 1) / 2) : P.grid;
    if (const int solver = cmpc_control_solver(d, P, split, grid, false, cmpc_control_pr_off(d.S, L.rec_len, L.naug))) {
      pl.control_fused = 1;
      pl.control_build_kernel = split ? CMPC_BUILD_SPLIT : CMPC_BUILD_WAVE;
      pl.control_solve_kernel = solver;
      pl.control_grid = grid;
      pl.control_polled = grid == 1;  // one workgroup: its last store can flag completion
    }
  }
  return pl;
}

// ---------------------------------------------------------------------------
// the query entry point (cmpc.h)
// ---------------------------------------------------------------------------
extern "C" const char* cmpc_plan_error_string(int e) {
  switch (e) {
    case CMPC_PLAN_OK: return "";
    case CMPC_PLAN_NO_ROWS_BUILD: return "row-layout build kernel not available for these dimensions";
    case CMPC_PLAN_NO_BUILD: return "build kernel not instantiated for these dimensions (ns, ny, nu, m)";
    case CMPC_PLAN_NO_ROWS_SOLVE: return "row solve kernel not available for these dimensions (S must divide 4)";
    case CMPC_PLAN_NO_SOLVE: return "solve kernel not instantiated for these dimensions";
    case CMPC_PLAN_NO_FUSED_STEP: return "cmpc_step: no fused step kernel for these dimensions";
    case CMPC_PLAN_PROFILE_NEEDS_SPLIT:
      return "cmpc_step: a reference profile is in force (cmpc_set/bind_scenario_reference_profile): its "
             "correction of f runs between the build and the solve, so CMPC_STEP_FUSED cannot be forced";
    case CMPC_PLAN_WEIGHTS_NEED_WAVE:
      return "per-scenario weights are in force (cmpc_set/bind_scenario_weights): only the one-QP-per-wave build "
             "takes them, so CMPC_BUILD_ROWS and CMPC_BUILD_SPLIT cannot be forced";
    case CMPC_PLAN_WEIGHTS_NEED_SPLIT:
      return "cmpc_step: per-scenario weights are in force (cmpc_set/bind_scenario_weights): no fused kernel takes "
             "them, so CMPC_STEP_FUSED cannot be forced";
    case CMPC_PLAN_NO_WEIGHTS_BUILD:
      return "per-scenario weights: no one-QP-per-wave build instance for these dimensions (ns, ny, nu, m), or its "
             "LDS does not fit with the per-wave weight tables";
  }
  return "unknown plan error";
}

const char* cmpc_plan_or_error(const cmpc_dims* dims, int cus, int build_variant, int solve_variant,
                               int step_variant, int K, uint32_t flags, cmpc_plan_t* plan) {
  if (!dims || !plan) return "null argument";
  if (cus < 1 || K < 0) return "cmpc_plan: cus must be >= 1 and K >= 0";
  if (build_variant < CMPC_BUILD_AUTO || build_variant > CMPC_BUILD_SPLIT || solve_variant < CMPC_SOLVE_AUTO ||
      solve_variant > CMPC_SOLVE_ROWS || step_variant < CMPC_STEP_AUTO || step_variant > CMPC_STEP_FUSED)
    return "cmpc_plan: unknown variant";
  cmpc_layout L;
  if (const char* e = cmpc_layout_error(dims, &L)) return e;
  if (const char* e = cmpc_context_dims_error(*dims, L)) return e;
  BuildParams P;
  if (const char* e = cmpc_dispatch_params(*dims, L, dims->B * dims->S, cus, &P)) return e;
  *plan = cmpc_dispatch_plan(*dims, L, P, build_variant, solve_variant, step_variant, K, (flags & CMPC_TRACE) != 0,
                             (flags & CMPC_PLAN_DU_OTHER) != 0, (flags & CMPC_PLAN_REF_PROFILE) != 0,
                             (flags & CMPC_PLAN_SCENARIO_WEIGHTS) != 0);
  return nullptr;
}
