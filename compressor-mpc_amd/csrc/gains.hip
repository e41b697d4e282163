// Steady-state gains, RGA and pressure feed-forward on the device
// (cmpc_sim_gains): the arithmetic of gains_body.h per
// scenario.
//
// Four scenarios per wave, one per 16-lane row, one wave per workgroup, as in
// the target kernel (target.hip).  Lanes 0 and 1 of a row (lane 0 alone for the
// serial plant) run the scalar plant model into the row's LDS region; lanes 0
// to 3 then evaluate the plant's derivative at the four pressure points of the
// central difference, side by side, and lanes 0 .. ns - 1 difference them into
// E.  Lane j < ns holds column j of A^T (row j of A) in registers, lanes ns ..
// ns + 3 the selected rows of C (zero from ny on).  The elimination is the
// equilibrium kernel's on ns rows: lane k searches its pivot and hands the row
// index and the multipliers to the row, every lane updates its own column, the
// row interchange is a chain of unrolled selects (eq_swap), and the four
// right-hand lanes back-substitute together.  Lane ns + i then holds Z[:, i]
// and forms row i of G and of Gp against B and E in LDS.
//
// The second stage, G [X | K] = [I | -Gp], goes through LDS: lanes 0 .. 9 of
// the same row read their column of [G | I | -Gp] (gn_stage2), eliminate on
// four rows, lanes 4 .. 9 back-substitute, lane 4 + i writes row i of the RGA
// and lane 8 + k column k of K_ff.  The record is assembled in LDS and stored
// by the row's 16 lanes, the NaN entries chosen by gn_keep.
//
// out and in are the same for every scenario (kernel arguments): they select
// LDS rows and columns at run time, and a lane finds its own entry of out by
// unrolled selects, so nothing indexed lives in registers.
//
// The wave stays converged: a skipped scenario, one in the dead zone and a
// row past the batch run the same instructions on a cleared region; a row past
// the batch stores nothing.  Nothing of the simulator is written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cmpc_internal.h"
#include "gains_body.h"

namespace {
using namespace cmpc_eq;
using namespace cmpc_gn;

// LDS hand-offs inside one wave: order the stores before the other lanes'
// loads (compiler and hardware, wavefront scope)
#define WAVE_SYNC()                                           \
  do {                                                        \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");    \
    __builtin_amdgcn_wave_barrier();                          \
  } while (0)

constexpr int kSpw = 4;            // scenarios per wave: one per 16-lane row
constexpr int kLanes = 64 / kSpw;  // lanes per scenario
// per scenario: A 121, B 44, C 44, f 11, x 11, u 9, the parallel plant's tank
// terms 4, the derivative at the four pressure points 44, E 22, the record 49
constexpr int kA = 0, kB = 121, kC = kB + 44, kF = kC + 44, kX = kF + 11, kU = kX + 11, kTk = kU + 9,
              kD = kTk + 4, kE = kD + 44, kR = kE + 22;
constexpr int kScnLds = kR + kLen;

template <int PLANT, bool SCP>
__global__ __launch_bounds__(64) void cmpc_gains_kernel(GainsParams P) {
  constexpr int ns = Dims<PLANT>::ns, ni = Dims<PLANT>::ni;
  static_assert(ns + kMaxSel <= kLanes, "one lane per column of [A^T | C_sel^T]");
  static_assert(kCols2 <= kLanes && kLen <= 4 * kLanes, "the second stage and the record's store fit a row");
  __shared__ double lds[kSpw * kScnLds];
  const int lane = threadIdx.x, g = lane / kLanes, l = lane - g * kLanes, base = lane - l;
  const int b = blockIdx.x * kSpw + g;
  const bool valid = b < P.B;
  const int ny = P.ny, nu = P.nu;
  double* const w = lds + g * kScnLds;
  double *A = w + kA, *Bc = w + kB, *Cc = w + kC, *fc = w + kF, *xs = w + kX, *us = w + kU, *tk = w + kTk,
         *Dd = w + kD, *Es = w + kE, *R = w + kR;

  // a scenario whose integration has failed (the simulator's sticky status)
  // is left alone
  const bool skip = valid && P.sim_status && P.sim_status[b] != 0;
  double p_in = P.p_in, p_out = P.p_out;
  if (SCP && valid) {
    const double2 pr = reinterpret_cast<const double2*>(P.pressures)[b];
    p_in = pr.x;
    p_out = pr.y;
  }
  // this lane's right-hand column r = l - ns: its output, when it has one
  const int r = l - ns;
  const bool zlane = r >= 0 && r < kMaxSel;
  int myout = 0;
#pragma unroll
  for (int j = 0; j < kMaxSel; ++j) myout = (r == j && j < ny) ? P.out[j] : myout;
  const bool selrow = zlane && r < ny;

  // the plant model writes only the nonzeros of A, B and C: clear the region once
  for (int e = l; e < kScnLds; e += kLanes) w[e] = 0.0;
  WAVE_SYNC();
  if (l < ns) xs[l] = valid ? P.x[(size_t)b * ns + l] : 0.0;
  if (l < ni) us[l] = valid ? P.u_full[(size_t)b * ni + l] : 0.0;
  WAVE_SYNC();

  // a selected recycle valve below the dead-zone bound: the same in the 16 lanes
  const bool dz = gn_deadzone(nu, P.in, us);
  const bool act = valid && !skip && !dz;
  // the scalar plant model, four scenarios side by side, inlined by request
  // (equilibrium.hip has the reason)
  if (PLANT == CMPC_PLANT_PARALLEL) {
    if (act && l < 2)
      [[clang::always_inline]] cmpc_plant::parallel_linearize_part(l, p_in, xs, us, A, Bc, Cc, fc, tk);
    WAVE_SYNC();
    if (act && l == 0)
      [[clang::always_inline]] cmpc_plant::parallel_linearize_tank(p_out, xs, us, A, Cc, fc, tk);
  } else if (act && l == 0) {
    [[clang::always_inline]] cmpc_plant::serial_linearize(p_in, p_out, xs, us, A, Bc, Cc, fc, false);
  }
  // the derivative at p_in + h, p_in - h, p_out + h, p_out - h: lanes 0 .. 3
  if (act && l < 4) {
    double pi, po;
    gn_point(l, p_in, p_out, &pi, &po);
    [[clang::always_inline]] gn_derivative<PLANT>(pi, po, xs, us, Dd + l * ns);
  }
  WAVE_SYNC();
  if (l < ns) {
    Es[l * 2] = gn_diff(Dd[l], Dd[ns + l]);
    Es[l * 2 + 1] = gn_diff(Dd[2 * ns + l], Dd[3 * ns + l]);
  }
  WAVE_SYNC();

  double col[ns];  // this lane's column of [A^T | C_sel^T]; zero in an idle lane
  {
    const double* src = l < ns ? A + l * ns : Cc + myout * ns;
    const bool have = l < ns || selrow;
#pragma unroll
    for (int i = 0; i < ns; ++i) col[i] = have ? src[i] : 0.0;
  }
  // f, E and the selected columns of B by rows, lane l < ns its own
  bool fin = eq_finite<ns>(col);
  {
    const int row = l < ns ? l : 0;
    fin = fin && finite(fc[row]) && finite(Es[row * 2]) && finite(Es[row * 2 + 1]);
#pragma unroll
    for (int j = 0; j < kMaxSel; ++j) {
      const int c = j < nu ? P.in[j] : 0;  // wave-uniform
      fin = fin && (j >= nu || finite(Bc[row * 4 + c]));
    }
  }
  const unsigned long long badm = __ballot(!fin);
  const bool bad = ((badm >> base) & 0xffffull) != 0;
  const double rf = eq_resid<ns>(fc);

  bool singular = false;
#pragma unroll
  for (int k = 0; k < ns; ++k) {
    // lane k's search; its answer to the row
    int p = eq_pivot<ns>(col, k);
    double pv = 0.0;
#pragma unroll
    for (int i = 0; i < ns; ++i) pv = i == p ? col[i] : pv;
    p = __shfl(p, base + k, 64);
    singular = singular || __shfl((int)eq_bad_pivot(pv), base + k, 64) != 0;
    eq_swap<ns>(col, k, p);
#pragma unroll
    for (int i = k + 1; i < ns; ++i) {
      const double m = __shfl(eq_mult(col[i], col[k]), base + k, 64);
      col[i] = eq_elim(col[i], m, col[k]);
    }
  }
  // back substitution of the four right-hand columns, lanes ns .. ns + 3:
  // column k of the triangle comes from lane k, whose registers stay as they are
#pragma unroll
  for (int k = ns - 1; k >= 0; --k) {
    const double dk = eq_step(col[k], __shfl(col[k], base + k, 64));
    col[k] = zlane ? dk : col[k];
#pragma unroll
    for (int i = 0; i < k; ++i) {
      const double v = eq_elim(col[i], __shfl(col[i], base + k, 64), dk);
      col[i] = zlane ? v : col[i];
    }
  }
  // lane ns + i holds Z[:, i]: row i of G and of Gp
#pragma unroll
  for (int j = 0; j < kMaxSel; ++j) {
    const int c = j < nu ? P.in[j] : 0;  // wave-uniform
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < ns; ++k) acc = gn_acc(acc, col[k], Bc[k * 4 + c]);
    if (zlane) R[kG + r * 4 + j] = -acc;
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    double acc = 0.0;
#pragma unroll
    for (int m = 0; m < ns; ++m) acc = gn_acc(acc, col[m], Es[m * 2 + k]);
    if (zlane) R[kGp + r * 2 + k] = -acc;
  }
  if (l == 0) R[kRf] = rf;
  WAVE_SYNC();

  // the second stage on lanes 0 .. 9: column l of [G | I | -Gp], the identity
  // when the selection is not square (its results are not kept)
  const int n = ny == nu ? ny : 0;
  const bool lane2 = l < kCols2, rhs2 = l >= 4 && l < kCols2;
  double c2[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) c2[i] = lane2 ? gn_stage2(l, i, n, R) : 0.0;
  bool singular2 = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int p = eq_pivot<4>(c2, k);
    double pv = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) pv = i == p ? c2[i] : pv;
    p = __shfl(p, base + k, 64);
    singular2 = singular2 || __shfl((int)eq_bad_pivot(pv), base + k, 64) != 0;
    eq_swap<4>(c2, k, p);
#pragma unroll
    for (int i = k + 1; i < 4; ++i) {
      const double m = __shfl(eq_mult(c2[i], c2[k]), base + k, 64);
      c2[i] = eq_elim(c2[i], m, c2[k]);
    }
  }
#pragma unroll
  for (int k = 3; k >= 0; --k) {
    const double dk = eq_step(c2[k], __shfl(c2[k], base + k, 64));
    c2[k] = rhs2 ? dk : c2[k];
#pragma unroll
    for (int i = 0; i < k; ++i) {
      const double v = eq_elim(c2[i], __shfl(c2[i], base + k, 64), dk);
      c2[i] = rhs2 ? v : c2[i];
    }
  }
  // lane 4 + i holds X[:, i]: RGA[i][j] = G[i][j] X[j][i]; lane 8 + k holds K[:, k]
  if (l >= 4 && l < 8) {
#pragma unroll
    for (int j = 0; j < 4; ++j) R[kRga + (l - 4) * 4 + j] = R[kG + (l - 4) * 4 + j] * c2[j];
  }
  if (l >= 8 && l < kCols2) {
#pragma unroll
    for (int i = 0; i < 4; ++i) R[kKff + i * 2 + (l - 8)] = c2[i];
  }
  WAVE_SYNC();

  if (!valid) return;
  const int st = skip                       ? CMPC_EQ_SKIPPED
                 : dz                       ? CMPC_EQ_DEADZONE
                 : bad                      ? CMPC_EQ_NONFINITE
                 : singular                 ? CMPC_EQ_SINGULAR
                 : (ny == nu && singular2)  ? CMPC_GAIN_SINGULAR_G
                                            : CMPC_EQ_OK;
  double* const rec = P.record + (size_t)b * kLen;
  for (int e = l; e < kLen; e += kLanes) rec[e] = gn_keep(e, ny, nu, st) ? R[e] : gn_nan();
  if (l == 0) P.status[b] = st;
}

template <bool SCP>
int launch(const GainsParams& P, int plant, hipStream_t s) {
  const int grid = (P.B + kSpw - 1) / kSpw;
  if (plant == CMPC_PLANT_PARALLEL)
    cmpc_launch(cmpc_gains_kernel<CMPC_PLANT_PARALLEL, SCP>, dim3(grid), dim3(64), 0, s, P);
  else if (plant == CMPC_PLANT_SERIAL)
    cmpc_launch(cmpc_gains_kernel<CMPC_PLANT_SERIAL, SCP>, dim3(grid), dim3(64), 0, s, P);
  else
    return -1;
  return 0;
}

}  // namespace

int cmpc_launch_gains(const GainsParams& P, int plant, void* stream) {
  if (P.B <= 0) return 0;
  if (P.ny < 1 || P.ny > kMaxSel || P.nu < 1 || P.nu > kMaxSel) return -1;
  for (int j = 0; j < P.ny; ++j)
    if (P.out[j] < 0 || P.out[j] >= 4) return -1;
  for (int j = 0; j < P.nu; ++j)
    if (P.in[j] < 0 || P.in[j] >= 4) return -1;
  if (!P.x || !P.u_full || !P.record || !P.status) return -1;
  return P.pressures ? launch<true>(P, plant, (hipStream_t)stream) : launch<false>(P, plant, (hipStream_t)stream);
}
