// Steady-state target solve on the device (cmpc_sim_target):
// the bordered Newton iteration of target_body.h per scenario.
//
// Four scenarios per wave, one per 16-lane row, one wave per workgroup, as in
// the equilibrium kernel (equilibrium.hip).  Lanes 0 and 1 of a row (lane 0
// alone for the serial plant) run the scalar plant model into the row's LDS
// region; lane 0 adds the plant output.  With N = ns + 4, lane j < ns then
// holds column j of [A; C_hold] in registers, lanes ns .. ns + 3 the free B
// columns over a zero block (the unit column for an unused border), and lane N
// the right-hand side [-f; t - y].  The elimination is the equilibrium
// kernel's on N rows: lane k searches its pivot and hands the row index and the
// multipliers to the row, every lane updates its own column, and the row
// interchange is a chain of unrolled selects (eq_swap).  The zero block makes
// an interchange with a border row part of every solve.
//
// hold and fre are the same for every scenario (kernel arguments): they select
// LDS rows and columns at run time, and a lane finds its own entry of fre by
// unrolled selects, so nothing indexed lives in registers.
//
// The wave stays converged: a row that has its status, a skipped scenario and
// a row past the batch run the same instructions and store nothing.  The
// Newton loop ends after max_iter + 1 passes at the latest.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cmpc_internal.h"
#include "target_body.h"

namespace {
using namespace cmpc_eq;
using namespace cmpc_tg;

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
// terms 4, y 4, the targets 4
constexpr int kA = 0, kB = 121, kC = kB + 44, kF = kC + 44, kX = kF + 11, kU = kX + 11, kTk = kU + 9,
              kY = kTk + 4, kT = kY + 4;
constexpr int kScnLds = kT + 4;
constexpr int kPending = -1;  // a row still iterating

template <int PLANT, bool SCP>
__global__ __launch_bounds__(64) void cmpc_target_kernel(TargetParams P) {
  constexpr int ns = Dims<PLANT>::ns, ni = Dims<PLANT>::ni, N = ns + kMaxHold;
  static_assert(ns + 4 + 1 <= kLanes, "one lane per column of the bordered system and one for its right-hand side");
  __shared__ double lds[kSpw * kScnLds];
  const int lane = threadIdx.x, g = lane / kLanes, l = lane - g * kLanes, base = lane - l;
  const int b = blockIdx.x * kSpw + g;
  const bool valid = b < P.B;
  const int nh = P.nh;
  double* const w = lds + g * kScnLds;
  double *A = w + kA, *Bc = w + kB, *Cc = w + kC, *fc = w + kF, *xs = w + kX, *us = w + kU, *tk = w + kTk,
         *ys = w + kY, *ts = w + kT;

  // a scenario whose integration has failed (the simulator's sticky status)
  // is left alone
  const bool skip = valid && P.sim_status && P.sim_status[b] != 0;
  double p_in = P.p_in, p_out = P.p_out;
  if (SCP && valid) {
    const double2 pr = reinterpret_cast<const double2*>(P.pressures)[b];
    p_in = pr.x;
    p_out = pr.y;
  }
  // this lane's border column c = l - ns: its free input, when it has one
  const int c = l - ns;
  const bool border = c >= 0 && c < kMaxHold;
  int myfree = 0;
#pragma unroll
  for (int j = 0; j < kMaxHold; ++j) myfree = c == j ? P.fre[j] : myfree;
  const bool freecol = border && c < nh;

  if (l < ns) xs[l] = valid ? P.x[(size_t)b * ns + l] : 0.0;
  if (l < ni) us[l] = valid ? P.u_full[(size_t)b * ni + l] : 0.0;
  if (l < kMaxHold) {
    ts[l] = valid && l < nh ? P.targets[(size_t)b * nh + l] : 0.0;
    ys[l] = 0.0;
  }
  // the plant model writes the same nonzeros of A, B and C in every pass:
  // clear once (the three areas are contiguous)
  for (int e = l; e < kF; e += kLanes) w[e] = 0.0;
  WAVE_SYNC();

  int st = !valid ? CMPC_EQ_OK : skip ? CMPC_EQ_SKIPPED : kPending;
  int iters = 0;
  double resid_f = 0.0, resid_y = 0.0;
  for (int it = 0; it <= P.max_iter; ++it) {
    if (__ballot(st == kPending) == 0) break;  // wave-uniform
    // a free recycle valve below the dead-zone bound: the same in the 16 lanes
    if (st == kPending && tg_deadzone(nh, P.fre, us)) {
      st = CMPC_EQ_DEADZONE;
      iters = it;
    }
    const bool act = st == kPending;
    // the scalar plant model, four scenarios side by side, inlined by request
    // (equilibrium.hip has the reason)
    if (PLANT == CMPC_PLANT_PARALLEL) {
      if (act && l < 2)
        [[clang::always_inline]] cmpc_plant::parallel_linearize_part(l, p_in, xs, us, A, Bc, Cc, fc, tk);
      WAVE_SYNC();
      if (act && l == 0) {
        [[clang::always_inline]] cmpc_plant::parallel_linearize_tank(p_out, xs, us, A, Cc, fc, tk);
        cmpc_plant::parallel_output(xs, ys);
      }
    } else if (act && l == 0) {
      [[clang::always_inline]] cmpc_plant::serial_linearize(p_in, p_out, xs, us, A, Bc, Cc, fc, false);
      cmpc_plant::serial_output(xs, ys);
    }
    WAVE_SYNC();

    double col[N];  // this lane's column of the bordered system; zero in an idle lane
#pragma unroll
    for (int i = 0; i < ns; ++i)
      col[i] = l < ns ? A[i * ns + l] : freecol ? Bc[i * 4 + myfree] : l == N ? -fc[i] : 0.0;
#pragma unroll
    for (int r = 0; r < kMaxHold; ++r) {
      const bool held = r < nh;           // wave-uniform
      const int h = held ? P.hold[r] : 0; // wave-uniform
      col[ns + r] = l < ns   ? (held ? Cc[h * ns + l] : 0.0)
                    : l == N ? (held ? ts[r] - ys[h] : 0.0)
                             : (border && !freecol && c == r ? 1.0 : 0.0);
    }
    const unsigned long long badm = __ballot(!eq_finite<N>(col));
    const bool bad = ((badm >> base) & 0xffffull) != 0;
    const double rf = __shfl(eq_resid<ns>(col), base + N, 64);
    const double ry = __shfl(eq_resid<kMaxHold>(col + ns), base + N, 64);
    if (act) {
      iters = it;
      resid_f = rf;
      resid_y = ry;
      st = bad                                   ? CMPC_EQ_NONFINITE
           : (rf <= P.tol_f && ry <= P.tol_y)    ? CMPC_EQ_OK
           : it == P.max_iter                    ? CMPC_EQ_NO_CONVERGENCE
                                                 : kPending;
    }

    bool singular = false;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      // lane k's search; its answer to the row
      int p = eq_pivot<N>(col, k);
      double pv = 0.0;
#pragma unroll
      for (int i = 0; i < N; ++i) pv = i == p ? col[i] : pv;
      p = __shfl(p, base + k, 64);
      singular = singular || __shfl((int)eq_bad_pivot(pv), base + k, 64) != 0;
      eq_swap<N>(col, k, p);
#pragma unroll
      for (int i = k + 1; i < N; ++i) {
        const double m = __shfl(eq_mult(col[i], col[k]), base + k, 64);
        col[i] = eq_elim(col[i], m, col[k]);
      }
    }
    // back substitution of the right-hand side, lane N: column k of the
    // triangle comes from lane k, whose registers stay as they are
    const bool rhs = l == N;
#pragma unroll
    for (int k = N - 1; k >= 0; --k) {
      const double dk = eq_step(col[k], __shfl(col[k], base + k, 64));
      col[k] = rhs ? dk : col[k];
#pragma unroll
      for (int i = 0; i < k; ++i) {
        const double v = eq_elim(col[i], __shfl(col[i], base + k, 64), dk);
        col[i] = rhs ? v : col[i];
      }
    }
    if (st == kPending && singular) st = CMPC_EQ_SINGULAR;
    if (st == kPending && rhs) {
#pragma unroll
      for (int i = 0; i < ns; ++i) xs[i] = xs[i] + col[i];
#pragma unroll
      for (int j = 0; j < kMaxHold; ++j) {
        if (j < nh) {
          const int pi = plant_input(P.fre[j]);
          us[pi] = us[pi] + col[ns + j];
        }
      }
    }
    WAVE_SYNC();
  }

  if (!valid) return;
  // every status but OK leaves state, plant input and offset as they were
  if (st == CMPC_EQ_OK) {
    if (l < ns) P.x[(size_t)b * ns + l] = xs[l];
    if (l < nh) {
      int fl = 0;
#pragma unroll
      for (int j = 0; j < kMaxHold; ++j) fl = l == j ? P.fre[j] : fl;
      const size_t e = (size_t)b * ni + plant_input(fl);
      // the offset moves with the plant input: what the delay line and the
      // controller have added on top of it stays
      const double v = us[plant_input(fl)], above = P.u_full[e] - P.u_offset[e];
      P.u_full[e] = v;
      P.u_offset[e] = v - above;
    }
  }
  if (l == 0) {
    P.status[b] = st;
    P.iters[b] = iters;
    P.resid[2 * (size_t)b] = resid_f;
    P.resid[2 * (size_t)b + 1] = resid_y;
  }
}

template <bool SCP>
int launch(const TargetParams& P, int plant, hipStream_t s) {
  const int grid = (P.B + kSpw - 1) / kSpw;
  if (plant == CMPC_PLANT_PARALLEL)
    cmpc_launch(cmpc_target_kernel<CMPC_PLANT_PARALLEL, SCP>, dim3(grid), dim3(64), 0, s, P);
  else if (plant == CMPC_PLANT_SERIAL)
    cmpc_launch(cmpc_target_kernel<CMPC_PLANT_SERIAL, SCP>, dim3(grid), dim3(64), 0, s, P);
  else
    return -1;
  return 0;
}

}  // namespace

int cmpc_launch_target(const TargetParams& P, int plant, void* stream) {
  if (P.B <= 0) return 0;
  if (P.max_iter < 0 || P.max_iter > kMaxIter) return -1;
  if (P.nh < 0 || P.nh > kMaxHold) return -1;
  for (int j = 0; j < P.nh; ++j)
    if (P.hold[j] < 0 || P.hold[j] >= 4 || P.fre[j] < 0 || P.fre[j] >= 4) return -1;
  if (!P.x || !P.u_full || !P.u_offset || !P.status || !P.iters || !P.resid || (P.nh > 0 && !P.targets)) return -1;
  return P.pressures ? launch<true>(P, plant, (hipStream_t)stream) : launch<false>(P, plant, (hipStream_t)stream);
}
