// Plant equilibrium on the device (cmpc_sim_equilibrium):
// Newton's method per scenario with the arithmetic of equilibrium_body.h.
//
// Four scenarios per wave, one per 16-lane row, one wave per workgroup.  Lanes
// 0 and 1 of a row (lane 0 alone for the serial plant) run the scalar plant
// model into the row's LDS region, as the record producer does
// (produce_body.h).  Lane j <= ns then holds column j of [A | -f] in
// registers: the pivot search of elimination step k is private to lane k, which
// hands the pivot row's index and the ns - k - 1 multipliers to the row; every
// lane updates its own column, and the row interchange is a chain of unrolled
// selects (eq_swap), so no column leaves the registers.  The right-hand side
// is back-substituted in lane ns from the other lanes' columns.
//
// The wave stays converged: a row that has its status, a skipped scenario and
// a row past the batch run the same instructions and store nothing.  The
// Newton loop ends after max_iter + 1 passes at the latest.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cmpc_internal.h"
#include "equilibrium_body.h"

namespace {
using namespace cmpc_eq;

// LDS hand-offs inside one wave: order the stores before the other lanes'
// loads (compiler and hardware, wavefront scope)
#define WAVE_SYNC()                                           \
  do {                                                        \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");    \
    __builtin_amdgcn_wave_barrier();                          \
  } while (0)

constexpr int kSpw = 4;            // scenarios per wave: one per 16-lane row
constexpr int kLanes = 64 / kSpw;  // lanes per scenario
// per scenario: A 121, B 44, C 44 (written by the plant model, not read), f 11,
// x 11, u 9, the parallel plant's tank terms 4
constexpr int kA = 0, kB = 121, kC = kB + 44, kF = kC + 44, kX = kF + 11, kU = kX + 11, kTk = kU + 9;
constexpr int kScnLds = kTk + 4;
constexpr int kPending = -1;  // a row still iterating

template <int PLANT, bool SCP>
__global__ __launch_bounds__(64) void cmpc_equilibrium_kernel(EquilibriumParams P) {
  constexpr int ns = Dims<PLANT>::ns, ni = Dims<PLANT>::ni;
  static_assert(ns + 1 <= kLanes, "one lane per column of [A | -f]");
  __shared__ double lds[kSpw * kScnLds];
  const int lane = threadIdx.x, g = lane / kLanes, l = lane - g * kLanes, base = lane - l;
  const int b = blockIdx.x * kSpw + g;
  const bool valid = b < P.B;
  double* const w = lds + g * kScnLds;
  double *A = w + kA, *Bc = w + kB, *Cc = w + kC, *fc = w + kF, *xs = w + kX, *us = w + kU, *tk = w + kTk;

  // a scenario whose integration has failed (the simulator's sticky status)
  // is left alone
  const bool skip = valid && P.sim_status && P.sim_status[b] != 0;
  double p_in = P.p_in, p_out = P.p_out;
  if (SCP && valid) {
    const double2 pr = reinterpret_cast<const double2*>(P.pressures)[b];
    p_in = pr.x;
    p_out = pr.y;
  }
  if (l < ns) xs[l] = valid ? P.x[(size_t)b * ns + l] : 0.0;
  if (l < ni) us[l] = valid ? P.u_full[(size_t)b * ni + l] : 0.0;
  // the plant model writes the same nonzeros of A in every pass: clear once
  for (int e = l; e < ns * ns; e += kLanes) A[e] = 0.0;
  WAVE_SYNC();

  int st = !valid ? CMPC_EQ_OK : skip ? CMPC_EQ_SKIPPED : kPending;
  int iters = 0;
  double resid = 0.0;
  for (int it = 0; it <= P.max_iter; ++it) {
    const bool act = st == kPending;  // the same in the 16 lanes of a row
    if (__ballot(act) == 0) break;    // wave-uniform
    // the scalar plant model, four scenarios side by side (produce_row's
    // split of the parallel plant).  Inlined by request: left as a call inside
    // the loop, serial_linearize spills and reads its arguments through flat
    // addresses
    if (PLANT == CMPC_PLANT_PARALLEL) {
      if (act && l < 2)
        [[clang::always_inline]] cmpc_plant::parallel_linearize_part(l, p_in, xs, us, A, Bc, Cc, fc, tk);
      WAVE_SYNC();
      if (act && l == 0)
        [[clang::always_inline]] cmpc_plant::parallel_linearize_tank(p_out, xs, us, A, Cc, fc, tk);
    } else if (act && l == 0) {
      [[clang::always_inline]] cmpc_plant::serial_linearize(p_in, p_out, xs, us, A, Bc, Cc, fc, false);
    }
    WAVE_SYNC();

    double col[ns];  // column l of [A | -f]; zero in the lanes past it
#pragma unroll
    for (int i = 0; i < ns; ++i) col[i] = l < ns ? A[i * ns + l] : l == ns ? -fc[i] : 0.0;
    const unsigned long long badm = __ballot(!eq_finite<ns>(col));
    const bool bad = ((badm >> base) & 0xffffull) != 0;
    const double r = __shfl(eq_resid<ns>(col), base + ns, 64);
    if (act) {
      iters = it;
      resid = r;
      st = bad ? CMPC_EQ_NONFINITE : r <= P.tol ? CMPC_EQ_OK : it == P.max_iter ? CMPC_EQ_NO_CONVERGENCE : kPending;
    }

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
    // back substitution of the right-hand side, lane ns: column k of the
    // triangle comes from lane k, whose registers stay as they are
    const bool rhs = l == ns;
#pragma unroll
    for (int k = ns - 1; k >= 0; --k) {
      const double dk = eq_step(col[k], __shfl(col[k], base + k, 64));
      col[k] = rhs ? dk : col[k];
#pragma unroll
      for (int i = 0; i < k; ++i) {
        const double v = eq_elim(col[i], __shfl(col[i], base + k, 64), dk);
        col[i] = rhs ? v : col[i];
      }
    }
    if (st == kPending && singular) st = CMPC_EQ_SINGULAR;
    if (st == kPending && l == ns) {
#pragma unroll
      for (int i = 0; i < ns; ++i) xs[i] = xs[i] + col[i];
    }
    WAVE_SYNC();
  }

  if (!valid) return;
  // every status but OK leaves the state as it was on entry
  if (st == CMPC_EQ_OK && l < ns) P.x[(size_t)b * ns + l] = xs[l];
  if (l == 0) {
    P.status[b] = st;
    P.iters[b] = iters;
    P.resid[b] = resid;
  }
}

template <bool SCP>
int launch(const EquilibriumParams& P, int plant, hipStream_t s) {
  const int grid = (P.B + kSpw - 1) / kSpw;
  if (plant == CMPC_PLANT_PARALLEL)
    cmpc_launch(cmpc_equilibrium_kernel<CMPC_PLANT_PARALLEL, SCP>, dim3(grid), dim3(64), 0, s, P);
  else if (plant == CMPC_PLANT_SERIAL)
    cmpc_launch(cmpc_equilibrium_kernel<CMPC_PLANT_SERIAL, SCP>, dim3(grid), dim3(64), 0, s, P);
  else
    return -1;
  return 0;
}

}  // namespace

int cmpc_launch_equilibrium(const EquilibriumParams& P, int plant, void* stream) {
  if (P.B <= 0) return 0;
  if (P.max_iter < 0 || P.max_iter > kMaxIter) return -1;
  if (!P.x || !P.u_full || !P.status || !P.iters || !P.resid) return -1;
  return P.pressures ? launch<true>(P, plant, (hipStream_t)stream) : launch<false>(P, plant, (hipStream_t)stream);
}
