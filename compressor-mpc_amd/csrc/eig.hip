// Eigenvalues of small real matrices and the plant's modes on the device
// (cmpc_eig_device, cmpc_sim_modes), with the arithmetic of
// eig_body.h.
//
// Four matrices per wave, one per 16-lane row, one wave per workgroup.  The
// matrix lives in the row's LDS region.  In the reduction and in each QR sweep
// lane j applies the current reflector to column j (from the left) and, after
// a wavefront-scope fence, to row j (from the right).  Every lane of a row
// computes the reflector, the shifts and the deflation window from the same
// LDS entries with the same operations and keeps its own copy of the counts,
// so the sixteen copies agree and nothing is handed over.
//
// The wave stays converged: a row that has its status, a skipped scenario and
// a row past the batch run the same instructions and store nothing in LDS;
// the loops leave on a wave-uniform ballot or at their bound.
//
// cmpc_modes_kernel first runs the scalar plant model into the row's region as
// the equilibrium kernel does (equilibrium.hip), then analyses A.  It reads x
// and does not write it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cmpc_internal.h"
#include "eig_body.h"
#include "equilibrium_body.h"

namespace {
using namespace cmpc_eig;

constexpr int kSpw = 4;            // matrices per wave: one per 16-lane row
constexpr int kLanes = 64 / kSpw;  // lanes per matrix
constexpr int kMat = kMaxN * kMaxN;
constexpr int kRowLds = kMat + kWork;  // the matrix, the roots

// results of one matrix; sm: the summary or null
template <int N>
__device__ __forceinline__ void store_results(const double* ev, int l, size_t b, int st, int iters, double* wr,
                                              double* wi, double* sm, int32_t* status, int32_t* it_out) {
  if (l < N) {
    wr[b * N + l] = ev[kSwr + l];
    wi[b * N + l] = ev[kSwi + l];
  }
  if (sm) {
    double s[CMPC_MODES_NSUM];
    eig_summary(N, ev + kSwr, ev + kSwi, st == CMPC_EIG_OK, s);
    if (l == 0) {
#pragma unroll
      for (int k = 0; k < CMPC_MODES_NSUM; ++k) sm[b * CMPC_MODES_NSUM + k] = s[k];
    }
  }
  if (l == 0) {
    status[b] = st;
    it_out[b] = iters;
  }
}

template <int N>
__global__ __launch_bounds__(64) void cmpc_eig_kernel(EigParams P) {
  static_assert(N <= kLanes, "one lane per column");
  __shared__ double lds[kSpw * kRowLds];
  const int lane = threadIdx.x, g = lane / kLanes, l = lane - g * kLanes;
  const int b = blockIdx.x * kSpw + g;
  const bool valid = b < P.B;
  double* const A = lds + g * kRowLds;
  double* const ev = A + kMat;
  for (int e = l; e < N * N; e += kLanes) A[e] = valid ? P.A[(size_t)b * (N * N) + e] : 0.0;
  EIG_SYNC();
  const Lanes L = {l, l < N ? l + 1 : l, l == 0};
  int32_t iters = 0;
  const int st = eig_run<N>(A, ev, L, valid ? kPending : CMPC_EIG_SKIPPED, P.max_iter, &iters);
  if (!valid) return;
  store_results<N>(ev, l, (size_t)b, st, iters, P.wr, P.wi, nullptr, P.status, P.iters);
}

// per scenario, as equilibrium.hip: A 121, B 44, C 44 (written by the plant
// model, not read), f 11, x 11, u 9, the parallel plant's tank terms 4; then
// the roots
constexpr int kA = 0, kB = 121, kC = kB + 44, kF = kC + 44, kX = kF + 11, kU = kX + 11, kTk = kU + 9;
constexpr int kEv = kTk + 4, kScnLds = kEv + kWork;

template <int PLANT, bool SCP>
__global__ __launch_bounds__(64) void cmpc_modes_kernel(ModesParams P) {
  constexpr int ns = cmpc_eq::Dims<PLANT>::ns, ni = cmpc_eq::Dims<PLANT>::ni;
  static_assert(ns <= kLanes, "one lane per column");
  __shared__ double lds[kSpw * kScnLds];
  const int lane = threadIdx.x, g = lane / kLanes, l = lane - g * kLanes;
  const int b = blockIdx.x * kSpw + g;
  const bool valid = b < P.B;
  double* const w = lds + g * kScnLds;
  double *A = w + kA, *Bc = w + kB, *Cc = w + kC, *fc = w + kF, *xs = w + kX, *us = w + kU, *tk = w + kTk;

  // a scenario whose integration has failed (the simulator's sticky status)
  // is not analysed
  const bool skip = valid && P.sim_status && P.sim_status[b] != 0;
  const bool act = valid && !skip;
  double p_in = P.p_in, p_out = P.p_out;
  if (SCP && valid) {
    const double2 pr = reinterpret_cast<const double2*>(P.pressures)[b];
    p_in = pr.x;
    p_out = pr.y;
  }
  if (l < ns) xs[l] = valid ? P.x[(size_t)b * ns + l] : 0.0;
  if (l < ni) us[l] = valid ? P.u_full[(size_t)b * ni + l] : 0.0;
  // the plant model writes only the nonzeros of A
  for (int e = l; e < ns * ns; e += kLanes) A[e] = 0.0;
  EIG_SYNC();
  // the scalar plant model, four scenarios side by side (inlined by request,
  // as in the equilibrium kernel)
  if (PLANT == CMPC_PLANT_PARALLEL) {
    if (act && l < 2) [[clang::always_inline]] cmpc_plant::parallel_linearize_part(l, p_in, xs, us, A, Bc, Cc, fc, tk);
    EIG_SYNC();
    if (act && l == 0) [[clang::always_inline]] cmpc_plant::parallel_linearize_tank(p_out, xs, us, A, Cc, fc, tk);
  } else if (act && l == 0) {
    [[clang::always_inline]] cmpc_plant::serial_linearize(p_in, p_out, xs, us, A, Bc, Cc, fc, false);
  }
  EIG_SYNC();

  const Lanes L = {l, l < ns ? l + 1 : l, l == 0};
  int32_t iters = 0;
  const int st = eig_run<ns>(A, w + kEv, L, act ? kPending : CMPC_EIG_SKIPPED, P.max_iter, &iters);
  if (!valid) return;
  store_results<ns>(w + kEv, l, (size_t)b, st, iters, P.wr, P.wi, P.summary, P.status, P.iters);
}

template <bool SCP>
int launch_modes(const ModesParams& P, int plant, hipStream_t s) {
  const int grid = (P.B + kSpw - 1) / kSpw;
  if (plant == CMPC_PLANT_PARALLEL)
    cmpc_launch(cmpc_modes_kernel<CMPC_PLANT_PARALLEL, SCP>, dim3(grid), dim3(64), 0, s, P);
  else if (plant == CMPC_PLANT_SERIAL)
    cmpc_launch(cmpc_modes_kernel<CMPC_PLANT_SERIAL, SCP>, dim3(grid), dim3(64), 0, s, P);
  else
    return -1;
  return 0;
}

}  // namespace

int cmpc_launch_eig(const EigParams& P, int n, void* stream) {
  if (P.B <= 0) return 0;
  if (P.max_iter < 1 || P.max_iter > kMaxIter) return -1;
  if (!P.A || !P.wr || !P.wi || !P.status || !P.iters) return -1;
  const int grid = (P.B + kSpw - 1) / kSpw;
  if (n == 10)
    cmpc_launch(cmpc_eig_kernel<10>, dim3(grid), dim3(64), 0, (hipStream_t)stream, P);
  else if (n == 11)
    cmpc_launch(cmpc_eig_kernel<11>, dim3(grid), dim3(64), 0, (hipStream_t)stream, P);
  else
    return -1;
  return 0;
}

int cmpc_launch_modes(const ModesParams& P, int plant, void* stream) {
  if (P.B <= 0) return 0;
  if (P.max_iter < 1 || P.max_iter > kMaxIter) return -1;
  if (!P.x || !P.u_full || !P.wr || !P.wi || !P.summary || !P.status || !P.iters) return -1;
  return P.pressures ? launch_modes<true>(P, plant, (hipStream_t)stream)
                     : launch_modes<false>(P, plant, (hipStream_t)stream);
}
