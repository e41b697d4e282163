// Steady-state target solve (cmpc_plant_target_host, cmpc_sim_target,
// DESIGN.md §3.21): the arithmetic of one scenario, shared by the host entry
// point (abi_analysis.cpp) and the device kernel (target.hip).  Given the boundary
// pressures, nh <= 4 held plant outputs with their targets t and as many free
// control inputs, find the state x and the free inputs with
//   f(x, u, p) = 0   and   y_h(x) = t_h  for the held outputs h,
// starting from the x and u given; the inputs that are not free stay.
//
// hold[j] is a plant output, fre[j] a column of the continuous B, that is
// control input fre[j] of the plant, plant input kPlantInput[fre[j]] (columns
// 0 and 2 are the torques, 1 and 3 the recycle valves).
//
//   for it = 0, 1, ...:
//     DEADZONE  a free recycle valve stands below 2e-2: the plant's recycle
//               flow jumps at 1e-2 and its B column is an approximation below
//               2e-2, so nothing iterates there
//     A, B, C, f  the continuous linearisation at (x, u); y the plant output
//     r_f, r_y  max_i |f_i| and max_j |t_j - y_hold[j]| (eq_resid's rule)
//     NONFINITE an entry of the bordered system is not finite
//     OK        r_f <= tol_f and r_y <= tol_y: iters = it
//     NO_CONVERGENCE  it == max_iter
//     [[A, B_free], [C_hold, 0]] d = [-f; t - y]
//               the elimination of equilibrium_body.h (eq_pivot, eq_swap,
//               eq_mult, eq_elim, eq_step) on ns + 4 rows: border row and
//               column j >= nh are the unit row and column with a zero
//               right-hand side, so one shape serves every nh
//     SINGULAR  a zero or non-finite pivot
//     x = x + d_x,  u_free = u_free + d_u
// Every status but OK leaves x and u as they were on entry; resid is the pair
// (r_f, r_y) of the last test, iters the iteration that returned.  With nh = 0
// the unit rows' multipliers are zero and the A block's arithmetic is
// eq_solve's: x, status and iters agree with it bit for bit.  exp() is reached
// only for a recycle valve that is not free and stands below 2e-2; its B
// column is computed and never read, so no transcendental enters a result.
#pragma once
#include "equilibrium_body.h"

namespace cmpc_tg {
using cmpc_eq::Dims;

constexpr int kMaxHold = 4;         // held outputs = free inputs, at most
constexpr double kDeadZone = 2e-2;  // Compressor::linearize's exact branch starts here

// plant input of control input c (both plants: ControlInputIndex)
CMPC_PHD int plant_input(int c) { return c == 0 ? 0 : c == 1 ? 3 : c == 2 ? 4 : 7; }
CMPC_PHD bool is_recycle(int c) { return (c & 1) != 0; }

template <int PLANT>
CMPC_PHD void tg_output(const double* x, double* y) {
  if (PLANT == CMPC_PLANT_PARALLEL)
    cmpc_plant::parallel_output(x, y);
  else
    cmpc_plant::serial_output(x, y);
}

// a free recycle valve below the dead-zone bound
CMPC_PHD bool tg_deadzone(int nh, const int32_t* fre, const double* u) {
  bool dz = false;
#pragma unroll
  for (int j = 0; j < kMaxHold; ++j)
    dz = dz || (j < nh && is_recycle(fre[j]) && u[plant_input(fre[j])] < kDeadZone);
  return dz;
}

// One scenario, start to finish (the host entry point's loop body): x and u
// in and out, the status returned.
template <int PLANT>
CMPC_PHD int tg_solve(double p_in, double p_out, int nh, const int32_t* hold, const int32_t* fre, const double* t,
                      double* u, double* x, int max_iter, double tol_f, double tol_y, int32_t* iters,
                      double* resid) {
  using namespace cmpc_eq;
  constexpr int ns = Dims<PLANT>::ns, ni = Dims<PLANT>::ni, N = ns + kMaxHold;
  double xc[ns], uc[ni], A[ns * ns], B[ns * 4], C[4 * ns], f[ns], y[4];
  double col[N + 1][N];  // column j of the bordered system, the right-hand side last
  for (int i = 0; i < ns; ++i) xc[i] = x[i];
  for (int i = 0; i < ni; ++i) uc[i] = u[i];
  resid[0] = resid[1] = 0.0;
  for (int it = 0;; ++it) {
    *iters = it;
    if (tg_deadzone(nh, fre, uc)) return CMPC_EQ_DEADZONE;
    eq_linearize<PLANT>(p_in, p_out, xc, uc, A, B, C, f);
    tg_output<PLANT>(xc, y);
    bool ok = true;
    for (int j = 0; j <= N; ++j) {
      const int c = j - ns;  // the border column, 0 <= c < 4
      for (int i = 0; i < ns; ++i)
        col[j][i] = j < ns ? A[i * ns + j] : j == N ? -f[i] : c < nh ? B[i * 4 + fre[c]] : 0.0;
      for (int r = 0; r < kMaxHold; ++r)
        col[j][ns + r] = j < ns   ? (r < nh ? C[hold[r] * ns + j] : 0.0)
                         : j == N ? (r < nh ? t[r] - y[hold[r]] : 0.0)
                                  : (c >= nh && c == r ? 1.0 : 0.0);
      ok = eq_finite<N>(col[j]) && ok;
    }
    resid[0] = eq_resid<ns>(col[N]);
    resid[1] = eq_resid<kMaxHold>(col[N] + ns);
    if (!ok) return CMPC_EQ_NONFINITE;
    if (resid[0] <= tol_f && resid[1] <= tol_y) {
      for (int i = 0; i < ns; ++i) x[i] = xc[i];
      for (int j = 0; j < nh; ++j) u[plant_input(fre[j])] = uc[plant_input(fre[j])];
      return CMPC_EQ_OK;
    }
    if (it == max_iter) return CMPC_EQ_NO_CONVERGENCE;
    for (int k = 0; k < N; ++k) {
      const int p = eq_pivot<N>(col[k], k);
      if (eq_bad_pivot(col[k][p])) return CMPC_EQ_SINGULAR;
      for (int j = k; j <= N; ++j) eq_swap<N>(col[j], k, p);
      for (int i = k + 1; i < N; ++i) {
        const double m = eq_mult(col[k][i], col[k][k]);
        for (int j = k + 1; j <= N; ++j) col[j][i] = eq_elim(col[j][i], m, col[j][k]);
      }
    }
    double* d = col[N];
    for (int k = N - 1; k >= 0; --k) {
      d[k] = eq_step(d[k], col[k][k]);
      for (int i = 0; i < k; ++i) d[i] = eq_elim(d[i], col[k][i], d[k]);
    }
    for (int i = 0; i < ns; ++i) xc[i] = xc[i] + d[i];
    for (int j = 0; j < nh; ++j) uc[plant_input(fre[j])] = uc[plant_input(fre[j])] + d[ns + j];
  }
}

}  // namespace cmpc_tg
