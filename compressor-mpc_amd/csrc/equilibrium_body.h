// Plant equilibrium by Newton's method (cmpc_plant_equilibrium_host,
// cmpc_sim_equilibrium): the arithmetic of one scenario,
// shared by the host entry point (abi_analysis.cpp) and the device kernel
// (equilibrium.hip).  Given the plant input u and the boundary pressures, find
// x with f(x, u, p) = 0, starting from the x given.
//
//   for it = 0, 1, ...:
//     A, f      the continuous linearisation at x (plant_model.h:
//               parallel_linearize / serial_linearize; B and C are not used,
//               so no transcendental enters)
//     r         max_i |f_i|, i ascending, a NaN entry left out (eq_resid)
//     NONFINITE an entry of f or A is not finite
//     OK        r <= tol: iters = it
//     NO_CONVERGENCE  it == max_iter
//     A d = -f  Gaussian elimination with partial pivoting on [A | -f], column
//               k = 0 .. ns - 1:
//                 pivot   the largest |a_ik| over i >= k, the lowest i on a
//                         tie (eq_pivot); rows k and pivot change places in
//                         every column
//                 SINGULAR  the pivot is zero or not finite
//                 m_i = a_ik / a_kk,  a_ij = a_ij - m_i a_kj  for i > k, j > k
//               back substitution by columns, k = ns - 1 .. 0:
//                 d_k = y_k / a_kk,  y_i = y_i - a_ik d_k  for i < k
//     x = x + d
// Every status but OK leaves x as it was on entry; resid is the last r, iters
// the iteration that returned.  Products, quotients and differences are
// separate operations in the order written (the tree builds with
// -ffp-contract=off), so host and device agree bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/cmpc.h"
#include "plant_model.h"

namespace cmpc_eq {

constexpr int kMaxIter = CMPC_EQ_MAX_ITER;  // the entry points refuse more

template <int PLANT>
struct Dims {
  static constexpr int ns = PLANT == CMPC_PLANT_PARALLEL ? 11 : 10;
  static constexpr int ni = PLANT == CMPC_PLANT_PARALLEL ? 9 : 8;
};

CMPC_PHD bool finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// every entry of a column of [A | -f] finite
template <int N>
CMPC_PHD bool eq_finite(const double* c) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < N; ++i) ok = ok && finite(c[i]);
  return ok;
}

// r = max_i |c_i| over the column -f
template <int N>
CMPC_PHD double eq_resid(const double* c) {
  double r = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double a = fabs(c[i]);
    r = a > r ? a : r;
  }
  return r;
}

// pivot row of elimination step k in column k
template <int N>
CMPC_PHD int eq_pivot(const double* c, int k) {
  int p = k;
  double best = fabs(c[k]);
#pragma unroll
  for (int i = 1; i < N; ++i) {
    const double a = fabs(c[i]);
    if (i > k && a > best) {
      best = a;
      p = i;
    }
  }
  return p;
}

CMPC_PHD bool eq_bad_pivot(double v) { return v == 0.0 || !finite(v); }
CMPC_PHD double eq_mult(double aik, double akk) { return aik / akk; }
CMPC_PHD double eq_elim(double aij, double m, double akj) { return aij - m * akj; }
CMPC_PHD double eq_step(double yk, double akk) { return yk / akk; }

// rows k and p of one column change places: unrolled selects, so that a
// column held in registers stays there
template <int N>
CMPC_PHD void eq_swap(double* c, int k, int p) {
  double ck = 0.0, cp = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    ck = i == k ? c[i] : ck;
    cp = i == p ? c[i] : cp;
  }
#pragma unroll
  for (int i = 0; i < N; ++i) c[i] = i == k ? cp : i == p ? ck : c[i];
}

template <int PLANT>
CMPC_PHD void eq_linearize(double p_in, double p_out, const double* x, const double* u, double* A, double* B,
                           double* C, double* f) {
  if (PLANT == CMPC_PLANT_PARALLEL)
    cmpc_plant::parallel_linearize(p_in, p_out, x, u, A, B, C, f);
  else
    cmpc_plant::serial_linearize(p_in, p_out, x, u, A, B, C, f);
}

// One scenario, start to finish (the host entry point's loop body): x in and
// out, the status returned.
template <int PLANT>
CMPC_PHD int eq_solve(double p_in, double p_out, const double* u, double* x, int max_iter, double tol,
                      int32_t* iters, double* resid) {
  constexpr int ns = Dims<PLANT>::ns;
  double xc[ns], A[ns * ns], B[ns * 4], C[4 * ns], f[ns];
  double col[ns + 1][ns];  // column j of [A | -f]
  for (int i = 0; i < ns; ++i) xc[i] = x[i];
  *resid = 0.0;
  for (int it = 0;; ++it) {
    *iters = it;
    eq_linearize<PLANT>(p_in, p_out, xc, u, A, B, C, f);
    bool ok = true;
    for (int j = 0; j <= ns; ++j) {
      for (int i = 0; i < ns; ++i) col[j][i] = j < ns ? A[i * ns + j] : -f[i];
      ok = eq_finite<ns>(col[j]) && ok;
    }
    *resid = eq_resid<ns>(col[ns]);
    if (!ok) return CMPC_EQ_NONFINITE;
    if (*resid <= tol) {
      for (int i = 0; i < ns; ++i) x[i] = xc[i];
      return CMPC_EQ_OK;
    }
    if (it == max_iter) return CMPC_EQ_NO_CONVERGENCE;
    for (int k = 0; k < ns; ++k) {
      const int p = eq_pivot<ns>(col[k], k);
      if (eq_bad_pivot(col[k][p])) return CMPC_EQ_SINGULAR;
      for (int j = k; j <= ns; ++j) eq_swap<ns>(col[j], k, p);
      for (int i = k + 1; i < ns; ++i) {
        const double m = eq_mult(col[k][i], col[k][k]);
        for (int j = k + 1; j <= ns; ++j) col[j][i] = eq_elim(col[j][i], m, col[j][k]);
      }
    }
    double* y = col[ns];
    for (int k = ns - 1; k >= 0; --k) {
      y[k] = eq_step(y[k], col[k][k]);
      for (int i = 0; i < k; ++i) y[i] = eq_elim(y[i], col[k][i], y[k]);
    }
    for (int i = 0; i < ns; ++i) xc[i] = xc[i] + y[i];
  }
}

}  // namespace cmpc_eq
