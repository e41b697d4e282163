// Steady-state gains, relative gain array and pressure feed-forward
// (cmpc_plant_gains_host, cmpc_sim_gains): the arithmetic of
// one scenario, shared by the host entry point (abi_analysis.cpp) and the device
// kernel (gains.hip).  Given the state x, the plant input u and the boundary
// pressures p, ny plant outputs out[] and nu control inputs in[] (columns of
// the continuous B, as the target solve's free inputs):
//
//   DEADZONE  a selected recycle valve stands below 2e-2, where its B column
//             is the dead-zone approximation (target_body.h has the reason);
//             an unselected valve may stand anywhere, its column is not read
//   A, B, C, f  the continuous linearisation at (x, u, p); r_f = max_i |f_i|
//             (eq_resid), reported and not tested
//   E         ns x 2, the central difference of the plant's derivative in
//             p_in and in p_out with h = 2^-21:
//               E[:, k] = (f(p + h e_k) - f(p - h e_k)) / (2 h)
//   NONFINITE an entry of A, of the selected columns of B or rows of C, of f
//             or of E is not finite
//   A^T Z = C_sel^T  the elimination of equilibrium_body.h (eq_pivot, eq_swap,
//             eq_mult, eq_elim, eq_step) on ns rows and ns + 4 columns: column
//             j < ns is row j of A, columns ns .. ns + 3 the selected rows of
//             C (zero from ny on), each back-substituted
//   SINGULAR  a zero or non-finite pivot
//   G[i][j]  = -sum_k Z[k][i] B[k][in_j]     sums ascending from 0.0, product
//   Gp[i][k] = -sum_m Z[m][i] E[m][k]        then add, negated once
//   ny == nu = n:  G [X | K] = [I | -Gp] by the same routines on 4 rows and 10
//             columns, rows and columns of G from n on being the unit ones;
//             RGA[i][j] = G[i][j] X[j][i],  K_ff = K
//   SINGULAR_G  a zero or non-finite pivot there: G, Gp and r_f stand, RGA and
//             K_ff are NaN
//   ny != nu: RGA and K_ff are NaN, the status is OK
//
// The record (CMPC_GAIN_LEN doubles): G 4 x 4 row-major, Gp 4 x 2, RGA 4 x 4,
// K_ff 4 x 2, r_f.  An entry outside ny / nu, and every entry for a status
// other than OK and SINGULAR_G, is the quiet NaN 0x7ff8000000000000
// (gn_keep).  Products, sums and quotients are separate operations in the
// order written (the tree builds with -ffp-contract=off), so host and device
// agree bit for bit.  exp() is reached only for a recycle valve that is not
// selected; its B column is computed and never read.
#pragma once
#include "equilibrium_body.h"
#include "target_body.h"

namespace cmpc_gn {
using cmpc_eq::Dims;
using cmpc_tg::is_recycle;
using cmpc_tg::kDeadZone;
using cmpc_tg::plant_input;

constexpr int kMaxSel = 4;                      // outputs and inputs selected, at most
constexpr double kTwoStep = 0x1p-20;            // 2 h
constexpr double kStep = 0x1p-21;               // h of the pressure difference
constexpr int kLen = CMPC_GAIN_LEN;             // the record
constexpr int kG = 0, kGp = 16, kRga = 24, kKff = 40, kRf = 48;
constexpr int kCols2 = 10;                      // [G | I | -Gp]
constexpr uint64_t kNanBits = 0x7ff8000000000000ull;

CMPC_PHD double gn_nan() {
  const uint64_t u = kNanBits;
  double v;
  __builtin_memcpy(&v, &u, sizeof v);
  return v;
}

// a selected recycle valve below the dead-zone bound
CMPC_PHD bool gn_deadzone(int nu, const int32_t* in, const double* u) {
  bool dz = false;
#pragma unroll
  for (int j = 0; j < kMaxSel; ++j) dz = dz || (j < nu && is_recycle(in[j]) && u[plant_input(in[j])] < kDeadZone);
  return dz;
}

// pressure point e of the difference: p_in + h, p_in - h, p_out + h, p_out - h
CMPC_PHD void gn_point(int e, double p_in, double p_out, double* pi, double* po) {
  const double d = (e & 1) ? -kStep : kStep;
  *pi = e < 2 ? p_in + d : p_in;
  *po = e < 2 ? p_out : p_out + d;
}

template <int PLANT>
CMPC_PHD void gn_derivative(double p_in, double p_out, const double* x, const double* u, double* dx) {
  if (PLANT == CMPC_PLANT_PARALLEL)
    cmpc_plant::parallel_derivative(p_in, p_out, x, u, dx);
  else
    cmpc_plant::serial_derivative(p_in, p_out, x, u, dx);
}

CMPC_PHD double gn_diff(double fp, double fm) { return (fp - fm) / kTwoStep; }

// acc + a b of the two gain sums
CMPC_PHD double gn_acc(double acc, double a, double b) { return acc + a * b; }

// entry i of column j of the second stage's [G | I | -Gp], the unit border from n on
CMPC_PHD double gn_stage2(int j, int i, int n, const double* R) {
  if (j < 4) return (i < n && j < n) ? R[kG + i * 4 + j] : (i == j ? 1.0 : 0.0);
  if (j < 8) return i == j - 4 ? 1.0 : 0.0;
  return i < n ? -R[kGp + i * 2 + (j - 8)] : 0.0;
}

// entry e of the record stands (else it is the NaN)
CMPC_PHD bool gn_keep(int e, int ny, int nu, int st) {
  if (st != CMPC_EQ_OK && st != CMPC_GAIN_SINGULAR_G) return false;
  const int n = (ny == nu && st == CMPC_EQ_OK) ? ny : 0;
  if (e < kGp) return (e >> 2) < ny && (e & 3) < nu;
  if (e < kRga) return ((e - kGp) >> 1) < ny;
  if (e < kKff) return ((e - kRga) >> 2) < n && ((e - kRga) & 3) < n;
  if (e < kRf) return ((e - kKff) >> 1) < n;
  return true;
}

// One scenario into R (kLen doubles, every entry that gn_keep lets stand for
// the returned status is written); the status returned.
template <int PLANT>
CMPC_PHD int gn_body(double p_in, double p_out, int ny, const int32_t* out, int nu, const int32_t* in,
                     const double* u, const double* x, double* R) {
  using namespace cmpc_eq;
  constexpr int ns = Dims<PLANT>::ns, M = ns + kMaxSel;
  double A[ns * ns], B[ns * 4], C[4 * ns], f[ns], D[4][ns], E[ns * 2];
  double col[M][ns];  // column j of [A^T | C_sel^T]
  if (gn_deadzone(nu, in, u)) return CMPC_EQ_DEADZONE;
  eq_linearize<PLANT>(p_in, p_out, x, u, A, B, C, f);
  for (int e = 0; e < 4; ++e) {
    double pi, po;
    gn_point(e, p_in, p_out, &pi, &po);
    gn_derivative<PLANT>(pi, po, x, u, D[e]);
  }
  bool ok = eq_finite<ns>(f);
  for (int i = 0; i < ns; ++i) {
    E[i * 2] = gn_diff(D[0][i], D[1][i]);
    E[i * 2 + 1] = gn_diff(D[2][i], D[3][i]);
    ok = ok && finite(E[i * 2]) && finite(E[i * 2 + 1]);
    for (int j = 0; j < nu; ++j) ok = ok && finite(B[i * 4 + in[j]]);
  }
  for (int j = 0; j < M; ++j) {
    const int r = j - ns;
    for (int i = 0; i < ns; ++i) col[j][i] = j < ns ? A[j * ns + i] : r < ny ? C[out[r] * ns + i] : 0.0;
    ok = eq_finite<ns>(col[j]) && ok;
  }
  if (!ok) return CMPC_EQ_NONFINITE;
  R[kRf] = eq_resid<ns>(f);
  for (int k = 0; k < ns; ++k) {
    const int p = eq_pivot<ns>(col[k], k);
    if (eq_bad_pivot(col[k][p])) return CMPC_EQ_SINGULAR;
    for (int j = k; j < M; ++j) eq_swap<ns>(col[j], k, p);
    for (int i = k + 1; i < ns; ++i) {
      const double m = eq_mult(col[k][i], col[k][k]);
      for (int j = k + 1; j < M; ++j) col[j][i] = eq_elim(col[j][i], m, col[j][k]);
    }
  }
  for (int r = 0; r < kMaxSel; ++r) {
    double* z = col[ns + r];
    for (int k = ns - 1; k >= 0; --k) {
      z[k] = eq_step(z[k], col[k][k]);
      for (int i = 0; i < k; ++i) z[i] = eq_elim(z[i], col[k][i], z[k]);
    }
    for (int j = 0; j < kMaxSel; ++j) {
      const int c = j < nu ? in[j] : 0;
      double acc = 0.0;
      for (int k = 0; k < ns; ++k) acc = gn_acc(acc, z[k], B[k * 4 + c]);
      R[kG + r * 4 + j] = -acc;
    }
    for (int k = 0; k < 2; ++k) {
      double acc = 0.0;
      for (int m = 0; m < ns; ++m) acc = gn_acc(acc, z[m], E[m * 2 + k]);
      R[kGp + r * 2 + k] = -acc;
    }
  }
  if (ny != nu) return CMPC_EQ_OK;
  const int n = ny;
  double c2[kCols2][4];
  for (int j = 0; j < kCols2; ++j)
    for (int i = 0; i < 4; ++i) c2[j][i] = gn_stage2(j, i, n, R);
  for (int k = 0; k < 4; ++k) {
    const int p = eq_pivot<4>(c2[k], k);
    if (eq_bad_pivot(c2[k][p])) return CMPC_GAIN_SINGULAR_G;
    for (int j = k; j < kCols2; ++j) eq_swap<4>(c2[j], k, p);
    for (int i = k + 1; i < 4; ++i) {
      const double m = eq_mult(c2[k][i], c2[k][k]);
      for (int j = k + 1; j < kCols2; ++j) c2[j][i] = eq_elim(c2[j][i], m, c2[j][k]);
    }
  }
  for (int c = 4; c < kCols2; ++c) {
    double* d = c2[c];
    for (int k = 3; k >= 0; --k) {
      d[k] = eq_step(d[k], c2[k][k]);
      for (int i = 0; i < k; ++i) d[i] = eq_elim(d[i], c2[k][i], d[k]);
    }
  }
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 4; ++j) R[kRga + i * 4 + j] = R[kG + i * 4 + j] * c2[4 + i][j];
    for (int k = 0; k < 2; ++k) R[kKff + i * 2 + k] = c2[8 + k][i];
  }
  return CMPC_EQ_OK;
}

// One scenario, start to finish (the host entry point's loop body): the record
// with its NaN entries, the status returned.
template <int PLANT>
CMPC_PHD int gn_solve(double p_in, double p_out, int ny, const int32_t* out, int nu, const int32_t* in,
                      const double* u, const double* x, double* rec) {
  double R[kLen];
  for (int e = 0; e < kLen; ++e) R[e] = gn_nan();
  const int st = gn_body<PLANT>(p_in, p_out, ny, out, nu, in, u, x, R);
  for (int e = 0; e < kLen; ++e) rec[e] = gn_keep(e, ny, nu, st) ? R[e] : gn_nan();
  return st;
}

}  // namespace cmpc_gn
