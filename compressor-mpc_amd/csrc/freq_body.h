// Plant frequency responses (cmpc_plant_freq_host, cmpc_freq_host,
// cmpc_sim_freq): the arithmetic of one scenario, shared by
// the host entry points (abi_analysis.cpp) and the device kernel (freq.hip).
// Given the state x, the plant input u and the boundary pressures p, ny plant
// outputs out[] and nu control inputs in[] (columns of the continuous B, as in
// gains_body.h), and nw frequencies omega[k] >= 0 in rad/s, the same for every
// scenario:
//
//   DEADZONE  a selected recycle valve stands below 2e-2 (gn_deadzone)
//   A, B, C, f  the continuous linearisation at (x, u, p); r_f = max_i |f_i|
//             (eq_resid), reported and not tested
//   E         ns x 2, gains_body.h's central difference in p_in and p_out
//   NONFINITE an entry of A, of the selected columns of B or rows of C, of f
//             or of E is not finite
//   balance   Parlett-Reinsch scaling of A by powers of two without
//             permutation, eig_body.h's stage 2 restated (fq_balance: the same
//             norms, the same 0.95 test, the same guards, kBalSweeps sweeps at
//             most) with the factors d[i] recorded:
//               A <- D^-1 A D,  B <- D^-1 B,  E <- D^-1 E,  C <- C D
//             every product and quotient by a power of two, so exact; j w I is
//             left alone by a diagonal similarity.  Once per scenario.
//   NONFINITE a scaled entry overflowed
//   per frequency w = omega[k], k ascending:
//     (A - j w I)^T Z = C_sel^T  on ns rows and ns + 4 complex columns: column
//             j < ns is row j of A with -w added to the imaginary part of its
//             entry j (fq_diag), columns ns .. ns + 3 the selected rows of C
//             (imaginary part 0, zero from ny on).  gn_body's loops: the pivot
//             of step k is the first row i >= k with the largest |re| + |im|
//             (fq_pivot), rows change places by eq_swap on each part, the
//             multiplier is Smith's quotient (fq_smith, fq_quot), x - m y is
//             fq_elim; each right-hand column is back-substituted
//     SINGULAR  a pivot whose |re| + |im| is 0.0 or not finite, at any
//             frequency: the scenario's status
//     G (j w)[i][j] = -sum_k Z[k][i] B[k][in_j]    real and imaginary sums
//     Gp(j w)[i][m] = -sum_k Z[k][i] E[k][m]       apart, each ascending from
//             0.0 by gn_acc, each negated once: C (j w I - A)^-1 [B | E]
//     peak    per entry m2 = re re + im im; the first k with the largest m2
//             stays (fq_peak: strict comparison, k ascending, from k = 0)
//
// The record, kLen = CMPC_FREQ_LEN doubles per scenario and frequency: G 4 x 4
// row-major in the order of out x in as (re, im) pairs, then Gp 4 x 2 as
// pairs.  The summary, kNsum = CMPC_FREQ_NSUM doubles per scenario: the peak
// m2 of the 16 + 8 entries, the index k of each peak as a double, r_f.  An
// entry outside ny / nu, and every entry of both for a status other than OK,
// is the quiet NaN 0x7ff8000000000000 (fq_keep).  Complex products and
// quotients are separate real operations in the order written (the tree builds
// with -ffp-contract=off; FP64 / is correctly rounded on both sides), so host
// and device agree bit for bit.  With w = 0 and D = I the arithmetic is
// gn_body's in value, every imaginary part a zero.
#pragma once
#include "equilibrium_body.h"
#include "gains_body.h"
#include "target_body.h"

#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
// LDS hand-offs inside one wave: order the stores before the other lanes'
// loads (compiler and hardware, wavefront scope)
#define FQ_SYNC()                                          \
  do {                                                     \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); \
    __builtin_amdgcn_wave_barrier();                       \
  } while (0)
#define FQ_ANY(p) (__ballot(p) != 0)
#else
#define FQ_SYNC() \
  do {            \
  } while (0)
#define FQ_ANY(p) (p)
#endif

namespace cmpc_fq {
using cmpc_eq::Dims;
using cmpc_eq::finite;
using cmpc_gn::gn_nan;
using cmpc_gn::kMaxSel;

constexpr int kMaxNw = CMPC_FREQ_MAX_NW;  // frequencies per call, at most
constexpr int kMaxN = CMPC_FREQ_MAX_N;    // the matrix-level host call
constexpr int kLen = CMPC_FREQ_LEN;       // the record of one frequency
constexpr int kNsum = CMPC_FREQ_NSUM;     // the summary
constexpr int kEnt = 24;                  // entries of G and Gp together
constexpr int kG = 0, kGp = 32;           // the record: (re, im) pairs
constexpr int kPk = 0, kPkIdx = kEnt, kRf = 2 * kEnt;  // the summary
constexpr int kBalSweeps = 32;            // balancing sweeps at most
constexpr int kBalShifts = 2200;          // doublings of f at most: past the exponent range
constexpr double kSfmin2 = 0x1p-969, kSfmax2 = 0x1p969;  // dgebal's guards

// the lanes this caller runs (host: all of them; device: its own) and whether
// it stores what belongs to no lane
struct Lanes {
  int lo, hi;
  bool lead;
};

CMPC_PHD double max2(double a, double b) { return a > b ? a : b; }
CMPC_PHD double min2(double a, double b) { return a < b ? a : b; }

// Balance A (N x N row-major, in place) and record the factors: d[i] is the
// power of two column i was multiplied and row i divided by, over all sweeps.
// eig_body.h's stage 2 with the record added; `on`: the matrix is balanced at
// all (a matrix that has its status runs the same statements and stores
// nothing).
template <int N>
CMPC_PHD void fq_balance(double* A, double* d, const Lanes L, const bool on0) {
  for (int l = L.lo; l < L.hi; ++l) d[l] = 1.0;
  FQ_SYNC();
  bool noconv = on0;
  for (int sweep = 0; sweep < kBalSweeps; ++sweep) {
    if (!FQ_ANY(noconv)) break;
    const bool on = noconv;
    noconv = false;
    for (int i = 0; i < N; ++i) {
      double c = 0.0, r = 0.0, ca = 0.0, ra = 0.0;
      for (int j = 0; j < N; ++j) {
        const double cj = fabs(A[j * N + i]), rj = fabs(A[i * N + j]);
        c = j != i ? c + cj : c;
        r = j != i ? r + rj : r;
        ca = max2(ca, cj);
        ra = max2(ra, rj);
      }
      const bool go = on && c != 0.0 && r != 0.0 && finite(c) && finite(r);
      const double s = c + r;
      double f = 1.0, g = r / 2.0;
      for (int t = 0; t < kBalShifts; ++t) {
        if (!go || c >= g || max2(f, max2(c, ca)) >= kSfmax2 || min2(r, min2(g, ra)) <= kSfmin2) break;
        f = f * 2.0;
        c = c * 2.0;
        ca = ca * 2.0;
        r = r / 2.0;
        g = g / 2.0;
        ra = ra / 2.0;
      }
      g = c / 2.0;
      for (int t = 0; t < kBalShifts; ++t) {
        if (!go || g < r || max2(r, ra) >= kSfmax2 || min2(min2(f, c), min2(g, ca)) <= kSfmin2) break;
        f = f / 2.0;
        c = c / 2.0;
        g = g / 2.0;
        ca = ca / 2.0;
        r = r * 2.0;
        ra = ra * 2.0;
      }
      const bool scale = go && (c + r) < 0.95 * s;
      g = 1.0 / f;
      FQ_SYNC();
      for (int l = L.lo; l < L.hi; ++l) {
        if (scale) {
          A[i * N + l] = A[i * N + l] * g;
          A[l * N + i] = A[l * N + i] * f;
        }
      }
      if (L.lead && scale) d[i] = d[i] * f;
      noconv = noconv || scale;
      FQ_SYNC();
    }
  }
}

// D^-1 on a row of B or E, D on a column of C: by a power of two, exact
CMPC_PHD double fq_rowscale(double v, double d) { return v / d; }
CMPC_PHD double fq_colscale(double v, double d) { return v * d; }

// the imaginary part of the diagonal entry of A - j w I
CMPC_PHD double fq_diag(double w) { return 0.0 - w; }

CMPC_PHD double fq_abs1(double re, double im) { return fabs(re) + fabs(im); }

// pivot row of elimination step k in column k: the first of the largest
template <int N>
CMPC_PHD int fq_pivot(const double* re, const double* im, int k) {
  int p = k;
  double best = fq_abs1(re[k], im[k]);
#pragma unroll
  for (int i = 1; i < N; ++i) {
    const double a = fq_abs1(re[i], im[i]);
    if (i > k && a > best) {
      best = a;
      p = i;
    }
  }
  return p;
}

CMPC_PHD bool fq_bad_pivot(double re, double im) {
  const double s = fq_abs1(re, im);
  return s == 0.0 || !finite(s);
}

// Smith's quotient a / b in two steps: what depends on b alone, then a's part.
// The two cases choose their operands by selects and share r, d and the two
// final divisions.
struct Smith {
  double r, d;
  bool big;  // |b.re| >= |b.im|
};
CMPC_PHD Smith fq_smith(double bre, double bim) {
  Smith s;
  s.big = fabs(bre) >= fabs(bim);
  const double num = s.big ? bim : bre, den = s.big ? bre : bim;
  s.r = num / den;
  s.d = den + num * s.r;
  return s;
}
CMPC_PHD void fq_quot(double are, double aim, const Smith s, double* qre, double* qim) {
  const double t1 = s.big ? are : aim, t2 = s.big ? aim : are;
  const double q = t1 * s.r;
  *qre = (t1 + t2 * s.r) / s.d;
  *qim = (s.big ? t2 - q : q - t2) / s.d;
}

// x = x - m y: the product, then a subtraction per part
CMPC_PHD void fq_elim(double* xre, double* xim, double mre, double mim, double yre, double yim) {
  const double pre = mre * yre - mim * yim;
  const double pim = mre * yim + mim * yre;
  *xre = *xre - pre;
  *xim = *xim - pim;
}

CMPC_PHD double fq_m2(double re, double im) { return re * re + im * im; }

// the running peak of one entry at frequency k
CMPC_PHD void fq_peak(double m2, int k, double* pk, double* idx) {
  const bool up = k == 0 || m2 > *pk;
  *pk = up ? m2 : *pk;
  *idx = up ? (double)k : *idx;
}

// entry q of [G 4 x 4 | Gp 4 x 2] lies inside ny / nu
CMPC_PHD bool fq_inside(int q, int ny, int nu) {
  if (q < 16) return (q >> 2) < ny && (q & 3) < nu;
  return ((q - 16) >> 1) < ny;
}
// entry e of a frequency's record, of the summary, stands (else it is the NaN)
CMPC_PHD bool fq_keep(int e, int ny, int nu, int st) { return st == CMPC_EQ_OK && fq_inside(e >> 1, ny, nu); }
CMPC_PHD bool fq_keep_sum(int e, int ny, int nu, int st) {
  if (st != CMPC_EQ_OK) return false;
  return e == kRf || fq_inside(e < kPkIdx ? e : e - kPkIdx, ny, nu);
}

// The matrix-level body: A N x N, B N x 4, C 4 x N, E N x 2 row-major, outputs
// and inputs the first ny rows and nu columns (the rest is not read).  fin:
// what the caller has tested is finite.  Writes rec (nw x kLen) and sum
// (kNsum) as far as it gets; the status returned.
template <int N>
CMPC_PHD int fq_matrix(const double* Ain, const double* Bin, const double* Cin, const double* Ein, int ny, int nu,
                       int nw, const double* omega, bool fin, double rf, double* rec, double* sum) {
  using namespace cmpc_eq;
  using cmpc_gn::gn_acc;
  static_assert(N >= 1 && N <= kMaxN, "matrix size");
  constexpr int M = N + kMaxSel;
  double A[N * N], B[N * 4], C[4 * N], E[N * 2], d[N];
  for (int e = 0; e < N * N; ++e) A[e] = Ain[e];
  for (int k = 0; k < N; ++k) {
    for (int j = 0; j < 4; ++j) B[k * 4 + j] = j < nu ? Bin[k * 4 + j] : 0.0;
    for (int r = 0; r < 4; ++r) C[r * N + k] = r < ny ? Cin[r * N + k] : 0.0;
    E[k * 2] = Ein[k * 2];
    E[k * 2 + 1] = Ein[k * 2 + 1];
  }
  const Lanes L = {0, N, true};
  for (int pass = 0; pass < 2; ++pass) {
    bool ok = fin;
    for (int e = 0; e < N * N; ++e) ok = ok && finite(A[e]);
    for (int e = 0; e < N * 4; ++e) ok = ok && finite(B[e]) && finite(C[e]);
    for (int e = 0; e < N * 2; ++e) ok = ok && finite(E[e]);
    if (!ok) return CMPC_EQ_NONFINITE;
    if (pass == 1) break;
    fq_balance<N>(A, d, L, true);
    for (int k = 0; k < N; ++k) {
      for (int j = 0; j < 4; ++j) B[k * 4 + j] = fq_rowscale(B[k * 4 + j], d[k]);
      for (int m = 0; m < 2; ++m) E[k * 2 + m] = fq_rowscale(E[k * 2 + m], d[k]);
      for (int r = 0; r < 4; ++r) C[r * N + k] = fq_colscale(C[r * N + k], d[k]);
    }
  }
  sum[kRf] = rf;
  for (int w = 0; w < nw; ++w) {
    double cre[M][N], cim[M][N];  // column j of [(A - j w I)^T | C_sel^T]
    for (int j = 0; j < M; ++j)
      for (int i = 0; i < N; ++i) {
        cre[j][i] = j < N ? A[j * N + i] : C[(j - N) * N + i];
        cim[j][i] = j == i ? fq_diag(omega[w]) : 0.0;
      }
    for (int k = 0; k < N; ++k) {
      const int p = fq_pivot<N>(cre[k], cim[k], k);
      if (fq_bad_pivot(cre[k][p], cim[k][p])) return CMPC_EQ_SINGULAR;
      for (int j = k; j < M; ++j) {
        eq_swap<N>(cre[j], k, p);
        eq_swap<N>(cim[j], k, p);
      }
      const Smith s = fq_smith(cre[k][k], cim[k][k]);
      for (int i = k + 1; i < N; ++i) {
        double mre, mim;
        fq_quot(cre[k][i], cim[k][i], s, &mre, &mim);
        for (int j = k + 1; j < M; ++j) fq_elim(&cre[j][i], &cim[j][i], mre, mim, cre[j][k], cim[j][k]);
      }
    }
    double* R = rec + (size_t)w * kLen;
    for (int r = 0; r < kMaxSel; ++r) {
      double *zre = cre[N + r], *zim = cim[N + r];
      for (int k = N - 1; k >= 0; --k) {
        fq_quot(zre[k], zim[k], fq_smith(cre[k][k], cim[k][k]), &zre[k], &zim[k]);
        for (int i = 0; i < k; ++i) fq_elim(&zre[i], &zim[i], cre[k][i], cim[k][i], zre[k], zim[k]);
      }
      for (int q = 0; q < 6; ++q) {
        // entries 0 .. 3 of the row against B, 4 and 5 against E
        const double* col = q < 4 ? B + q : E + (q - 4);
        const int stride = q < 4 ? 4 : 2, at = q < 4 ? r * 4 + q : 16 + r * 2 + (q - 4);
        double are = 0.0, aim = 0.0;
        for (int k = 0; k < N; ++k) {
          are = gn_acc(are, zre[k], col[k * stride]);
          aim = gn_acc(aim, zim[k], col[k * stride]);
        }
        R[2 * at] = -are;
        R[2 * at + 1] = -aim;
        fq_peak(fq_m2(R[2 * at], R[2 * at + 1]), w, sum + kPk + at, sum + kPkIdx + at);
      }
    }
  }
  return CMPC_EQ_OK;
}

// the NaN entries of a finished scenario: rec nw x kLen, sum kNsum
CMPC_PHD void fq_mask(int ny, int nu, int nw, int st, double* rec, double* sum) {
  for (int w = 0; w < nw; ++w)
    for (int e = 0; e < kLen; ++e)
      if (!fq_keep(e, ny, nu, st)) rec[(size_t)w * kLen + e] = gn_nan();
  for (int e = 0; e < kNsum; ++e)
    if (!fq_keep_sum(e, ny, nu, st)) sum[e] = gn_nan();
}

// One matrix set on the host, start to finish; n at run time (1 .. kMaxN).
template <int N>
inline int fq_host_one(const double* A, const double* B, const double* C, const double* E, int ny, int nu, int nw,
                       const double* omega, double* rec, double* sum) {
  const int st = fq_matrix<N>(A, B, C, E, ny, nu, nw, omega, true, 0.0, rec, sum);
  fq_mask(ny, nu, nw, st, rec, sum);
  return st;
}
inline int fq_host(int n, const double* A, const double* B, const double* C, const double* E, int ny, int nu, int nw,
                   const double* omega, double* rec, double* sum) {
  switch (n) {
    case 1: return fq_host_one<1>(A, B, C, E, ny, nu, nw, omega, rec, sum);
    case 2: return fq_host_one<2>(A, B, C, E, ny, nu, nw, omega, rec, sum);
    case 3: return fq_host_one<3>(A, B, C, E, ny, nu, nw, omega, rec, sum);
    case 4: return fq_host_one<4>(A, B, C, E, ny, nu, nw, omega, rec, sum);
    case 5: return fq_host_one<5>(A, B, C, E, ny, nu, nw, omega, rec, sum);
    case 6: return fq_host_one<6>(A, B, C, E, ny, nu, nw, omega, rec, sum);
    case 7: return fq_host_one<7>(A, B, C, E, ny, nu, nw, omega, rec, sum);
    case 8: return fq_host_one<8>(A, B, C, E, ny, nu, nw, omega, rec, sum);
    case 9: return fq_host_one<9>(A, B, C, E, ny, nu, nw, omega, rec, sum);
    case 10: return fq_host_one<10>(A, B, C, E, ny, nu, nw, omega, rec, sum);
    case 11: return fq_host_one<11>(A, B, C, E, ny, nu, nw, omega, rec, sum);
    case 12: return fq_host_one<12>(A, B, C, E, ny, nu, nw, omega, rec, sum);
  }
  return -1;
}

// One plant scenario, start to finish (the host entry point's loop body): the
// dead zone, the linearisation and E, the selection gathered into the first
// rows and columns, then the matrix-level body; the records and the summary
// with their NaN entries, the status returned.
template <int PLANT>
CMPC_PHD int fq_solve(double p_in, double p_out, int ny, const int32_t* out, int nu, const int32_t* in,
                      const double* u, const double* x, int nw, const double* omega, double* rec, double* sum) {
  using namespace cmpc_eq;
  using namespace cmpc_gn;
  constexpr int ns = Dims<PLANT>::ns;
  int st = CMPC_EQ_DEADZONE;
  if (!gn_deadzone(nu, in, u)) {
    double A[ns * ns], B[ns * 4], C[4 * ns], f[ns], D[4][ns], E[ns * 2], Bs[ns * 4], Cs[4 * ns];
    eq_linearize<PLANT>(p_in, p_out, x, u, A, B, C, f);
    for (int e = 0; e < 4; ++e) {
      double pi, po;
      gn_point(e, p_in, p_out, &pi, &po);
      gn_derivative<PLANT>(pi, po, x, u, D[e]);
    }
    for (int i = 0; i < ns; ++i) {
      E[i * 2] = gn_diff(D[0][i], D[1][i]);
      E[i * 2 + 1] = gn_diff(D[2][i], D[3][i]);
      for (int j = 0; j < 4; ++j) Bs[i * 4 + j] = j < nu ? B[i * 4 + in[j]] : 0.0;
      for (int r = 0; r < 4; ++r) Cs[r * ns + i] = r < ny ? C[out[r] * ns + i] : 0.0;
    }
    st = fq_matrix<ns>(A, Bs, Cs, E, ny, nu, nw, omega, eq_finite<ns>(f), eq_resid<ns>(f), rec, sum);
  }
  fq_mask(ny, nu, nw, st, rec, sum);
  return st;
}

}  // namespace cmpc_fq
