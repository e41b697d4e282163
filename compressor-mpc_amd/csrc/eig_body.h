// Eigenvalues of a small real nonsymmetric matrix (cmpc_eig_host,
// cmpc_eig_device, cmpc_plant_modes_host, cmpc_sim_modes):
// the arithmetic of one N x N matrix, N <= 12, no eigenvectors, shared by the
// host entry points (abi_analysis.cpp) and the device kernels (eig.hip).
//
// One text serves both sides.  The work of a stage is written per "lane": lane
// j owns column j where a transformation multiplies from the left and row j
// where it multiplies from the right.  The host runs the lanes 0 .. N - 1 of
// a stage one after the other; on the device the sixteen lanes of a row run
// one lane each, with EIG_SYNC between the stages.  Whatever decides the
// course (norms, reflectors, shifts, the deflation window, the counts) is
// computed by every lane from the same entries with the same operations, so
// the copies agree and nothing is handed over.  A matrix that has its status
// runs the same statements and stores nothing; the loops leave on EIG_ANY (a
// wave-uniform vote) or at their bound.
//
//   1 finite     an entry that is not finite: NONFINITE
//   2 balance    Parlett-Reinsch (dgebal's scaling, no permutation): for i = 0
//                .. N - 1, c and r the 1-norms of column and row i without the
//                diagonal, f the power of two with c f^2 about r (the loops
//                of dgebal, with its guards against over- and underflow); if
//                (c f + r / f) < 0.95 (c + r): row i times 1 / f, column i
//                times f.  Swept until no i scales, kBalSweeps at most.  Exact.
//   3 Hessenberg Householder (orthes): for m = 1 .. N - 2, scale = sum |a_i,m-1|
//                over i >= m; zero: skip.  ort_i = a_i,m-1 / scale, h = sum
//                ort_i^2 (i descending), g = -sign(ort_m) sqrt h, h = h - ort_m g,
//                ort_m = ort_m - g.  Left (lane j >= m, column j): f = (sum
//                ort_i a_ij, i descending) / h, a_ij = a_ij - f ort_i; lane m - 1
//                writes a_m,m-1 = scale g and zeros below.  Right (lane i, row
//                i): f = (sum ort_j a_ij, j descending) / h, a_ij = a_ij - f ort_j.
//   4 QR         Francis double shift with deflation (EISPACK hqr) on the
//                window [l, en], en = N - 1 at first.  One pass:
//                  l     the largest i <= en with |a_i,i-1| <= eps s, s =
//                        |a_i-1,i-1| + |a_ii| (the Hessenberg norm where that
//                        is zero); 0 without one
//                  l = en      one root a_en,en; en = en - 1
//                  l = en - 1  two roots of the trailing block (below);
//                              en = en - 2
//                  else  NO_CONVERGENCE if iters = max_iter; otherwise one
//                        sweep (iters = iters + 1): shifts x = a_en,en, y =
//                        a_en-1,en-1, w = a_en,en-1 a_en-1,en; after 10
//                        sweeps without a deflation s = |a_l+1,l| + |a_l+2,l+1|,
//                        x = y = 0.75 s + a_ll, w = -0.4375 s s, after 20 the
//                        same from the bottom (s = |a_en,en-1| + |a_en-1,en-2|,
//                        a_en,en); the start m of the bulge by hqr's test of
//                        two small subdiagonals; reflectors k = m .. en - 1,
//                        lane j in [k, en] on column j, lane i in [l, min(en,
//                        k + 3)] on row i.
//                en < 0: OK.  max_iter + N + 1 passes at most.
//                The trailing block [[y, b], [c, x]]: w = c b, p = (y - x) / 2,
//                q = p p + w, z = sqrt |q|.  q >= 0: z = p + z (p >= 0) or
//                p - z, roots x + z and x - w / z (x + z twice where z = 0);
//                q < 0: x + p +- z i.
//   5 order      real part descending, then imaginary part descending, equal
//                keys in the order found: a pair sits together, + first.
//   6 results    wr, wi; for a status other than OK both are kNanBits.  An OK
//                matrix whose roots overflowed reports NO_CONVERGENCE.
// The summary of CMPC_MODES_NSUM doubles (eig_summary) is formed from the
// ordered roots.  Products, quotients, sums and square roots are separate
// operations in the order written (the tree builds with -ffp-contract=off;
// FP64 sqrt and / are correctly rounded on both sides), so host and device
// agree bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#endif

#include "../../include/cmpc.h"
#include "plant_model.h"

#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
// LDS hand-offs inside one wave: order the stores before the other lanes'
// loads (compiler and hardware, wavefront scope)
#define EIG_SYNC()                                         \
  do {                                                     \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); \
    __builtin_amdgcn_wave_barrier();                       \
  } while (0)
#define EIG_ANY(p) (__ballot(p) != 0)
#else
#define EIG_SYNC() \
  do {             \
  } while (0)
#define EIG_ANY(p) (p)
#endif

namespace cmpc_eig {

constexpr int kMaxN = CMPC_EIG_MAX_N;
constexpr int kMaxIter = CMPC_EIG_MAX_ITER;  // the entry points refuse more
constexpr int kPending = -1;                 // a matrix still at work
constexpr int kBalSweeps = 32;               // balancing sweeps at most
constexpr int kBalShifts = 2200;             // doublings of f at most: past the exponent range
constexpr double kEps = 2.220446049250313e-16;
constexpr double kSfmin2 = 0x1p-969, kSfmax2 = 0x1p969;  // dgebal's guards
constexpr uint64_t kNanBits = 0x7ff8000000000000ull;
// workspace next to the matrix: roots as found, roots in order
constexpr int kWr = 0, kWi = 16, kSwr = 32, kSwi = 48, kWork = 64;

// the lanes this caller runs (host: all of them; device: its own) and whether
// it stores what belongs to no lane
struct Lanes {
  int lo, hi;
  bool lead;
};

CMPC_PHD bool finite(double v) { return fabs(v) <= 1.7976931348623157e308; }
CMPC_PHD double eig_nan() {
  const uint64_t u = kNanBits;
  double v;
  __builtin_memcpy(&v, &u, sizeof v);
  return v;
}
CMPC_PHD double max2(double a, double b) { return a > b ? a : b; }
CMPC_PHD double min2(double a, double b) { return a < b ? a : b; }

// A: N x N row-major, destroyed.  ev: kWork doubles.  st: kPending, or the
// status the matrix already has.  Returns the status; the ordered roots are
// ev[kSwr ..], ev[kSwi ..].
template <int N>
CMPC_PHD int eig_run(double* A, double* ev, const Lanes L, int st, const int max_iter, int32_t* iters_out) {
  static_assert(N >= 1 && N <= kMaxN, "matrix size");
  double *wr = ev + kWr, *wi = ev + kWi, *swr = ev + kSwr, *swi = ev + kSwi;
  for (int i = L.lo; i < L.hi; ++i) {
    wr[i] = 0.0;
    wi[i] = 0.0;
  }

  // 1 finite
  bool fin = true;
  for (int e = 0; e < N * N; ++e) fin = fin && finite(A[e]);
  if (st == kPending && !fin) st = CMPC_EIG_NONFINITE;

  // 2 balance
  bool noconv = st == kPending;
  for (int sweep = 0; sweep < kBalSweeps; ++sweep) {
    if (!EIG_ANY(noconv)) break;
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
      EIG_SYNC();
      for (int l = L.lo; l < L.hi; ++l) {
        if (scale) {
          A[i * N + l] = A[i * N + l] * g;
          A[l * N + i] = A[l * N + i] * f;
        }
      }
      noconv = noconv || scale;
      EIG_SYNC();
    }
  }

  // 3 Hessenberg
  for (int m = 1; m < N - 1; ++m) {
    double scale = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) scale = i >= m ? scale + fabs(A[i * N + m - 1]) : scale;
    const bool on = st == kPending && scale != 0.0;
    const double sc = on ? scale : 1.0;
    double ort[N], h = 0.0, om = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) ort[i] = i >= m ? A[i * N + m - 1] / sc : 0.0;
#pragma unroll
    for (int i = N - 1; i >= 0; --i) h = i >= m ? h + ort[i] * ort[i] : h;
#pragma unroll
    for (int i = 0; i < N; ++i) om = i == m ? ort[i] : om;
    double g = sqrt(h);
    g = om > 0.0 ? -g : g;
    h = h - om * g;
#pragma unroll
    for (int i = 0; i < N; ++i) ort[i] = i == m ? om - g : ort[i];
    EIG_SYNC();
    for (int l = L.lo; l < L.hi; ++l) {
      if (on && l >= m) {
        double f = 0.0;
#pragma unroll
        for (int i = N - 1; i >= 0; --i) f = i >= m ? f + ort[i] * A[i * N + l] : f;
        f = f / h;
#pragma unroll
        for (int i = 0; i < N; ++i)
          if (i >= m) A[i * N + l] = A[i * N + l] - f * ort[i];
      }
      if (on && l == m - 1) {
#pragma unroll
        for (int i = 0; i < N; ++i)
          if (i >= m) A[i * N + l] = i == m ? scale * g : 0.0;
      }
    }
    EIG_SYNC();
    for (int l = L.lo; l < L.hi; ++l) {
      if (on) {
        double f = 0.0;
#pragma unroll
        for (int j = N - 1; j >= 0; --j) f = j >= m ? f + ort[j] * A[l * N + j] : f;
        f = f / h;
#pragma unroll
        for (int j = 0; j < N; ++j)
          if (j >= m) A[l * N + j] = A[l * N + j] - f * ort[j];
      }
    }
    EIG_SYNC();
  }

  // 4 QR
  double norm = 0.0;
  for (int i = 0; i < N; ++i)
    for (int j = i > 0 ? i - 1 : 0; j < N; ++j) norm = norm + fabs(A[i * N + j]);
  int en = N - 1, its = 0, iters = 0;
  const int passes = max_iter + N + 1;
  for (int pass = 0; pass < passes; ++pass) {
    const bool act = st == kPending;
    if (!EIG_ANY(act)) break;
    const int e = en > 0 ? en : 0, e1 = e > 0 ? e - 1 : 0, e2 = e > 1 ? e - 2 : 0;
    int l = 0;
    for (int i = N - 1; i >= 1; --i) {
      double s = fabs(A[(i - 1) * N + i - 1]) + fabs(A[i * N + i]);
      s = s == 0.0 ? norm : s;
      const bool small = fabs(A[i * N + i - 1]) <= kEps * s;
      l = i <= e && l == 0 && small ? i : l;
    }
    const double x = A[e * N + e], y = A[e1 * N + e1], w = A[e * N + e1] * A[e1 * N + e];
    const bool one = act && l == e, two = act && e > 0 && l == e - 1;
    {
      const double p = (y - x) / 2.0;
      const double q = p * p + w;
      double z = sqrt(fabs(q)), r0, r1, i0, i1;
      if (q >= 0.0) {
        z = p >= 0.0 ? p + z : p - z;
        r0 = x + z;
        r1 = z != 0.0 ? x - w / z : r0;
        i0 = 0.0;
        i1 = 0.0;
      } else {
        r0 = x + p;
        r1 = r0;
        i0 = z;
        i1 = -z;
      }
      if (L.lead && one) {
        wr[e] = x;
        wi[e] = 0.0;
      }
      if (L.lead && two) {
        wr[e1] = r0;
        wi[e1] = i0;
        wr[e] = r1;
        wi[e] = i1;
      }
    }
    en = one ? en - 1 : two ? en - 2 : en;
    its = one || two ? 0 : its;
    if (act && en < 0) st = CMPC_EIG_OK;
    bool sweep = act && !one && !two;
    if (sweep && iters >= max_iter) {
      st = CMPC_EIG_NO_CONVERGENCE;
      sweep = false;
    }
    if (!EIG_ANY(sweep)) continue;

    // the shifts
    double sx = x, sy = y, sw = w;
    if (its == 10) {
      const int l1 = l + 1 < N ? l + 1 : N - 1, l2 = l + 2 < N ? l + 2 : N - 1;
      const double s = fabs(A[l1 * N + l]) + fabs(A[l2 * N + l1]);
      sx = 0.75 * s + A[l * N + l];
      sy = sx;
      sw = -0.4375 * s * s;
    } else if (its == 20) {
      const double s = fabs(A[e * N + e1]) + fabs(A[e1 * N + e2]);
      sx = 0.75 * s + x;
      sy = sx;
      sw = -0.4375 * s * s;
    }
    if (sweep) {
      ++its;
      ++iters;
    }
    // the start of the bulge
    int m = l;
    double pm = 0.0, qm = 0.0, rm = 0.0;
    bool found = false;
    for (int mm = N - 3; mm >= 0; --mm) {
      const int mk = mm > 0 ? mm - 1 : 0;
      const double z = A[mm * N + mm], d1 = A[(mm + 1) * N + mm + 1];
      const double rr = sx - z, ss = sy - z;
      double pp = (rr * ss - sw) / A[(mm + 1) * N + mm] + A[mm * N + mm + 1];
      double qq = d1 - z - rr - ss;
      double r2 = A[(mm + 2) * N + mm + 1];
      const double s = fabs(pp) + fabs(qq) + fabs(r2);
      pp = pp / s;
      qq = qq / s;
      r2 = r2 / s;
      const double lhs = fabs(A[mm * N + mk]) * (fabs(qq) + fabs(r2));
      const double rhs = kEps * (fabs(pp) * (fabs(A[mk * N + mk]) + fabs(z) + fabs(d1)));
      if (!found && mm <= e - 2 && mm >= l && (mm == l || lhs < rhs)) {
        m = mm;
        pm = pp;
        qm = qq;
        rm = r2;
        found = true;
      }
    }
    EIG_SYNC();
    for (int i = L.lo; i < L.hi; ++i) {
      if (sweep && i >= m + 2 && i <= e) {
        A[i * N + i - 2] = 0.0;
        if (i != m + 2) A[i * N + i - 3] = 0.0;
      }
    }
    EIG_SYNC();
    for (int k = 0; k < N - 1; ++k) {
      const bool in = sweep && k >= m && k <= e - 1;
      const bool notlast = k != e - 1;
      const int km = k > 0 ? k - 1 : 0, k2 = k + 2 < N ? k + 2 : N - 1;
      double p = pm, q = qm, r = rm, xx = 0.0;
      if (k != m) {
        p = A[k * N + km];
        q = A[(k + 1) * N + km];
        r = notlast ? A[k2 * N + km] : 0.0;
        xx = fabs(p) + fabs(q) + fabs(r);
        if (xx != 0.0) {
          p = p / xx;
          q = q / xx;
          r = r / xx;
        }
      }
      double s = sqrt(p * p + q * q + r * r);
      s = p < 0.0 ? -s : s;
      const bool go = in && (k == m || xx != 0.0) && s != 0.0;
      const bool seth = go && (k != m || l != m);
      const double hk = k != m ? -s * xx : -A[k * N + km];
      p = p + s;
      const double hx = p / s, hy = q / s, hz = r / s;
      q = q / p;
      r = r / p;
      EIG_SYNC();
      for (int j = L.lo; j < L.hi; ++j) {
        if (seth && j == k - 1) A[k * N + j] = hk;
        if (go && j >= k && j <= e) {
          double t = A[k * N + j] + q * A[(k + 1) * N + j];
          if (notlast) {
            t = t + r * A[k2 * N + j];
            A[k2 * N + j] = A[k2 * N + j] - t * hz;
          }
          A[k * N + j] = A[k * N + j] - t * hx;
          A[(k + 1) * N + j] = A[(k + 1) * N + j] - t * hy;
        }
      }
      EIG_SYNC();
      const int ihi = e < k + 3 ? e : k + 3;
      for (int i = L.lo; i < L.hi; ++i) {
        if (go && i >= l && i <= ihi) {
          double t = hx * A[i * N + k] + hy * A[i * N + k + 1];
          if (notlast) {
            t = t + hz * A[i * N + k2];
            A[i * N + k2] = A[i * N + k2] - t * r;
          }
          A[i * N + k] = A[i * N + k] - t;
          A[i * N + k + 1] = A[i * N + k + 1] - t * q;
        }
      }
      EIG_SYNC();
    }
  }
  if (st == kPending) st = CMPC_EIG_NO_CONVERGENCE;
  EIG_SYNC();

  // 5 order, 6 results
  bool evfin = true;
  for (int i = 0; i < N; ++i) evfin = evfin && finite(wr[i]) && finite(wi[i]);
  if (st == CMPC_EIG_OK && !evfin) st = CMPC_EIG_NO_CONVERGENCE;
  const bool ok = st == CMPC_EIG_OK;
  for (int i = L.lo; i < L.hi; ++i) {
    int rank = 0;
    for (int j = 0; j < N; ++j) {
      const bool before = wr[j] > wr[i] || (wr[j] == wr[i] && (wi[j] > wi[i] || (wi[j] == wi[i] && j < i)));
      rank += before ? 1 : 0;
    }
    const int at = ok ? rank : i;
    swr[at] = ok ? wr[i] : eig_nan();
    swi[at] = ok ? wi[i] : eig_nan();
  }
  EIG_SYNC();
  *iters_out = iters;
  return st;
}

// The CMPC_MODES_NSUM doubles of include/cmpc.h from the ordered roots; all
// NaN when the status is not OK.
CMPC_PHD void eig_summary(int n, const double* swr, const double* swi, bool ok, double* out) {
  double absc = swr[0], remin = swr[0], nun = 0.0, zeta = 1.0, wd = 0.0, wn = 0.0;
  bool have = false;
  for (int i = 0; i < n; ++i) {
    const double a = swr[i], b = swi[i];
    absc = a > absc ? a : absc;
    remin = a < remin ? a : remin;
    nun = a > 0.0 ? nun + 1.0 : nun;
    const double mod = sqrt(a * a + b * b);
    const double z = -a / mod;
    if (b > 0.0 && (!have || z < zeta)) {
      zeta = z;
      wd = b;
      wn = mod;
      have = true;
    }
  }
  out[0] = ok ? absc : eig_nan();
  out[1] = ok ? nun : eig_nan();
  out[2] = ok ? zeta : eig_nan();
  out[3] = ok ? wd : eig_nan();
  out[4] = ok ? wn : eig_nan();
  out[5] = ok ? remin : eig_nan();
}

// One matrix on the host, start to finish: A is left as it is.
template <int N>
inline int eig_host_one(const double* Ain, int max_iter, double* wr, double* wi, int32_t* iters, double* summary) {
  double A[N * N], ev[kWork];
  for (int e = 0; e < N * N; ++e) A[e] = Ain[e];
  const Lanes L = {0, N, true};
  const int st = eig_run<N>(A, ev, L, kPending, max_iter, iters);
  for (int i = 0; i < N; ++i) {
    wr[i] = ev[kSwr + i];
    wi[i] = ev[kSwi + i];
  }
  if (summary) eig_summary(N, ev + kSwr, ev + kSwi, st == CMPC_EIG_OK, summary);
  return st;
}

// n at run time
inline int eig_host(int n, const double* A, int max_iter, double* wr, double* wi, int32_t* iters, double* summary) {
  switch (n) {
    case 1: return eig_host_one<1>(A, max_iter, wr, wi, iters, summary);
    case 2: return eig_host_one<2>(A, max_iter, wr, wi, iters, summary);
    case 3: return eig_host_one<3>(A, max_iter, wr, wi, iters, summary);
    case 4: return eig_host_one<4>(A, max_iter, wr, wi, iters, summary);
    case 5: return eig_host_one<5>(A, max_iter, wr, wi, iters, summary);
    case 6: return eig_host_one<6>(A, max_iter, wr, wi, iters, summary);
    case 7: return eig_host_one<7>(A, max_iter, wr, wi, iters, summary);
    case 8: return eig_host_one<8>(A, max_iter, wr, wi, iters, summary);
    case 9: return eig_host_one<9>(A, max_iter, wr, wi, iters, summary);
    case 10: return eig_host_one<10>(A, max_iter, wr, wi, iters, summary);
    case 11: return eig_host_one<11>(A, max_iter, wr, wi, iters, summary);
    case 12: return eig_host_one<12>(A, max_iter, wr, wi, iters, summary);
  }
  return -1;
}

}  // namespace cmpc_eig
