// Lagrange multipliers and KKT certificate per QP slot (cmpc_certify,
// DESIGN.md §3.16): one launch after the solve that reads what the context
// holds (the QP record [H | f | G], the plans, the working-set words, status,
// the slot's limits, u_old) and writes one record per slot,
//   g = H x + f + G d,  cx = C x,  C = [I; A]  (A = I, A[i][i - nu] = -1)
//   lam: on the working set W the least-squares solution of C_W' lam_W = g
//        (qpOASES sign: >= 0 on a lower side, <= 0 on an upper side), 0 off W
//   r_stat = max|g - C' lam|,  r_prim = worst violation of lo <= cx <= hi,
//   r_dual = largest wrong-signed |lam| over W,  r_comp = max_W |lam| |cx - t|,
//   obj = 1/2 x'Hx + (f + G d)'x,  scale, n_active, status, rank_def
// (the field table of include/cmpc.h).  W is empty where status != OK.
//
// The rows decouple by own input c: variable x[k nu + c] of move k meets its
// bound e_k and its rate row e_k - e_{k-1} (e_0 for k = 0) only.  Per input
// the 2M x 2M normal matrix C_c C_c' (entries in {-1, 0, 1, 2}, compile-time
// constants) is masked by the working set (an inactive row becomes the unit
// row with a zero right-hand side, so its lam comes out 0) and factored
// LDL' without pivoting, fully unrolled: N = 8 is four 4 x 4 systems, not
// one 8 x 8.  A pivot <= kPivotMin (the true pivots are ratios of integer
// Gram determinants, >= 1/64 here) means dependent normals: rank_def = 1 and
// lam = 0 for the slot.
//
// One lane per QP slot q = b * S + s, 64-lane workgroups; a lane past the
// batch returns before any access.  Loads: a lane reads its own record, which
// is contiguous and 16-byte aligned (qp_len is even), so the compiler issues
// global_load_dwordx4; consecutive lanes are qp_len doubles apart, the wave
// covers one contiguous 64 * qp_len * 8 byte run and every byte of every
// line it touches is used (by the same lane's later loads, out of L1/L2).
// This is how the iterate's prologue reads the buffer (lane_solve.h); staging
// the run through LDS measured slower there.  Stores are
// field-major (row r of slot q at r * nqp + q): one contiguous 512-byte run
// per wave and row.  H is streamed a row at a time, never held whole.
// No LDS, no cross-lane traffic, no inline assembly.
//
// cmpc_certify_summary: a two-pass reduction over the record's residual rows
// (maxima with the lowest slot on ties, and counts: exact in any order).
#include <algorithm>

#include "cmpc_internal.h"

namespace {

// Waves per SIMD the register allocation leaves room for, at least.  The
// scheduler hoists a slot's record loads to the top (what a memory-bound lane
// wants) and pays in registers: N = 8 takes 256 VGPRs + 40 AGPRs at one wave
// per SIMD and spills 144 B per lane when held to two, so it runs at one.
#ifndef CMPC_CERTIFY_WPE
#define CMPC_CERTIFY_WPE(N) ((N) >= 8 ? 1 : 2)
#endif

constexpr double kPivotMin = 1.0 / 1048576.0;

// row i of the per-input constraint block C_c (2M x M): bounds e_k, then the
// rate rows e_k - e_{k-1}
template <int M>
__host__ __device__ constexpr int chain_c(int i, int k) {
  if (i < M) return i == k ? 1 : 0;
  const int r = i - M;
  return r == k ? 1 : (r - 1 == k ? -1 : 0);
}
template <int M>
__host__ __device__ constexpr int chain_gram(int i, int j) {
  int v = 0;
  for (int k = 0; k < M; ++k) v += chain_c<M>(i, k) * chain_c<M>(j, k);
  return v;
}

template <int N, int NU, int NVO>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(CMPC_CERTIFY_WPE(N))))
void cmpc_certify_kernel(CertifyParams P) {
  constexpr int M = N / NU, L = 2 * M;
  constexpr int NVOA = NVO > 0 ? NVO : 1;
  constexpr int NUO = NVO / M, SM1 = NUO / NU;  // other inputs per move, other sub-controllers
  constexpr int QL = N * N + N + N * NVO;
  static_assert(QL % 2 == 0, "a slot's QP record starts 16-byte aligned");
  constexpr CertifyFields F = cmpc_certify_fields(N);
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= P.nqp) return;
  const int s = q % P.S;
  const size_t n = (size_t)P.nqp;
  const double* rec = static_cast<const double*>(__builtin_assume_aligned(P.qp + (size_t)q * QL, 16));

  double x[N];
#pragma unroll
  for (int a = 0; a < N; ++a) x[a] = P.du[(size_t)q * N + a];

  // the other controllers' plans, d[mv * nuo + rank * nu + c]
  double d[NVOA];
#pragma unroll
  for (int c = 0; c < NVOA; ++c) d[c] = 0.0;
  if constexpr (NVO > 0) {
    if (P.d) {
#pragma unroll
      for (int c = 0; c < NVO; ++c) d[c] = P.d[(size_t)q * NVO + c];
    } else {
#pragma unroll
      for (int rk = 0; rk < SM1; ++rk) {
        const int s2 = rk < s ? rk : rk + 1;  // the rank-th other sub-controller
        const double* po = P.du + (size_t)(q - s + s2) * N;
#pragma unroll
        for (int mv = 0; mv < M; ++mv)
#pragma unroll
          for (int c = 0; c < NU; ++c) d[mv * NUO + rk * NU + c] = po[mv * NU + c];
      }
    }
  }

  // gd = f + G d, hx = H x (H a row at a time), max|H|
  double gd[N], hx[N], hmax = 0.0;
#pragma unroll
  for (int a = 0; a < N; ++a) {
    double h = 0.0;
#pragma unroll
    for (int b = 0; b < N; ++b) {
      const double v = rec[a * N + b];
      h = fma(v, x[b], h);
      hmax = fabs(v) > hmax ? fabs(v) : hmax;
    }
    hx[a] = h;
    double t = rec[N * N + a];
    if constexpr (NVO > 0) {
#pragma unroll
      for (int c = 0; c < NVO; ++c) t = fma(rec[N * N + N + a * NVO + c], d[c], t);
    }
    gd[a] = t;
  }
  double g[N], obj = 0.0, lin = 0.0, xmax = 1.0, gmax = 0.0;
#pragma unroll
  for (int a = 0; a < N; ++a) {
    g[a] = hx[a] + gd[a];
    obj = fma(x[a], hx[a], obj);
    lin = fma(gd[a], x[a], lin);
    xmax = fabs(x[a]) > xmax ? fabs(x[a]) : xmax;
    gmax = fabs(gd[a]) > gmax ? fabs(gd[a]) : gmax;
  }
  obj = 0.5 * obj + lin;
  const double scale = hmax * xmax + gmax + 1.0;

  // the slot's limits, as the solver forms them (lane_solve.h)
  const double* lim = P.limits ? P.limits + (size_t)q * (4 * NU) : P.cfg + (size_t)s * P.co.len + P.co.lower;
  double blo[NU], bhi[NU], rlo[NU], rhi[NU];
#pragma unroll
  for (int c = 0; c < NU; ++c) {
    const double uo = P.u_old[(size_t)q * P.nu_tot + c];
    blo[c] = lim[c] - uo;
    bhi[c] = lim[NU + c] - uo;
    rlo[c] = lim[2 * NU + c];
    rhi[c] = lim[3 * NU + c];
  }
  const int status = P.status[q];
  const uint32_t low = (1u << (2 * N)) - 1u;
  const uint32_t wsw = P.ws[q];
  const uint32_t ws = status == CMPC_QP_OK ? (wsw & low) : 0u;
  const uint32_t up = status == CMPC_QP_OK ? ((wsw >> 16) & low) : 0u;

  double lam[2 * N];
  double r_prim = 0.0, r_comp_res[2 * N];
  bool def = false;
#pragma unroll
  for (int c = 0; c < NU; ++c) {
    // local row i: bound of move i (i < M), rate row of move i - M; global row gj
    bool act[L];
    double rhs[L];
#pragma unroll
    for (int i = 0; i < L; ++i) {
      const int gj = i < M ? i * NU + c : N + (i - M) * NU + c;
      act[i] = (ws >> gj) & 1u;
      double r = 0.0, v = 0.0;
#pragma unroll
      for (int k = 0; k < M; ++k) {
        if (chain_c<M>(i, k) == 1) { r = r + g[k * NU + c]; v = v + x[k * NU + c]; }
        if (chain_c<M>(i, k) == -1) { r = r - g[k * NU + c]; v = v - x[k * NU + c]; }
      }
      rhs[i] = act[i] ? r : 0.0;
      const double lo = i < M ? blo[c] : rlo[c], hi = i < M ? bhi[c] : rhi[c];
      const double viol = lo - v > v - hi ? lo - v : v - hi;
      r_prim = viol > r_prim ? viol : r_prim;
      const double t = ((up >> gj) & 1u) ? hi : lo;
      r_comp_res[gj] = fabs(v - t);
    }
    // masked normal matrix, LDL' in place (lower triangle), then the solves
    double A[L][L];
#pragma unroll
    for (int i = 0; i < L; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j)
        A[i][j] = i == j ? (act[i] ? (double)chain_gram<M>(i, i) : 1.0)
                         : (act[i] && act[j] ? (double)chain_gram<M>(i, j) : 0.0);
    double dg[L];
#pragma unroll
    for (int j = 0; j < L; ++j) {
      double p = A[j][j];
#pragma unroll
      for (int k = 0; k < j; ++k) p = p - A[j][k] * A[j][k] * dg[k];
      if (!(p > kPivotMin)) { def = true; p = 1.0; }
      dg[j] = p;
#pragma unroll
      for (int i = j + 1; i < L; ++i) {
        double t = A[i][j];
#pragma unroll
        for (int k = 0; k < j; ++k) t = t - A[i][k] * A[j][k] * dg[k];
        A[i][j] = t / p;
      }
    }
#pragma unroll
    for (int i = 0; i < L; ++i) {  // L y = rhs
#pragma unroll
      for (int k = 0; k < i; ++k) rhs[i] = rhs[i] - A[i][k] * rhs[k];
    }
#pragma unroll
    for (int i = L - 1; i >= 0; --i) {  // D L' lam = y
      double t = rhs[i] / dg[i];
#pragma unroll
      for (int k = i + 1; k < L; ++k) t = t - A[k][i] * rhs[k];
      rhs[i] = t;
    }
#pragma unroll
    for (int i = 0; i < L; ++i) {
      const int gj = i < M ? i * NU + c : N + (i - M) * NU + c;
      lam[gj] = act[i] ? rhs[i] : 0.0;
    }
  }
  if (def) {
#pragma unroll
    for (int j = 0; j < 2 * N; ++j) lam[j] = 0.0;
  }

  // residuals
  double r_stat = 0.0, r_dual = 0.0, r_comp = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) {  // (C' lam)_i = lam_i + lam_{N+i} - lam_{N+i+NU}
    double t = g[i] - lam[i] - lam[N + i];
    if (i + NU < N) t = t + lam[N + i + NU];
    r_stat = fabs(t) > r_stat ? fabs(t) : r_stat;
  }
  int nact = 0;
#pragma unroll
  for (int j = 0; j < 2 * N; ++j) {
    const bool a = (ws >> j) & 1u, u = (up >> j) & 1u;
    nact += a ? 1 : 0;
    const double al = fabs(lam[j]);
    const bool wrong = a && (u ? lam[j] > 0.0 : lam[j] < 0.0);
    r_dual = wrong && al > r_dual ? al : r_dual;
    const double cp = al * r_comp_res[j];
    r_comp = a && cp > r_comp ? cp : r_comp;
  }

  double* out = P.rec + q;
#pragma unroll
  for (int j = 0; j < 2 * N; ++j) out[(F.lam + j) * n] = lam[j];
  out[F.r_stat * n] = r_stat;
  out[F.r_prim * n] = r_prim;
  out[F.r_dual * n] = r_dual;
  out[F.r_comp * n] = r_comp;
  out[F.obj * n] = obj;
  out[F.scale * n] = scale;
  out[F.n_active * n] = (double)nact;
  out[F.status * n] = (double)status;
  out[F.rank_def * n] = def ? 1.0 : 0.0;
}

// ---- summary -------------------------------------------------------------
// One partial: the four maxima with their slots, and the two counts.  A
// candidate wins on a larger value, or the same value and a lower slot: a
// total order, so the result does not depend on the order of combination.
struct CertPart {
  double v[4];
  int32_t idx[4];
  int32_t n_above, n_bad;
};
static_assert(sizeof(CertPart) <= kCertifySummaryHead, "the host copies the head of the work buffer");
constexpr int kSumThreads = 256, kSumBlocksMax = 256;

__device__ __forceinline__ void cert_take(double& v, int32_t& i, double v2, int32_t i2) {
  if (v2 > v || (v2 == v && i2 < i)) {
    v = v2;
    i = i2;
  }
}

__device__ __forceinline__ void cert_block_reduce(CertPart& p, CertPart* out) {
  __shared__ CertPart sh[kSumThreads / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double v2 = __shfl_down(p.v[k], off, 64);
      const int32_t i2 = __shfl_down(p.idx[k], off, 64);
      cert_take(p.v[k], p.idx[k], v2, i2);
    }
    p.n_above += __shfl_down(p.n_above, off, 64);
    p.n_bad += __shfl_down(p.n_bad, off, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = p;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kSumThreads / 64; ++w) {
      for (int k = 0; k < 4; ++k) cert_take(p.v[k], p.idx[k], sh[w].v[k], sh[w].idx[k]);
      p.n_above += sh[w].n_above;
      p.n_bad += sh[w].n_bad;
    }
    *out = p;
  }
}

__device__ __forceinline__ CertPart cert_empty() {
  CertPart p;
  for (int k = 0; k < 4; ++k) {
    p.v[k] = -1.0;  // (every residual is >= 0: the first OK slot wins)
    p.idx[k] = INT32_MAX;
  }
  p.n_above = p.n_bad = 0;
  return p;
}

// pass 1: every block's partial over its slots (grid-stride)
__global__ __launch_bounds__(kSumThreads) void cmpc_certify_sum1_kernel(const double* rec, int nqp, int r0, int r_scale,
                                                                         int r_status, double tol, CertPart* part) {
  CertPart p = cert_empty();
  const size_t n = (size_t)nqp;
  for (int q = blockIdx.x * kSumThreads + threadIdx.x; q < nqp; q += gridDim.x * kSumThreads) {
    if (rec[r_status * n + q] != (double)CMPC_QP_OK) {
      p.n_bad += 1;
      continue;
    }
    const double sc = rec[r_scale * n + q];
    bool above = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double r = rec[(r0 + k) * n + q];
      const double v = k == 1 ? r : r / sc;  // r_prim is in the rows' own units
      cert_take(p.v[k], p.idx[k], v, q);
      above = above || v > tol;
    }
    p.n_above += above ? 1 : 0;
  }
  cert_block_reduce(p, part + blockIdx.x);
}

// pass 2: one block over the partials
__global__ __launch_bounds__(kSumThreads) void cmpc_certify_sum2_kernel(const CertPart* part, int nparts, CertPart* out) {
  CertPart p = cert_empty();
  if ((int)threadIdx.x < nparts) p = part[threadIdx.x];
  cert_block_reduce(p, out);
}

}  // namespace

bool cmpc_certify_instance(int nV, int nu, int nVo) {
#define CMPC_CERTIFY_HAS(N_, NU_, NVO_) \
  if (nV == N_ && nu == NU_ && nVo == NVO_) return true;
  CMPC_FOR_SOLVE(CMPC_CERTIFY_HAS)
#undef CMPC_CERTIFY_HAS
  return false;
}

int cmpc_launch_certify(const CertifyParams& P, int nV, int nu, int nVo, void* stream) {
  if (P.nqp < 1 || !P.rec || P.qp_len != nV * nV + nV + nV * nVo) return -1;
  const dim3 grid((unsigned)((P.nqp + 63) / 64)), block(64);
#define CMPC_CERTIFY_LAUNCH(N_, NU_, NVO_)                                                       \
  if (nV == N_ && nu == NU_ && nVo == NVO_) {                                                    \
    cmpc_launch(cmpc_certify_kernel<N_, NU_, NVO_>, grid, block, 0, (hipStream_t)stream, P);     \
    return 0;                                                                                    \
  }
  CMPC_FOR_SOLVE(CMPC_CERTIFY_LAUNCH)
#undef CMPC_CERTIFY_LAUNCH
  return -1;
}

size_t cmpc_certify_summary_bytes() { return sizeof(CertPart) * (kSumBlocksMax + 1); }

int cmpc_launch_certify_summary(const double* rec, int nqp, int nV, double tol, void* work, void* stream) {
  if (nqp < 1 || !rec || !work) return -1;
  const CertifyFields F = cmpc_certify_fields(nV);
  CertPart* part = static_cast<CertPart*>(work);
  const int blocks = std::min(kSumBlocksMax, (nqp + kSumThreads - 1) / kSumThreads);
  cmpc_launch(cmpc_certify_sum1_kernel, dim3(blocks), dim3(kSumThreads), 0, (hipStream_t)stream, rec, nqp, F.r_stat,
              F.scale, F.status, tol, part + 1);
  cmpc_launch(cmpc_certify_sum2_kernel, dim3(1), dim3(kSumThreads), 0, (hipStream_t)stream,
              (const CertPart*)(part + 1), blocks, part);
  return 0;
}

void cmpc_certify_summary_unpack(const void* work0, cmpc_certify_summary_t* out) {
  const CertPart* p = static_cast<const CertPart*>(work0);
  double* v[4] = {&out->r_stat, &out->r_prim, &out->r_dual, &out->r_comp};
  int32_t* i[4] = {&out->slot_stat, &out->slot_prim, &out->slot_dual, &out->slot_comp};
  for (int k = 0; k < 4; ++k) {
    const bool none = p->idx[k] == INT32_MAX;
    *v[k] = none ? 0.0 : p->v[k];
    *i[k] = none ? -1 : p->idx[k];
  }
  out->n_above = p->n_above;
  out->n_not_ok = p->n_bad;
}
