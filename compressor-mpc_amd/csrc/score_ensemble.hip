// Ensemble statistics of the score record (cmpc_score_ensemble, DESIGN.md
// §3.17): for every record row f and sub-controller s, over the B scenarios'
// values x_b = rec[f * nqp + b * S + s],
//   mean, std (the population value about that mean, from a second pass),
//   min, max, argmax (the lower scenario on a tie), count of x_b > thr[f]
// so a Monte Carlo run downloads len * S * 6 doubles, not the len * B * S record.
//
// Shape (cmpc_certify_summary's): a grid of (blocks, len * S); a block walks
// its (f, s) row grid-stride, reduces within a wave by shuffles and across its
// four waves through a few hundred bytes of LDS, and stores one partial.  The
// second launch does the same for the centred squares, each thread forming the
// mean from the partial sums in block order; the last, a wave per row, combines
// both sets of partials and forms the mean in that same order (so every block
// used the mean it reports).  No floating-point atomics: the sums have a fixed order for a given
// B, and min, max, argmax (a total order) and the count are exact in any order.
#include <algorithm>
#include <limits>

#include "cmpc_internal.h"

namespace {

struct EnsPart {
  double sum, mn, mx;
  int32_t arg, cnt;
};
constexpr int kEnsThreads = 256, kEnsBlocksMax = 64;  // (a row's partials: one per lane of the last launch)

__device__ __forceinline__ void ens_take(double& v, int32_t& i, double v2, int32_t i2) {
  if (v2 > v || (v2 == v && i2 < i)) {
    v = v2;
    i = i2;
  }
}

__device__ __forceinline__ void ens_combine(EnsPart& p, const EnsPart& o) {
  p.sum = p.sum + o.sum;
  p.mn = o.mn < p.mn ? o.mn : p.mn;
  ens_take(p.mx, p.arg, o.mx, o.arg);
  p.cnt += o.cnt;
}

__device__ __forceinline__ EnsPart ens_empty() {
  EnsPart p;
  p.sum = 0.0;
  p.mn = std::numeric_limits<double>::infinity();
  p.mx = -std::numeric_limits<double>::infinity();
  p.arg = INT32_MAX;
  p.cnt = 0;
  return p;
}

// the mean of a row from its partial sums, in block order
__device__ __forceinline__ double ens_mean(const EnsPart* part, int nparts, int B) {
  double t = 0.0;
  for (int k = 0; k < nparts; ++k) t = t + part[k].sum;
  return t / (double)B;
}

// pass 1: every block's partial of its row (grid-stride over the scenarios)
__global__ __launch_bounds__(kEnsThreads) void cmpc_score_ens1_kernel(const double* rec, int B, int S,
                                                                       const double* thr, EnsPart* part) {
  __shared__ EnsPart sh[kEnsThreads / 64];
  const int row = blockIdx.y, f = row / S, s = row - f * S;
  const double* x = rec + (size_t)f * B * S + s;
  const double th = thr ? thr[f] : 0.0;
  EnsPart p = ens_empty();
  for (int64_t b = (int64_t)blockIdx.x * kEnsThreads + threadIdx.x; b < B; b += (int64_t)gridDim.x * kEnsThreads) {
    const double v = x[(size_t)b * S];
    p.sum = p.sum + v;
    p.mn = v < p.mn ? v : p.mn;
    ens_take(p.mx, p.arg, v, (int32_t)b);
    p.cnt += thr && v > th ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    EnsPart o;
    o.sum = __shfl_down(p.sum, off, 64);
    o.mn = __shfl_down(p.mn, off, 64);
    o.mx = __shfl_down(p.mx, off, 64);
    o.arg = __shfl_down(p.arg, off, 64);
    o.cnt = __shfl_down(p.cnt, off, 64);
    ens_combine(p, o);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = p;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kEnsThreads / 64; ++w) ens_combine(p, sh[w]);
    part[(size_t)row * gridDim.x + blockIdx.x] = p;
  }
}

// pass 2: every block's sum of (x - mean)^2 over the same scenarios
__global__ __launch_bounds__(kEnsThreads) void cmpc_score_ens2_kernel(const double* rec, int B, int S,
                                                                       const EnsPart* part, double* sq) {
  __shared__ double sh[kEnsThreads / 64];
  const int row = blockIdx.y, f = row / S, s = row - f * S;
  const double* x = rec + (size_t)f * B * S + s;
  const double mean = ens_mean(part + (size_t)row * gridDim.x, (int)gridDim.x, B);
  double a = 0.0;
  for (int64_t b = (int64_t)blockIdx.x * kEnsThreads + threadIdx.x; b < B; b += (int64_t)gridDim.x * kEnsThreads) {
    const double d = x[(size_t)b * S] - mean;
    a = a + d * d;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a = a + __shfl_down(a, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kEnsThreads / 64; ++w) a = a + sh[w];
    sq[(size_t)row * gridDim.x + blockIdx.x] = a;
  }
}

// the last launch: a wave per row over both sets of partials (at most 64 per
// row, one per lane); the mean again from the partial sums in block order
__global__ __launch_bounds__(kEnsThreads) void cmpc_score_ens3_kernel(const EnsPart* part, const double* sq, int nparts,
                                                                       int rows, int B, double* head) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (kEnsThreads / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;  // (the whole wave)
  const EnsPart* pr = part + (size_t)row * nparts;
  EnsPart p = ens_empty();
  double ss = 0.0;
  if (lane < nparts) {
    p = pr[lane];
    ss = sq[(size_t)row * nparts + lane];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    EnsPart o;
    o.sum = 0.0;
    o.mn = __shfl_down(p.mn, off, 64);
    o.mx = __shfl_down(p.mx, off, 64);
    o.arg = __shfl_down(p.arg, off, 64);
    o.cnt = __shfl_down(p.cnt, off, 64);
    ens_combine(p, o);
    ss = ss + __shfl_down(ss, off, 64);
  }
  const double mean = ens_mean(pr, nparts, B);
  if (lane == 0) {
    double* o = head + (size_t)row * kScoreEnsembleStats;
    o[0] = mean;
    o[1] = sqrt(ss / (double)B);
    o[2] = p.mn;
    o[3] = p.mx;
    o[4] = (double)p.arg;
    o[5] = (double)p.cnt;
  }
}

size_t up16(size_t v) { return (v + 15) / 16 * 16; }
size_t ens_head_bytes(int len, int S) { return up16(sizeof(double) * (size_t)len * S * kScoreEnsembleStats); }
size_t ens_thr_bytes(int len) { return up16(sizeof(double) * (size_t)len); }

}  // namespace

size_t cmpc_score_ensemble_bytes(int len, int S) {
  const size_t rows = (size_t)len * S;
  return ens_head_bytes(len, S) + ens_thr_bytes(len) + rows * kEnsBlocksMax * (sizeof(EnsPart) + sizeof(double));
}

double* cmpc_score_ensemble_thresholds(void* work, int len, int S) {
  return reinterpret_cast<double*>(static_cast<char*>(work) + ens_head_bytes(len, S));
}

int cmpc_launch_score_ensemble(const double* rec, int len, int B, int S, bool has_thr, void* work, void* stream) {
  if (!rec || !work || len < 1 || B < 1 || S < 1 || (size_t)len * S > 65535) return -1;
  const int rows = len * S;
  const int blocks = (int)std::min<int64_t>(kEnsBlocksMax, ((int64_t)B + kEnsThreads - 1) / kEnsThreads);
  double* head = static_cast<double*>(work);
  const double* thr = cmpc_score_ensemble_thresholds(work, len, S);
  EnsPart* part = reinterpret_cast<EnsPart*>(static_cast<char*>(work) + ens_head_bytes(len, S) + ens_thr_bytes(len));
  double* sq = reinterpret_cast<double*>(part + (size_t)rows * kEnsBlocksMax);
  const hipStream_t st = (hipStream_t)stream;
  cmpc_launch(cmpc_score_ens1_kernel, dim3(blocks, rows), dim3(kEnsThreads), 0, st, rec, B, S,
              has_thr ? thr : (const double*)nullptr, part);
  cmpc_launch(cmpc_score_ens2_kernel, dim3(blocks, rows), dim3(kEnsThreads), 0, st, rec, B, S, (const EnsPart*)part,
              sq);
  cmpc_launch(cmpc_score_ens3_kernel, dim3((rows + kEnsThreads / 64 - 1) / (kEnsThreads / 64)), dim3(kEnsThreads), 0, st, (const EnsPart*)part, (const double*)sq,
              blocks, rows, B, head);
  return 0;
}
