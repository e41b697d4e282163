// Exact ensemble quantiles and the per-step envelope (cmpc_score_quantiles,
// cmpc_envelope_step): for every row of an EnsRowMap, over the
// B scenarios' values, the order statistics at up to CMPC_QUANTILE_MAX_LEVELS
// ranks, by an MSB-first radix selection on the keys of ensemble_select.h.
//
// Shape: a grid of (blocks, rows), blocks = cmpc_quantile_blocks(rows, B) <= 64.
// Two launches per 8-bit digit and two more, 18 in all:
//   count    a block walks its row grid-stride and counts the digit of the keys
//            that carry a target's prefix, in one LDS histogram per distinct
//            prefix (integer LDS adds), and stores the histogram as its partial
//            with plain stores
//   narrow   a block per row: thread d adds digit d's counts over the row's
//            partials in block order; then every target finds the digit that
//            holds its rank (cmpc_select_narrow) and stores its new prefix and
//            rank
//   last     per target: the lowest scenario that holds the key, the count of
//            keys <= it and the smallest key above it, a partial per block
//   finish   a thread per (row, target) combines the partials and writes x_lo,
//            x_hi (and arg); x_hi needs no second selection
// All sums are integers and all minima are over a total order, so the results
// equal a sort's and do not depend on the launch shape.  No floating-point
// atomics, no host synchronisation; lanes past B read nothing.  (A form with 9
// launches, in which the block that arrives last at a row's counter narrows,
// needs a device-scope fence per block; on this device that is a write-back of
// the L2, and the call took 2.9 ms in place of 0.4: DESIGN.md §3.18.)
//
// The envelope's six statistics per channel are score_ensemble.hip's three
// passes over an EnsRowMap (two arrays in one launch, a threshold per row, the
// results written with a stride): kernels of their own here, so that the score
// record's kernels stay what they are.
#include <algorithm>
#include <limits>

#include "cmpc_internal.h"
#include "ensemble_select.h"

namespace {

constexpr int kQThreads = 256, kQBlocksMax = 64, kQWaves = kQThreads / 64, kQLevels = CMPC_QUANTILE_MAX_LEVELS;
constexpr int kQRowBlocks = 4096;  // rows * blocks kept at or under this where rows allow (the partials' size)

struct QState {
  uint64_t prefix;  // the digits fixed so far, right-aligned
  uint32_t rank;    // the target's position among the keys that carry them
  uint32_t pad;
};
struct QFinal {
  uint64_t next;  // the smallest key above the target's, or the largest key
  uint32_t n_le;  // keys <= the target's
  int32_t arg;    // the lowest scenario that holds the target's key
};

__device__ __forceinline__ const double* ens_row(const EnsRowMap& M, int row, int* stride) {
  if (row < M.rows0) {
    const int f = row / M.S0, s = row - f * M.S0;
    *stride = M.S0;
    return M.p0 + (int64_t)f * M.fstride0 + s;
  }
  *stride = M.S1;
  return M.p1 + (row - M.rows0);
}

// The targets' prefixes before `pass` into pre[0..T-1], and rep[t], the lowest
// target with t's prefix (the histogram both use).  Returns the mask of the
// targets that count into their own histogram.  Ends with a barrier.
__device__ __forceinline__ uint32_t targets_of(const QState* state, int row, int T, int pass, uint64_t* pre,
                                               int* rep) {
  const int tid = threadIdx.x;
  if (tid < T) pre[tid] = pass ? state[(size_t)row * T + tid].prefix : 0;
  __syncthreads();
  if (tid < T) {
    int r = tid;
    for (int j = tid - 1; j >= 0; --j)
      if (pre[j] == pre[tid]) r = j;
    rep[tid] = r;
  }
  __syncthreads();
  uint32_t own = 0;
  for (int t = 0; t < T; ++t) own |= rep[t] == t ? 1u << t : 0u;
  return own;
}

__global__ __launch_bounds__(kQThreads) void cmpc_quantile_count_kernel(EnsRowMap M, int B, int pass, int T,
                                                                         const QState* state, uint32_t* part) {
  __shared__ uint32_t hist[kQLevels * kSelectDigits];
  __shared__ uint64_t pre[kQLevels];
  __shared__ int rep[kQLevels];
  const int row = blockIdx.y, tid = threadIdx.x;
  for (int i = tid; i < T * kSelectDigits; i += kQThreads) hist[i] = 0;
  const uint32_t own = targets_of(state, row, T, pass, pre, rep);  // (its barriers cover the zeroing)
  int stride;
  const double* x = ens_row(M, row, &stride);
  for (int64_t b = (int64_t)blockIdx.x * kQThreads + tid; b < B; b += (int64_t)gridDim.x * kQThreads) {
    const uint64_t key = cmpc_select_key(x[(size_t)b * stride]);
    const uint32_t d = cmpc_select_digit(key, pass);
    const uint64_t hi = cmpc_select_prefix(key, pass);
    for (int t = 0; t < T; ++t)
      if (((own >> t) & 1u) && hi == pre[t]) atomicAdd(&hist[t * kSelectDigits + d], 1u);
  }
  __syncthreads();
  uint32_t* mine = part + ((size_t)row * gridDim.x + blockIdx.x) * T * kSelectDigits;
  for (int i = tid; i < T * kSelectDigits; i += kQThreads) mine[i] = hist[i];
}

// a block per row; thread d holds digit d (kQThreads == kSelectDigits)
__global__ __launch_bounds__(kQThreads) void cmpc_quantile_narrow_kernel(int pass, QuantileRanks R, int nparts,
                                                                          const uint32_t* part, QState* state) {
  __shared__ uint32_t hist[kQLevels * kSelectDigits];
  __shared__ uint64_t pre[kQLevels];
  __shared__ int rep[kQLevels];
  const int T = R.n, row = blockIdx.x, tid = threadIdx.x;
  const uint32_t own = targets_of(state, row, T, pass, pre, rep);
  const uint32_t* pr = part + (size_t)row * nparts * T * kSelectDigits;
  for (int t = 0; t < T; ++t) {
    if (!((own >> t) & 1u)) continue;
    uint32_t c = 0;
#pragma unroll 8
    for (int k = 0; k < nparts; ++k) c += pr[((size_t)k * T + t) * kSelectDigits + tid];
    hist[t * kSelectDigits + tid] = c;
  }
  __syncthreads();
  if (tid < T) {
    uint32_t r = pass ? state[(size_t)row * T + tid].rank : R.k_lo[tid];
    const uint32_t d = cmpc_select_narrow(hist + rep[tid] * kSelectDigits, &r);
    QState s;
    s.prefix = (pre[tid] << 8) | d;
    s.rank = r;
    s.pad = 0;
    state[(size_t)row * T + tid] = s;
  }
}
static_assert(kQThreads == kSelectDigits, "the narrowing holds one digit per thread");

__global__ __launch_bounds__(kQThreads) void cmpc_quantile_last_kernel(EnsRowMap M, int B, int T, const QState* state,
                                                                        QFinal* fin) {
  __shared__ QFinal sh[kQWaves][kQLevels];
  __shared__ uint64_t kt[kQLevels];
  const int row = blockIdx.y, tid = threadIdx.x;
  if (tid < T) kt[tid] = state[(size_t)row * T + tid].prefix;
  __syncthreads();
  uint64_t nxt[kQLevels];
  uint32_t nle[kQLevels];
  int32_t arg[kQLevels];
#pragma unroll
  for (int t = 0; t < kQLevels; ++t) {
    nxt[t] = kSelectNanKey;
    nle[t] = 0;
    arg[t] = INT32_MAX;
  }
  int stride;
  const double* x = ens_row(M, row, &stride);
  for (int64_t b = (int64_t)blockIdx.x * kQThreads + tid; b < B; b += (int64_t)gridDim.x * kQThreads) {
    const uint64_t key = cmpc_select_key(x[(size_t)b * stride]);
#pragma unroll
    for (int t = 0; t < kQLevels; ++t) {
      if (t >= T) continue;
      const uint64_t k = kt[t];
      if (key <= k) {
        nle[t] += 1;
        if (key == k && (int32_t)b < arg[t]) arg[t] = (int32_t)b;
      } else if (key < nxt[t]) {
        nxt[t] = key;
      }
    }
  }
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int t = 0; t < kQLevels; ++t) {
    if (t >= T) continue;  // (uniform over the block)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint64_t n2 = __shfl_down((unsigned long long)nxt[t], off, 64);
      const uint32_t c2 = __shfl_down(nle[t], off, 64);
      const int32_t a2 = __shfl_down(arg[t], off, 64);
      nxt[t] = n2 < nxt[t] ? n2 : nxt[t];
      nle[t] += c2;
      arg[t] = a2 < arg[t] ? a2 : arg[t];
    }
    if (lane == 0) {
      QFinal f;
      f.next = nxt[t];
      f.n_le = nle[t];
      f.arg = arg[t];
      sh[wave][t] = f;
    }
  }
  __syncthreads();
  if (tid < T) {
    QFinal f = sh[0][tid];
    for (int w = 1; w < kQWaves; ++w) {
      const QFinal o = sh[w][tid];
      f.next = o.next < f.next ? o.next : f.next;
      f.n_le += o.n_le;
      f.arg = o.arg < f.arg ? o.arg : f.arg;
    }
    fin[((size_t)row * gridDim.x + blockIdx.x) * T + tid] = f;
  }
}

// a thread per (row, target) over the row's partials of the last pass
__global__ __launch_bounds__(kQThreads) void cmpc_quantile_finish_kernel(int rows, QuantileRanks R, int nparts,
                                                                          const QState* state, const QFinal* fin,
                                                                          QuantileOut O) {
  const int T = R.n, i = blockIdx.x * kQThreads + threadIdx.x;
  if (i >= rows * T) return;
  const int row = i / T, t = i - row * T;
  const QFinal* pr = fin + (size_t)row * nparts * T + t;
  QFinal f = pr[0];
  for (int k = 1; k < nparts; ++k) {
    const QFinal o = pr[(size_t)k * T];
    f.next = o.next < f.next ? o.next : f.next;
    f.n_le += o.n_le;
    f.arg = o.arg < f.arg ? o.arg : f.arg;
  }
  const uint64_t key_lo = state[i].prefix;
  double* o = O.out + (int64_t)row * O.row_stride + (int64_t)t * O.lvl_stride;
  o[0] = cmpc_select_value_of(key_lo);
  o[1] = cmpc_select_value_of(cmpc_select_key_hi(key_lo, R.k_hi[t], f.n_le, f.next));
  if (O.lvl_stride == 3) o[2] = (double)f.arg;
}

// ---- the envelope's six statistics per channel (score_ensemble.hip's passes) -------------

struct MomPart {
  double sum, mn, mx;
  int32_t arg, cnt;
};

__device__ __forceinline__ void mom_take(double& v, int32_t& i, double v2, int32_t i2) {
  if (v2 > v || (v2 == v && i2 < i)) {
    v = v2;
    i = i2;
  }
}

__device__ __forceinline__ void mom_combine(MomPart& p, const MomPart& o) {
  p.sum = p.sum + o.sum;
  p.mn = o.mn < p.mn ? o.mn : p.mn;
  mom_take(p.mx, p.arg, o.mx, o.arg);
  p.cnt += o.cnt;
}

__device__ __forceinline__ MomPart mom_empty() {
  MomPart p;
  p.sum = 0.0;
  p.mn = std::numeric_limits<double>::infinity();
  p.mx = -std::numeric_limits<double>::infinity();
  p.arg = INT32_MAX;
  p.cnt = 0;
  return p;
}

// the mean of a row from its partial sums, in block order
__device__ __forceinline__ double mom_mean(const MomPart* part, int nparts, int B) {
  double t = 0.0;
  for (int k = 0; k < nparts; ++k) t = t + part[k].sum;
  return t / (double)B;
}

__global__ __launch_bounds__(kQThreads) void cmpc_envelope_mom1_kernel(EnsRowMap M, int B, const double* thr,
                                                                        MomPart* part) {
  __shared__ MomPart sh[kQWaves];
  const int row = blockIdx.y;
  int stride;
  const double* x = ens_row(M, row, &stride);
  const double th = thr ? thr[row] : 0.0;
  MomPart p = mom_empty();
  for (int64_t b = (int64_t)blockIdx.x * kQThreads + threadIdx.x; b < B; b += (int64_t)gridDim.x * kQThreads) {
    const double v = x[(size_t)b * stride];
    p.sum = p.sum + v;
    p.mn = v < p.mn ? v : p.mn;
    mom_take(p.mx, p.arg, v, (int32_t)b);
    p.cnt += thr && v > th ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    MomPart o;
    o.sum = __shfl_down(p.sum, off, 64);
    o.mn = __shfl_down(p.mn, off, 64);
    o.mx = __shfl_down(p.mx, off, 64);
    o.arg = __shfl_down(p.arg, off, 64);
    o.cnt = __shfl_down(p.cnt, off, 64);
    mom_combine(p, o);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = p;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kQWaves; ++w) mom_combine(p, sh[w]);
    part[(size_t)row * gridDim.x + blockIdx.x] = p;
  }
}

__global__ __launch_bounds__(kQThreads) void cmpc_envelope_mom2_kernel(EnsRowMap M, int B, const MomPart* part,
                                                                        double* sq) {
  __shared__ double sh[kQWaves];
  const int row = blockIdx.y;
  int stride;
  const double* x = ens_row(M, row, &stride);
  const double mean = mom_mean(part + (size_t)row * gridDim.x, (int)gridDim.x, B);
  double a = 0.0;
  for (int64_t b = (int64_t)blockIdx.x * kQThreads + threadIdx.x; b < B; b += (int64_t)gridDim.x * kQThreads) {
    const double d = x[(size_t)b * stride] - mean;
    a = a + d * d;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a = a + __shfl_down(a, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kQWaves; ++w) a = a + sh[w];
    sq[(size_t)row * gridDim.x + blockIdx.x] = a;
  }
}

// a wave per row over both sets of partials (at most 64 per row, one per lane)
__global__ __launch_bounds__(kQThreads) void cmpc_envelope_mom3_kernel(const MomPart* part, const double* sq,
                                                                        int nparts, int rows, int B, double* out,
                                                                        int64_t row_stride) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kQWaves + (threadIdx.x >> 6);
  if (row >= rows) return;  // (the whole wave)
  const MomPart* pr = part + (size_t)row * nparts;
  MomPart p = mom_empty();
  double ss = 0.0;
  if (lane < nparts) {
    p = pr[lane];
    ss = sq[(size_t)row * nparts + lane];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    MomPart o;
    o.sum = 0.0;
    o.mn = __shfl_down(p.mn, off, 64);
    o.mx = __shfl_down(p.mx, off, 64);
    o.arg = __shfl_down(p.arg, off, 64);
    o.cnt = __shfl_down(p.cnt, off, 64);
    mom_combine(p, o);
    ss = ss + __shfl_down(ss, off, 64);
  }
  const double mean = mom_mean(pr, nparts, B);
  if (lane == 0) {
    double* o = out + (int64_t)row * row_stride;
    o[0] = mean;
    o[1] = sqrt(ss / (double)B);
    o[2] = p.mn;
    o[3] = p.mx;
    o[4] = (double)p.arg;
    o[5] = (double)p.cnt;
  }
}

size_t up16(size_t v) { return (v + 15) / 16 * 16; }

bool rows_ok(const EnsRowMap& M, int B) {
  if (B < 1 || M.rows0 < 0 || M.rows1 < 0 || (int64_t)M.rows0 + M.rows1 < 1 || (int64_t)M.rows0 + M.rows1 > 65535)
    return false;
  if (M.rows0 && (!M.p0 || M.S0 < 1)) return false;
  if (M.rows1 && (!M.p1 || M.S1 < M.rows1)) return false;
  return true;
}

// the work buffer: head | state | last-pass partials | histograms
struct QLayout {
  size_t state, fin, part, bytes;
};
QLayout q_layout(int rows, int B, int T) {
  const size_t nb = (size_t)cmpc_quantile_blocks(rows, B), r = (size_t)rows, t = (size_t)T;
  QLayout L;
  L.state = up16(sizeof(double) * r * t * 3);
  L.fin = L.state + sizeof(QState) * r * t;
  L.part = L.fin + sizeof(QFinal) * r * nb * t;
  L.bytes = L.part + sizeof(uint32_t) * r * nb * t * kSelectDigits;
  return L;
}

}  // namespace

int cmpc_quantile_blocks(int rows, int B) {
  const int64_t by_b = ((int64_t)B + kQThreads - 1) / kQThreads;
  const int64_t by_rows = std::max(1, kQRowBlocks / std::max(rows, 1));
  return (int)std::max<int64_t>(1, std::min<int64_t>(kQBlocksMax, std::min(by_b, by_rows)));
}

size_t cmpc_quantile_work_bytes(int rows, int B, int n_levels) { return q_layout(rows, B, n_levels).bytes; }

int cmpc_launch_quantiles(const EnsRowMap& M, int B, const QuantileRanks& R, const QuantileOut& O, void* work,
                          void* stream) {
  if (!work || !O.out || !rows_ok(M, B) || R.n < 1 || R.n > kQLevels || (O.lvl_stride != 2 && O.lvl_stride != 3))
    return -1;
  for (int l = 0; l < R.n; ++l)
    if (R.k_lo[l] >= (uint32_t)B || R.k_hi[l] >= (uint32_t)B || R.k_hi[l] < R.k_lo[l]) return -1;
  const int rows = M.rows0 + M.rows1, blocks = cmpc_quantile_blocks(rows, B), T = R.n;
  const QLayout L = q_layout(rows, B, T);
  char* w = static_cast<char*>(work);
  QState* state = reinterpret_cast<QState*>(w + L.state);
  QFinal* fin = reinterpret_cast<QFinal*>(w + L.fin);
  uint32_t* part = reinterpret_cast<uint32_t*>(w + L.part);
  const hipStream_t st = (hipStream_t)stream;
  for (int pass = 0; pass < kSelectPasses; ++pass) {
    cmpc_launch(cmpc_quantile_count_kernel, dim3(blocks, rows), dim3(kQThreads), 0, st, M, B, pass, T,
                (const QState*)state, part);
    cmpc_launch(cmpc_quantile_narrow_kernel, dim3(rows), dim3(kQThreads), 0, st, pass, R, blocks,
                (const uint32_t*)part, state);
  }
  cmpc_launch(cmpc_quantile_last_kernel, dim3(blocks, rows), dim3(kQThreads), 0, st, M, B, T, (const QState*)state,
              fin);
  cmpc_launch(cmpc_quantile_finish_kernel, dim3((rows * T + kQThreads - 1) / kQThreads), dim3(kQThreads), 0, st, rows,
              R, blocks, (const QState*)state, (const QFinal*)fin, O);
  return 0;
}

size_t cmpc_envelope_moments_bytes(int rows) {
  return (size_t)rows * kQBlocksMax * (sizeof(MomPart) + sizeof(double));
}

int cmpc_launch_envelope_moments(const EnsRowMap& M, int B, const double* thr, double* out, int64_t row_stride,
                                 void* work, void* stream) {
  if (!work || !out || !rows_ok(M, B) || row_stride < 6) return -1;
  const int rows = M.rows0 + M.rows1;
  const int blocks = (int)std::min<int64_t>(kQBlocksMax, ((int64_t)B + kQThreads - 1) / kQThreads);
  MomPart* part = static_cast<MomPart*>(work);
  double* sq = reinterpret_cast<double*>(part + (size_t)rows * kQBlocksMax);
  const hipStream_t st = (hipStream_t)stream;
  cmpc_launch(cmpc_envelope_mom1_kernel, dim3(blocks, rows), dim3(kQThreads), 0, st, M, B, thr, part);
  cmpc_launch(cmpc_envelope_mom2_kernel, dim3(blocks, rows), dim3(kQThreads), 0, st, M, B, (const MomPart*)part, sq);
  cmpc_launch(cmpc_envelope_mom3_kernel, dim3((rows + kQWaves - 1) / kQWaves), dim3(kQThreads), 0, st,
              (const MomPart*)part, (const double*)sq, blocks, rows, B, out, row_stride);
  return 0;
}
