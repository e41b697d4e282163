// Prediction kernel (cmpc_predict): the predicted controlled
// outputs of every QP slot over the horizon for given plans,
//   y_pred[r] = y_prev + (Su du + Su_other d + Sf fd + Sx xa)[r],
// and the two parts of the objective [J_track, J_move].  Su is never formed:
// the kernel steps the augmented model forward,
//   x_{k+1} = A x_k + fd + sum_c Bin[:, c] v_c(k),   y_pred[k] = ybase + Cx x_{k+1},
// with ybase = y_prev + Cdist xdist.  v_c(k) is what input c feeds the plant
// state at step k: an undelayed input its plan entry min(k, m - 1); an input
// delayed by D the adjusted delay states for k < D (the delayed-input state,
// then the shift block front to back) and the plan entry min(k - D, m - 1)
// after.  The shift blocks are never shifted.
//
// One QP per 16-lane DPP row, four per wave, one wave per workgroup.  Lane
// j < NS holds x[j], row j of A, row j of Bin and fd[j]; lane NS + o holds
// row o of Cx A, Cx Bin and ybase[o] + Cx fd, so one chain of NS
// v_fmac_f64_dpp (row_newbcast of x_k) gives x_{k+1} and y_pred[k] together.
// The horizon runs in chunks of 16 steps: lane t fetches the four inputs of
// step k0 + t, step t takes them by row_newbcast:t; the chunk's outputs go to
// LDS, from where the row's lanes store them in 128-byte pieces and add up
// J_track = 1/2 sum |L_W' (y - dy_ref - dref) - yhat|^2, one step per lane
// (dref: the slot's reference profile where one is in force; L_W', yhat and
// uwt are the slot's own where per-slot weights are, PredictParams::sc_w).
#include "cmpc_internal.h"
#include "dispatch.h"
#include "dpp_blocks.inc"

namespace {

constexpr int kChunk = 16;  // horizon steps per chunk: one per lane of a row

// acc += sum_c bcast_T(uv[c]) * w[c]: the inputs of step T of the chunk, held
// by lane T of the row.  s_nop 1: a VALU write of a VGPR needs two wait states
// before a DPP read of it (cdna_hip_programming.md §5.7 item 2).
template <int T>
__device__ __forceinline__ void inputs_dpp(const double* uv, const double* w, double& acc) {
  static_assert(CMPC_DIMS_NUT == 4, "four plant inputs");
  asm("s_nop 1\n\t"
      "v_fmac_f64_dpp %0, %1, %5 row_newbcast:%9 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %2, %6 row_newbcast:%9 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %3, %7 row_newbcast:%9 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %4, %8 row_newbcast:%9 row_mask:0xf bank_mask:0xf\n\t"
      : "+v"(acc)
      : "v"(uv[0]), "v"(uv[1]), "v"(uv[2]), "v"(uv[3]), "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3]), "i"(T));
}

template <int NS, int NY, int NU, int M>
__global__ __launch_bounds__(64) void cmpc_predict_kernel(PredictParams P) {
  constexpr int NUT = CMPC_DIMS_NUT, NV = NU * M, NUO = NUT - NU, NVO = NUO * M;
  static_assert(NS + NY <= 16, "plant and output lanes share a 16-lane row");
  __shared__ double ybuf[4][kChunk * NY];

  const int lane = threadIdx.x & 15, row = threadIdx.x >> 4;
  const int q0 = blockIdx.x * 4 + row;
  const bool live = q0 < P.nqp;
  const int q = live ? q0 : P.nqp - 1;  // a row past the batch repeats the last QP and stores nothing
  const int s = q % P.S;
  const double* rec = P.lin + (size_t)q * P.rec_len;
  const double* cfg = P.cfg + (size_t)s * P.co.len;
  const double* xa = rec + P.off_x;
  const double* uo = P.u_old + (size_t)q * NUT;
  const bool is_x = lane < NS, is_y = lane >= NS && lane < NS + NY;
  const int xl = is_x ? lane : 0, o = is_y ? lane - NS : 0;

  // plant lanes: their rows of A, Bin and fd; output lanes: row o of Cx
  double m[NS], w[NUT], cx[NS], bias;
#pragma unroll
  for (int l = 0; l < NS; ++l) {
    const double a = rec[P.off_A + xl * NS + l], c = rec[P.off_C + o * P.nobs + l];
    m[l] = is_x ? a : 0.0;
    cx[l] = is_y ? c : 0.0;
  }
#pragma unroll
  for (int c = 0; c < NUT; ++c) {
    const double b = rec[P.off_B + xl * NUT + c];
    w[c] = is_x ? b : 0.0;
  }
  {
    const double f = rec[P.off_f + xl];
    bias = is_x ? f : 0.0;
  }
  // output lanes: Cx A, Cx Bin and ybase + Cx fd (every lane runs the chains;
  // the sources are the plant lanes, which keep their own values)
#pragma unroll
  for (int l = 0; l < NS; ++l) {
    double t = 0.0;
    prop1_dpp<NS>(m[l], cx, t);
    m[l] = is_y ? t : m[l];
  }
#pragma unroll
  for (int c = 0; c < NUT; ++c) {
    double t = 0.0;
    prop1_dpp<NS>(w[c], cx, t);
    w[c] = is_y ? t : w[c];
  }
  {
    double t = rec[P.off_y + o];
    for (int k = 0; k < P.ndist; ++k) t = fma(rec[P.off_C + o * P.nobs + NS + k], xa[k], t);
    prop1_dpp<NS>(bias, cx, t);
    bias = is_y ? t : bias;
  }

  // plan entry (move mv) of input c: own plans, then the other controllers'
  auto plan = [&](int c, int mv) -> double {
    if (c < NU) return P.du[(size_t)q * NV + mv * NU + c];
    if constexpr (NUO > 0) {
      const int oc = c - NU;
      if (P.d) return P.d[(size_t)q * NVO + mv * NUO + oc];
      const int rank = oc / NU, s2 = rank < s ? rank : rank + 1;  // the rank-th other sub-controller
      return P.du[(size_t)(q - s + s2) * NV + mv * NU + oc % NU];
    }
    return 0.0;
  };

  double dy[NY], lw[NY * NY];
#pragma unroll
  for (int j = 0; j < NY; ++j) dy[j] = P.dy_ref ? P.dy_ref[(size_t)q * NY + j] : 0.0;
#pragma unroll
  for (int i = 0; i < NY * NY; ++i) lw[i] = cfg[P.co.lwt + i];
  const double* yhat = cfg + P.co.yhat;
  const double* uw = cfg + P.co.uwt;
  // per-slot weights: the slot's [L_W' | uwt] block, and
  // yhat[q] = L_W'[q] y_ref[s] formed from the raw references below
  const double* yraw = nullptr;
  if (P.sc_w) {
    const double* wq = P.sc_w + (size_t)q * (NY * NY + NU * NU);
#pragma unroll
    for (int i = 0; i < NY * NY; ++i) lw[i] = wq[i];
    uw = wq + NY * NY;
    yraw = P.yref + (size_t)s * P.p * NY;
  }
  double* yout = P.y_pred + (size_t)q * P.p * NY;

  double x = 0.0, jt = 0.0;
  for (int k0 = 0; k0 < P.p; k0 += kChunk) {
    // lane t: what each input feeds the plant state at step k0 + t
    const int k = k0 + lane;
    double uv[NUT];
#pragma unroll
    for (int c = 0; c < NUT; ++c) {
      const int D = P.delay[c];
      double v = 0.0;
      if (k < P.p) {
        if (k >= D) {
          const int mv = k - D < M - 1 ? k - D : M - 1;
          v = plan(c, mv);
        } else {  // AdjustAllDelayedStates: the stored entries less u_old
          v = xa[k == 0 ? P.dslot[c] : P.dblk[c] + k - 1] - uo[c];
        }
      }
      uv[c] = v;
    }
#define CMPC_PREDICT_STEP(T)                          \
  if (k0 + T < P.p) {                                 \
    double acc = bias;                                \
    inputs_dpp<T>(uv, w, acc);                        \
    prop1_dpp<NS>(x, m, acc);                         \
    x = acc;                                          \
    if (is_y) ybuf[row][T * NY + o] = acc;            \
  }
    CMPC_PREDICT_STEP(0) CMPC_PREDICT_STEP(1) CMPC_PREDICT_STEP(2) CMPC_PREDICT_STEP(3)
    CMPC_PREDICT_STEP(4) CMPC_PREDICT_STEP(5) CMPC_PREDICT_STEP(6) CMPC_PREDICT_STEP(7)
    CMPC_PREDICT_STEP(8) CMPC_PREDICT_STEP(9) CMPC_PREDICT_STEP(10) CMPC_PREDICT_STEP(11)
    CMPC_PREDICT_STEP(12) CMPC_PREDICT_STEP(13) CMPC_PREDICT_STEP(14) CMPC_PREDICT_STEP(15)
#undef CMPC_PREDICT_STEP
    __syncthreads();
    const int nrow = P.p - k0 < kChunk ? P.p - k0 : kChunk;
    if (lane < nrow) {  // J_track of step k0 + lane
      double e[NY];
#pragma unroll
      for (int j = 0; j < NY; ++j) e[j] = ybuf[row][lane * NY + j] - dy[j];
      if (P.dref) {  // the slot's reference profile
#pragma unroll
        for (int j = 0; j < NY; ++j) e[j] -= P.dref[((size_t)q * P.p + k) * NY + j];
      }
#pragma unroll
      for (int i = 0; i < NY; ++i) {
        double yh = 0.0;
        if (yraw) {  // the build's order: from 0, ascending j, a product then a sum
#pragma unroll
          for (int j = i; j < NY; ++j) yh += lw[i * NY + j] * yraw[(size_t)k * NY + j];
        } else {
          yh = yhat[(size_t)k * NY + i];
        }
        double r = -yh;
#pragma unroll
        for (int j = 0; j < NY; ++j) r = fma(lw[i * NY + j], e[j], r);
        jt = fma(r, r, jt);
      }
    }
    if (live) {
#pragma unroll
      for (int i = 0; i < NY; ++i) {
        const int idx = i * kChunk + lane;
        if (idx < nrow * NY) yout[(size_t)k0 * NY + idx] = ybuf[row][idx];
      }
    }
    __syncthreads();
  }

  // the row's J_track; J_move = 1/2 sum_mv du_mv' uwt du_mv
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) jt += __shfl_xor(jt, off, 16);
  if (live && lane == 0) {
    double jm = 0.0;
#pragma unroll
    for (int mv = 0; mv < M; ++mv)
#pragma unroll
      for (int a = 0; a < NU; ++a) {
        double t = 0.0;
#pragma unroll
        for (int b = 0; b < NU; ++b) t = fma(uw[a * NU + b], plan(b, mv), t);
        jm = fma(plan(a, mv), t, jm);
      }
    P.cost[(size_t)q * 2] = 0.5 * jt;
    P.cost[(size_t)q * 2 + 1] = 0.5 * jm;
  }
}

}  // namespace

int cmpc_launch_predict(const PredictParams& P, const cmpc_dims& d, void* stream) {
  cmpc_layout L;
  if (cmpc_layout_error(&d, &L) || !cmpc_predict_instance(d, L)) return -1;
  const dim3 grid((unsigned)((P.nqp + 3) / 4)), block(64);
#define CMPC_PREDICT_LAUNCH(NS_, NY_, NU_, M_)                                              \
  if (d.ns == NS_ && d.ny == NY_ && d.nu == NU_ && d.m == M_) {                             \
    cmpc_launch(cmpc_predict_kernel<NS_, NY_, NU_, M_>, grid, block, 0, (hipStream_t)stream, P); \
    return 0;                                                                               \
  }
  CMPC_FOR_BUILD_WAVE(CMPC_PREDICT_LAUNCH)
#undef CMPC_PREDICT_LAUNCH
  return -1;
}
