// Reference-profile correction (cmpc_set_scenario_reference_profile,
// DESIGN.md §3.12): with slot q tracking y_ref[s][r] + dy_ref[q] + dref[q][r]
// the QP of the build changes only in
//   f <- f - g,   g = Su' w,   w[r] = ywt[s] dref[q][r]   (r = 0..p-1;
//   ywt[q] where per-slot weights are in force, RefshiftParams::sc_w);
// H and G do not depend on the reference.  Su is never formed: Su' w is the
// adjoint of the forward model predict.hip steps, one backward sweep
//   lam <- A' lam + Cx' w[k],   k = p-1 .. 0,
//   g[min(k - D_c, m-1)][c] += Bin[:, c] . lam   for k >= D_c,
// over the slot's record (D_c: the delay of own input c; the column rule is
// predict.hip's v_c(k), transposed).
//
// One QP per 16-lane DPP row, four per wave, one wave per workgroup.  Lane
// j < NS holds lam[j], column j of A and column j of Cx; lane NS + c holds
// (A Bin[:, c])' and (Cx Bin[:, c])', so one chain of NS v_fmac_f64_dpp
// (row_newbcast of lam) gives the new lam on the plant lanes and
// Bin[:, c]' lam_new on the input lanes together.  The horizon runs backward
// in chunks of 16 steps: lane t fetches dref[q][k0 + t] and forms its w, step
// t takes it by row_newbcast:t.  Each input lane keeps M accumulators and
// subtracts them from f in place at the end.
#include "cmpc_internal.h"
#include "dispatch.h"
#include "dpp_blocks.inc"

namespace {

constexpr int kChunk = 16;  // horizon steps per chunk: one per lane of a row

// acc += sum_o bcast_T(w[o]) * cx[o]: the weighted profile row of step T of
// the chunk, held by lane T of the row.  s_nop 1: a VALU write of a VGPR needs
// two wait states before a DPP read of it (cdna_hip_programming.md §5.7 item 2).
template <int NY, int T>
__device__ __forceinline__ void profile_dpp(const double* w, const double* cx, double& acc) {
  static_assert(NY >= 2 && NY <= 4, "two to four controlled outputs");
  if constexpr (NY == 2)
    asm("s_nop 1\n\t"
        "v_fmac_f64_dpp %0, %1, %3 row_newbcast:%5 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %0, %2, %4 row_newbcast:%5 row_mask:0xf bank_mask:0xf\n\t"
        : "+v"(acc)
        : "v"(w[0]), "v"(w[1]), "v"(cx[0]), "v"(cx[1]), "i"(T));
  else if constexpr (NY == 3)
    asm("s_nop 1\n\t"
        "v_fmac_f64_dpp %0, %1, %4 row_newbcast:%7 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %0, %2, %5 row_newbcast:%7 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %0, %3, %6 row_newbcast:%7 row_mask:0xf bank_mask:0xf\n\t"
        : "+v"(acc)
        : "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(cx[0]), "v"(cx[1]), "v"(cx[2]), "i"(T));
  else
    asm("s_nop 1\n\t"
        "v_fmac_f64_dpp %0, %1, %5 row_newbcast:%9 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %0, %2, %6 row_newbcast:%9 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %0, %3, %7 row_newbcast:%9 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %0, %4, %8 row_newbcast:%9 row_mask:0xf bank_mask:0xf\n\t"
        : "+v"(acc)
        : "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3]), "v"(cx[0]), "v"(cx[1]), "v"(cx[2]), "v"(cx[3]), "i"(T));
}

template <int NS, int NY, int NU, int M>
__global__ __launch_bounds__(64) void cmpc_refshift_kernel(RefshiftParams P) {
  constexpr int NUT = CMPC_DIMS_NUT, NV = NU * M;
  static_assert(NS + NU <= 15, "plant and input lanes share a 16-lane row");

  const int lane = threadIdx.x & 15, row = threadIdx.x >> 4;
  const int q0 = blockIdx.x * 4 + row;
  const bool live = q0 < P.nqp;
  const int q = live ? q0 : P.nqp - 1;  // a row past the batch repeats the last QP and stores nothing
  const int s = q % P.S;
  const double* rec = P.lin + (size_t)q * P.rec_len;
  const double* cfg = P.cfg + (size_t)s * P.co.len;
  const bool is_x = lane < NS, is_u = lane >= NS && lane < NS + NU;
  const int xl = is_x ? lane : 0, c = is_u ? lane - NS : 0;

  // plant lanes: their columns of A and Cx; input lanes: column c of Bin
  double m[NS], cx[NY], b[NS];
#pragma unroll
  for (int l = 0; l < NS; ++l) {
    const double a = rec[P.off_A + l * NS + xl], bc = rec[P.off_B + l * NUT + c];
    m[l] = is_x ? a : 0.0;
    b[l] = is_u ? bc : 0.0;
  }
#pragma unroll
  for (int o = 0; o < NY; ++o) {
    const double v = rec[P.off_C + o * P.nobs + xl];
    cx[o] = is_x ? v : 0.0;
  }
  // input lanes: (A Bin[:, c])' and (Cx Bin[:, c])' (every lane runs the
  // chains; the sources are the plant lanes, which keep their own values)
#pragma unroll
  for (int l = 0; l < NS; ++l) {
    double t = 0.0;
    prop1_dpp<NS>(m[l], b, t);
    m[l] = is_u ? t : m[l];
  }
#pragma unroll
  for (int o = 0; o < NY; ++o) {
    double t = 0.0;
    prop1_dpp<NS>(cx[o], b, t);
    cx[o] = is_u ? t : cx[o];
  }

  // the lane's own input's delay; the other lanes never accumulate
  int D = 1 << 30;
#pragma unroll
  for (int i = 0; i < NU; ++i) D = is_u && c == i ? P.delay[i] : D;

  double lw[NY * NY];
#pragma unroll
  for (int i = 0; i < NY * NY; ++i) lw[i] = cfg[P.co.lwt + i];
  if (P.sc_w) {  // per-slot weights: w = L_W[q] (L_W'[q] dref)
    const double* wq = P.sc_w + (size_t)q * (NY * NY + NU * NU);
#pragma unroll
    for (int i = 0; i < NY * NY; ++i) lw[i] = wq[i];
  }
  const double* dq = P.dref + (size_t)q * P.p * NY;

  double g[M];
#pragma unroll
  for (int mv = 0; mv < M; ++mv) g[mv] = 0.0;

  double lam = 0.0;
  for (int k0 = (P.p - 1) / kChunk * kChunk; k0 >= 0; k0 -= kChunk) {
    // lane t: w = ywt dref of step k0 + t, ywt = L_W L_W' (cfg holds L_W')
    const int k = k0 + lane;
    double dr[NY], e[NY], w[NY];
#pragma unroll
    for (int j = 0; j < NY; ++j) dr[j] = k < P.p ? dq[(size_t)k * NY + j] : 0.0;
#pragma unroll
    for (int i = 0; i < NY; ++i) {
      double r = 0.0;
#pragma unroll
      for (int j = 0; j < NY; ++j) r = fma(lw[i * NY + j], dr[j], r);
      e[i] = r;
    }
#pragma unroll
    for (int j = 0; j < NY; ++j) {
      double r = 0.0;
#pragma unroll
      for (int i = 0; i < NY; ++i) r = fma(lw[i * NY + j], e[i], r);
      w[j] = r;
    }
#define CMPC_REFSHIFT_STEP(T)                                  \
  if (k0 + T < P.p) {                                          \
    double acc = 0.0;                                          \
    profile_dpp<NY, T>(w, cx, acc);                            \
    prop1_dpp<NS>(lam, m, acc);                                \
    lam = acc;                                                 \
    const int kk = k0 + T - D;                                 \
    const int sel = kk < 0 ? -1 : (kk < M - 1 ? kk : M - 1);   \
    _Pragma("unroll") for (int mv = 0; mv < M; ++mv)           \
      g[mv] += sel == mv ? acc : 0.0;                          \
  }
    CMPC_REFSHIFT_STEP(15) CMPC_REFSHIFT_STEP(14) CMPC_REFSHIFT_STEP(13) CMPC_REFSHIFT_STEP(12)
    CMPC_REFSHIFT_STEP(11) CMPC_REFSHIFT_STEP(10) CMPC_REFSHIFT_STEP(9) CMPC_REFSHIFT_STEP(8)
    CMPC_REFSHIFT_STEP(7) CMPC_REFSHIFT_STEP(6) CMPC_REFSHIFT_STEP(5) CMPC_REFSHIFT_STEP(4)
    CMPC_REFSHIFT_STEP(3) CMPC_REFSHIFT_STEP(2) CMPC_REFSHIFT_STEP(1) CMPC_REFSHIFT_STEP(0)
#undef CMPC_REFSHIFT_STEP
  }

  // f[mv * NU + c] -= g[mv][c], in place; H and G are not touched
  if (live && is_u) {
    double* f = P.qp + (size_t)q * P.qp_len + NV * NV;
#pragma unroll
    for (int mv = 0; mv < M; ++mv) f[mv * NU + c] -= g[mv];
  }
}

}  // namespace

int cmpc_launch_refshift(const RefshiftParams& P, const cmpc_dims& d, void* stream) {
  cmpc_layout L;
  if (cmpc_layout_error(&d, &L) || !cmpc_refshift_instance(d, L)) return -1;
  const dim3 grid((unsigned)((P.nqp + 3) / 4)), block(64);
#define CMPC_REFSHIFT_LAUNCH(NS_, NY_, NU_, M_)                                               \
  if (d.ns == NS_ && d.ny == NY_ && d.nu == NU_ && d.m == M_) {                               \
    cmpc_launch(cmpc_refshift_kernel<NS_, NY_, NU_, M_>, grid, block, 0, (hipStream_t)stream, P); \
    return 0;                                                                                 \
  }
  CMPC_FOR_BUILD_WAVE(CMPC_REFSHIFT_LAUNCH)
#undef CMPC_REFSHIFT_LAUNCH
  return -1;
}
