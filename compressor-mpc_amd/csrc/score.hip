// Closed-loop performance indices (cmpc_score_step): one
// launch per sampling instant that reads the step's results where the context
// keeps them (plans, status, nWSR, working-set words, the slot's weights and
// setpoint offset) and the measured plant outputs, and updates a running
// record per QP slot in place:
//   e[o] = y[b][out_idx[s][o]] - r[q][o],   r = target[q] or y_ref[s][0] + dy_ref[q]
//   n += 1; ise += (e e) Ts; iae += |e| Ts; peak = max(peak, |e|);
//   last_out = k where |e| > band[s][o];
//   j_track += 1/2 |L_W' e|^2;  j_move += 1/2 du' uwt du;  tv += |du|
//   sat_bound / sat_rate += 1 per own input whose first-move bound / rate row is
//   in the working set of a successful solve; n_fail, nwsr_sum, plant_fail_step
// (the field table of include/cmpc.h).  L_W', uwt: the sub-controller's cfg
// block, or the slot's own where per-slot weights are in force (a uniform
// branch on the null pointer, as in refshift.hip / predict.hip).
//
// One lane per QP slot q = b * S + s, 64-lane workgroups; lanes past the batch
// return before any access.  The record is field-major (field row f of slot q
// at f * nqp + q): every load and store of a wave is one contiguous 512-byte
// run.  No LDS, no cross-lane traffic.  The sums are plain multiplies and adds
// in the order written (the tree builds with -ffp-contract=off), so a float64
// host mirror reproduces every field but j_track and j_move bit for bit.
//
// Capture: the lane of slot s == 0 of a chosen scenario also stores the row
// [y | u_control | x] of step k < t_cap; membership is one load of a B-long map.
#include "cmpc_internal.h"

namespace {

#define CMPC_FOR_SCORE(F) F(2, 2) F(3, 2) F(4, 2) F(3, 4) F(4, 4)

template <int NY, int NU>
__global__ __launch_bounds__(64) void cmpc_score_kernel(ScoreParams P) {
  constexpr ScoreFields F = cmpc_score_fields(NY, NU);
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= P.nqp) return;
  const int b = q / P.S, s = q - b * P.S;
  const size_t n = (size_t)P.nqp;
  double* rec = P.rec + q;
  const double kd = (double)P.k;

  // tracking error of the instant
  double e[NY], ae[NY];
#pragma unroll
  for (int o = 0; o < NY; ++o) {
    const double y = P.y[(size_t)b * P.n_out + P.out_idx[s * NY + o]];
    double r;
    if (P.target) {
      r = P.target[(size_t)q * NY + o];
    } else {
      r = P.yref[(size_t)s * P.p * NY + o];
      if (P.dy_ref) r = r + P.dy_ref[(size_t)q * NY + o];
    }
    e[o] = y - r;
    ae[o] = fabs(e[o]);
  }
  // the slot's weights and own first move
  const double* cfg = P.cfg + (size_t)s * P.co.len;
  const double* lw = cfg + P.co.lwt;
  const double* uw = cfg + P.co.uwt;
  if (P.sc_w) {  // per-slot weights: the slot's [L_W' | uwt] block
    lw = P.sc_w + (size_t)q * (NY * NY + NU * NU);
    uw = lw + NY * NY;
  }
  double du[NU];
#pragma unroll
  for (int c = 0; c < NU; ++c) du[c] = P.du[(size_t)q * P.nV + c];
  const int status = P.status[q];
  const uint32_t ws = P.ws[q];

  rec[F.n * n] = rec[F.n * n] + 1.0;
#pragma unroll
  for (int o = 0; o < NY; ++o) {
    double* r = rec + (size_t)o * n;
    r[F.ise * n] = r[F.ise * n] + (e[o] * e[o]) * P.Ts;
    r[F.iae * n] = r[F.iae * n] + ae[o] * P.Ts;
    const double pk = r[F.peak * n];
    r[F.peak * n] = ae[o] > pk ? ae[o] : pk;
    if (ae[o] > P.band[s * NY + o]) r[F.last_out * n] = kd;
  }
  {  // realised stage cost in the controller's own weights: 1/2 |L_W' e|^2
    double jt = 0.0;
#pragma unroll
    for (int i = 0; i < NY; ++i) {
      double z = 0.0;
#pragma unroll
      for (int j = 0; j < NY; ++j) z = z + lw[i * NY + j] * e[j];
      jt = jt + z * z;
    }
    rec[F.j_track * n] = rec[F.j_track * n] + 0.5 * jt;
    double jm = 0.0;
#pragma unroll
    for (int a = 0; a < NU; ++a) {
      double t = 0.0;
#pragma unroll
      for (int c = 0; c < NU; ++c) t = t + uw[a * NU + c] * du[c];
      jm = jm + du[a] * t;
    }
    rec[F.j_move * n] = rec[F.j_move * n] + 0.5 * jm;
  }
  const bool ok = status == CMPC_QP_OK;
#pragma unroll
  for (int c = 0; c < NU; ++c) {
    double* r = rec + (size_t)c * n;
    r[F.tv * n] = r[F.tv * n] + fabs(du[c]);
    // working-set word (qp_solver.h, wset_word): bit j, constraint j in the set
    // (either side); j = c the first move's bound, j = nV + c its rate row
    r[F.sat_bound * n] = r[F.sat_bound * n] + (ok && ((ws >> c) & 1u) ? 1.0 : 0.0);
    r[F.sat_rate * n] = r[F.sat_rate * n] + (ok && ((ws >> (P.nV + c)) & 1u) ? 1.0 : 0.0);
  }
  rec[F.n_fail * n] = rec[F.n_fail * n] + (ok ? 0.0 : 1.0);
  rec[F.nwsr_sum * n] = rec[F.nwsr_sum * n] + (double)P.nwsr[q];
  if (P.plant_status && P.plant_status[b] != 0 && rec[F.plant_fail_step * n] < 0.0)
    rec[F.plant_fail_step * n] = kd;

  if (P.cap_map && s == 0 && P.k < P.t_cap) {
    const int j = P.cap_map[b];
    if (j >= 0) {
      double* row = P.cap + ((size_t)P.k * P.n_sel + j) * P.cap_w;
      for (int i = 0; i < P.n_out; ++i) row[i] = P.y[(size_t)b * P.n_out + i];
      row += P.n_out;
      if (P.u_control)
        for (int i = 0; i < P.nu_tot; ++i) row[i] = P.u_control[(size_t)b * P.nu_tot + i];
      row += P.nu_tot;
      if (P.x)
        for (int i = 0; i < P.ns; ++i) row[i] = P.x[(size_t)b * P.ns + i];
    }
  }
}

// cmpc_score_reset: the record of every slot to its start values
__global__ __launch_bounds__(64) void cmpc_score_reset_kernel(double* rec, int nqp, int len, int lo0, int lo1,
                                                              int pf) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= nqp) return;
  for (int f = 0; f < len; ++f) rec[(size_t)f * nqp + q] = ((f >= lo0 && f < lo1) || f == pf) ? -1.0 : 0.0;
}

}  // namespace

bool cmpc_score_instance(int ny, int nu) {
#define CMPC_SCORE_HAS(NY_, NU_) \
  if (ny == NY_ && nu == NU_) return true;
  CMPC_FOR_SCORE(CMPC_SCORE_HAS)
#undef CMPC_SCORE_HAS
  return false;
}

int cmpc_launch_score(const ScoreParams& P, int ny, int nu, void* stream) {
  if (P.nqp < 1) return -1;
  const dim3 grid((unsigned)((P.nqp + 63) / 64)), block(64);
#define CMPC_SCORE_LAUNCH(NY_, NU_)                                                         \
  if (ny == NY_ && nu == NU_) {                                                             \
    cmpc_launch(cmpc_score_kernel<NY_, NU_>, grid, block, 0, (hipStream_t)stream, P);       \
    return 0;                                                                               \
  }
  CMPC_FOR_SCORE(CMPC_SCORE_LAUNCH)
#undef CMPC_SCORE_LAUNCH
  return -1;
}

int cmpc_launch_score_reset(double* rec, int nqp, int ny, int nu, void* stream) {
  if (nqp < 1 || !rec) return -1;
  const ScoreFields F = cmpc_score_fields(ny, nu);
  const dim3 grid((unsigned)((nqp + 63) / 64)), block(64);
  cmpc_launch(cmpc_score_reset_kernel, grid, block, 0, (hipStream_t)stream, rec, nqp, F.len, F.last_out,
              F.last_out + ny, F.plant_fail_step);
  return 0;
}
