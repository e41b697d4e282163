// Plant frequency responses on the device (cmpc_sim_freq):
// the arithmetic of freq_body.h per scenario.
//
// The shape of the gains kernel (gains.hip): four scenarios per wave, one per
// 16-lane row, one wave per workgroup, the row's LDS region cleared once at
// entry.  Once per scenario lanes 0 and 1 of a row (lane 0 alone for the
// serial plant) run the scalar plant model into the region, lanes 0 to 3
// evaluate the derivative at the four pressure points, lanes 0 .. ns - 1
// difference them into E, and the row balances A in LDS by fq_balance: every
// lane computes the norms and decisions from the same entries, lane l scales
// its entries of row and column i, lane 0 records the factors, and the sweep
// loop leaves on a wave-uniform vote.  Lane l < ns then scales row l of B and
// of E and column l of C.
//
// Per frequency (a loop over the nw entries of a device array read
// wave-uniformly) lane j < ns reloads its complex column of (A - j w I)^T from
// LDS, ns real and ns imaginary registers, lanes ns .. ns + 3 the selected rows
// of C.  The elimination and the back substitution are the gains kernel's with
// complex entries: lane k searches its pivot, the row index, the bad-pivot
// flag and the multipliers go to the row by __shfl, the interchange is eq_swap
// on each part.  Lane ns + i then holds Z[:, i], forms row i of G and of Gp
// against B and E in LDS and keeps the running peaks of its six entries in
// registers.  The 48 doubles of the frequency are assembled in LDS and stored
// by the row's 16 lanes, 8 bytes per lane, consecutive per (scenario,
// frequency).  The summary is stored once after the loop; a scenario that met
// a bad pivot has its earlier records overwritten with the NaN there.
//
// out and in select LDS rows and columns at run time, as in gains.hip, so
// nothing indexed lives in registers.  The wave stays converged: a skipped
// scenario, one in the dead zone, a non-finite one and a row past the batch
// run the same instructions on the cleared region; a row past the batch stores
// nothing.  Nothing of the simulator is written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cmpc_internal.h"
#include "freq_body.h"

namespace {
using namespace cmpc_eq;
using namespace cmpc_fq;
using cmpc_gn::gn_acc;
using cmpc_gn::gn_deadzone;
using cmpc_gn::gn_derivative;
using cmpc_gn::gn_diff;
using cmpc_gn::gn_point;

constexpr int kSpw = 4;            // scenarios per wave: one per 16-lane row
constexpr int kLanes = 64 / kSpw;  // lanes per scenario
constexpr int kRows = 6;           // entries of a row of [G | Gp]
// per scenario: A 121, B 44, C 44, f 11, x 11, u 9, the parallel plant's tank
// terms 4, the derivative at the four pressure points 44, E 22, the balancing
// factors 12, one frequency's record or the summary 49
constexpr int kA = 0, kB = 121, kC = kB + 44, kF = kC + 44, kX = kF + 11, kU = kX + 11, kTk = kU + 9,
              kD = kTk + 4, kE = kD + 44, kDd = kE + 22, kR = kDd + 12;
constexpr int kScnLds = kR + kNsum;

template <int PLANT, bool SCP>
__global__ __launch_bounds__(64) void cmpc_freq_kernel(FreqParams P) {
  constexpr int ns = Dims<PLANT>::ns, ni = Dims<PLANT>::ni;
  static_assert(ns + kMaxSel <= kLanes, "one lane per column of [(A - j w I)^T | C_sel^T]");
  static_assert(kLen <= 3 * kLanes && kNsum <= 4 * kLanes, "the record's and the summary's store fit a row");
  __shared__ double lds[kSpw * kScnLds];
  const int lane = threadIdx.x, g = lane / kLanes, l = lane - g * kLanes, base = lane - l;
  const int b = blockIdx.x * kSpw + g;
  const bool valid = b < P.B;
  const int ny = P.ny, nu = P.nu, nw = P.nw;
  double* const w = lds + g * kScnLds;
  double *A = w + kA, *Bc = w + kB, *Cc = w + kC, *fc = w + kF, *xs = w + kX, *us = w + kU, *tk = w + kTk,
         *Dd = w + kD, *Es = w + kE, *dd = w + kDd, *R = w + kR;

  // a scenario whose integration has failed (the simulator's sticky status)
  // is left alone
  const bool skip = valid && P.sim_status && P.sim_status[b] != 0;
  double p_in = P.p_in, p_out = P.p_out;
  if (SCP && valid) {
    const double2 pr = reinterpret_cast<const double2*>(P.pressures)[b];
    p_in = pr.x;
    p_out = pr.y;
  }
  // this lane's right-hand column r = l - ns: its output, when it has one
  const int r = l - ns;
  const bool zlane = r >= 0 && r < kMaxSel;
  int myout = 0;
#pragma unroll
  for (int j = 0; j < kMaxSel; ++j) myout = (r == j && j < ny) ? P.out[j] : myout;
  const bool selrow = zlane && r < ny;

  // the plant model writes only the nonzeros of A, B and C: clear the region once
  for (int e = l; e < kScnLds; e += kLanes) w[e] = 0.0;
  FQ_SYNC();
  if (l < ns) xs[l] = valid ? P.x[(size_t)b * ns + l] : 0.0;
  if (l < ni) us[l] = valid ? P.u_full[(size_t)b * ni + l] : 0.0;
  FQ_SYNC();

  // a selected recycle valve below the dead-zone bound: the same in the 16 lanes
  const bool dz = gn_deadzone(nu, P.in, us);
  const bool act = valid && !skip && !dz;
  // the scalar plant model, four scenarios side by side, inlined by request
  // (equilibrium.hip has the reason)
  if (PLANT == CMPC_PLANT_PARALLEL) {
    if (act && l < 2)
      [[clang::always_inline]] cmpc_plant::parallel_linearize_part(l, p_in, xs, us, A, Bc, Cc, fc, tk);
    FQ_SYNC();
    if (act && l == 0)
      [[clang::always_inline]] cmpc_plant::parallel_linearize_tank(p_out, xs, us, A, Cc, fc, tk);
  } else if (act && l == 0) {
    [[clang::always_inline]] cmpc_plant::serial_linearize(p_in, p_out, xs, us, A, Bc, Cc, fc, false);
  }
  // the derivative at p_in + h, p_in - h, p_out + h, p_out - h: lanes 0 .. 3
  if (act && l < 4) {
    double pi, po;
    gn_point(l, p_in, p_out, &pi, &po);
    [[clang::always_inline]] gn_derivative<PLANT>(pi, po, xs, us, Dd + l * ns);
  }
  FQ_SYNC();
  if (l < ns) {
    Es[l * 2] = gn_diff(Dd[l], Dd[ns + l]);
    Es[l * 2 + 1] = gn_diff(Dd[2 * ns + l], Dd[3 * ns + l]);
  }
  FQ_SYNC();

  // A by rows, the selected rows of C, f, E and the selected columns of B:
  // before the balancing and again on the scaled entries
  const double* const src = l < ns ? A + l * ns : Cc + myout * ns;
  const bool have = l < ns || selrow;
  const int row = l < ns ? l : 0;
  bool bad = false;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    bool fin = true;
#pragma unroll
    for (int i = 0; i < ns; ++i) fin = fin && (!have || finite(src[i]));
    fin = fin && finite(fc[row]) && finite(Es[row * 2]) && finite(Es[row * 2 + 1]);
#pragma unroll
    for (int j = 0; j < kMaxSel; ++j) {
      const int c = j < nu ? P.in[j] : 0;  // wave-uniform
      fin = fin && (j >= nu || finite(Bc[row * 4 + c]));
    }
    const unsigned long long badm = __ballot(!fin);
    bad = bad || ((badm >> base) & 0xffffull) != 0;
    if (pass == 1) break;
    const Lanes L = {l, l < ns ? l + 1 : l, l == 0};
    fq_balance<ns>(A, dd, L, act && !bad);
    if (l < ns) {
      const double d = dd[l];
#pragma unroll
      for (int j = 0; j < 4; ++j) Bc[l * 4 + j] = fq_rowscale(Bc[l * 4 + j], d);
#pragma unroll
      for (int m = 0; m < 2; ++m) Es[l * 2 + m] = fq_rowscale(Es[l * 2 + m], d);
#pragma unroll
      for (int q = 0; q < 4; ++q) Cc[q * ns + l] = fq_colscale(Cc[q * ns + l], d);
    }
    FQ_SYNC();
  }
  const double rf = eq_resid<ns>(fc);

  bool singular = false;
  double pk[kRows], pidx[kRows];  // the running peaks of this lane's row of [G | Gp]
#pragma unroll
  for (int q = 0; q < kRows; ++q) pk[q] = pidx[q] = 0.0;
#pragma unroll 1
  for (int kw = 0; kw < nw; ++kw) {
    const double om = P.omega[kw];
    double cre[ns], cim[ns];  // this lane's column of [(A - j w I)^T | C_sel^T]; zero in an idle lane
#pragma unroll
    for (int i = 0; i < ns; ++i) {
      cre[i] = have ? src[i] : 0.0;
      cim[i] = i == l ? fq_diag(om) : 0.0;
    }
#pragma unroll
    for (int k = 0; k < ns; ++k) {
      // lane k's search; its answer to the row
      int p = fq_pivot<ns>(cre, cim, k);
      double pvr = 0.0, pvi = 0.0;
#pragma unroll
      for (int i = 0; i < ns; ++i) {
        pvr = i == p ? cre[i] : pvr;
        pvi = i == p ? cim[i] : pvi;
      }
      p = __shfl(p, base + k, 64);
      singular = singular || __shfl((int)fq_bad_pivot(pvr, pvi), base + k, 64) != 0;
      eq_swap<ns>(cre, k, p);
      eq_swap<ns>(cim, k, p);
      const Smith s = fq_smith(cre[k], cim[k]);
#pragma unroll
      for (int i = k + 1; i < ns; ++i) {
        double mre, mim;
        fq_quot(cre[i], cim[i], s, &mre, &mim);
        mre = __shfl(mre, base + k, 64);
        mim = __shfl(mim, base + k, 64);
        fq_elim(&cre[i], &cim[i], mre, mim, cre[k], cim[k]);
      }
    }
    // back substitution of the four right-hand columns, lanes ns .. ns + 3:
    // column k of the triangle comes from lane k, whose registers stay as they are
#pragma unroll
    for (int k = ns - 1; k >= 0; --k) {
      double qre, qim;
      fq_quot(cre[k], cim[k], fq_smith(__shfl(cre[k], base + k, 64), __shfl(cim[k], base + k, 64)), &qre, &qim);
      cre[k] = zlane ? qre : cre[k];
      cim[k] = zlane ? qim : cim[k];
#pragma unroll
      for (int i = 0; i < k; ++i) {
        double vre = cre[i], vim = cim[i];
        fq_elim(&vre, &vim, __shfl(cre[i], base + k, 64), __shfl(cim[i], base + k, 64), qre, qim);
        cre[i] = zlane ? vre : cre[i];
        cim[i] = zlane ? vim : cim[i];
      }
    }
    // lane ns + i holds Z[:, i]: row i of G and of Gp, and their peaks
    const int rr = zlane ? r : 0;
#pragma unroll
    for (int q = 0; q < kRows; ++q) {
      const int c = q < nu ? P.in[q & 3] : 0;  // wave-uniform (nu <= 4: an entry of G)
      const double* col = q < 4 ? Bc + c : Es + (q - 4);
      const int stride = q < 4 ? 4 : 2, at = q < 4 ? rr * 4 + q : 16 + rr * 2 + (q - 4);
      double are = 0.0, aim = 0.0;
#pragma unroll
      for (int k = 0; k < ns; ++k) {
        are = gn_acc(are, cre[k], col[k * stride]);
        aim = gn_acc(aim, cim[k], col[k * stride]);
      }
      const double gre = -are, gim = -aim;
      if (zlane) {
        R[2 * at] = gre;
        R[2 * at + 1] = gim;
      }
      fq_peak(fq_m2(gre, gim), kw, &pk[q], &pidx[q]);
    }
    FQ_SYNC();
    if (valid) {
      const int st = !act ? CMPC_EQ_SKIPPED : (bad || singular) ? CMPC_EQ_SINGULAR : CMPC_EQ_OK;  // OK or not
      double* const rec = P.record + ((size_t)b * nw + kw) * kLen;
      for (int e = l; e < kLen; e += kLanes) rec[e] = fq_keep(e, ny, nu, st) ? R[e] : gn_nan();
    }
    FQ_SYNC();
  }

  const int st = skip       ? CMPC_EQ_SKIPPED
                 : dz       ? CMPC_EQ_DEADZONE
                 : bad      ? CMPC_EQ_NONFINITE
                 : singular ? CMPC_EQ_SINGULAR
                            : CMPC_EQ_OK;
  // a bad pivot at a later frequency: the records stored before it
  const bool redo = valid && st == CMPC_EQ_SINGULAR;
  if (__ballot(redo) != 0) {
#pragma unroll 1
    for (int kw = 0; kw < nw; ++kw) {
      if (redo) {
        double* const rec = P.record + ((size_t)b * nw + kw) * kLen;
        for (int e = l; e < kLen; e += kLanes) rec[e] = gn_nan();
      }
    }
  }
  if (zlane) {
#pragma unroll
    for (int q = 0; q < kRows; ++q) {
      const int at = q < 4 ? r * 4 + q : 16 + r * 2 + (q - 4);
      R[kPk + at] = pk[q];
      R[kPkIdx + at] = pidx[q];
    }
  }
  if (l == 0) R[kRf] = rf;
  FQ_SYNC();
  if (!valid) return;
  double* const sum = P.summary + (size_t)b * kNsum;
  for (int e = l; e < kNsum; e += kLanes) sum[e] = fq_keep_sum(e, ny, nu, st) ? R[e] : gn_nan();
  if (l == 0) P.status[b] = st;
}

template <bool SCP>
int launch(const FreqParams& P, int plant, hipStream_t s) {
  const int grid = (P.B + kSpw - 1) / kSpw;
  if (plant == CMPC_PLANT_PARALLEL)
    cmpc_launch(cmpc_freq_kernel<CMPC_PLANT_PARALLEL, SCP>, dim3(grid), dim3(64), 0, s, P);
  else if (plant == CMPC_PLANT_SERIAL)
    cmpc_launch(cmpc_freq_kernel<CMPC_PLANT_SERIAL, SCP>, dim3(grid), dim3(64), 0, s, P);
  else
    return -1;
  return 0;
}

}  // namespace

int cmpc_launch_freq(const FreqParams& P, int plant, void* stream) {
  if (P.B <= 0) return 0;
  if (P.ny < 1 || P.ny > kMaxSel || P.nu < 1 || P.nu > kMaxSel || P.nw < 1 || P.nw > kMaxNw) return -1;
  for (int j = 0; j < P.ny; ++j)
    if (P.out[j] < 0 || P.out[j] >= 4) return -1;
  for (int j = 0; j < P.nu; ++j)
    if (P.in[j] < 0 || P.in[j] >= 4) return -1;
  if (!P.x || !P.u_full || !P.omega || !P.record || !P.summary || !P.status) return -1;
  return P.pressures ? launch<true>(P, plant, (hipStream_t)stream) : launch<false>(P, plant, (hipStream_t)stream);
}
