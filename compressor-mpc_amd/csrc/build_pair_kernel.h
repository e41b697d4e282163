// Shared-form row build kernel: one cooperative SCENARIO (its two QPs) per
// 16-lane DPP row, four scenarios = eight QPs per wave64.
//
// Both sub-controllers of a cooperative scenario linearise the same plant at
// the same point: A, C and f of their records are equal and slot 1's B is slot
// 0's with the columns rotated by nu (plant.cpp, produce_body.h).  The P chain
// P_{r+1} = P_r [A | B] and the Markov values P_r B_c depend on nothing else,
// so the row computes them once, in slot 0's ("canonical") column order, and
// both QPs gather from the same hand-off lines.  What differs per slot
// (dx_aug, y_prev, u_old, y_hat, dy_ref, uwt) feeds two free-response chains.
//
// Roles, extending build_rows_kernel.h (lane j of row R, scenario 4 g + R):
//   pP / aP / mP    : the one P chain (state lanes j < ns: A's column j; Markov
//                     lanes ns + c: canonical B column c)
//   pS0, pS1 / aS.. : the two free-response chains.  They share the multipliers
//                     mS (A row j, the two Adelay columns, C_hat row o); each has
//                     its own start f + Adelay w_0, kappa, -y_hat line and w
//                     tables.  Slot 1's delayed inputs are the same physical
//                     inputs in swapped order, so carrier lane 16 - ND + k
//                     holds slot 1's w line ND - 1 - k, and the generated block
//                     adds slot 1's carriers in its own order (gen_rows.py).
//   cv[o], acc[a]   : gather lane b < m nu_tot holds canonical column b, lanes
//                     m nu_tot and m nu_tot + 1 hold z of slot 0 and of slot 1;
//                     acc[a] = sum_{r,o} column_a column_b for all m nu_tot
//                     canonical columns a: the full Gram.  H_0 is its (own_0,
//                     own_0) block, G_0 (own_0, own_1), H_1 (own_1, own_1), G_1
//                     (own_1, own_0), f_s = own_s x z_s.  Per accumulator the
//                     FMAs run r outer, o inner with the factors of the
//                     one-QP-per-row kernel: with bitwise equal plants the QP
//                     buffer is bit-identical to that kernel's.
//
// Staging (one round trip per group): slot 0's records whole and slot 1's
// tails (dx_aug, y_prev) by LDS-DMA with per-lane source addresses; slot 1's
// head (A, B, C, f) is fetched with coalesced vector loads in the same round
// trip and only compared, as 64-bit integers, against the staged slot-0 head
// under the column rotation.  If any scenario of the group differs, the wave
// builds the group twice with the same body: pass h takes the plant from slot
// h's records (restaged for h = 1) and stores slot h's QPs only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "dispatch.h"
#include "rows_blocks.inc"

// How many steps ahead the horizon loop reads a step's zeroed P accumulators
// from LDS (CMPC_PAIR_STEP).  Both forms are bit-identical; 1 measured faster
// (DESIGN §3.2b).
#ifndef CMPC_PAIR_ZDEPTH
#define CMPC_PAIR_ZDEPTH 1
#endif
static_assert(CMPC_PAIR_ZDEPTH == 1 || CMPC_PAIR_ZDEPTH == 2, "CMPC_PAIR_ZDEPTH");

// Wait for the staging DMA.  This is an S_WAITCNT instruction of the compiler's
// own (vmcnt(0), the other counters left alone), not inline assembly: a
// global_load_lds counts on vmcnt and on lgkmcnt, so the wait-count pass keeps
// it as a pending "flat" access until it has seen a wait on BOTH counters, and
// while one is pending it turns every counted lgkmcnt(N) into lgkmcnt(0).  It
// cannot read a wait inside an asm string: with `asm("s_waitcnt vmcnt(0)")`
// the DMA of pass 1's restaging stayed pending round the pass loop's back
// edge, and every horizon step drained the LDS queue before its first FMA.
__device__ __forceinline__ void pair_wait_dma() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(0x0F70);  // gfx9 encoding: vmcnt 0, expcnt 7, lgkmcnt 15
  asm volatile("" ::: "memory");
}

template <int NS, int NY, int NUT, int NU, int M, int ND>
__global__ __launch_bounds__(64 * CMPC_BUILD_WAVES) __attribute__((amdgpu_waves_per_eu(2, 2)))
void cmpc_build_pair_kernel(BuildParams P) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  constexpr int WPG = CMPC_BUILD_WAVES;
  constexpr int NV = NU * M;   // own columns of one QP
  constexpr int NC = M * NUT;  // canonical columns of the scenario
  constexpr int NG = NC + 2;   // gather lanes: the columns, z of slot 0, z of slot 1
  constexpr int U = cmpc_rows_unroll(NY);
  constexpr int NCMP = CMPC_PAIR_CMP;
  static_assert(U == 5, "the unrolled block has 5 steps");
  static_assert(M == 2 && ND == 2 && NUT == 2 * NU, "two sub-controllers, two delayed inputs");
  static_assert(NG <= 16 && NS + NUT <= 16 && NS + NY + ND <= 16, "lane budget");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // uniform: group indices stay scalar
  const int R = lane >> 4, j = lane & 15;
  const int pp = P.p, nobs = P.nobs, rl = P.rec_len, ndist = P.ndist;
  const int LQ = P.rows.LQ, WL = P.pair.WL, yls = P.rows.yls;
  const int nscn = P.nqp >> 1;
  const int ngroups = (nscn + 3) / 4;
  const int nwaves = gridDim.x * WPG;

  double* zeros = smem;
  double* ylT = smem + P.rows.yl_off;  // [2][NY][yls]  -L_W' y_ref, output-major
  double* lw_all = smem + P.rows.lw_off;
  double* uw_all = smem + P.rows.uw_off;
  double* wreg = smem + P.rows.lds_block + wave * P.pair.per_wave;
  double* lines = wreg;                 // [4][LQ]: per scenario, the hand-off entries
  double* chs = wreg + P.rows.ch_off;   // [4][NY][16]  C_hat rows
  double* z1s = wreg + P.pair.z1_off;   // [4][U][NY]   z entries of slot 1
  double* wtab = wreg + P.pair.w_off;   // [4][2][ND][WL]  delay-line inputs w_t per slot

  const int nthr = 64 * WPG;
  for (int e = threadIdx.x; e < 2 * NY * yls; e += nthr) {
    const int ss = e / (NY * yls), rem = e - ss * NY * yls;
    const int o = rem / yls, r = rem - o * yls;
    ylT[e] = (r < pp) ? -P.cfg[(size_t)ss * P.co.len + P.co.yhat + r * NY + o] : 0.0;
  }
  for (int e = threadIdx.x; e < 2 * NY * NY; e += nthr)
    lw_all[e] = P.cfg[(size_t)(e / (NY * NY)) * P.co.len + P.co.lwt + e % (NY * NY)];
  for (int e = threadIdx.x; e < 2 * NU * NU; e += nthr)
    uw_all[e] = P.cfg[(size_t)(e / (NU * NU)) * P.co.len + P.co.uwt + e % (NU * NU)];
  if (threadIdx.x < 16) zeros[threadIdx.x] = 0.0;
  for (int e = lane; e < P.pair.per_wave; e += 64) wreg[e] = 0.0;
  // the coverage counters alternate between launches: this launch adds to
  // pair_cnt and clears the next launch's (launches of a context are ordered)
  if (blockIdx.x == 0 && threadIdx.x == 0) *P.pair_cnt_next = 0u;
  __syncthreads();

  // ---- per-lane roles (identical for every group) ----
  const bool st = j < NS;
  const bool mk = j >= NS && j < NS + NUT;
  const int cm = mk ? j - NS : 0;
  const bool ol = j >= NS && j < NS + NY;
  const int oo = ol ? j - NS : 0;
  const bool cl = j >= 16 - ND;
  const int kc = cl ? j - (16 - ND) : 0;
  const bool gl = j < NG;
  const bool zl0 = j == NC, zl1 = j == NC + 1, zlane = zl0 || zl1;
  const int gk = (gl && !zlane) ? j / NUT : 0;
  const int gc = (gl && !zlane) ? j - gk * NUT : 0;
  const double smask = (gl && !zlane && gk == M - 1) ? 1.0 : 0.0;
  int dg = 0, dm = 0, log_ = 0, lom = 0, dinp[ND], dlen[ND], boff[ND];
#pragma unroll
  for (int c = 0; c < NUT; ++c) {
    if (c == gc) { dg = P.delay[c]; log_ = P.rows.lo[c]; }
    if (c == cm) { dm = P.delay[c]; lom = P.rows.lo[c]; }
  }
#pragma unroll
  for (int k = 0; k < ND; ++k) {
    dinp[k] = P.dinput[k];
    dlen[k] = P.dlen[k];
    boff[k] = P.boff[k];
  }
  // (the two delays are equal: the delay set is invariant under the rotation)
  int ysw = -1;
#pragma unroll
  for (int k = 0; k < ND; ++k)
    if (cl && k == kc && dlen[k] < pp) ysw = dlen[k];
  const int nseg = P.rows.nseg;
  constexpr int NSEG = 2 * ND;
  int segb[NSEG];
#pragma unroll
  for (int i = 0; i < NSEG; ++i) segb[i] = P.rows.seg[i];
  double* const qlines = lines + R * LQ;
  const bool rdel = gl && !zlane && dg > 0;
  const int rsw = (rdel && dg < pp) ? dg : -1;
  double* const zrow = qlines + P.rows.zr_off;  // never written
  double* const r_start = !gl ? zrow
                          : zl0 ? qlines + P.rows.z_off
                          : zl1 ? z1s + R * U * NY
                          : (dg == 0) ? qlines + log_ + (1 - gk) * NY
                                      : zrow;
  double* const r_line = qlines + log_ + (M - 1 - gk) * NY;
  const bool wdel = mk && dm > 0;
  double* const dump = qlines + P.rows.dump_off;
  double* const w_start = !mk ? dump
                          : (dm == 0) ? qlines + lom + NY
                          : (pp - dm > 0) ? qlines + lom + (M - 1) * NY
                                          : dump;
  const int winc0 = (wdel && pp - dm > 0) ? NY : 0;
  const int wsw = (wdel && pp - dm > 0) ? pp - dm : -1;
  const bool tl = mk && dm == 0;  // ring writer: copies each group's last value to entry -1
  double* const tq = qlines + lom;
  double* const zq0 = ol ? qlines + P.rows.z_off + oo : dump;
  double* const zq1 = ol ? z1s + R * U * NY + oo : dump;

  // ---- staging ----
  // Scenario sc of the group occupies doubles [sc sps, (sc + 1) sps) of the
  // wave's region: [one slot's whole record | the other slot's record from t0
  // on].  Every LDS-DMA instruction copies one 1 KiB block (or a lane-masked
  // rest) of one record: a uniform base plus 16 bytes per lane on both sides,
  // so no per-lane source offsets are kept.
  const int t0 = P.pair.tail0, wch = rl >> 1, tch = (rl - t0) >> 1, sps = 2 * rl - t0;
  // head compare: lane l compares entries idx = 64 i + l < hd of slot 1's record
  // against the staged slot-0 entry under the rotation of B's columns (pli)
  const int hd = P.off_x;
  int pli[NCMP];
#pragma unroll
  for (int i = 0; i < NCMP; ++i) {
    const int idx = 64 * i + lane;
    pli[i] = idx;
    if (idx >= P.off_B && idx < P.off_C) {
      const int t = idx - P.off_B, l = t / NUT, c = t - l * NUT;
      pli[i] = P.off_B + l * NUT + (c + NU) % NUT;
    }
  }

  const int share = (ngroups + nwaves - 1) / nwaves;
  const int g_first = blockIdx.x * WPG + wave;
  int done_groups = 0;
  uint32_t shared_scn = 0;
  __builtin_amdgcn_s_setprio(3);
  for (int g = g_first; g < ngroups; g += nwaves) {
    {
      const int level = 3 - (4 * done_groups) / share;  // fair progress (build_rows_kernel.h)
      if (level <= 0) __builtin_amdgcn_s_setprio(0);
      else if (level == 1) __builtin_amdgcn_s_setprio(1);
      else if (level == 2) __builtin_amdgcn_s_setprio(2);
      ++done_groups;
    }
    const int scn = 4 * g + R;
    const bool qv = scn < nscn;
    const int scc = qv ? scn : nscn - 1;
    const int nsc = min(4, nscn - 4 * g);
    const double* gbase = P.lin + (size_t)8 * g * rl;
    // pass h: slot h's records whole, slot 1 - h's from t0 on
    auto stage = [&](int h) {
#pragma unroll
      for (int sc = 0; sc < 4; ++sc) {
        if (sc >= nsc) break;
        const double* rec = gbase + (2 * sc + h) * rl + 2 * lane;
        const double* tal = gbase + (2 * sc + 1 - h) * rl + t0 + 2 * lane;
        double* dst = wreg + sc * sps;
        auto* gp = (__attribute__((address_space(1))) void*)rec;
        auto* lp = (__attribute__((address_space(3))) void*)dst;
        // rec_len <= 384: at most three blocks
        if (wch >= 64) __builtin_amdgcn_global_load_lds(gp, lp, 16, 0, 0);
        else if (lane < wch) __builtin_amdgcn_global_load_lds(gp, lp, 16, 0, 0);
        if (wch >= 128) __builtin_amdgcn_global_load_lds(gp, lp, 16, 1024, 0);
        else if (lane < wch - 64) __builtin_amdgcn_global_load_lds(gp, lp, 16, 1024, 0);
        if (wch >= 192) __builtin_amdgcn_global_load_lds(gp, lp, 16, 2048, 0);
        else if (lane < wch - 128) __builtin_amdgcn_global_load_lds(gp, lp, 16, 2048, 0);
        if (lane < tch)  // tch <= 64 (cmpc_pair_layout)
          __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)tal,
                                           (__attribute__((address_space(3))) void*)(dst + rl), 16, 0, 0);
      }
    };
    const double* lwt = lw_all;  // both sub-controllers' tables are bitwise equal (the host predicate)

    // ---- one round trip: slot 0's records + slot 1's tails -> LDS, slot 1's heads -> registers ----
    // (the previous group's LDS stores have landed before the DMA writes over them)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    stage(0);
    // entries 64 i + lane < 64 NCMP <= rec_len of slot 1's record (those from
    // hd on are masked out of the compare); a partial group's missing
    // scenarios repeat its last one: no branch, no read outside the batch
    uint64_t hv[4][NCMP];
#pragma unroll
    for (int sc = 0; sc < 4; ++sc) {
      const int scl = min(sc, nsc - 1);
#pragma unroll
      for (int i = 0; i < NCMP; ++i)
        hv[sc][i] = reinterpret_cast<const uint64_t*>(gbase + (2 * scl + 1) * rl + 64 * i)[(uint32_t)lane];
    }
    double uo[2][ND], dyr[2][NY];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int k = 0; k < ND; ++k) uo[s][k] = P.u_old[(size_t)(2 * scc + s) * NUT + dinp[k]];
#pragma unroll
      for (int o2 = 0; o2 < NY; ++o2) dyr[s][o2] = 0.0;
    }
    if (P.dy_ref) {
      uint32_t qo = (uint32_t)(2 * scc) * NY;
      asm volatile("" : "+v"(qo));
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int o2 = 0; o2 < NY; ++o2) dyr[s][o2] = P.dy_ref[qo + s * NY + o2];
    }
    pair_wait_dma();
    uint64_t diff = 0ull;
#pragma unroll
    for (int sc = 0; sc < 4; ++sc) {
      const uint64_t* s0 = reinterpret_cast<const uint64_t*>(wreg + min(sc, nsc - 1) * sps);
#pragma unroll
      for (int i = 0; i < NCMP; ++i) {
        const uint64_t x = hv[sc][i] ^ s0[pli[i]];
        diff |= (64 * i + lane < hd) ? x : 0ull;
      }
    }
    const bool mism = __ballot(diff != 0ull) != 0ull;
    if (!mism) shared_scn += (uint32_t)nsc;

    for (int h = 0;; ++h) {  // the shared pass, or pass 0 and pass 1 of a group that differs
      // (opaque copies of the lane's position: what is derived from them is
      // formed here, per pass, and not kept in registers across the group loop)
      int jg = j, Rg = R;
      asm volatile("" : "+v"(jg), "+v"(Rg));
      double* chq = chs + Rg * NY * 16;
      const double* srec = wreg + Rg * sps;  // slot h's record; slot 1 - h's from t0 on behind it
      const int rot = h * NU;               // canonical B column c is slot h's column (c + rot) % NUT
      const double *xa[2], *yv[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const double* tb = (s == h) ? srec : srec + rl - t0;
        xa[s] = tb + P.off_x;
        yv[s] = tb + P.off_y;
      }
      // delay-line inputs of both QPs, AdjustAllDelayedStates applied; zero once
      // the line has drained.  The w tables lie behind the staged records
      // (PairLayout), so they are written while the records are still read.
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int k = 0; k < ND; ++k) {
          double* wk = wtab + ((Rg * 2 + s) * ND + k) * WL;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int t = jg + 16 * i;  // WL <= 64 (cmpc_pair_layout)
            if (t < WL)
              wk[t] = (t < dlen[k]) ? ((t == 0) ? xa[s][ndist + k] : xa[s][boff[k] + t - 1]) - uo[s][k] : 0.0;
          }
        }
      double cs[NY];
#pragma unroll
      for (int o2 = 0; o2 < NY; ++o2) cs[o2] = (j < nobs) ? srec[P.off_C + o2 * nobs + jg] : 0.0;
      constexpr int KX = 16 - NS;
      double kx[2][KX], ky[2][NY];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int d = 0; d < KX; ++d) kx[s][d] = (d < ndist) ? xa[s][d] : 0.0;
#pragma unroll
        for (int o2 = 0; o2 < NY; ++o2) ky[s][o2] = yv[s][o2];
#pragma unroll
        for (int o2 = 0; o2 < NY; ++o2) ky[s][o2] = ky[s][o2] - dyr[s][o2];
      }
      double mP[NS];
      if (st) {
        const double* src = srec + P.off_A + jg;
#pragma unroll
        for (int l = 0; l < NS; ++l) mP[l] = src[l * NS];
      } else if (mk) {
        const double* src = srec + P.off_B + (cm + rot) % NUT;
#pragma unroll
        for (int l = 0; l < NS; ++l) mP[l] = src[l * NUT];
      } else {
#pragma unroll
        for (int l = 0; l < NS; ++l) mP[l] = 0.0;
      }
      double mS[NS + ND], fj = 0.0;
      if (st) {
        const double* arow = srec + P.off_A + jg * NS;
        const double* brow = srec + P.off_B + jg * NUT;
#pragma unroll
        for (int l = 0; l < NS; ++l) mS[l] = arow[l];
#pragma unroll
        for (int k = 0; k < ND; ++k) mS[NS + k] = brow[(dinp[k] + rot) % NUT];
        fj = srec[P.off_f + jg];
      } else {
#pragma unroll
        for (int l = 0; l < NS + ND; ++l) mS[l] = 0.0;
      }
      // every staged read is issued before the first write over the staged records below
      __builtin_amdgcn_sched_barrier(0);

      double pP[NY];
#pragma unroll
      for (int o = 0; o < NY; ++o) {
        double t = 0.0;
#pragma unroll
        for (int o2 = 0; o2 < NY; ++o2)
          if (o2 >= o) t = __builtin_fma(lwt[o * NY + o2], cs[o2], t);
        if (j < nobs) chq[o * 16 + jg] = t;
        pP[o] = st ? t : 0.0;
      }
      double base0 = 0.0, base1 = 0.0, pS0 = 0.0, pS1 = 0.0, yh0 = 0.0, yh1 = 0.0;
      const double *yp0 = zeros, *yp1 = zeros;
      int yinc = 0;
      if (st) {
        base0 = base1 = fj;
        pS0 = pS1 = fj;
        // x_1 = f + Adelay w_0, each slot's delayed inputs in its own order
#pragma unroll
        for (int k = 0; k < ND; ++k) {
          pS0 = __builtin_fma(mS[NS + k], wtab[((Rg * 2 + 0) * ND + k) * WL], pS0);
          pS1 = __builtin_fma(mS[NS + ND - 1 - k], wtab[((Rg * 2 + 1) * ND + k) * WL], pS1);
        }
      } else if (ol) {
#pragma unroll
        for (int l = 0; l < NS; ++l) mS[l] = chq[oo * 16 + l];
        double t[2] = {0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
#pragma unroll
          for (int d = 0; d < KX; ++d)
            if (d < ndist) t[s] = __builtin_fma(chq[oo * 16 + NS + d], kx[s][d], t[s]);
#pragma unroll
          for (int o2 = 0; o2 < NY; ++o2)
            if (o2 >= oo) t[s] = __builtin_fma(lwt[oo * NY + o2], ky[s][o2], t[s]);
        }
        base0 = t[0];
        base1 = t[1];
        const double* yl = ylT + oo * yls;
        yh0 = yl[0];
        yh1 = yl[NY * yls];
        yp0 = yl + 1;
        yp1 = yl + NY * yls + 1;
        yinc = 1;
      } else if (cl) {
        const double* wk0 = wtab + ((Rg * 2 + 0) * ND + kc) * WL;
        const double* wk1 = wtab + ((Rg * 2 + 1) * ND + (ND - 1 - kc)) * WL;
        pS0 = wk0[1];
        yh0 = wk0[2];
        yp0 = wk0 + 3;
        pS1 = wk1[1];
        yh1 = wk1[2];
        yp1 = wk1 + 3;
        yinc = 1;
      }
      // restore the zero areas the staging and the C_hat rows overwrote
#pragma unroll
      for (int c = 0; c < NUT; ++c)
        if (P.delay[c] > 0 && j < (M - 1) * NY) qlines[P.rows.lo[c] + j] = 0.0;
      for (int e = j; e < U * NY; e += 16) qlines[P.rows.zr_off + e] = 0.0;
      if (tl) {
#pragma unroll
        for (int o = 0; o < NY; ++o) tq[o] = 0.0;
      }
      double cv[NY], rd[NY], acc[NC];
#pragma unroll
      for (int o = 0; o < NY; ++o) cv[o] = rd[o] = 0.0;
#pragma unroll
      for (int a = 0; a < NC; ++a) acc[a] = 0.0;
      double* wq = w_start;
      double* rq = r_start;
      int winc = winc0, rinc = 0;

// one horizon step (build_rows_kernel.h, its PIPE and ZL forms): the first
// link groups of the five chains, the gather columns' running sums, then the
// other link groups with the 24 gather FMAs spread between them.
// z1 / z2: the zeroed P accumulators of the coming steps, read from LDS
// CMPC_PAIR_ZDEPTH steps before they are consumed.  1: a step reads the next
// step's set at its end and the head waits for those reads alone
// (lgkmcnt(8): the step's own hand-off traffic stays in flight).  2: it reads
// the set of step u + 2, and no step's first FMA waits on an LDS read.
#define CMPC_PAIR_STEP(u)                                                                  \
  {                                                                                        \
    double aS0 = aN0, aS1 = aN1;                                                           \
    yh0 = yp0[u];                                                                          \
    yh1 = yp1[u];                                                                          \
    double aP[NY];                                                                         \
    _Pragma("unroll") for (int o = 0; o < NY; ++o) aP[o] = z1[o];                          \
    rows_pair_head<NS, NY, ND, NUT, M>(pP, pS0, pS1, mP, mS, aP, aS0, aS1, cv, acc);       \
    __builtin_amdgcn_sched_barrier(0);                                                     \
    _Pragma("unroll") for (int o = 0; o < NY; ++o) cv[o] = __builtin_fma(smask, cv[o], rd[o]); \
    __builtin_amdgcn_sched_barrier(0);                                                     \
    rows_pair_part0<NS, NY, ND, NUT, M>(pP, pS0, pS1, mP, mS, aP, aS0, aS1, cv, acc);      \
    rows_pair_part1<NS, NY, ND, NUT, M>(pP, pS0, pS1, mP, mS, aP, aS0, aS1, cv, acc);      \
    __builtin_amdgcn_sched_barrier(0);                                                     \
    _Pragma("unroll") for (int o = 0; o < NY; ++o) pP[o] = aP[o];                          \
    pS0 = aS0;                                                                             \
    pS1 = aS1;                                                                             \
    if constexpr (CMPC_PAIR_ZDEPTH == 2) {                                                 \
      _Pragma("unroll") for (int o = 0; o < NY; ++o) z1[o] = z2[o];                        \
      _Pragma("unroll") for (int o = 0; o < NY; ++o) z2[o] = zeros[o];                     \
    } else {                                                                               \
      _Pragma("unroll") for (int o = 0; o < NY; ++o) z1[o] = zeros[o];                     \
    }                                                                                      \
    _Pragma("unroll") for (int o = 0; o < NY; ++o) wq[(u) * NY + o] = aP[o];               \
    zq0[(u) * NY] = aS0;                                                                   \
    zq1[(u) * NY] = aS1;                                                                   \
    _Pragma("unroll") for (int o = 0; o < NY; ++o) rd[o] = rq[(u) * NY + o];               \
    aN0 = base0 + yh0;                                                                     \
    aN1 = base1 + yh1;                                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                     \
  }
#define CMPC_PAIR_TAIL()                                        \
  if (tl) {                                                     \
    _Pragma("unroll") for (int o = 0; o < NY; ++o) tq[o] = pP[o]; \
  }

      int r = 0;
      double aN0 = base0 + yh0, aN1 = base1 + yh1;  // start values of the next step's free responses
      double z1[NY], z2[NY];                        // zeroed P accumulators of the coming steps (from LDS)
#pragma unroll
      for (int o = 0; o < NY; ++o) z1[o] = z2[o] = zeros[o];
      for (int sg = 0; sg <= nseg; ++sg) {
        int r_end = pp;
#pragma unroll
        for (int i = 0; i < NSEG; ++i)
          if (i == sg && sg < nseg) r_end = segb[i];
        for (; r + U <= r_end; r += U) {
          CMPC_PAIR_STEP(0)
          CMPC_PAIR_STEP(1)
          CMPC_PAIR_STEP(2)
          CMPC_PAIR_STEP(3)
          CMPC_PAIR_STEP(4)
          CMPC_PAIR_TAIL()
          wq += U * winc;
          rq += U * rinc;
          yp0 += U * yinc;
          yp1 += U * yinc;
        }
        while (r + 2 <= r_end) {
          CMPC_PAIR_STEP(0)
          CMPC_PAIR_STEP(1)
          CMPC_PAIR_TAIL()
          wq += 2 * winc;
          rq += 2 * rinc;
          yp0 += 2 * yinc;
          yp1 += 2 * yinc;
          r += 2;
        }
        for (; r < r_end; ++r) {
          CMPC_PAIR_STEP(0)
          CMPC_PAIR_TAIL()
          wq += winc;
          rq += rinc;
          yp0 += yinc;
          yp1 += yinc;
        }
        if (r == rsw) { rq = r_line; rinc = NY; }
        if (r == wsw) { wq = dump; winc = 0; }
        if (r == ysw) { yp0 = yp1 = zeros; yinc = 0; }
      }
#undef CMPC_PAIR_STEP
#undef CMPC_PAIR_TAIL
#pragma unroll
      for (int o = 0; o < NY; ++o) cv[o] = __builtin_fma(smask, cv[o], rd[o]);
      rows_pair_gacc<NY, NUT, M>(cv, acc);  // row p - 1

      // ---- each slot's H, f, G to its own QP in its own column order ----
      if (qv && gl) {
        constexpr int nuo = NUT - NU, nVo = M * nuo;
        const int k2 = j / NUT, c2 = j - k2 * NUT;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          if (mism && s != h) continue;
          double* out = P.qp + (size_t)(2 * scn + s) * P.qp_len;
          const double* uwt = uw_all + s * NU * NU;
          // slot s's own column a = (ka, ca) is canonical column ka NUT + (ca + s NU) % NUT
          double own[NV];
#pragma unroll
          for (int a = 0; a < NV; ++a) own[a] = acc[(a / NU) * NUT + (a % NU + s * NU) % NUT];
          if (zlane) {
            if (j == NC + s) {
#pragma unroll
              for (int a = 0; a < NV; ++a) out[NV * NV + a] = own[a];  // f
            }
          } else {
            const int cs_ = (c2 + NUT - s * NU) % NUT;  // the lane's column in slot s's order
            if (cs_ < NU) {
#pragma unroll
              for (int a = 0; a < NV; ++a) {  // H = Su' W Su + blkdiag_m(uwt)
                const double rw = (a / NU == k2) ? uwt[(a % NU) * NU + cs_] : 0.0;
                out[a * NV + k2 * NU + cs_] = own[a] + rw;
              }
            } else {
#pragma unroll
              for (int a = 0; a < NV; ++a) out[NV * NV + NV + a * nVo + k2 * nuo + (cs_ - NU)] = own[a];  // G
            }
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
      if (!mism || h == 1) break;
      // pass 1: slot 1's records whole, slot 0's tails
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      stage(1);
      pair_wait_dma();
    }
  }
  if (lane == 0 && shared_scn) atomicAdd(P.pair_cnt, shared_scn);
}

template <int NS, int NY, int NU, int M>
static int pair_launch(const BuildParams& P, hipStream_t s) {
  auto kern = cmpc_build_pair_kernel<NS, NY, CMPC_DIMS_NUT, NU, M, CMPC_DIMS_ND>;
  constexpr int WPG = CMPC_BUILD_WAVES;
  const size_t lds = sizeof(double) * ((size_t)P.rows.lds_block + (size_t)P.pair.per_wave * WPG);
  if (lds > 64 * 1024) cmpc_allow_lds(reinterpret_cast<const void*>(kern), lds);
  const int per_cu = 2;  // two waves per SIMD: the kernel's register budget (cmpc_pair_layout checks the LDS)
  const int nscn = P.nqp / 2;
  const int need = std::max(1, ((nscn + 3) / 4 + WPG - 1) / WPG);
  const int grid = std::max(1, std::min(need, P.cus * per_cu));
  cmpc_launch(kern, dim3(grid), dim3(64 * WPG), lds, s, P);
  return 0;
}
