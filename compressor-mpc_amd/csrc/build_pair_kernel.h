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

// Diagnostic build (tools/rows_timing.py ... pair), as CMPC_ROWS_TIMING in
// build_rows_kernel.h: per-wave s_memtime cycle totals of a group's phases,
// written over the QP output (results invalid).  Slots: 0 staging issue,
// 1 staging wait, 2 head compare, 3 w tables, 4 the rest of the prologue,
// 5 horizon loop, 6 epilogue and back edge.  Reading the counter drains the
// LDS queue, so a phase is charged the latency of what it issued.
#ifndef CMPC_PAIR_TIMING
#define CMPC_PAIR_TIMING 0
#endif
// Two A/B arms of the set-up (profiles/pair_setup_ab).  SETUP_PRIO runs a
// group's staging and set-up at top issue priority and drops to the
// fair-progress level at the first horizon step: the set-up's few VALU no
// longer queue behind the partner wave's FMA stream (headline build 212.9 ->
// 210.1 us; on).  TOUCH reads one dword of every 128-byte line of the wave's
// next group of records at the start of the last horizon segment, so that its
// staging would find them in the L2: 233.7 us, as the row kernel's prefetch
// (off).
#ifndef CMPC_PAIR_SETUP_PRIO
#define CMPC_PAIR_SETUP_PRIO 1
#endif
#ifndef CMPC_PAIR_TOUCH
#define CMPC_PAIR_TOUCH 0
#endif
#if CMPC_PAIR_TIMING
#define CMPC_PT(i)                                         \
  {                                                        \
    __builtin_amdgcn_sched_barrier(0);                     \
    const uint64_t now_ = __builtin_amdgcn_s_memtime();    \
    tsum[i] += now_ - tlast;                               \
    tlast = now_;                                          \
    __builtin_amdgcn_sched_barrier(0);                     \
  }
#else
#define CMPC_PT(i)
#endif

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
#if CMPC_PAIR_TIMING
  uint64_t tsum[7] = {0, 0, 0, 0, 0, 0, 0}, tlast = __builtin_amdgcn_s_memtime();
  const uint64_t t0c = tlast, t0r = __builtin_amdgcn_s_memrealtime();
  int ngrp = 0;
#endif
  __builtin_amdgcn_s_setprio(3);
  float touch[3] = {0.f, 0.f, 0.f};
  for (int g = g_first; g < ngroups; g += nwaves) {
    CMPC_PT(6)  // back edge
    const int level = 3 - (4 * done_groups) / share;  // fair progress (build_rows_kernel.h)
    ++done_groups;
    auto fair_prio = [&]() {
      if (level <= 0) __builtin_amdgcn_s_setprio(0);
      else if (level == 1) __builtin_amdgcn_s_setprio(1);
      else if (level == 2) __builtin_amdgcn_s_setprio(2);
    };
    if (CMPC_PAIR_SETUP_PRIO) __builtin_amdgcn_s_setprio(3);
    else fair_prio();
    const int scn = 4 * g + R;
    const bool qv = scn < nscn;
    const int scc = qv ? scn : nscn - 1;
    const int nsc = min(4, nscn - 4 * g);
    const double* gbase = P.lin + (size_t)8 * g * rl;
    // pass h: slot h's records whole, slot 1 - h's from t0 on
    // (ln: the lane; pass 1 hands in an opaque copy, so that the addresses of
    // its rare restaging are formed there and not kept across the horizon loop)
    auto stage = [&](int h, int ln) {
#pragma unroll
      for (int sc = 0; sc < 4; ++sc) {
        if (sc >= nsc) break;
        const double* rec = gbase + (2 * sc + h) * rl + 2 * ln;
        const double* tal = gbase + (2 * sc + 1 - h) * rl + t0 + 2 * ln;
        double* dst = wreg + sc * sps;
        auto* gp = (__attribute__((address_space(1))) void*)rec;
        auto* lp = (__attribute__((address_space(3))) void*)dst;
        // rec_len <= 384: at most three blocks
        if (wch >= 64) __builtin_amdgcn_global_load_lds(gp, lp, 16, 0, 0);
        else if (ln < wch) __builtin_amdgcn_global_load_lds(gp, lp, 16, 0, 0);
        if (wch >= 128) __builtin_amdgcn_global_load_lds(gp, lp, 16, 1024, 0);
        else if (ln < wch - 64) __builtin_amdgcn_global_load_lds(gp, lp, 16, 1024, 0);
        if (wch >= 192) __builtin_amdgcn_global_load_lds(gp, lp, 16, 2048, 0);
        else if (ln < wch - 128) __builtin_amdgcn_global_load_lds(gp, lp, 16, 2048, 0);
        if (ln < tch)  // tch <= 64 (cmpc_pair_layout)
          __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)tal,
                                           (__attribute__((address_space(3))) void*)(dst + rl), 16, 0, 0);
      }
    };
    const double* lwt = lw_all;  // both sub-controllers' tables are bitwise equal (the host predicate)

    // ---- one round trip: slot 0's records + slot 1's tails -> LDS, slot 1's heads -> registers ----
    // (the previous group's LDS stores have landed before the DMA writes over them)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    stage(0, lane);
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
    CMPC_PT(0)  // staging issue
    pair_wait_dma();
    CMPC_PT(1)  // staging wait
    if (CMPC_PAIR_TOUCH) asm volatile("" ::"v"(touch[0]), "v"(touch[1]), "v"(touch[2]));  // (loaded; not used)
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
    CMPC_PT(2)  // head compare

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
      // ---- set-up: two batches of LDS reads, no branch ----
      // A lane without a role reads the zero slots, or an entry that a lane
      // with the role reads anyway and drops the value by a select; a lane
      // with nothing to store stores to the row's dump slot, as in the loop.
      // A guarded link of an FMA chain is computed and the old accumulator kept
      // by a select where the guard is false, so the chain's bits are those
      // of the guarded form.
      //
      // Batch 1: every read of the staged records.  The w tables' sources are
      // the delay-line inputs of both QPs (entry t of line k: x_aug[ndist + k]
      // at t = 0, then x_aug[boff[k] + t - 1]); a lane whose entry lies past the
      // line's length or the table's reads entry t = 0 instead, which lane 0
      // reads, and its store goes to the dump slot: those table entries are
      // zero from the kernel's start and nothing else writes the tables.
      static_assert(U * NY <= 16, "one zero-restore store per lane");
      static_assert((NUT & (NUT - 1)) == 0, "column rotation by a mask");
      // (the lane's role indices from the opaque copy, as above)
      const int oog = ol ? jg - NS : 0, kcg = cl ? jg - (16 - ND) : 0, cmg = mk ? jg - NS : 0;
      double wv[2][ND][4];
      bool wlive[ND][4];
#pragma unroll
      for (int k = 0; k < ND; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int t = jg + 16 * i;  // WL <= 64 (cmpc_pair_layout)
          wlive[k][i] = t < WL && t < dlen[k];
          const int src = (wlive[k][i] && t > 0) ? boff[k] + t - 1 : ndist + k;
#pragma unroll
          for (int s = 0; s < 2; ++s) wv[s][k][i] = xa[s][src];
        }
      const bool jo = j < nobs;
      double cs[NY];
      {
        const double* src = jo ? srec + P.off_C + jg : zeros;
        const int str = jo ? nobs : 0;
#pragma unroll
        for (int o2 = 0; o2 < NY; ++o2) cs[o2] = src[o2 * str];
      }
      constexpr int KX = 16 - NS;
      double kx[2][KX], ky[2][NY];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int d = 0; d < KX; ++d) kx[s][d] = xa[s][(d < ndist) ? d : 0];
#pragma unroll
        for (int o2 = 0; o2 < NY; ++o2) ky[s][o2] = yv[s][o2];
      }
      double mP[NS];
      {
        const double* src = st ? srec + P.off_A + jg : mk ? srec + P.off_B + ((cmg + rot) & (NUT - 1)) : zeros;
        const int str = st ? NS : mk ? NUT : 0;
#pragma unroll
        for (int l = 0; l < NS; ++l) mP[l] = src[l * str];
      }
      double ma[NS], mb[ND], fj;
      {
        // (16 zero slots: NS, NUT <= 16)
        const double* arow = st ? srec + P.off_A + jg * NS : zeros;
        const double* brow = st ? srec + P.off_B + jg * NUT : zeros;
        const double* frow = st ? srec + P.off_f + jg : zeros;
#pragma unroll
        for (int l = 0; l < NS; ++l) ma[l] = arow[l];
#pragma unroll
        for (int k = 0; k < ND; ++k) mb[k] = brow[(dinp[k] + rot) % NUT];
        fj = *frow;
      }
      double lu[NY][NY];  // L_W' (upper triangle), the same for every lane
#pragma unroll
      for (int o = 0; o < NY; ++o)
#pragma unroll
        for (int o2 = o; o2 < NY; ++o2) lu[o][o2] = lwt[o * NY + o2];
      // every staged read is issued before the first write over the staged records below
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int o2 = 0; o2 < NY; ++o2) ky[s][o2] = ky[s][o2] - dyr[s][o2];

      // the w tables (AdjustAllDelayedStates applied; the entries past a line's
      // length stay zero), then the C_hat rows, which may lie over the dump slots
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int k = 0; k < ND; ++k) {
          double* wk = wtab + ((Rg * 2 + s) * ND + k) * WL;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int t = jg + 16 * i;
            double* dst = wlive[k][i] ? wk + t : dump;
            *dst = wv[s][k][i] - uo[s][k];
          }
        }
      CMPC_PT(3)  // staged reads and w tables
      double pP[NY];
#pragma unroll
      for (int o = 0; o < NY; ++o) {
        double t = 0.0;
#pragma unroll
        for (int o2 = 0; o2 < NY; ++o2)
          if (o2 >= o) t = __builtin_fma(lu[o][o2], cs[o2], t);
        // every lane stores its own entry of the row: an entry from nobs on is
        // never used (below), and a store to the dump slot instead could hit
        // another row's C_hat entry in the same instruction (the rows overlay
        // the hand-off areas, dump slots included)
        chq[o * 16 + jg] = t;
        pP[o] = st ? t : 0.0;
      }

      // Batch 2: what the stores above hand over.  Row oo of C_hat (an output
      // lane's multipliers and its kappa factors), the lane's weight row and
      // y_ref heads, a carrier's w_1 and w_2, a state lane's w_0 of every line.
      const double* yl = ylT + oog * yls;
      const double* wk0 = cl ? wtab + ((Rg * 2 + 0) * ND + kcg) * WL : zeros;
      const double* wk1 = cl ? wtab + ((Rg * 2 + 1) * ND + (ND - 1 - kcg)) * WL : zeros;
      double ch[16], lw[NY], w0[2][ND];
#pragma unroll
      for (int l = 0; l < 16; ++l) ch[l] = chq[oog * 16 + l];
#pragma unroll
      for (int o2 = 0; o2 < NY; ++o2) lw[o2] = lwt[oog * NY + o2];
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int k = 0; k < ND; ++k) w0[s][k] = wtab[((Rg * 2 + s) * ND + k) * WL];
      const double yl0 = yl[0], yl1 = yl[NY * yls];
      const double c01 = wk0[1], c02 = wk0[2], c11 = wk1[1], c12 = wk1[2];
      // the first steps' zeroed P accumulators (CMPC_PAIR_STEP): read here, ahead
      // of the stores below, so that the loop's first head waits like the others
      double z1[NY], z2[NY];
#pragma unroll
      for (int o = 0; o < NY; ++o) z1[o] = z2[o] = zeros[o];
      // restore the zero areas the staging and the C_hat rows overwrote
#pragma unroll
      for (int c = 0; c < NUT; ++c) {
        double* dst = (P.delay[c] > 0 && jg < (M - 1) * NY) ? qlines + P.rows.lo[c] + jg : dump;
        *dst = 0.0;
      }
      qlines[P.rows.zr_off + min(jg, U * NY - 1)] = 0.0;
#pragma unroll
      for (int o = 0; o < NY; ++o) {
        double* dst = tl ? tq + o : dump;
        *dst = 0.0;
      }
      // x_1 = f + Adelay w_0, each slot's delayed inputs in its own order
      double x0 = fj, x1 = fj;
#pragma unroll
      for (int k = 0; k < ND; ++k) {
        x0 = __builtin_fma(mb[k], w0[0][k], x0);
        x1 = __builtin_fma(mb[ND - 1 - k], w0[1][k], x1);
      }
      double kap[2] = {0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int d = 0; d < KX; ++d) {
          const double tn = __builtin_fma(ch[NS + d], kx[s][d], kap[s]);
          kap[s] = (d < ndist) ? tn : kap[s];
        }
#pragma unroll
        for (int o2 = 0; o2 < NY; ++o2) {
          const double tn = __builtin_fma(lw[o2], ky[s][o2], kap[s]);
          kap[s] = (o2 >= oog) ? tn : kap[s];
        }
      }
      double mS[NS + ND];
#pragma unroll
      for (int l = 0; l < NS; ++l) mS[l] = ol ? ch[l] : ma[l];
#pragma unroll
      for (int k = 0; k < ND; ++k) mS[NS + k] = mb[k];
      // (fj, mb, hence x0 and x1, are zero off the state lanes; c01 .. c12 off the carriers)
      const double base0 = ol ? kap[0] : fj, base1 = ol ? kap[1] : fj;
      double pS0 = st ? x0 : c01, pS1 = st ? x1 : c11;
      double yh0 = ol ? yl0 : c02, yh1 = ol ? yl1 : c12;
      const double* yp0 = ol ? yl + 1 : wk0 + 3;
      const double* yp1 = ol ? yl + NY * yls + 1 : wk1 + 3;
      int yinc = (ol || cl) ? 1 : 0;
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
      CMPC_PT(4)  // the rest of the prologue
      if (CMPC_PAIR_SETUP_PRIO) fair_prio();
      for (int sg = 0; sg <= nseg; ++sg) {
        if (CMPC_PAIR_TOUCH && sg == nseg) {
          // the wave's next group (its own again after the last): 8 records, 3 x 64 lines
          // of 128 bytes cover rec_len <= 384; clamped into the group's records
          const int gn = (g + nwaves < ngroups) ? g + nwaves : g;
          const char* nb = reinterpret_cast<const char*>(P.lin + (size_t)8 * gn * rl);
          const int nbytes = 2 * min(4, nscn - 4 * gn) * rl * (int)sizeof(double);
#pragma unroll
          for (int i = 0; i < 3; ++i)
            touch[i] = *reinterpret_cast<const float*>(nb + min((lane + 64 * i) * 128, nbytes - 4));
        }
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
#if CMPC_PAIR_TIMING
#pragma unroll
      for (int a = 0; a < NC; ++a) asm volatile("" ::"v"(acc[a]));  // the stores below are left out
#endif
      CMPC_PT(5)  // horizon loop

      // ---- each slot's H, f, G to its own QP in its own column order ----
      // (addressed from the pass's opaque copies, so that the pointers are formed
      // here and not kept across the horizon loop)
      if (qv && gl && !CMPC_PAIR_TIMING) {
        constexpr int nuo = NUT - NU, nVo = M * nuo;
        const int k2 = jg / NUT, c2 = jg - k2 * NUT;
        const int scg = 4 * g + Rg;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          if (mism && s != h) continue;
          double* out = P.qp + (size_t)(2 * scg + s) * P.qp_len;
          const double* uwt = uw_all + s * NU * NU;
          // slot s's own column a = (ka, ca) is canonical column ka NUT + (ca + s NU) % NUT
          double own[NV];
#pragma unroll
          for (int a = 0; a < NV; ++a) own[a] = acc[(a / NU) * NUT + (a % NU + s * NU) % NUT];
          if (zlane) {
            if (jg == NC + s) {
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
      CMPC_PT(6)  // epilogue
      if (!mism || h == 1) break;
      // pass 1: slot 1's records whole, slot 0's tails
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      int l1 = lane;
      asm volatile("" : "+v"(l1));
      stage(1, l1);
      pair_wait_dma();
      CMPC_PT(1)  // restaging, issue and wait
    }
#if CMPC_PAIR_TIMING
    ++ngrp;
#endif
  }
  if (lane == 0 && shared_scn) atomicAdd(P.pair_cnt, shared_scn);
#if CMPC_PAIR_TIMING
  // one 16-double record per wave, as far as the QP buffer reaches
  const size_t wid = (size_t)blockIdx.x * WPG + wave;
  if (lane == 0 && (wid + 1) * 16 <= (size_t)P.nqp * P.qp_len) {
    const uint64_t t1c = __builtin_amdgcn_s_memtime(), t1r = __builtin_amdgcn_s_memrealtime();
    double* dbg = P.qp + wid * 16;
    for (int i = 0; i < 7; ++i) dbg[i] = (double)tsum[i];
    dbg[7] = 1.0;
    dbg[8] = (double)(t1c - t0c);  // shader cycles of the wave's lifetime
    dbg[9] = (double)(t1r - t0r);  // 100 MHz ticks of the same span
    dbg[10] = (double)t0r;
    dbg[11] = (double)t1r;
    dbg[12] = (double)ngrp;
    dbg[13] = (double)wid;
  }
#endif
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
