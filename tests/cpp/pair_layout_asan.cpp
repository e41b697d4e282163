// Host-side check of the shared-form row build's LDS region
// (compressor-mpc_amd/csrc/rows_layout.cpp, cmpc_pair_layout) under
// AddressSanitizer and UndefinedBehaviorSanitizer, on the row layouts of
// random two-sub-controller dimension sets: every region the kernel
// (build_pair_kernel.h) addresses lies inside the wave's LDS.  A stand-alone
// program built by tests/test_build_pairing.py with rows_layout.cpp
// instrumented; the other symbols come from libcmpc.so.  Prints "ok <n>" or
// the first violation.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../compressor-mpc_amd/csrc/cmpc_internal.h"

static int fail(const char* what, const cmpc_dims& d) {
  std::printf("FAIL %s: ns %d ny %d nu %d m %d p %d S %d delays %d %d %d %d\n", what, d.ns, d.ny, d.nu,
              d.m, d.p, d.S, d.delay[0], d.delay[1], d.delay[2], d.delay[3]);
  return 1;
}

int main(int argc, char** argv) {
  const int n = argc > 1 ? std::atoi(argv[1]) : 400;
  std::mt19937 rng(4321);
  auto pick = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
  int checked = 0, usable = 0;
  for (int it = 0; it < n; ++it) {
    cmpc_dims d{};
    const bool par = pick(0, 1);
    d.ns = par ? 11 : 10;
    d.ndist = 4;
    d.nu_tot = 4;
    d.nu = 2;
    d.S = 2;
    d.ny = pick(0, 1) ? 2 : (par ? 3 : 4);
    d.p = pick(2, 250);
    d.m = pick(1, 2);
    if (d.m > d.p) d.m = d.p;
    d.delay[1] = d.delay[3] = pick(2, 120);
    if (pick(0, 3) == 0) d.delay[3] = pick(2, 120);  // not rotation-invariant: the layout must still be sound
    d.B = 64;
    cmpc_layout L;
    if (cmpc_layout_of(&d, &L)) continue;
    RowsLayout R;
    cmpc_rows_layout(d, L.nd, L.nobs, L.rec_len, &R);
    PairLayout Q;
    cmpc_pair_layout(d, R, L.nd, L.rec_len, L.off_x, &Q);
    ++checked;
    if (!R.ok && Q.ok) return fail("shared form without a row layout", d);
    if (!Q.ok) continue;
    ++usable;
    const int stage = 4 * (2 * L.rec_len - Q.tail0);
    if (Q.tail0 % 2 || Q.tail0 > L.off_x || L.rec_len - Q.tail0 > 128 || L.rec_len > 384 || L.rec_len % 2)
      return fail("staged tail", d);
    if (L.off_x > 64 * CMPC_PAIR_CMP || L.rec_len < 64 * CMPC_PAIR_CMP) return fail("compared head", d);
    if (Q.z1_off < R.w_off || Q.z1_off < 4 * R.LQ || Q.z1_off < R.ch_off + 4 * d.ny * 16 ||
        Q.z1_off + 4 * R.U * d.ny > Q.w_off)
      return fail("slot 1's z entries", d);
    int dmax = 0;
    for (int c = 0; c < d.nu_tot; ++c) dmax = d.delay[c] > dmax ? d.delay[c] : dmax;
    const int need = d.p + 2 + R.U < dmax + 3 ? d.p + 2 + R.U : dmax + 3;  // entries a carrier reads
    if (Q.w_off < stage || Q.WL > 64 || Q.WL < need || Q.w_off + 4 * 2 * L.nd * Q.WL > Q.per_wave)
      return fail("w tables", d);
    // a workgroup's allocation: the request rounded up to 512 B, plus 512 B (rows_layout.cpp)
    if (2 * ((8L * (R.lds_block + 4L * Q.per_wave) + 511) / 512 * 512 + 512) > 160 * 1024)
      return fail("LDS of two workgroups over 160 KB", d);
  }
  std::printf("ok %d checked, %d with a shared-form layout\n", checked, usable);
  return usable > 0 ? 0 : 1;
}
