// Host-side check of the kernel selection (compressor-mpc_amd/csrc/dispatch.cpp)
// under AddressSanitizer and UndefinedBehaviorSanitizer: random valid
// dimension sets, batch sizes, CU counts in [1, 512], variants, K and flags;
// every plan checked against the availability predicates.  Built by the
// Makefile's dispatch_asan target with dispatch.cpp and rows_layout.cpp
// instrumented; the other symbols come from libcmpc.so.  The row layout
// search takes 0.6 s per new dimension set under the sanitizers, so the
// dimension sets are drawn from a pool of `npool` (second argument) and the
// batch, CU count, variants and call vary over `n` cases (first argument).
// Prints "ok <n>" or the first violation.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../compressor-mpc_amd/csrc/dispatch.h"

struct Case {
  cmpc_dims d;
  int cus, bv, sv, stv, K;
  bool trace, du_other;
};

static int fail(const char* what, const Case& c) {
  std::printf("FAIL %s: ns %d ny %d nu %d m %d p %d S %d B %d delays %d %d cus %d variants %d %d %d K %d trace %d du_other %d\n",
              what, c.d.ns, c.d.ny, c.d.nu, c.d.m, c.d.p, c.d.S, c.d.B, c.d.delay[1], c.d.delay[3], c.cus, c.bv,
              c.sv, c.stv, c.K, (int)c.trace, (int)c.du_other);
  return 1;
}

int main(int argc, char** argv) {
  const int n = argc > 1 ? std::atoi(argv[1]) : 4000;
  const int npool = argc > 2 ? std::atoi(argv[2]) : 24;
  std::mt19937 rng(2468);
  auto pick = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
  std::vector<cmpc_dims> pool;
  while ((int)pool.size() < npool) {
    cmpc_dims d{};
    const bool par = pick(0, 1);
    d.ns = par ? 11 : 10;
    d.ndist = 4;
    d.nu_tot = 4;
    const int ct = pick(0, 3);  // cent, coop, ncoop, one stand-alone sub-controller
    d.nu = ct == 0 ? 4 : 2;
    d.S = ct == 0 || ct == 3 ? 1 : 2;
    d.ny = ct == 2 ? 2 : (par ? 3 : 4);
    d.p = pick(3, 220);
    d.m = pick(0, 2) ? 2 : ct == 0 ? pick(1, 2) : pick(1, 3);  // mostly the instantiated m = 2
    d.delay[1] = pick(2, 60);
    d.delay[3] = pick(2, 60);
    if (pick(0, 9) == 0) d.delay[0] = pick(2, 20);  // a third delayed input: no build instance
    d.B = 1;
    cmpc_layout L;
    if (cmpc_layout_error(&d, &L) || cmpc_context_dims_error(d, L)) continue;
    pool.push_back(d);
  }
  int planned = 0, refused = 0, fused = 0, control = 0, errors = 0, rows = 0;
  for (int it = 0; it < n; ++it) {
    Case c{};
    c.d = pool[pick(0, npool - 1)];
    const int scale = pick(0, 3);  // batches around the switch points (multiples of the CU count) and far from them
    c.cus = pick(1, 512);
    c.d.B = scale == 0 ? pick(1, 70) : scale == 1 ? std::max(1, c.cus * pick(1, 17) / c.d.S + pick(-2, 2))
                                                  : scale == 2 ? pick(8000, 8300) : pick(1, 70000);
    c.bv = pick(CMPC_BUILD_AUTO, CMPC_BUILD_SPLIT);
    c.sv = pick(CMPC_SOLVE_AUTO, CMPC_SOLVE_ROWS);
    c.stv = pick(CMPC_STEP_AUTO, CMPC_STEP_FUSED);
    if (pick(0, 2) == 0) c.bv = c.sv = c.stv = 0;  // all AUTO more often than one in 36
    c.K = pick(0, 2) * pick(0, 5);
    c.trace = pick(0, 3) == 0;
    c.du_other = pick(0, 5) == 0;
    const cmpc_dims& d = c.d;
    cmpc_layout L;
    if (cmpc_layout_error(&d, &L) || cmpc_context_dims_error(d, L)) return fail("pool dims refused", c);
    const int nqp = d.B * d.S;
    BuildParams P;
    if (cmpc_dispatch_params(d, L, nqp, c.cus, &P)) {
      ++refused;  // record or LDS too long for any build kernel
      continue;
    }
    const cmpc_plan_t pl = cmpc_dispatch_plan(d, L, P, c.bv, c.sv, c.stv, c.K, c.trace, c.du_other);
    // the entry point, from the dimensions alone, gives the same plan
    cmpc_plan_t pe;
    const uint32_t flags = (c.trace ? CMPC_TRACE : 0u) | (c.du_other ? CMPC_PLAN_DU_OTHER : 0u);
    if (cmpc_plan_or_error(&d, c.cus, c.bv, c.sv, c.stv, c.K, flags, &pe)) return fail("cmpc_plan refused", c);
    if (std::memcmp(&pl, &pe, sizeof pl)) return fail("cmpc_plan differs from cmpc_dispatch_plan", c);
    ++planned;
    fused += pl.step_fused;
    control += pl.control_fused;
    errors += pl.build_error || pl.solve_error || pl.step_error;
    rows += pl.build_kernel == CMPC_BUILD_ROWS;

    const bool strace = c.trace && c.K > 0;
    const bool wave_ok = cmpc_build_wave_available(d, P), rows_ok = cmpc_build_rows_available(d, P);
    const bool lane_ok = cmpc_solve_lane_available(L.nV, d.nu, L.nVo, P.qp_len, strace, c.du_other);
    const bool srows_ok = cmpc_solve_rows_available(L.nV, d.nu, L.nVo, d.S, P.qp_len, strace, c.du_other);

    // 1. the plan never names a kernel whose availability predicate is false
    if ((pl.build_kernel != 0) == (pl.build_error != 0)) return fail("build: kernel xor error", c);
    if (pl.build_kernel == CMPC_BUILD_ROWS && !rows_ok) return fail("row build named, not available", c);
    if ((pl.build_kernel == CMPC_BUILD_WAVE || pl.build_kernel == CMPC_BUILD_SPLIT) && !wave_ok)
      return fail("wave / split build named, not available", c);
    if ((pl.solve_kernel != 0) == (pl.solve_error != 0)) return fail("solve: kernel xor error", c);
    if (pl.solve_kernel == CMPC_SOLVE_ROWS && !srows_ok) return fail("row solve named, not available", c);
    if (pl.solve_kernel == CMPC_SOLVE_LANE && !lane_ok) return fail("lane solve named, not available", c);
    if (pl.step_fused) {
      const int s = pl.step_build_kernel == CMPC_BUILD_WAVE   ? cmpc_step_wave_solver(d, P)
                    : pl.step_build_kernel == CMPC_BUILD_ROWS ? cmpc_step_rows_solver(d, P)
                                                              : 0;
      if (!s || s != pl.step_solve_kernel) return fail("fused step named, not available", c);
      if (c.K == 0 || pl.step_error) return fail("fused step with K = 0 or an error", c);
    } else if (pl.step_build_kernel != pl.build_kernel || pl.step_solve_kernel != pl.solve_kernel) {
      return fail("two-launch step differs from build + solve", c);
    }
    if (pl.control_fused) {
      const bool split = pl.control_build_kernel == CMPC_BUILD_SPLIT;
      if (!split && pl.control_build_kernel != CMPC_BUILD_WAVE) return fail("control step build kernel", c);
      if (pl.control_grid < 1 || (long long)pl.control_grid * (split ? 2 : 4) < nqp)
        return fail("control step grid does not cover the batch", c);
      const int s = cmpc_control_solver(d, P, split, pl.control_grid, false,
                                        cmpc_control_pr_off(d.S, L.rec_len, L.naug));
      if (!s || s != pl.control_solve_kernel) return fail("control step named, not available", c);
      if (pl.control_polled != (pl.control_grid == 1)) return fail("polled completion off one workgroup", c);
      if (c.K == 0 || c.stv == CMPC_STEP_SPLIT || c.bv || c.sv) return fail("control step fused against the variants", c);
    } else if (pl.control_build_kernel != pl.step_build_kernel || pl.control_solve_kernel != pl.step_solve_kernel ||
               pl.control_grid || pl.control_polled) {
      return fail("three-call control step differs from the step", c);
    }

    // 2. forcing a variant yields that variant or an error
    if (c.bv != CMPC_BUILD_AUTO && pl.build_kernel != c.bv && !pl.build_error) return fail("forced build ignored", c);
    if (c.sv != CMPC_SOLVE_AUTO && pl.solve_kernel != c.sv && !pl.solve_error) return fail("forced solve ignored", c);
    if (c.stv == CMPC_STEP_SPLIT && pl.step_fused) return fail("forced split step fused", c);
    if (c.stv == CMPC_STEP_FUSED && c.K > 0 && L.nuo == (d.S - 1) * d.nu && !pl.step_fused && !pl.step_error)
      return fail("forced fused step ignored", c);

    // 3. AUTO never fails where the wave build and the lane solve have an instance
    if (c.bv == CMPC_BUILD_AUTO && wave_ok && pl.build_error) return fail("AUTO build error", c);
    if (c.sv == CMPC_SOLVE_AUTO && lane_ok && pl.solve_error) return fail("AUTO solve error", c);
    if (c.stv != CMPC_STEP_FUSED && pl.step_error) return fail("step error without FUSED", c);
  }
  // (the cases must reach every kind of outcome, or the checks above are idle)
  if (!fused || !control || !errors || !rows) {
    std::printf("FAIL coverage: %d fused steps, %d one-launch control steps, %d errors, %d row builds\n", fused,
                control, errors, rows);
    return 1;
  }
  std::printf("ok %d planned (%d fused steps, %d one-launch control steps, %d row builds, %d with an error), "
              "%d without a build kernel, %d dimension sets\n", planned, fused, control, rows, errors, refused, npool);
  return 0;
}
