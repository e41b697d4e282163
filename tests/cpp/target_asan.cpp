// The steady-state target solve's host arithmetic (csrc/target_body.h) under
// ASan + UBSan: both plants, nh = 0 .. 4 with random distinct held outputs and
// free inputs, seeded pressures and targets near each scenario's equilibrium,
// every iteration budget from 0 to 6 and the full one, pressures without an
// equilibrium and a free recycle valve in the dead zone, on heap arrays of
// exactly the documented sizes.  Checks the invariants: a known status, iters
// <= max_iter, residuals within the tolerances on OK, and x and u bitwise
// untouched for every other status.  Stand-alone: no device, no library.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../compressor-mpc_amd/csrc/target_body.h"

static const double kXp[11] = {0.916, 1.145, 0.152, 440, 0, 0.916, 1.145, 0.152, 440, 0, 1.12};
static const double kUp[9] = {0.304, 0.43, 1.0, 0, 0.304, 0.43, 1.0, 0, 0.7};
static const double kXs[10] = {0.867, 1.03, 0.176, 395, 0, 0.999, 1.19, 0.176, 395, 0};
static const double kUs[8] = {0.304, 0.405, 1, 0, 0.304, -1, 0.393, 0};

static long g_count[6];

template <int PLANT>
static int solve(double p_in, double p_out, const std::vector<int32_t>& hold, const std::vector<int32_t>& fre,
                 const std::vector<double>& t, std::vector<double>& u, std::vector<double>& x, int max_iter) {
  const std::vector<double> x0 = x, u0 = u;
  std::vector<double> resid(2, -1.0);
  std::vector<int32_t> iters(1, -1);
  const double tol_f = 1e-12, tol_y = 1e-10;
  const int st = cmpc_tg::tg_solve<PLANT>(p_in, p_out, (int)hold.size(), hold.data(), fre.data(), t.data(), u.data(),
                                          x.data(), max_iter, tol_f, tol_y, iters.data(), resid.data());
  if (st < CMPC_EQ_OK || st > CMPC_EQ_DEADZONE || st == CMPC_EQ_SKIPPED) return 1;
  if (iters[0] < 0 || iters[0] > max_iter) return 2;
  if (st == CMPC_EQ_OK) {
    if (!(resid[0] <= tol_f) || !(resid[1] <= tol_y)) return 3;
  } else if (std::memcmp(x.data(), x0.data(), x.size() * sizeof(double)) ||
             std::memcmp(u.data(), u0.data(), u.size() * sizeof(double))) {
    return 4;
  }
  if (st == CMPC_EQ_NO_CONVERGENCE && iters[0] != max_iter) return 5;
  ++g_count[st];
  return 0;
}

template <int PLANT>
static int run(std::mt19937_64& rng) {
  constexpr int ns = cmpc_eq::Dims<PLANT>::ns, ni = cmpc_eq::Dims<PLANT>::ni;
  std::uniform_real_distribution<double> pr(0.95, 1.05), mv(-1.0, 1.0), rec(0.05, 0.2);
  const double* xd = PLANT == CMPC_PLANT_PARALLEL ? kXp : kXs;
  const double* ud = PLANT == CMPC_PLANT_PARALLEL ? kUp : kUs;
  for (int nh = 0; nh <= cmpc_tg::kMaxHold; ++nh) {
    for (int trial = 0; trial < 24; ++trial) {
      std::vector<int32_t> hold = {0, 1, 2, 3}, fre = {0, 1, 2, 3};
      std::shuffle(hold.begin(), hold.end(), rng);
      std::shuffle(fre.begin(), fre.end(), rng);
      hold.resize(nh);
      fre.resize(nh);
      hold.shrink_to_fit();
      fre.shrink_to_fit();
      const double p_in = pr(rng), p_out = pr(rng);
      std::vector<double> x(xd, xd + ns), u(ud, ud + ni), none;
      // trial 0: the recycle valves stay shut, so a free one is in the dead zone
      if (trial > 0) u[3] = rec(rng), u[7] = rec(rng);
      int rc = solve<PLANT>(p_in, p_out, {}, {}, none, u, x, 20);  // to the equilibrium first
      if (rc) return 100 + rc;
      double y[4];
      cmpc_tg::tg_output<PLANT>(x.data(), y);
      std::vector<double> t(nh);
      for (int j = 0; j < nh; ++j) t[j] = y[hold[j]] + 0.02 * mv(rng);
      const int budgets[] = {0, 1, 2, 3, 4, 5, 6, CMPC_EQ_MAX_ITER};
      for (int max_iter : budgets) {
        std::vector<double> xc = x, uc = u;
        if ((rc = solve<PLANT>(p_in, p_out, hold, fre, t, uc, xc, max_iter))) return 200 + rc;
      }
      std::vector<double> xc(xd, xd + ns), uc = u;
      if ((rc = solve<PLANT>(1.0, 1.2, hold, fre, t, uc, xc, 20))) return 300 + rc;
    }
  }
  return 0;
}

int main() {
  std::mt19937_64 rng(20261023);
  int rc = run<CMPC_PLANT_PARALLEL>(rng);
  if (!rc) rc = run<CMPC_PLANT_SERIAL>(rng);
  if (rc) {
    std::printf("failure %d\n", rc);
    return 1;
  }
  if (!g_count[CMPC_EQ_OK] || !g_count[CMPC_EQ_NO_CONVERGENCE] || !g_count[CMPC_EQ_NONFINITE] ||
      !g_count[CMPC_EQ_DEADZONE]) {
    std::printf("a status was never reached: %ld %ld %ld %ld %ld %ld\n", g_count[0], g_count[1], g_count[2],
                g_count[3], g_count[4], g_count[5]);
    return 1;
  }
  std::printf("target_asan ok: OK %ld, NO_CONVERGENCE %ld, NONFINITE %ld, SINGULAR %ld, DEADZONE %ld\n", g_count[0],
              g_count[1], g_count[2], g_count[3], g_count[5]);
  return 0;
}
