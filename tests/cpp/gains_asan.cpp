// The steady-state gains' host arithmetic (csrc/gains_body.h) under ASan +
// UBSan: both plants, every pair of selection sizes ny, nu = 1 .. 4 with random
// distinct outputs and inputs, seeded pressures, each scenario first brought to
// its equilibrium, then a recycle valve in the dead zone and a state with a NaN
// entry, on heap arrays of exactly the documented sizes.  Checks the
// invariants: a known status, the NaN pattern of the record for that status
// and those sizes, and finite entries everywhere else.  Stand-alone: no
// device, no library.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../compressor-mpc_amd/csrc/gains_body.h"

static const double kXp[11] = {0.916, 1.145, 0.152, 440, 0, 0.916, 1.145, 0.152, 440, 0, 1.12};
static const double kUp[9] = {0.304, 0.43, 1.0, 0, 0.304, 0.43, 1.0, 0, 0.7};
static const double kXs[10] = {0.867, 1.03, 0.176, 395, 0, 0.999, 1.19, 0.176, 395, 0};
static const double kUs[8] = {0.304, 0.405, 1, 0, 0.304, -1, 0.393, 0};

static long g_count[7];
// expected of a scenario at rest: OK, or SINGULAR_G for a square selection whose
// inputs do not reach its outputs independently
constexpr int kRegular = -2, kAny = -1;

template <int PLANT>
static int gains(double p_in, double p_out, const std::vector<int32_t>& out, const std::vector<int32_t>& in,
                 const std::vector<double>& u, const std::vector<double>& x, int expect) {
  const int ny = (int)out.size(), nu = (int)in.size();
  std::vector<double> rec(CMPC_GAIN_LEN, -1.0);
  const int st = cmpc_gn::gn_solve<PLANT>(p_in, p_out, ny, out.data(), nu, in.data(), u.data(), x.data(), rec.data());
  if (st < CMPC_EQ_OK || st > CMPC_GAIN_SINGULAR_G || st == CMPC_EQ_SKIPPED || st == CMPC_EQ_NO_CONVERGENCE) return 1;
  if (expect >= 0 && st != expect) return 2;
  if (expect == kRegular && st != CMPC_EQ_OK && !(ny == nu && st == CMPC_GAIN_SINGULAR_G)) return 2;
  for (int e = 0; e < CMPC_GAIN_LEN; ++e) {
    uint64_t b;
    std::memcpy(&b, &rec[e], sizeof b);
    if (cmpc_gn::gn_keep(e, ny, nu, st) ? !std::isfinite(rec[e]) : b != cmpc_gn::kNanBits) return 3;
  }
  if (st == CMPC_EQ_OK && ny == 4 && nu == 4) {
    // an RGA's rows sum to 1: far looser than rounding, a wrong index is of order 1 (the full
    // selection only: a smaller one may take both inputs of one compressor, whose G is rank-deficient)
    for (int i = 0; i < ny; ++i) {
      double s = 0;
      for (int j = 0; j < nu; ++j) s += rec[cmpc_gn::kRga + i * 4 + j];
      if (!(std::fabs(s - 1.0) < 1e-8)) return 4;
    }
  }
  ++g_count[st];
  return 0;
}

template <int PLANT>
static int run(std::mt19937_64& rng) {
  constexpr int ns = cmpc_eq::Dims<PLANT>::ns, ni = cmpc_eq::Dims<PLANT>::ni;
  std::uniform_real_distribution<double> pr(0.95, 1.05), rec(0.05, 0.2);
  const double* xd = PLANT == CMPC_PLANT_PARALLEL ? kXp : kXs;
  const double* ud = PLANT == CMPC_PLANT_PARALLEL ? kUp : kUs;
  for (int ny = 1; ny <= cmpc_gn::kMaxSel; ++ny) {
    for (int nu = 1; nu <= cmpc_gn::kMaxSel; ++nu) {
      for (int trial = 0; trial < 6; ++trial) {
        std::vector<int32_t> out = {0, 1, 2, 3}, in = {0, 1, 2, 3};
        std::shuffle(out.begin(), out.end(), rng);
        std::shuffle(in.begin(), in.end(), rng);
        out.resize(ny);
        in.resize(nu);
        out.shrink_to_fit();
        in.shrink_to_fit();
        const double p_in = pr(rng), p_out = pr(rng);
        std::vector<double> x(xd, xd + ns), u(ud, ud + ni), resid(2);
        u[3] = rec(rng), u[7] = rec(rng);
        int32_t iters = 0;
        if (cmpc_tg::tg_solve<PLANT>(p_in, p_out, 0, nullptr, nullptr, nullptr, u.data(), x.data(), 20, 1e-12, 1e-10,
                                     &iters, resid.data()) != CMPC_EQ_OK)
          return 100;
        int rc = gains<PLANT>(p_in, p_out, out, in, u, x, kRegular);
        if (rc) return 200 + rc;
        // a recycle valve in the dead zone: DEADZONE exactly when it is selected
        std::vector<double> uz = u;
        uz[3] = 0.01;
        const bool sel = std::find(in.begin(), in.end(), 1) != in.end();
        if ((rc = gains<PLANT>(p_in, p_out, out, in, uz, x, sel ? CMPC_EQ_DEADZONE : kRegular))) return 300 + rc;
        std::vector<double> xn = x;
        xn[trial % ns] = std::numeric_limits<double>::quiet_NaN();
        if ((rc = gains<PLANT>(p_in, p_out, out, in, u, xn, CMPC_EQ_NONFINITE))) return 400 + rc;
        // a zero state: some status, the record's pattern whatever it is
        std::vector<double> xz(ns, 0.0);
        if ((rc = gains<PLANT>(p_in, p_out, out, in, u, xz, kAny))) return 500 + rc;
      }
    }
  }
  return 0;
}

int main() {
  std::mt19937_64 rng(20261024);
  int rc = run<CMPC_PLANT_PARALLEL>(rng);
  if (!rc) rc = run<CMPC_PLANT_SERIAL>(rng);
  if (rc) {
    std::printf("failure %d\n", rc);
    return 1;
  }
  if (!g_count[CMPC_EQ_OK] || !g_count[CMPC_EQ_NONFINITE] || !g_count[CMPC_EQ_DEADZONE]) {
    std::printf("a status was never reached: %ld %ld %ld %ld\n", g_count[0], g_count[2], g_count[3], g_count[5]);
    return 1;
  }
  std::printf("gains_asan ok: OK %ld, NONFINITE %ld, SINGULAR %ld, DEADZONE %ld, SINGULAR_G %ld\n", g_count[0],
              g_count[2], g_count[3], g_count[5], g_count[6]);
  return 0;
}
