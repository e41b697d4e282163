// The plant analysis entry points that run on the host (csrc/abi_analysis.cpp:
// cmpc_plant_equilibrium_host, cmpc_plant_target_host, cmpc_plant_gains_host,
// cmpc_plant_modes_host, cmpc_eig_host, cmpc_target_check, cmpc_gain_check)
// under ASan + UBSan, on heap arrays of exactly the documented sizes: both
// plants, B = 3 at the default operating point, then one bad argument of
// every kind, each refused with its message and nothing written.  Its own
// main; abi_analysis.cpp and abi_common.cpp are compiled in, the rest comes
// from libcmpc.so.  No device is touched.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/cmpc.h"

static int g_fail = 0;

static void expect(bool ok, const char* what) {
  if (ok) return;
  std::printf("FAILED: %s (last error: %s)\n", what, cmpc_last_error());
  ++g_fail;
}

// rc != 0 and the message holds `fragment`
static void refused(int rc, const char* fragment) {
  if (rc != 0 && std::strstr(cmpc_last_error(), fragment)) return;
  std::printf("FAILED: expected a refusal with '%s', got rc %d, '%s'\n", fragment, rc, cmpc_last_error());
  ++g_fail;
}

static void run_plant(int plant) {
  constexpr int B = 3;
  int ns = 0, ni = 0, no = 0, nc = 0;
  expect(cmpc_plant_dims(plant, &ns, &ni, &no, &nc) == 0, "cmpc_plant_dims");
  double x0[16], u0[16];
  expect(cmpc_plant_default(plant, x0, u0) == 0, "cmpc_plant_default");
  std::vector<double> pr(2 * B, 1.0), u((size_t)B * ni), x((size_t)B * ns);
  for (int b = 0; b < B; ++b) {
    std::memcpy(&u[(size_t)b * ni], u0, sizeof(double) * ni);
    std::memcpy(&x[(size_t)b * ns], x0, sizeof(double) * ns);
  }
  std::vector<int32_t> st(B, -1), it(B, -1);

  // equilibrium: the default point is close to one, Newton converges
  std::vector<double> xe = x, res(B, -1.0);
  expect(cmpc_plant_equilibrium_host(plant, B, pr.data(), u.data(), xe.data(), 30, 1e-10, st.data(), it.data(),
                                     res.data()) == 0, "cmpc_plant_equilibrium_host");
  for (int b = 0; b < B; ++b) expect(st[b] == CMPC_EQ_OK && res[b] <= 1e-10, "equilibrium status");

  // target: hold output 3 at its equilibrium value + 1 %, free input 0
  std::vector<double> y(16);
  expect(cmpc_plant_output(plant, xe.data(), y.data()) == 0, "cmpc_plant_output");
  const int32_t hold[1] = {3}, fre[1] = {0};
  std::vector<double> tg(B, y[3] * 1.01), ut = u, xt = xe, res2(2 * B, -1.0);
  expect(cmpc_plant_target_host(plant, B, pr.data(), 1, hold, fre, tg.data(), ut.data(), xt.data(), 30, 1e-10, 1e-10,
                                st.data(), it.data(), res2.data()) == 0, "cmpc_plant_target_host");
  for (int b = 0; b < B; ++b) expect(st[b] >= CMPC_EQ_OK && st[b] <= CMPC_EQ_DEADZONE, "target status");
  // nh = 0: the index and target arrays may be null
  ut = u, xt = x;
  expect(cmpc_plant_target_host(plant, B, pr.data(), 0, nullptr, nullptr, nullptr, ut.data(), xt.data(), 30, 1e-10,
                                1e-10, st.data(), it.data(), res2.data()) == 0, "cmpc_plant_target_host, nh = 0");
  for (int b = 0; b < B; ++b) expect(st[b] == CMPC_EQ_OK, "target status, nh = 0");

  // gains at the equilibrium
  const int32_t out[4] = {0, 1, 2, 3}, in[4] = {0, 1, 2, 3};
  std::vector<double> rec((size_t)B * CMPC_GAIN_LEN, -1.0);
  expect(cmpc_plant_gains_host(plant, B, pr.data(), u.data(), xe.data(), 4, out, 4, in, rec.data(), st.data()) == 0,
         "cmpc_plant_gains_host");
  for (int b = 0; b < B; ++b) expect(st[b] >= CMPC_EQ_OK && st[b] <= CMPC_GAIN_SINGULAR_G, "gains status");

  // modes at the equilibrium, and the same eigenvalue count from cmpc_eig_host on a diagonal matrix
  std::vector<double> wr((size_t)B * ns, 0.0), wi((size_t)B * ns, 0.0), sum((size_t)B * CMPC_MODES_NSUM, 0.0);
  expect(cmpc_plant_modes_host(plant, B, pr.data(), u.data(), xe.data(), CMPC_EIG_MAX_ITER, wr.data(), wi.data(),
                               sum.data(), st.data(), it.data()) == 0, "cmpc_plant_modes_host");
  for (int b = 0; b < B; ++b) expect(st[b] == CMPC_EIG_OK && std::isfinite(wr[(size_t)b * ns]), "modes status");
  std::vector<double> A((size_t)B * ns * ns, 0.0);
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < ns; ++i) A[((size_t)b * ns + i) * ns + i] = -(i + 1.0);
  expect(cmpc_eig_host(ns, B, A.data(), CMPC_EIG_MAX_ITER, wr.data(), wi.data(), st.data(), it.data()) == 0,
         "cmpc_eig_host");
  for (int b = 0; b < B; ++b) {
    double s = 0;
    for (int i = 0; i < ns; ++i) s += wr[(size_t)b * ns + i];
    expect(st[b] == CMPC_EIG_OK && std::fabs(s + ns * (ns + 1) / 2.0) < 1e-9, "eig of a diagonal matrix");
  }

  // refusals of the host forms: nothing is written
  std::fill(st.begin(), st.end(), 77);
  refused(cmpc_plant_equilibrium_host(plant, 0, pr.data(), u.data(), xe.data(), 30, 1e-10, st.data(), it.data(),
                                      res.data()), "cmpc_plant_equilibrium_host: B must be >= 1");
  refused(cmpc_plant_equilibrium_host(plant, B, nullptr, u.data(), xe.data(), 30, 1e-10, st.data(), it.data(),
                                      res.data()), "cmpc_plant_equilibrium_host: null argument");
  refused(cmpc_plant_equilibrium_host(plant, B, pr.data(), u.data(), xe.data(), CMPC_EQ_MAX_ITER + 1, 1e-10, st.data(),
                                      it.data(), res.data()), "max_iter must be in [0, 64]");
  refused(cmpc_plant_equilibrium_host(plant, B, pr.data(), u.data(), xe.data(), 30, 0.0, st.data(), it.data(),
                                      res.data()), "tol must be finite and positive");
  refused(cmpc_plant_target_host(plant, 0, pr.data(), 1, hold, fre, tg.data(), ut.data(), xt.data(), 30, 1e-10, 1e-10,
                                 st.data(), it.data(), res2.data()), "cmpc_plant_target_host: B must be >= 1");
  refused(cmpc_plant_target_host(plant, B, pr.data(), 1, hold, fre, nullptr, ut.data(), xt.data(), 30, 1e-10, 1e-10,
                                 st.data(), it.data(), res2.data()), "cmpc_plant_target_host: null argument");
  refused(cmpc_plant_gains_host(plant, 0, pr.data(), u.data(), xe.data(), 4, out, 4, in, rec.data(), st.data()),
          "cmpc_plant_gains_host: B must be >= 1");
  refused(cmpc_plant_gains_host(plant, B, pr.data(), u.data(), nullptr, 4, out, 4, in, rec.data(), st.data()),
          "cmpc_plant_gains_host: null argument");
  refused(cmpc_plant_modes_host(plant, 0, pr.data(), u.data(), xe.data(), 100, wr.data(), wi.data(), sum.data(),
                                st.data(), it.data()), "cmpc_plant_modes_host: B must be >= 1");
  refused(cmpc_plant_modes_host(plant, B, pr.data(), u.data(), xe.data(), 100, wr.data(), nullptr, sum.data(),
                                st.data(), it.data()), "cmpc_plant_modes_host: null argument");
  refused(cmpc_plant_modes_host(plant, B, pr.data(), u.data(), xe.data(), 0, wr.data(), wi.data(), sum.data(),
                                st.data(), it.data()), "cmpc_plant_modes_host: max_iter must be in [1, 360]");
  for (int b = 0; b < B; ++b) expect(st[b] == 77, "a refused call wrote a status");
}

static void run_checks() {
  const int32_t ok[4] = {0, 1, 2, 3}, neg[2] = {0, -1}, big[2] = {4, 0}, rep[3] = {2, 1, 2};
  const double nan = std::nan("");
  refused(cmpc_plant_equilibrium_host(7, 1, nullptr, nullptr, nullptr, 1, 1.0, nullptr, nullptr, nullptr),
          "cmpc_plant_equilibrium_host: unknown plant");
  refused(cmpc_plant_modes_host(7, 1, nullptr, nullptr, nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr),
          "cmpc_plant_modes_host: unknown plant");
  // cmpc_target_check
  expect(cmpc_target_check(0, 4, ok, ok, 20, 1e-10, 1e-10) == 0, "cmpc_target_check, a good call");
  expect(cmpc_target_check(1, 0, nullptr, nullptr, 0, 1e-10, 1e-10) == 0, "cmpc_target_check, nh = 0");
  refused(cmpc_target_check(2, 1, ok, ok, 20, 1e-10, 1e-10), "cmpc_target_check: unknown plant");
  refused(cmpc_target_check(0, -1, ok, ok, 20, 1e-10, 1e-10), "cmpc_target_check: nh must be in [0, 4]");
  refused(cmpc_target_check(0, 5, ok, ok, 20, 1e-10, 1e-10), "cmpc_target_check: nh must be in [0, 4]");
  refused(cmpc_target_check(0, 1, nullptr, ok, 20, 1e-10, 1e-10), "cmpc_target_check: null index array");
  refused(cmpc_target_check(0, 1, ok, nullptr, 20, 1e-10, 1e-10), "cmpc_target_check: null index array");
  refused(cmpc_target_check(0, 2, neg, ok, 20, 1e-10, 1e-10),
          "cmpc_target_check: hold_idx[1] is not a plant output in [0, 4)");
  refused(cmpc_target_check(0, 2, ok, big, 20, 1e-10, 1e-10),
          "cmpc_target_check: free_idx[0] is not a control input in [0, 4)");
  refused(cmpc_target_check(0, 3, rep, ok, 20, 1e-10, 1e-10), "cmpc_target_check: hold_idx repeats output 2");
  refused(cmpc_target_check(0, 3, ok, rep, 20, 1e-10, 1e-10), "cmpc_target_check: free_idx repeats control input 2");
  refused(cmpc_target_check(0, 1, ok, ok, -1, 1e-10, 1e-10), "cmpc_target_check: max_iter must be in [0, 64]");
  refused(cmpc_target_check(0, 1, ok, ok, 65, 1e-10, 1e-10), "cmpc_target_check: max_iter must be in [0, 64]");
  refused(cmpc_target_check(0, 1, ok, ok, 20, nan, 1e-10), "cmpc_target_check: tol_f must be finite and positive");
  refused(cmpc_target_check(0, 1, ok, ok, 20, 1e-10, -1.0), "cmpc_target_check: tol_y must be finite and positive");
  // cmpc_gain_check
  expect(cmpc_gain_check(1, 4, ok, 3, ok) == 0, "cmpc_gain_check, a good call");
  refused(cmpc_gain_check(-1, 1, ok, 1, ok), "cmpc_gain_check: unknown plant");
  refused(cmpc_gain_check(0, 0, ok, 1, ok), "cmpc_gain_check: ny must be in [1, 4]");
  refused(cmpc_gain_check(0, 1, ok, 5, ok), "cmpc_gain_check: nu must be in [1, 4]");
  refused(cmpc_gain_check(0, 1, nullptr, 1, ok), "cmpc_gain_check: null index array");
  refused(cmpc_gain_check(0, 1, ok, 1, nullptr), "cmpc_gain_check: null index array");
  refused(cmpc_gain_check(0, 2, big, 1, ok), "cmpc_gain_check: out_idx[0] is not a plant output in [0, 4)");
  refused(cmpc_gain_check(0, 3, rep, 1, ok), "cmpc_gain_check: out_idx repeats output 2");
  refused(cmpc_gain_check(0, 1, ok, 2, neg), "cmpc_gain_check: in_idx[1] is not a control input in [0, 4)");
  refused(cmpc_gain_check(0, 1, ok, 3, rep), "cmpc_gain_check: in_idx repeats control input 2");
  // cmpc_eig_host
  double a = 1, wr = 0, wi = 0;
  int32_t st = 0, it = 0;
  expect(cmpc_eig_host(1, 1, &a, 1, &wr, &wi, &st, &it) == 0 && wr == 1.0, "cmpc_eig_host, n = 1");
  refused(cmpc_eig_host(0, 1, &a, 1, &wr, &wi, &st, &it), "cmpc_eig_host: n must be in [1, 12]");
  refused(cmpc_eig_host(13, 1, &a, 1, &wr, &wi, &st, &it), "cmpc_eig_host: n must be in [1, 12]");
  refused(cmpc_eig_host(1, 0, &a, 1, &wr, &wi, &st, &it), "cmpc_eig_host: B must be >= 1");
  refused(cmpc_eig_host(1, 1, nullptr, 1, &wr, &wi, &st, &it), "cmpc_eig_host: null argument");
  refused(cmpc_eig_host(1, 1, &a, 0, &wr, &wi, &st, &it), "cmpc_eig_host: max_iter must be in [1, 360]");
  refused(cmpc_eig_host(1, 1, &a, 361, &wr, &wi, &st, &it), "cmpc_eig_host: max_iter must be in [1, 360]");
}

int main() {
  run_plant(CMPC_PLANT_PARALLEL);
  run_plant(CMPC_PLANT_SERIAL);
  run_checks();
  if (g_fail) {
    std::printf("%d failures\n", g_fail);
    return 1;
  }
  std::printf("analysis_asan ok\n");
  return 0;
}
