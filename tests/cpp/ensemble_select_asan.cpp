// The selection's host arithmetic (csrc/ensemble_select.h) under ASan + UBSan:
// cmpc_quantiles_host's loops over heap arrays of exactly the documented sizes,
// over random dimensions (len, B, S, levels), against std::sort of the keys.
// Stand-alone: no device, no library.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../compressor-mpc_amd/csrc/ensemble_select.h"

static uint64_t bits(double v) {
  uint64_t u;
  std::memcpy(&u, &v, sizeof u);
  return u;
}

static int run(std::mt19937_64& rng, int len, int B, int S, int T) {
  const double special[] = {0.0, -0.0, std::numeric_limits<double>::infinity(),
                            -std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN(),
                            -std::numeric_limits<double>::quiet_NaN(), 5e-324, -1e300, 1e300};
  std::vector<double> x((size_t)len * B * S), out((size_t)len * S * T * 3), levels(T);
  std::normal_distribution<double> nd;
  for (double& v : x) {
    const unsigned r = (unsigned)(rng() % 24);
    v = r < 9 ? special[r] : r < 16 ? (double)(rng() % 4) : nd(rng);
  }
  for (int l = 0; l < T; ++l) levels[l] = l == 0 ? 0.0 : l == 1 ? 1.0 : (double)(rng() % 1001) / 1000.0;
  std::vector<uint32_t> k_lo(T), k_hi(T);
  std::vector<double> g(T);
  for (int l = 0; l < T; ++l) {
    cmpc_select_rank(B, levels[l], &k_lo[l], &k_hi[l], &g[l]);
    if (k_lo[l] >= (uint32_t)B || k_hi[l] >= (uint32_t)B || k_hi[l] < k_lo[l] || !(g[l] >= 0.0 && g[l] < 1.0)) return 1;
  }
  for (int f = 0; f < len; ++f)
    for (int s = 0; s < S; ++s)
      cmpc_select_row_host(x.data() + (size_t)f * B * S + s, (size_t)S, B, T, k_lo.data(), k_hi.data(),
                           out.data() + ((size_t)f * S + s) * T * 3);
  std::vector<uint64_t> keys(B);
  for (int f = 0; f < len; ++f)
    for (int s = 0; s < S; ++s) {
      for (int b = 0; b < B; ++b) keys[b] = cmpc_select_key(x[(size_t)f * B * S + (size_t)b * S + s]);
      std::vector<uint64_t> sorted(keys);
      std::sort(sorted.begin(), sorted.end());
      for (int l = 0; l < T; ++l) {
        const double* o = out.data() + (((size_t)f * S + s) * T + l) * 3;
        if (bits(o[0]) != bits(cmpc_select_value_of(sorted[k_lo[l]]))) return 2;
        if (bits(o[1]) != bits(cmpc_select_value_of(sorted[k_hi[l]]))) return 3;
        const int arg = (int)(std::find(keys.begin(), keys.end(), sorted[k_lo[l]]) - keys.begin());
        if (o[2] != (double)arg) return 4;
        (void)cmpc_select_interpolate(o[0], o[1], g[l]);
      }
    }
  return 0;
}

int main() {
  // the key map's order and its round trip
  const double order[] = {-std::numeric_limits<double>::infinity(), -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0,
                          1e300, std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN()};
  for (size_t i = 0; i + 1 < sizeof order / sizeof *order; ++i) {
    if (!(cmpc_select_key(order[i]) < cmpc_select_key(order[i + 1]))) {
      std::printf("key order: entry %zu\n", i);
      return 1;
    }
    if (bits(cmpc_select_value_of(cmpc_select_key(order[i]))) != bits(order[i])) {
      std::printf("key round trip: entry %zu\n", i);
      return 1;
    }
  }
  if (cmpc_select_key(-std::numeric_limits<double>::quiet_NaN()) != kSelectNanKey ||
      bits(cmpc_select_value_of(kSelectNanKey)) != 0x7ff8000000000000ull) {
    std::printf("NaN key\n");
    return 1;
  }
  std::mt19937_64 rng(20261020);
  for (int it = 0; it < 300; ++it) {
    const int len = 1 + (int)(rng() % 3), S = 1 + (int)(rng() % 3), T = 1 + (int)(rng() % 8);
    const int B = it < 8 ? 1 + it : 1 + (int)(rng() % 700);
    if (int rc = run(rng, len, B, S, T)) {
      std::printf("len %d B %d S %d levels %d: failure %d\n", len, B, S, T, rc);
      return 1;
    }
  }
  std::printf("ensemble_select_asan ok\n");
  return 0;
}
