// The seeded noise's host arithmetic (csrc/noise_body.h) under ASan + UBSan:
// the loops of cmpc_noise_uniforms_host / cmpc_noise_step_host over heap arrays
// of exactly the documented sizes (odd and even n, every optional array left
// out in turn), and the first published known answer of Philox4x32-10.
// Stand-alone: no device, no library.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../compressor-mpc_amd/csrc/noise_body.h"

static int run(int B, int n, bool has_sigma, bool has_rho, bool has_base) {
  const int np = (n + 1) / 2;
  const NoiseKeyWords key{0x12345678u, 0x9abcdef0u, 1u, 0xffffffffu - (uint32_t)(B - 1)};
  std::vector<double> u((size_t)B * np * 2), sigma((size_t)B * n, 0.5), rho((size_t)B * n, -0.75),
      w((size_t)B * n, 0.25), base((size_t)B * n, 1.0), out((size_t)B * n);
  for (uint32_t step : {0u, 0xffffffffu})
    for (int b = 0; b < B; ++b)
      for (int j = 0; j < np; ++j) {
        double* o = u.data() + ((size_t)b * np + j) * 2;
        cmpc_noise_uniforms(key, key.scenario0 + (uint32_t)b, step, (uint32_t)j, o, o + 1);
        if (!(o[0] > 0.0 && o[0] <= 1.0 && o[1] >= 0.0 && o[1] < 1.0)) return 1;
        double z0, z1;
        cmpc_noise_normals(o[0], o[1], &z0, &z1);
        const size_t e = (size_t)b * n + 2 * (size_t)j;
        const double* sg = has_sigma ? sigma.data() : nullptr;
        const double* rh = has_rho ? rho.data() : nullptr;
        const double* bs = has_base ? base.data() : nullptr;
        cmpc_noise_element(z0, e, sg, rh, w.data(), bs, out.data());
        if (2 * j + 1 < n) cmpc_noise_element(z1, e + 1, sg, rh, w.data(), bs, out.data());
      }
  for (double v : out)
    if (!(v == v)) return 2;
  return 0;
}

int main() {
  const uint32_t ctr[4] = {0, 0, 0, 0}, want[4] = {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u};
  uint32_t x[4];
  cmpc_philox4x32_10(ctr, 0, 0, x);
  for (int i = 0; i < 4; ++i)
    if (x[i] != want[i]) {
      std::printf("known answer: word %d is %08x\n", i, x[i]);
      return 1;
    }
  for (int B : {1, 7})
    for (int n : {1, 4, 5})
      for (int m = 0; m < 8; ++m)
        if (int rc = run(B, n, m & 1, m & 2, m & 4)) {
          std::printf("B %d n %d mask %d: failure %d\n", B, n, m, rc);
          return 1;
        }
  std::printf("noise_body_asan ok\n");
  return 0;
}
