// Seeded per-scenario noise (cmpc_noise_*): the arithmetic of
// one draw, shared by the host entry points (abi_free.cpp) and the device
// kernels (noise.hip).  A draw is a pure function of (seed, stream, global
// scenario, step, channel): no generator state, no dependence on the batch
// size or the launch shape.
//
//   bits      Philox4x32-10, key (seed low 32, seed high 32), counter
//             (scenario0 + b, step, pair j = c / 2, stream)
//   uniforms  k1 = (x0 >> 5) 2^26 + (x1 >> 6), k2 likewise from x2, x3;
//             u1 = (k1 + 1) 2^-53 in (0, 1], u2 = k2 2^-53 in [0, 1): exact
//   normals   r = sqrt(-2 log u1); channel 2j is r cospi(2 u2), channel 2j + 1
//             r sinpi(2 u2) (one Box-Muller pair per Philox call)
//   element   s = sigma ? sigma[e] : 1
//             rho:  g = sqrt(1 - rho rho) s;  w = rho w + g z;  d = w
//             else: d = s z
//             out = d == 0 ? base : base + d     (a NULL base counts as 0)
// Products and sums are separate operations in the order written (the tree
// builds with -ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CMPC_NOISE_HD __host__ __device__
#else
#define CMPC_NOISE_HD
#endif

// (seed, stream, scenario0) as the kernels take them
struct NoiseKeyWords {
  uint32_t k0, k1, stream, scenario0;
};

CMPC_NOISE_HD inline void cmpc_philox4x32_10(const uint32_t ctr[4], uint32_t k0, uint32_t k1, uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// the uniforms of pair j of global scenario `scen` at `step`
CMPC_NOISE_HD inline void cmpc_noise_uniforms(const NoiseKeyWords& key, uint32_t scen, uint32_t step, uint32_t j,
                                              double* u1, double* u2) {
  const uint32_t ctr[4] = {scen, step, j, key.stream};
  uint32_t x[4];
  cmpc_philox4x32_10(ctr, key.k0, key.k1, x);
  const uint64_t k1 = ((uint64_t)(x[0] >> 5) << 26) + (x[1] >> 6);
  const uint64_t k2 = ((uint64_t)(x[2] >> 5) << 26) + (x[3] >> 6);
  *u1 = (double)(k1 + 1) * 0x1p-53;
  *u2 = (double)k2 * 0x1p-53;
}

// sin(pi x), cos(pi x) for x in [0, 2).  Device: the math library's sincospi.
// Host: x is reduced exactly to x = q / 2 + t with |t| <= 1/4 (x is a multiple
// of 2^-52, so the difference is exact), then sin and cos of pi t are rotated
// by the quadrant: the only argument error is the rounding of the product pi t.
CMPC_NOISE_HD inline void cmpc_noise_sincospi(double x, double* s, double* c) {
#if defined(__HIP_DEVICE_COMPILE__)
  sincospi(x, s, c);
#else
  const double q = rint(2.0 * x);
  const double a = 3.14159265358979323846 * (x - 0.5 * q);
  const double sa = sin(a), ca = cos(a);
  switch ((int)q & 3) {
    case 0: *s = sa; *c = ca; break;
    case 1: *s = ca; *c = -sa; break;
    case 2: *s = -sa; *c = -ca; break;
    default: *s = -ca; *c = sa; break;
  }
#endif
}

// the Box-Muller pair of (u1, u2): z0 the even channel, z1 the odd one
CMPC_NOISE_HD inline void cmpc_noise_normals(double u1, double u2, double* z0, double* z1) {
  const double r = sqrt(-2.0 * log(u1));
  double s, c;
  cmpc_noise_sincospi(2.0 * u2, &s, &c);
  *z0 = r * c;
  *z1 = r * s;
}

// element e given its normal z (header comment); sigma, rho, base may be null
// (rho non-null needs w)
CMPC_NOISE_HD inline void cmpc_noise_element(double z, size_t e, const double* sigma, const double* rho, double* w,
                                             const double* base, double* out) {
  const double s = sigma ? sigma[e] : 1.0;
  double d;
  if (rho) {
    const double rh = rho[e];
    const double g = sqrt(1.0 - rh * rh) * s;
    const double wn = rh * w[e] + g * z;
    w[e] = wn;
    d = wn;
  } else {
    d = s * z;
  }
  const double b = base ? base[e] : 0.0;
  out[e] = d == 0.0 ? b : b + d;
}
