// Seeded per-scenario noise on the device (cmpc_noise_step,
// cmpc_noise_uniforms).  The draw's arithmetic is
// noise_body.h's, the same text the host entry points compile: counter-based
// Philox4x32-10 bits, exact 53-bit uniforms, one Box-Muller pair per call,
// then the element update (white or AR(1)) fused into the same launch.
//
// One lane per (scenario b, pair j), 64-lane workgroups: the lane draws the
// pair and updates channels 2j and 2j + 1 of scenario b (the sine is dropped
// where 2j + 1 == n).  A lane past the batch returns before any access.  The
// optional arrays are null-pointer branches, uniform over the launch.  A wave's
// loads and stores of one array cover a contiguous run of 64 pairs.  No LDS,
// no cross-lane traffic, no inline assembly.
#include "cmpc_internal.h"
#include "noise_body.h"

namespace {

__global__ __launch_bounds__(64) void cmpc_noise_step_kernel(NoiseParams P) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= (size_t)P.B * P.np) return;
  const uint32_t b = (uint32_t)(i / P.np), j = (uint32_t)(i - (size_t)b * P.np);
  const NoiseKeyWords key{P.k0, P.k1, P.stream, P.scenario0};
  double u1, u2, z0, z1;
  cmpc_noise_uniforms(key, P.scenario0 + b, P.step, j, &u1, &u2);
  cmpc_noise_normals(u1, u2, &z0, &z1);
  const size_t e = (size_t)b * P.n + 2 * (size_t)j;
  cmpc_noise_element(z0, e, P.sigma, P.rho, P.w, P.base, P.out);
  if (2 * (int)j + 1 < P.n) cmpc_noise_element(z1, e + 1, P.sigma, P.rho, P.w, P.base, P.out);
}

__global__ __launch_bounds__(64) void cmpc_noise_uniforms_kernel(NoiseParams P) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= (size_t)P.B * P.np) return;
  const uint32_t b = (uint32_t)(i / P.np), j = (uint32_t)(i - (size_t)b * P.np);
  const NoiseKeyWords key{P.k0, P.k1, P.stream, P.scenario0};
  double u1, u2;
  cmpc_noise_uniforms(key, P.scenario0 + b, P.step, j, &u1, &u2);
  P.u[2 * i] = u1;
  P.u[2 * i + 1] = u2;
}

// workgroups of a launch, 0 where a grid cannot hold them
unsigned noise_blocks(const NoiseParams& P) {
  if (P.B < 1 || P.n < 1 || P.np != (P.n + 1) / 2) return 0;
  const size_t blocks = ((size_t)P.B * P.np + 63) / 64;
  return blocks > 0x7fffffffu ? 0u : (unsigned)blocks;
}

}  // namespace

int cmpc_launch_noise_step(const NoiseParams& P, void* stream) {
  const unsigned blocks = noise_blocks(P);
  if (!blocks || !P.out || (P.rho && !P.w)) return -1;
  cmpc_launch(cmpc_noise_step_kernel, dim3(blocks), dim3(64), 0, (hipStream_t)stream, P);
  return 0;
}

int cmpc_launch_noise_uniforms(const NoiseParams& P, void* stream) {
  const unsigned blocks = noise_blocks(P);
  if (!blocks || !P.u) return -1;
  cmpc_launch(cmpc_noise_uniforms_kernel, dim3(blocks), dim3(64), 0, (hipStream_t)stream, P);
  return 0;
}
