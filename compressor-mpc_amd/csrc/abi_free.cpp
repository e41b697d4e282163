// The entry points of the C ABI (include/cmpc.h) that need neither a context
// nor a simulator: plan and layout queries, checks, seeded noise, the batched
// QP solve over host arrays.
#include <cmath>
#include <type_traits>
#include <vector>

#include "abi_common.h"
#include "noise_body.h"

using namespace cmpc_abi;

extern "C" {

int cmpc_plan(const cmpc_dims* dims, int cus, int build_variant, int solve_variant, int step_variant, int K,
              uint32_t flags, cmpc_plan_t* plan) {
  if (const char* e = cmpc_plan_or_error(dims, cus, build_variant, solve_variant, step_variant, K, flags, plan))
    return fail(e);
  return 0;
}

int cmpc_layout_of(const cmpc_dims* d, cmpc_layout* L) { return layout_of(d, L); }

int cmpc_weight_factor(int ny, const double* ywt, double* lwt) {
  if (const char* e = cmpc_weight_factor_error(ny, ywt, lwt)) return fail(std::string("cmpc_weight_factor: ") + e);
  return 0;
}

int cmpc_check_pressures(int B, const double* pressures) {
  if (!pressures || B < 1) return fail("cmpc_check_pressures: null array or empty batch");
  return pressures_check("cmpc_check_pressures", pressures, (size_t)B);
}

// Seeded per-scenario noise (include/cmpc.h, noise_body.h, noise.hip).
int cmpc_noise_check(const cmpc_noise_key* key, uint64_t step, int B, int n) {
  if (!key) return fail("cmpc_noise: null key");
  if (B < 1) return fail("cmpc_noise: B must be >= 1");
  if (n < 1) return fail("cmpc_noise: n must be >= 1");
  if (step >> 32) return fail("cmpc_noise: step must be below 2^32 (the counter's word)");
  if ((uint64_t)key->scenario0 + (uint64_t)B > (1ull << 32))
    return fail("cmpc_noise: scenario0 + B must be at most 2^32 (the counter's word)");
  if (((uint64_t)B * (uint64_t)((n + 1) / 2) + 63) / 64 > 0x7fffffffull)
    return fail("cmpc_noise: B * ceil(n / 2) is more than one launch covers");
  return 0;
}

int cmpc_noise_check_params(int B, int n, const double* sigma, const double* rho) {
  if (B < 1 || n < 1) return fail("cmpc_noise_check_params: B and n must be >= 1");
  const size_t m = (size_t)B * n;
  for (size_t e = 0; sigma && e < m; ++e)
    if (!std::isfinite(sigma[e]) || sigma[e] < 0)
      return fail("cmpc_noise_check_params: scenario " + std::to_string(e / n) + ", channel " + std::to_string(e % n) +
                  ": sigma must be finite and >= 0");
  for (size_t e = 0; rho && e < m; ++e)
    if (!(rho[e] >= -1.0 && rho[e] <= 1.0))
      return fail("cmpc_noise_check_params: scenario " + std::to_string(e / n) + ", channel " + std::to_string(e % n) +
                  ": rho must be inside [-1, 1]");
  return 0;
}

static NoiseKeyWords noise_words(const cmpc_noise_key* key) {
  return NoiseKeyWords{(uint32_t)key->seed, (uint32_t)(key->seed >> 32), key->stream, key->scenario0};
}

int cmpc_noise_uniforms_host(const cmpc_noise_key* key, uint64_t step, int B, int n, double* u) {
  if (cmpc_noise_check(key, step, B, n)) return -1;
  if (!u) return fail("cmpc_noise_uniforms_host: null u");
  const NoiseKeyWords k = noise_words(key);
  const int np = (n + 1) / 2;
  for (int b = 0; b < B; ++b)
    for (int j = 0; j < np; ++j) {
      double* o = u + ((size_t)b * np + j) * 2;
      cmpc_noise_uniforms(k, key->scenario0 + (uint32_t)b, (uint32_t)step, (uint32_t)j, o, o + 1);
    }
  return 0;
}

int cmpc_noise_step_host(const cmpc_noise_key* key, uint64_t step, int B, int n, const double* sigma,
                         const double* rho, double* w, const double* base, double* out) {
  if (cmpc_noise_check(key, step, B, n)) return -1;
  if (!out) return fail("cmpc_noise_step_host: null out");
  if (rho && !w) return fail("cmpc_noise_step_host: rho needs the AR(1) state w");
  const NoiseKeyWords k = noise_words(key);
  const int np = (n + 1) / 2;
  for (int b = 0; b < B; ++b)
    for (int j = 0; j < np; ++j) {
      double u1, u2, z0, z1;
      cmpc_noise_uniforms(k, key->scenario0 + (uint32_t)b, (uint32_t)step, (uint32_t)j, &u1, &u2);
      cmpc_noise_normals(u1, u2, &z0, &z1);
      const size_t e = (size_t)b * n + 2 * (size_t)j;
      cmpc_noise_element(z0, e, sigma, rho, w, base, out);
      if (2 * j + 1 < n) cmpc_noise_element(z1, e + 1, sigma, rho, w, base, out);
    }
  return 0;
}

// cmpc_bind_state's check of a device pointer (device_ptr_ok) without a
// context: a device allocation on `device` that holds `bytes` from p on,
// 8-byte aligned.  The last pointers that passed are remembered per host
// thread, as a context remembers its own: the queries cost host time per call.
static bool noise_ptr_ok(int device, const void* p, size_t bytes) {
  struct Entry {
    int dev;
    const void* p;
    size_t bytes;
  };
  static thread_local Entry cache[16];
  static thread_local int n = 0;
  if (reinterpret_cast<uintptr_t>(p) % 8) return false;
  for (int i = 0; i < n && i < 16; ++i)
    if (cache[i].dev == device && cache[i].p == p && cache[i].bytes >= bytes) return true;
  if (!device_range_ok(device, p, bytes)) return false;
  cache[n % 16] = Entry{device, p, bytes};
  ++n;
  return true;
}

static NoiseParams noise_params(const cmpc_noise_key* key, uint64_t step, int B, int n) {
  NoiseParams P{};
  const NoiseKeyWords k = noise_words(key);
  P.k0 = k.k0, P.k1 = k.k1, P.stream = k.stream, P.scenario0 = k.scenario0;
  P.step = (uint32_t)step;
  P.B = B, P.n = n, P.np = (n + 1) / 2;
  return P;
}

static int noise_device(int device) {
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail("cmpc_noise: no such HIP device");
  HIP_TRY(hipSetDevice(device));
  return 0;
}

int cmpc_noise_uniforms(int device, void* stream, const cmpc_noise_key* key, uint64_t step, int B, int n,
                        double* u_dev) {
  if (cmpc_noise_check(key, step, B, n)) return -1;
  if (!u_dev) return fail("cmpc_noise_uniforms: null u");
  if (noise_device(device)) return -1;
  const int np = (n + 1) / 2;
  if (!noise_ptr_ok(device, u_dev, sizeof(double) * (size_t)B * np * 2))
    return fail("cmpc_noise_uniforms: u is not an 8-byte aligned device allocation of B * ceil(n / 2) * 2 doubles "
                "on the device");
  NoiseParams P = noise_params(key, step, B, n);
  P.u = u_dev;
  if (cmpc_launch_noise_uniforms(P, stream)) return plan_mismatch("noise uniforms");
  return check_launch("noise uniforms kernel");
}

int cmpc_noise_step(int device, void* stream, const cmpc_noise_key* key, uint64_t step, int B, int n,
                    const double* sigma_dev, const double* rho_dev, double* w_dev, const double* base_dev,
                    double* out_dev) {
  if (cmpc_noise_check(key, step, B, n)) return -1;
  if (!out_dev) return fail("cmpc_noise_step: null out");
  if (rho_dev && !w_dev) return fail("cmpc_noise_step: rho needs the AR(1) state w");
  if (noise_device(device)) return -1;
  const size_t bytes = sizeof(double) * (size_t)B * n;
  const struct {
    const void* p;
    const char* name;
  } ptrs[] = {{sigma_dev, "sigma"}, {rho_dev, "rho"}, {rho_dev ? w_dev : nullptr, "w"}, {base_dev, "base"},
              {out_dev, "out"}};
  for (const auto& a : ptrs)
    if (a.p && !noise_ptr_ok(device, a.p, bytes))
      return fail(std::string("cmpc_noise_step: ") + a.name +
                  " is not an 8-byte aligned device allocation of B * n doubles on the device");
  NoiseParams P = noise_params(key, step, B, n);
  P.sigma = sigma_dev;
  P.rho = rho_dev;
  P.w = rho_dev ? w_dev : nullptr;
  P.base = base_dev;
  P.out = out_dev;
  if (cmpc_launch_noise_step(P, stream)) return plan_mismatch("noise step");
  return check_launch("noise kernel");
}

int cmpc_qp_solve_batch(int device, int n, int nu, int nqp, const double* H, const double* g,
                        const double* lb, const double* ub, const double* lbA, const double* ubA,
                        const uint32_t* ws_in, int max_chg, double* x, int32_t* status,
                        int32_t* nchg, uint32_t* ws_out, uint8_t* trace, int32_t* ntrace) {
  return cmpc_qp_solve_batch_map(device, n, nu, 0, nqp, H, g, nullptr, nullptr, lb, ub, lbA, ubA, ws_in, max_chg, x,
                                 status, nchg, ws_out, trace, ntrace);
}

// cmpc_qp_solve_batch(_map): host arrays in, host arrays out.  The dimensions
// are checked against the kernel instances before anything is allocated, the
// device buffers are released on every exit path, and only the stream of the
// launch is waited for.
int cmpc_qp_solve_batch_map(int device, int n, int nu, int nvo, int nqp, const double* H, const double* f,
                            const double* G, const double* d, const double* lb, const double* ub,
                            const double* lbA, const double* ubA, const uint32_t* ws_in, int max_chg, double* x,
                            int32_t* status, int32_t* nchg, uint32_t* ws_out, uint8_t* trace, int32_t* ntrace) {
  if (nvo < 0) return fail("cmpc_qp_solve_batch_map: nvo < 0");
  if (nvo > 0 && (!G || !d)) return fail("cmpc_qp_solve_batch_map: G and d required for nvo > 0");
  if (nvo > 0 ? !cmpc_qp_batch_map_supported(n, nu, nvo) : !cmpc_qp_batch_supported(n, nu))
    return fail(nvo > 0 ? "map-form qp batch kernel not instantiated for (n, nu, nvo) = (" + std::to_string(n) +
                              ", " + std::to_string(nu) + ", " + std::to_string(nvo) + ")"
                        : "qp batch kernel not instantiated for (n, nu) = (" + std::to_string(n) + ", " +
                              std::to_string(nu) + ")");
  if (nqp <= 0) return 0;
  HIP_TRY(hipSetDevice(device));
  const size_t q = (size_t)nqp;
  struct Bufs {  // scope guard: every buffer allocated below is freed on return
    std::vector<void*> p;
    ~Bufs() {
      for (void* b : p) (void)hipFree(b);
    }
  } bufs;
  auto alloc = [&](auto** ptr, size_t bytes) -> hipError_t {
    void* v = nullptr;
    const hipError_t e = hipMalloc(&v, bytes ? bytes : 8);
    if (e == hipSuccess) bufs.p.push_back(v);
    *ptr = static_cast<std::remove_pointer_t<decltype(ptr)>>(v);
    return e;
  };
  double *dH, *dg, *dG = nullptr, *dd = nullptr, *dlb, *dub, *dlbA, *dubA, *dx;
  uint32_t *dws, *dwo;
  int32_t *dst, *dnc, *dnt;
  uint8_t* dtr;
  HIP_TRY(alloc(&dH, sizeof(double) * q * n * n));
  HIP_TRY(alloc(&dg, sizeof(double) * q * n));
  if (nvo > 0) {
    HIP_TRY(alloc(&dG, sizeof(double) * q * n * nvo));
    HIP_TRY(alloc(&dd, sizeof(double) * q * nvo));
  }
  HIP_TRY(alloc(&dlb, sizeof(double) * q * n));
  HIP_TRY(alloc(&dub, sizeof(double) * q * n));
  HIP_TRY(alloc(&dlbA, sizeof(double) * q * n));
  HIP_TRY(alloc(&dubA, sizeof(double) * q * n));
  HIP_TRY(alloc(&dx, sizeof(double) * q * n));
  HIP_TRY(alloc(&dws, sizeof(uint32_t) * q));
  HIP_TRY(alloc(&dwo, sizeof(uint32_t) * q));
  HIP_TRY(alloc(&dst, sizeof(int32_t) * q));
  HIP_TRY(alloc(&dnc, sizeof(int32_t) * q));
  HIP_TRY(alloc(&dnt, sizeof(int32_t) * q));
  HIP_TRY(alloc(&dtr, 16 * q));
  HIP_TRY(hipMemcpy(dH, H, sizeof(double) * q * n * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dg, f, sizeof(double) * q * n, hipMemcpyHostToDevice));
  if (nvo > 0) {
    HIP_TRY(hipMemcpy(dG, G, sizeof(double) * q * n * nvo, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dd, d, sizeof(double) * q * nvo, hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy(dlb, lb, sizeof(double) * q * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dub, ub, sizeof(double) * q * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dlbA, lbA, sizeof(double) * q * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dubA, ubA, sizeof(double) * q * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dws, ws_in, sizeof(uint32_t) * q, hipMemcpyHostToDevice));
  QpBatchParams P{dH, dg, dlb, dub, dlbA, dubA, dws, dx, dst, dnc, dnt, dwo, dtr, nqp, max_chg, dG, dd, nvo};
  const int lr = nvo > 0 ? cmpc_launch_qp_batch_map(P, n, nu, nvo, nullptr) : cmpc_launch_qp_batch(P, n, nu, nullptr);
  if (lr) return fail("qp batch kernel not instantiated");
  if (check_launch("qp batch kernel")) return -1;
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipMemcpy(x, dx, sizeof(double) * q * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(status, dst, sizeof(int32_t) * q, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(nchg, dnc, sizeof(int32_t) * q, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(ws_out, dwo, sizeof(uint32_t) * q, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(trace, dtr, 16 * q, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(ntrace, dnt, sizeof(int32_t) * q, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
