// The shared part of the C ABI's host implementation (abi_common.h).
#include "abi_common.h"

#include <algorithm>
#include <cmath>

namespace cmpc_abi {

thread_local std::string g_err;

int fail(const std::string& msg) {
  g_err = msg;
  return -1;
}

int layout_of(const cmpc_dims* d, cmpc_layout* L) {
  if (const char* e = cmpc_layout_error(d, L)) return fail(e);
  return 0;
}

int plan_mismatch(const char* what) {
  return fail(std::string("internal error: plan and launcher disagree (") + what + ")");
}

int pinned_acquire(PinnedIO& p, size_t bytes) {
  if (p.pending) {
    HIP_TRY(hipEventSynchronize(p.busy));
    p.pending = false;
  }
  if (bytes > p.cap) {
    if (p.buf) HIP_TRY(hipHostFree(p.buf));
    p.buf = nullptr;
    p.cap = 0;
    const size_t cap = std::max<size_t>(bytes, 4096);
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&p.buf), cap, hipHostMallocCoherent));
    p.cap = cap;
    void* dv = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&dv, p.buf, 0));
    p.dev = reinterpret_cast<char*>(dv);
  }
  return 0;
}

int pinned_release(PinnedIO& p, hipStream_t s) {
  if (!p.busy) HIP_TRY(hipEventCreateWithFlags(&p.busy, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(p.busy, s));
  p.pending = true;
  return 0;
}

void pinned_free(PinnedIO& p) {
  if (p.pending) (void)hipEventSynchronize(p.busy);
  if (p.buf) (void)hipHostFree(p.buf);
  if (p.busy) (void)hipEventDestroy(p.busy);
  p = PinnedIO{};
}

constexpr size_t kPad = 2;  // keep every array 16-byte aligned
int pinned_upload(PinnedIO& pin, hipStream_t s, double* dev_base, const double* const* host,
                  const size_t* n, int k, const double** dev) {
  size_t tot = 0;
  for (int i = 0; i < k; ++i) tot += host[i] ? (n[i] + kPad - 1) / kPad * kPad : 0;
  if (pinned_acquire(pin, sizeof(double) * std::max<size_t>(tot, 1))) return -1;
  double* h = reinterpret_cast<double*>(pin.buf);
  size_t off = 0;
  for (int i = 0; i < k; ++i) {
    if (dev) dev[i] = nullptr;
    if (!host[i]) continue;
    std::memcpy(h + off, host[i], sizeof(double) * n[i]);
    if (dev) dev[i] = (dev_base ? dev_base : reinterpret_cast<double*>(pin.dev)) + off;
    off += (n[i] + kPad - 1) / kPad * kPad;
  }
  if (!dev_base) return 0;
  if (off) HIP_TRY(hipMemcpyAsync(dev_base, h, sizeof(double) * off, hipMemcpyHostToDevice, s));
  return pinned_release(pin, s);
}

int pinned_download(PinnedIO& pin, hipStream_t s, std::initializer_list<DownloadSpan> spans) {
  auto up = [](size_t v) { return (v + 15) / 16 * 16; };
  size_t off = 0, end = 0;
  for (const DownloadSpan& a : spans) {
    end = off + a.bytes;
    off += up(a.bytes);
  }
  if (pinned_acquire(pin, end)) return -1;
  // device -> page-locked buffer (DMA), then host copies after one sync
  off = 0;
  for (const DownloadSpan& a : spans) {
    if (a.host) HIP_TRY(hipMemcpyAsync(pin.buf + off, a.dev, a.bytes, hipMemcpyDeviceToHost, s));
    off += up(a.bytes);
  }
  HIP_TRY(hipStreamSynchronize(s));
  off = 0;
  for (const DownloadSpan& a : spans) {
    if (a.host) std::memcpy(a.host, pin.buf + off, a.bytes);
    off += up(a.bytes);
  }
  return 0;
}

int direct_download(hipStream_t s, std::initializer_list<DownloadSpan> spans) {
  for (const DownloadSpan& a : spans)
    if (a.host) HIP_TRY(hipMemcpyAsync(a.host, a.dev, a.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

bool device_range_ok(int device, const void* p, size_t bytes) {
  hipPointerAttribute_t a;
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  const bool ok = hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeDevice && a.device == device &&
                  !(hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) == hipSuccess && base &&
                    (uintptr_t)p + bytes > (uintptr_t)base + size);
  if (!ok) (void)hipGetLastError();
  return ok;
}

int pressures_check(const char* who, const double* p, size_t B) {
  for (size_t i = 0; i < 2 * B; ++i)
    if (!std::isfinite(p[i]) || !(p[i] > 0))
      return fail(std::string(who) + ": scenario " + std::to_string(i / 2) +
                  ": pressures must be finite and positive");
  return 0;
}

}  // namespace cmpc_abi

extern "C" const char* cmpc_last_error(void) { return cmpc_abi::g_err.c_str(); }
