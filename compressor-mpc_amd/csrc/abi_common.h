// What every translation unit of the C ABI (abi_*.cpp, include/cmpc.h) shares:
// the error text, the launch check, page-locked staging, and the checks and
// small helpers more than one subsystem uses.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <initializer_list>
#include <string>

#include "dispatch.h"

namespace cmpc_abi {

extern thread_local std::string g_err;  // cmpc_last_error

int fail(const std::string& msg);

#define HIP_TRY(expr)                                                              \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess)                                                          \
      return fail(std::string(#expr) + ": " + hipGetErrorString(e_));             \
  } while (0)

int layout_of(const cmpc_dims* d, cmpc_layout* L);

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(std::string(what) + ": " + hipGetErrorString(e));
  return 0;
}

int plan_mismatch(const char* what);

// Page-locked host buffer for the host-array entry points.  A hipMemcpy from or
// to pageable memory costs ~17 us per call here: the runtime stages it through
// its own bounce buffer (rocprofv3 --hip-trace of the B = 1 harness,
// DESIGN.md §3.6).  From pinned memory it is one DMA.  `busy` is recorded after
// the copies that read the buffer, and the next writer waits on it.
struct PinnedIO {
  char* buf = nullptr;
  char* dev = nullptr;  // the device's address of buf (kernels read it in place)
  size_t cap = 0;
  hipEvent_t busy = nullptr;
  bool pending = false;
};

int pinned_acquire(PinnedIO& p, size_t bytes);
int pinned_release(PinnedIO& p, hipStream_t s);
void pinned_free(PinnedIO& p);

// host -> device: the k arrays (nullptr skipped) are packed into `pin` and
// copied by one DMA to `dev_base`; dev[i] receives each array's device address.
// dev_base == nullptr: no copy, the kernels read the page-locked buffer in
// place (dev[i] = its device address) and the caller calls pinned_release
// after the launch that reads it.
int pinned_upload(PinnedIO& pin, hipStream_t s, double* dev_base, const double* const* host,
                  const size_t* n, int k, const double** dev);

// device -> host: every span with a host array is copied into `pin` (each at
// its own 16-byte aligned offset) on `s`, the stream is synchronised once, and
// the host arrays are filled from the buffer.
struct DownloadSpan {
  const void* dev;
  void* host;  // null: skipped
  size_t bytes;
};
int pinned_download(PinnedIO& pin, hipStream_t s, std::initializer_list<DownloadSpan> spans);
// the same straight into the host arrays (pageable or not), then the one sync
int direct_download(hipStream_t s, std::initializer_list<DownloadSpan> spans);

// p is device memory of `device` and [p, p + bytes) lies inside its
// allocation.  The one query behind every bind check (the context's and the
// noise calls' caches sit on top of it; alignment is the caller's rule).  A
// failed query is not a later launch's error: the runtime's last error is
// cleared before a refusal is returned.
bool device_range_ok(int device, const void* p, size_t bytes);

// a device buffer allocated by the first call that needs it
template <class T>
int ensure_device(T** p, size_t bytes) {
  if (!*p) HIP_TRY(hipMalloc(p, bytes));
  return 0;
}

// B x [p_in, p_out]: finite and positive
int pressures_check(const char* who, const double* p, size_t B);

}  // namespace cmpc_abi
