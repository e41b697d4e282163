// Row-layout build kernel launcher (the kernel: build_rows_kernel.h).
#include "build_rows_kernel.h"

// four-wave workgroups whose layout admits at most two waves per SIMD run the
// 256-register (WPE = 2) instantiation
#define ROWS_CASE(NS_, NY_, NU_, M_)                                                  \
  if (d.ns == NS_ && d.ny == NY_ && d.nu == NU_ && d.m == M_) {                       \
    if (ring) {                                                                        \
      if (two) return rows_launch<NS_, NY_, NU_, M_, 4, true, 2>(P, s);                \
      if (w == 4) return rows_launch<NS_, NY_, NU_, M_, 4, true>(P, s);                \
      return rows_launch<NS_, NY_, NU_, M_, 2, true>(P, s);                            \
    }                                                                                  \
    if (two) return rows_launch<NS_, NY_, NU_, M_, 4, false, 2>(P, s);                 \
    if (w == 4) return rows_launch<NS_, NY_, NU_, M_, 4, false>(P, s);                 \
    return rows_launch<NS_, NY_, NU_, M_, 2, false>(P, s);                             \
  }

int cmpc_launch_build_rows(const BuildParams& P, const cmpc_dims& d, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (P.use_pair) return cmpc_launch_build_pair(P, d, stream);  // the shared form (cmpc_set_build_pairing)
  const int w = cmpc_build_rows_waves(d, P);  // 4 or 2
  if (!w) return -1;
  const bool ring = rows_has_ring(P.rows);
  const bool two = w == 4 && cmpc_rows_resident_groups(P.rows, 4) * 4 <= 8;
  CMPC_FOR_BUILD_ROWS(ROWS_CASE)
  return -1;
}
