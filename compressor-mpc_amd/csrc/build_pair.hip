// Shared-form row build launcher (the kernel: build_pair_kernel.h).
#include "build_pair_kernel.h"

#define PAIR_CASE(NS_, NY_, NU_, M_) \
  if (d.ns == NS_ && d.ny == NY_ && d.nu == NU_ && d.m == M_) return pair_launch<NS_, NY_, NU_, M_>(P, s);

int cmpc_launch_build_pair(const BuildParams& P, const cmpc_dims& d, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!P.pair.ok || !P.pair_cnt || !P.pair_cnt_next || P.S != 2 || P.nd != CMPC_DIMS_ND ||
      P.nu_tot != CMPC_DIMS_NUT || rows_has_ring(P.rows))
    return -1;
  CMPC_FOR_BUILD_PAIR(PAIR_CASE)
  return -1;
}
