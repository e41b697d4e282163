// Fused small-batch steps on the row build kernel (build_rows_kernel.h):
// the build kernel runs the K Jacobi iterations of the QPs it built (one
// per lane after its groups, or one per 16-lane row inside each group).
// Compiled with the solver objects' flags (Makefile SOLVERFLAGS).
#include "build_rows_kernel.h"

#define DIMS_ARE(NS_, NY_, NU_, M_) (d.ns == NS_ && d.ny == NY_ && d.nu == NU_ && d.m == M_)

// fused build + K iterations with the row solver inside each group:
// four-wave workgroups at one wave per SIMD (the row solver's state on top of
// the build's live registers)
#define ROWS_FUSED_CASE(NS_, NY_, NU_, M_)                                             \
  if (DIMS_ARE(NS_, NY_, NU_, M_)) {                                                   \
    if (ring) {                                                                        \
      if (trace) return rows_launch<NS_, NY_, NU_, M_, 4, true, 1, 2>(P, s);          \
      return rows_launch<NS_, NY_, NU_, M_, 4, true, 1, 1>(P, s);                     \
    }                                                                                  \
    if (trace) return rows_launch<NS_, NY_, NU_, M_, 4, false, 1, 2>(P, s);           \
    return rows_launch<NS_, NY_, NU_, M_, 4, false, 1, 1>(P, s);                      \
  }
// the same with the lane solver (nV <= 4: faster than the row solver there):
// a wave solves its groups' QPs after building them all, one QP per lane
#define ROWS_FUSED_LANE_CASE(NS_, NY_, NU_, M_)                                        \
  if (DIMS_ARE(NS_, NY_, NU_, M_)) {                                                   \
    if (trace) return rows_launch<NS_, NY_, NU_, M_, 4, false, 2, 4>(P, s);           \
    return rows_launch<NS_, NY_, NU_, M_, 4, false, 2, 3>(P, s);                      \
  }

int cmpc_launch_step_rows(const BuildParams& P, const cmpc_dims& d, int solver, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!solver || solver != cmpc_step_rows_solver(d, P)) return -1;
  const bool ring = rows_has_ring(P.rows);
  const bool trace = P.sv.trace != nullptr;
  if (solver == CMPC_SOLVE_LANE) {
    CMPC_FOR_STEP_ROWS_LANE(ROWS_FUSED_LANE_CASE)
  } else {
    CMPC_FOR_STEP_ROWS_ROW(ROWS_FUSED_CASE)
  }
  return -1;
}
