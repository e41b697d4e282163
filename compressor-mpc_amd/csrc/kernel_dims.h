// The dimension sets the kernels are instantiated for, each list written once.
// The launchers (cmpc_kernels.hip, build_rows.hip, step_rows.hip,
// solve_rows.hip) expand these lists into their template instantiations; the
// availability predicates (dispatch.cpp) expand them into membership tests.
// Preprocessor only: no HIP, no types.
#pragma once

// Every build-side kernel is instantiated for four plant inputs, two of them
// delayed (the reference's compressor plants).
#define CMPC_DIMS_NUT 4
#define CMPC_DIMS_ND 2

// fused nV = 4 steps on the row build kernel solve one QP per lane (0: per
// 16-lane row; the lane-solver instances are not compiled then)
#ifndef CMPC_FUSED_LANE_SOLVE
#define CMPC_FUSED_LANE_SOLVE 1
#endif

// Build side: (ns, ny, nu, m) and, per kernel family, whether the family has
// an instance for the set.
//   WAVE  one-QP-per-wave build (cmpc_build_kernel), its role-split form too;
//         the predict kernel (predict.hip) is instantiated over this column
//   ROWS  row build (cmpc_build_rows_kernel)
//   SWR   fused step on the wave kernel, row solver in the QP's wave (S = 1)
//   SWL   fused step on the wave kernel, lane solver of wave 0
//   SRR   fused step on the row kernel, row solver inside each group
//   SRL   fused step on the row kernel, lane solver after the groups; where
//         a set has both SRR and SRL, SRL is the one selected
//   CTC   one-launch control step, centralized (S = 1)
//   CTD   one-launch control step, distributed
//                       ns  ny nu m  WAVE ROWS SWR SWL SRR SRL CTC CTD
#define CMPC_BUILD_DIMS(X, F)                                                               \
  X(F, 11, 3, 2, 2, 1, 1, 0, 1, 1, 1, 0, 1) /* parallel coop (outputs <0,1,3>) */          \
  X(F, 11, 2, 2, 2, 1, 1, 0, 1, 1, 1, 0, 1) /* parallel ncoop */                           \
  X(F, 11, 3, 4, 2, 1, 1, 1, 0, 1, 0, 1, 0) /* parallel centralized */                     \
  X(F, 10, 2, 2, 2, 1, 1, 0, 1, 1, 1, 0, 1) /* serial ncoop */                             \
  X(F, 10, 4, 2, 2, 1, 1, 0, 1, 1, 1, 0, 1) /* serial coop (all four outputs) */           \
  X(F, 10, 4, 4, 2, 1, 1, 1, 0, 1, 0, 1, 0) /* serial centralized */                       \
  X(F, 11, 3, 2, 1, 1, 1, 0, 0, 0, 0, 0, 0)                                                 \
  X(F, 11, 3, 2, 3, 1, 0, 0, 0, 0, 0, 0, 0)

#define CMPC_SEL_1(...) __VA_ARGS__
#define CMPC_SEL_0(...)
#define CMPC_COL_WAVE(F, NS, NY, NU, M, WAVE, ROWS, SWR, SWL, SRR, SRL, CTC, CTD) CMPC_SEL_##WAVE(F(NS, NY, NU, M))
#define CMPC_COL_ROWS(F, NS, NY, NU, M, WAVE, ROWS, SWR, SWL, SRR, SRL, CTC, CTD) CMPC_SEL_##ROWS(F(NS, NY, NU, M))
#define CMPC_COL_SWR(F, NS, NY, NU, M, WAVE, ROWS, SWR, SWL, SRR, SRL, CTC, CTD) CMPC_SEL_##SWR(F(NS, NY, NU, M))
#define CMPC_COL_SWL(F, NS, NY, NU, M, WAVE, ROWS, SWR, SWL, SRR, SRL, CTC, CTD) CMPC_SEL_##SWL(F(NS, NY, NU, M))
#define CMPC_COL_SRR(F, NS, NY, NU, M, WAVE, ROWS, SWR, SWL, SRR, SRL, CTC, CTD) CMPC_SEL_##SRR(F(NS, NY, NU, M))
#define CMPC_COL_SRL(F, NS, NY, NU, M, WAVE, ROWS, SWR, SWL, SRR, SRL, CTC, CTD) CMPC_SEL_##SRL(F(NS, NY, NU, M))
#define CMPC_COL_CTC(F, NS, NY, NU, M, WAVE, ROWS, SWR, SWL, SRR, SRL, CTC, CTD) CMPC_SEL_##CTC(F(NS, NY, NU, M))
#define CMPC_COL_CTD(F, NS, NY, NU, M, WAVE, ROWS, SWR, SWL, SRR, SRL, CTC, CTD) CMPC_SEL_##CTD(F(NS, NY, NU, M))

// F(ns, ny, nu, m) for every set of one family
#define CMPC_FOR_BUILD_WAVE(F) CMPC_BUILD_DIMS(CMPC_COL_WAVE, F)
#define CMPC_FOR_BUILD_ROWS(F) CMPC_BUILD_DIMS(CMPC_COL_ROWS, F)
#define CMPC_FOR_STEP_WAVE_ROW(F) CMPC_BUILD_DIMS(CMPC_COL_SWR, F)
#define CMPC_FOR_STEP_WAVE_LANE(F) CMPC_BUILD_DIMS(CMPC_COL_SWL, F)
#define CMPC_FOR_STEP_ROWS_ROW(F) CMPC_BUILD_DIMS(CMPC_COL_SRR, F)
#if CMPC_FUSED_LANE_SOLVE
#define CMPC_FOR_STEP_ROWS_LANE(F) CMPC_BUILD_DIMS(CMPC_COL_SRL, F)
#else
#define CMPC_FOR_STEP_ROWS_LANE(F)
#endif
#define CMPC_FOR_CONTROL_CENT(F) CMPC_BUILD_DIMS(CMPC_COL_CTC, F)
#define CMPC_FOR_CONTROL_DIST(F) CMPC_BUILD_DIMS(CMPC_COL_CTD, F)

// the shared form of the row build (build_pair_kernel.h: one cooperative
// scenario, S = 2, per row): F(ns, ny, nu, m)
#define CMPC_FOR_BUILD_PAIR(F) F(11, 3, 2, 2) /* parallel coop */

// Solve side: F(nV, nu, nVo) of the lane and the row iterate kernels
#define CMPC_FOR_SOLVE(F)                          \
  F(4, 2, 4) /* coop / ncoop, S = 2, m = 2 */      \
  F(8, 4, 0) /* centralized, m = 2 */              \
  F(2, 2, 2) /* m = 1 */                           \
  F(6, 2, 6) /* m = 3 */
// the stand-alone batched solvers (cmpc_qp_solve_batch[_map]): F(n, nu), F(n, nu, nvo)
#define CMPC_FOR_QP_BATCH(F) F(4, 2) F(8, 4)
#define CMPC_FOR_QP_BATCH_MAP(F) F(4, 2, 4) F(6, 2, 6) F(2, 2, 2)
