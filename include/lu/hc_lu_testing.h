/* hc_lu_testing.h -- test hooks of the tracker LU's fused levels
   (csrc/hc_lu.hpp), beside include/hc_trifocal_testing.h, whose hc_lu_candidates
   and hc_lu_struct_pattern they go with.  No reference counterpart. */
#ifndef HC_LU_TESTING_H
#define HC_LU_TESTING_H

#include "../hc_trifocal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The level of pivot step `step` in the forest of independent steps: 0 when no
   earlier step shares a candidate row with it, else one more than the highest
   level among the earlier steps that do; -1 out of range.  Steps of one level
   have pairwise disjoint candidates and commute exactly. */
int hc_lu_step_level(int step);

/* The throughput tracker's solve alone, in the layout of
   hc_cgesv_30x30_batched: the structure-specialised sparse solve with the
   tracker's template arguments and row patterns (hc_lu_struct_pattern), and
   its fallback, the dense solve of the same system, where the sparse solve
   asks for it.  HC_ERROR_INVALID_VALUE, with x untouched, when an entry
   outside the patterns is non-zero (NaN included).  Blocks until the inputs
   are checked. */
hcStatus hc_cgesv_30x30_struct_batched(int n, const hcComplex *A, const hcComplex *b, hcComplex *x,
                                       hcStream stream);

#ifdef __cplusplus
}
#endif
#endif /* HC_LU_TESTING_H */
