/* hc_lu_testing.h -- test hooks of the tracker LU (csrc/hc_lu.hpp): its fused
   levels (csrc/hc_lu_struct.hpp LU_LEVELS, csrc/hc_lu_levels.hpp), and each of its instantiations alone; beside include/hc_trifocal_testing.h, whose hc_lu_candidates
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

/* The instantiations of the tracker's sparse solve (csrc/hc_lu.hpp lu_solve),
   by the kernels that run them: each variant names a tracking kernel's
   parameters (csrc/hc_track.hpp: ABORT, ARCH, LULAT, LUS), and lu_mode() of
   hc_lu.hpp, which the tracking kernels read as well, gives the solve's
   template arguments from them.  A "twin" (LUS = false) is the
   structure-agnostic solve of the kernel named before it, which tracks a table
   whose structure is not the compiled-in one (e.g. the same system with its
   equations permuted). */
typedef enum {
    HC_LU_VARIANT_THROUGHPUT = 0,      /* k_track<false, ...>: no abort, not archived, LULAT 0; the fused levels
                                          (hc_cgesv_30x30_struct_batched) */
    HC_LU_VARIANT_THROUGHPUT_TWIN = 1,
    HC_LU_VARIANT_ABORT = 2,           /* abort, grouped and gated: ABORT, LULAT HC_LU_LATB_COLS */
    HC_LU_VARIANT_ABORT_TWIN = 3,
    HC_LU_VARIANT_SMALL = 4,           /* k_track_small: LULAT HC_SMALL_LAT */
    HC_LU_VARIANT_SMALL_TWIN = 5,
    HC_LU_VARIANT_ARCHIVED = 6,        /* archived PH / PH_CodeOpt / P2C: ARCH, LULAT 0 */
    HC_LU_VARIANT_ARCHIVED_TWIN = 7,   /* (hc_cgesv_30x30_batched's solve) */
    HC_LU_VARIANT_COUNT = 8
} hcLuVariant;

/* One of those solves alone, in the layout of hc_cgesv_30x30_batched, with the
   tracker's fallback: the dense solve of the same system where the sparse one
   asks for it.  The variants with the problem's structure (the even ones) take
   their row patterns from hc_lu_struct_pattern and return
   HC_ERROR_INVALID_VALUE, with x untouched, when an entry outside the patterns
   is non-zero (NaN included); they block until the inputs are checked.  The
   twins take a row's pattern from its non-zero entries and accept any matrix.
   HC_ERROR_INVALID_VALUE for a variant outside hcLuVariant. */
hcStatus hc_cgesv_30x30_variant_batched(int variant, int n, const hcComplex *A, const hcComplex *b, hcComplex *x,
                                        hcStream stream);

#ifdef __cplusplus
}
#endif
#endif /* HC_LU_TESTING_H */
