/* hc_lu_compact_testing.h -- test hooks of the fused solve's compact row
   (csrc/hc_lu_struct.hpp LuRowForm), beside include/lu/hc_lu_rowtable_testing.h.
   A row can hold at most one of the columns 0..17 per level of the forest of
   independent pivot steps, so the throughput tracker keeps it in 16 positions:
   position L < 4 is the row's level-L column, positions 4..15 are columns
   18..29.  No reference counterpart. */
#ifndef HC_LU_COMPACT_TESTING_H
#define HC_LU_COMPACT_TESTING_H

#include "../hc_trifocal.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HC_LU_COMPACT_WIDTH 16

/* The column that position `position` (0..15) of row `row` (0..29) holds; -1
   where the row has no column at that level; -2 out of range. */
int hc_lu_compact_column(int row, int position);

/* The compact rows the throughput tracker's gather produces, at n points: the
   evaluations of hc_trifocal_eval_variant_batched (include/eval/hc_eval_testing.h)
   with HC_EVAL_VARIANT_ABS and no flags, point for point and argument for
   argument, but dH/dx gathered through the compact map that k_prep_tables writes
   beside the 30-column one.  rows: n x 30 x HC_LU_COMPACT_WIDTH, row-major;
   rhs and ent_ok as there.  Errors as there.  Takes no stream: it runs on the
   null stream and blocks until the kernel has run. */
hcStatus hc_trifocal_compact_rows_batched(int n, const int32_t *unified_index, const hcComplex *x,
                                          const hcComplex *target, const hcComplex *diff,
                                          const hcComplex *start_params, const float *t, const uint8_t *kind,
                                          hcComplex *rows, hcComplex *rhs, uint8_t *ent_ok, void *workspace,
                                          size_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* HC_LU_COMPACT_TESTING_H */
