/* hc_eval_testing.h -- test hook of the tracking kernels' evaluations (csrc/hc_eval.hpp) as
   csrc/hc_track_body.inc runs them: the prefix tables from the path's own t and sample,
   the right-hand side by the stage kinds of the wave's two paths, and dH/dx through the
   packed tables or the slot-absolute ones; beside include/lu/hc_lu_testing.h, whose solves
   take what these produce.  No reference counterpart. */
#ifndef HC_EVAL_TESTING_H
#define HC_EVAL_TESTING_H

#include "../hc_trifocal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Which tables the evaluations read their operand addresses from, by the kernels that do. */
typedef enum {
    HC_EVAL_VARIANT_PACKED = 0,   /* k_track_small, the abort kernels, the archived ones: the packed tables,
                                     read from the workspace */
    HC_EVAL_VARIANT_ABS = 1,      /* the throughput kernel: the slot-absolute tables, and the finiteness
                                     verdict on the dH/dx entries */
    HC_EVAL_VARIANT_COUNT = 2
} hcEvalVariant;

/* flags: return the values of the evaluations the tracker repeats before a dense re-solve,
   after the slot's dH/dx entry block (all of it but the structural zero, so every word the
   sparse solve may use as scratch) has been overwritten with quiet NaNs */
#define HC_EVAL_REDO 1u

/* kind: the slot is left without a point, as a tracker's slot whose path has ended and that
   found no other: its lanes run the wave's instructions but are not active for the
   right-hand side, and nothing is written for it (its x, target, diff and t are not used
   beyond staging).  This makes a point in an odd slot beside an idle even one possible. */
#define HC_EVAL_KIND_IDLE 2

/* One stage's evaluations at n points, as a tracking kernel runs them.  Point i is served
   by path slot i % 8 of workgroup i / 8, so points 2k and 2k + 1 share a wave as two paths
   do; an odd n leaves the last half-wave idle.  Per point: x (31 values; x[30] is taken as
   1), the sample's target and diff parameters (34 each), t, and the stage kind (0: a
   predictor stage, the right-hand side is the negated dH/dt; 1: the corrector, H;
   HC_EVAL_KIND_IDLE or above: no point).  p(t) is
   staged on the device from target, start_params and t as the tracker stages it.  A wave
   whose two points differ in kind runs the merged right-hand side pass, otherwise the pass
   of its kind.  Hx: n x 30 x 30 row-major, rhs: n x 30.  ent_ok (HC_EVAL_VARIANT_ABS only;
   PACKED leaves it untouched): n x 32, one byte per lane of the point's half-wave: the lane's
   finiteness verdict on the dH/dx entries it computed, before the wave's ballot.  The
   entries are packed over all 32 lanes and any lane may compute any row's, so byte r is not
   row r's verdict, and lanes 30 and 31 have one too.  With HC_EVAL_REDO it is still the
   first evaluation's: the tracker does not take the verdict again.
   unified_index: the reference's padded table, as hc_trifocal_eval_batched takes it.
   HC_ERROR_INVALID_VALUE for a variant outside hcEvalVariant, unknown flag bits, n < 0 or a
   null pointer with n > 0; HC_ERROR_WORKSPACE as hc_trifocal_eval_batched; HC_ERROR_TABLE,
   with the outputs untouched, for a table the compaction rejects.  n == 0 succeeds.  Blocks
   until the kernel has run: the workspace's status is read back. */
hcStatus hc_trifocal_eval_variant_batched(int variant, unsigned flags, int n, const int32_t *unified_index,
                                          const hcComplex *x, const hcComplex *target, const hcComplex *diff,
                                          const hcComplex *start_params, const float *t, const uint8_t *kind,
                                          hcComplex *Hx, hcComplex *rhs, uint8_t *ent_ok, void *workspace,
                                          size_t workspace_bytes, hcStream stream);

#ifdef __cplusplus
}
#endif
#endif /* HC_EVAL_TESTING_H */
