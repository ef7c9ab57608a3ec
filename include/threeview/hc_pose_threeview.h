/*
 * hc_pose_threeview.h -- the trifocal pose and its scale refined jointly in
 * three views, on the device (not in the reference).
 *
 * The refinement of refine/hc_pose_refine.h fits view 2 and view 3 separately
 * and scale/hc_pose_scale.h then takes scale31 from one edgel's proposal.  The
 * mode below adds a third stage that ties them together: Gauss-Newton on eleven
 * local parameters -- view 2's five, view 3's five and the log of the scale --
 * over the edgels the pose explains in all three views, with the view-2 pixel
 * residual and the three-view transfer residual stacked.  The iterate under
 * which the most triangulated edgels land within 2 px of their view-3
 * observation is returned.
 *
 * A header of its own, beside scale/hc_pose_scale.h (same rules of the
 * boundary).  It declares no function: the stage is a mode of the four refine
 * calls (hc_trifocal_pose_refine, _grouped, hc_trifocal_pose_refine_topk,
 * _topk_grouped), selected by hcRefineSettings::pad, and no struct of the other
 * headers changes for it (the ABI version stays 2).
 *
 * The rule.  The state is double: R21, t21, R31, t31 (unit translations) and
 * s > 0; iterate 0 is the floats of the selection that the two-view refinement
 * (stage 1) and the scale vote (stage 2) produced, widened, s the voted
 * scale31.  The local parameters are (w2, u2, w3, u3, sigma):
 *     w in R^3:  R <- Exp(w) R
 *     u in R^2:  t <- normalize(t + u0 b1 + u1 b2), b1 and b2 as in
 *                refine/hc_pose_refine.h
 *     sigma:     s <- s exp(sigma)
 * For k = 0, 1, ..., iterations3:
 *   1. The state and s are rounded to float, element by element, and the
 *      float32 operations of scale/hc_pose_scale.h are applied to those floats:
 *      its step 1 gives the joint mask m, its step 2 rho, Y and the tested set
 *      (m and rho > 0), its step 3 Z and T(e, s).  The fit set is
 *      F = tested and Z2 > 0, the transfer count c_T = |{e in F : T(e, s)}|.
 *      The joint count and the per-view counts are those of the refinement.
 *      Every count is an integer function of the floats.
 *   2. If c_T >= the best so far, this iterate becomes the best (a tie goes to
 *      the later iterate): its 24 pose floats, its float s and its counts.
 *   3. The loop ends when |F| < min_inliers (HC_THREEVIEW_TOO_FEW) or
 *      k == iterations3.
 *   4. Over e in F, in double at the double state, four residual rows:
 *        rows 0, 1: the view-2 pixel residual of the refinement (reprojected
 *                   minus observed); it depends on (w2, u2);
 *        rows 2, 3: the transfer residual
 *                     Z = R31 (rho (g0, g1, 1)) + s t31
 *                     ((Z0 / Z2) K0 + K2) - (q0 K0 + K2),
 *                     ((Z1 / Z2) K4 + K5) - (q1 K4 + K5)
 *                   with rho the view-1-2 depth in double; it depends on all
 *                   eleven parameters.
 *      The rows are differentiated analytically and summed into A = sum J'J
 *      (66 upper entries), g = sum J'r (11) and the squared error of each row
 *      pair.  Every thread sums a fixed set of edgels and the reduction tree is
 *      fixed (the lanes of a wave by an xor butterfly, then the four waves as
 *      (w0 + w1) + (w2 + w3)): two calls give the same bits.
 *   5. (A + 1e-9 diag A) d = -g is solved by Cholesky in double and d is
 *      applied.  A pivot that is not positive or a value that is not finite
 *      ends the loop with HC_THREEVIEW_SINGULAR.
 * Output: the selection carries the best iterate -- its pose floats, scale31 =
 * (float) s, and inliers, inliers21, inliers31 and key re-scored for it.  A
 * selection whose best iterate is 0 keeps the values it came in with, bit for
 * bit.
 */
#ifndef HC_POSE_THREEVIEW_H
#define HC_POSE_THREEVIEW_H

#include "../scale/hc_pose_scale.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hcRefineSettings::pad[0] of settings that are the head of an
   hcRefineThreeViewSettings ("TV31"). */
#define HC_REFINE_THREEVIEW 0x54563331

/* hcRefineSettings::pad[1] in that mode: mode bits (any other bit is refused) */
#define HC_THREEVIEW_SELECT_BY_TRANSFER 2   /* the top-k calls only: best = the largest final transfer key */

/* hcThreeViewReport::status bits */
#define HC_THREEVIEW_NONE     1   /* the selection has no path: passed through                              */
#define HC_THREEVIEW_TOO_FEW  2   /* an iterate's fit set had fewer than min_inliers edgels                  */
#define HC_THREEVIEW_SINGULAR 4   /* a pivot was not positive, or a value not finite                        */
#define HC_THREEVIEW_SKIPPED  8   /* stage 2 fitted no scale (HC_SCALE_NONE, HC_SCALE_NO_VOTER): its output */

/* What one three-view refinement did (device memory, written by the entry point). */
typedef struct {
    int32_t status;             /* HC_THREEVIEW_* bits, 0: the loop ran to its end                           */
    int32_t iterations_run;     /* steps applied = the index of the last iterate scored                      */
    int32_t best_iteration;     /* the iterate returned                                                      */
    int32_t transfer_history[HC_REFINE_MAX_ITERATIONS + 1];   /* c_T of iterate k, -1 beyond the last scored */
    int32_t joint_history[HC_REFINE_MAX_ITERATIONS + 1];      /* its joint count, -1 beyond the last scored  */
    int32_t fit_set;            /* |F| of the best iterate (0 when skipped)                                  */
    int32_t transfer_inliers;   /* c_T of the best iterate (0 when skipped)                                  */
    float scale_in;             /* scale31 as stage 2 left it                                                */
    float scale_out;            /* as it went out                                                            */
    int32_t pad;
    double rms_px_in[2];        /* RMS (px) of the view-2 rows, the transfer rows over iterate 0's fit set   */
    double rms_px_out[2];       /* the same of the best iterate over its own fit set (0 without one)         */
} hcThreeViewReport;            /* 328 bytes */

/* The settings of the mode.  The caller sets head.pad[0] = HC_REFINE_THREEVIEW,
   head.pad[1] to the mode bits, and passes (const hcRefineSettings *)&settings
   (a HOST pointer, read before the call returns) to a refine call.  The call
   then, on the same stream,
     1. refines every selection as refine/hc_pose_refine.h says (head.iterations,
        head.min_inliers; the hcRefineReport argument as without the mode),
     2. fits its scale31 by the vote of scale/hc_pose_scale.h and writes
        scale_reports[i] as that header says,
     3. runs the rule above for iterations3 steps (0: the default, 10; at most
        HC_REFINE_MAX_ITERATIONS) with head.min_inliers and writes reports[i].
   scale_reports and reports are DEVICE pointers, one entry per selection (1,
   num_groups, k or num_groups * k, in the order of out / refined), both
   required.  A selection for which stage 2 reports HC_SCALE_NONE or
   HC_SCALE_NO_VOTER is stage 2's output: status HC_THREEVIEW_SKIPPED (and
   HC_THREEVIEW_NONE without a path), the histories -1.
   transfer_mask (a DEVICE pointer or NULL; hc_trifocal_pose_refine only, NULL in
   the three other calls): (num_edgels + 63) / 64 words, bit e % 64 of word
   e / 64 set iff e is in F and T(e, out->scale31) holds under the pose that
   went out; the number of set bits is transfer_inliers.  All words are 0 when
   the stage was skipped.
   The top-k calls run all three stages on all k selections; best and best_rank
   are chosen by the final joint key as without the mode, or with
   HC_THREEVIEW_SELECT_BY_TRANSFER by the largest transfer_inliers << 32 | path
   of the three-view reports, among equal keys the larger joint key.
   A NULL scale_reports or reports, a mode bit that is not defined or does not
   apply to the call, iterations3 outside 0..HC_REFINE_MAX_ITERATIONS, a nonzero
   pad, or a transfer_mask where it does not apply returns
   HC_ERROR_INVALID_VALUE before anything is enqueued.  No allocation, copy or
   synchronisation, as in every stream call; the call's own kernels zero what
   its atomics accumulate into, so a recorded graph replays without the caller
   restoring anything. */
typedef struct {
    hcRefineSettings head;          /* offset 0; head.pad[0] == HC_REFINE_THREEVIEW */
    hcScaleReport *scale_reports;   /* device */
    hcThreeViewReport *reports;     /* device */
    uint64_t *transfer_mask;        /* device, or NULL */
    int32_t iterations3;            /* 0: the default, 10 */
    int32_t pad;                    /* 0 */
} hcRefineThreeViewSettings;        /* 48 bytes */

#ifdef __cplusplus
}
#endif
#endif /* HC_POSE_THREEVIEW_H */
