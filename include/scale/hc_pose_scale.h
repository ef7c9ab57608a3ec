/*
 * hc_pose_scale.h -- the relative scale of a trifocal pose, fitted by
 * three-view transfer support on the device (not in the reference).
 *
 * The joint calls and the refinement return two two-view poses, R21 | t21 and
 * R31 | t31, both translations of unit length.  What makes them one trifocal
 * pose is the length of t31 in units of t21, hcTrifocalSelection::scale31,
 * which the joint calls take from the minimal solver's three noisy edgels and
 * the refinement copies.  The mode below fits it: every joint inlier is
 * triangulated from views 1-2, proposes the scale that puts it closest to its
 * observation in view 3, and the proposal under which the most triangulated
 * edgels land within 2 px of their view-3 observation wins.  That count,
 * transfer_inliers, is the pose's support in all three views at once.
 *
 * A header of its own, beside refine/hc_pose_refine.h (same rules of the
 * boundary).  It declares no function: the fit is a mode of the four refine
 * calls (hc_trifocal_pose_refine, _grouped, hc_trifocal_pose_refine_topk,
 * _topk_grouped), selected by hcRefineSettings::pad, and no struct of the
 * other headers changes for it (the ABI version stays 2).
 *
 * The rule.  All arithmetic is float32, no contraction, IEEE division and
 * square root; a matrix-vector product accumulates its row from 0.0f, as
 * ((0.0f + r0 x0) + r1 x1) + r2 x2.  Given the pose (R21, t21, R31, t31 as the
 * selection's floats) and the scene (E edgels (g0 g1 h0 h1 q0 q1), K):
 *   1. m: the joint inlier mask of the pose, the 2 px test of
 *      hc_trifocal_pose_inlier_mask in both views.
 *   2. For e in m:
 *        a    = ((0.0f + R21[2] h0) + R21[5] h1) + R21[8] 1.0f
 *        rho  = t21[2] a
 *        rho  = rho - (((0.0f + R21[2] t21[0]) + R21[5] t21[1]) + R21[8] t21[2])
 *        m2   = ((0.0f + R21[6] g0) + R21[7] g1) + R21[8] 1.0f
 *        rho  = rho / (1.0f - m2 a)             (the depth the 2 px test forms)
 *        X    = (rho g0, rho g1, rho)
 *        Y_i  = ((0.0f + R31[3i] X0) + R31[3i+1] X1) + R31[3i+2] X2,  i = 0, 1, 2
 *        a    = (q1 Y2 - 1.0f Y1,  1.0f Y0 - q0 Y2,  q0 Y1 - q1 Y0)              gamma3 x Y
 *        b    = (q1 t31[2] - 1.0f t31[1],  1.0f t31[0] - q0 t31[2],  q0 t31[1] - q1 t31[0])
 *        s_e  = -(((a0 b0 + a1 b1) + a2 b2) / ((b0 b0 + b1 b1) + b2 b2))
 *      e is in the tested set iff rho > 0; it is a voter iff, in addition,
 *      s_e is finite and > 0.
 *   3. The transfer test T(e, s), for e in the tested set:
 *        Z_i  = Y_i + s t31[i]                  (the product, then the sum)
 *        Z2 > 0 is required
 *        d0   = ((Z0 / Z2) K0 + K2) - (q0 K0 + K2)
 *        d1   = ((Z1 / Z2) K4 + K5) - (q1 K4 + K5)
 *        T    = sqrt((d0 d0 + d1 d1) + 0.0f 0.0f) < 2.0f
 *   4. For every voter v, c_v = the number of e in the tested set with
 *      T(e, s_v).  The winner has the largest key c_v << 32 | v (ties go to the
 *      later edgel).  scale31 = s_v, transfer_inliers = c_v.
 * There is no polish over the winner's set and no double arithmetic: every
 * count is an integer function of the inputs and does not depend on the launch.
 */
#ifndef HC_POSE_SCALE_H
#define HC_POSE_SCALE_H

#include "../refine/hc_pose_refine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hcRefineSettings::pad[0] of settings that are the head of an
   hcRefineScaleSettings ("SC31").  Any other value of pad -- 0, or whatever a
   caller left there -- is the refine call as its own header describes it. */
#define HC_REFINE_SCALE31 0x53433331

/* hcRefineSettings::pad[1] in that mode: mode bits (any other bit is refused) */
#define HC_SCALE_ONLY               1   /* skip the Gauss-Newton loop: the pose comes back bit for bit;
                                           head.iterations must be 0 and no hcRefineReport is written */
#define HC_SCALE_SELECT_BY_TRANSFER 2   /* the top-k calls only: best = the largest transfer key */

/* hcScaleReport::status bits: nothing was fitted, scale31 is the input's */
#define HC_SCALE_NONE     1   /* the selection has no path (path < 0)                      */
#define HC_SCALE_NO_VOTER 2   /* no joint inlier with positive depth and a positive scale  */

/* What one fit did (device memory, written by the entry point). */
typedef struct {
    int32_t status;             /* HC_SCALE_* bits, 0: fitted                                       */
    int32_t num_voters;
    int32_t voter;              /* the winning edgel, -1 without a fit                               */
    int32_t transfer_inliers;   /* c_v of the winner: tested edgels within 2 px in view 3; 0 without a fit */
    int32_t tested;             /* the size of the tested set (0 without a path)                     */
    int32_t joint;              /* the size of m (0 without a path)                                  */
    float scale_in;             /* scale31 as it came in                                             */
    float scale31;              /* as it went out                                                    */
    uint64_t key;               /* transfer_inliers << 32 | voter; the vote's atomicMax word         */
} hcScaleReport;                /* 40 bytes */

/* The settings of the mode.  The caller sets head.pad[0] = HC_REFINE_SCALE31,
   head.pad[1] to the mode bits, and passes (const hcRefineSettings *)&settings
   (a HOST pointer, read before the call returns) to a refine call:

       hcRefineScaleSettings ss = {{10, 16, {HC_REFINE_SCALE31, 0}}, reports, mask};
       hc_trifocal_pose_refine(in, E, locations, K, (const hcRefineSettings *)&ss, out, report, stream);

   The call then refines as its header says and, on the same stream, fits the
   scale of every selection it has written:
     - out is the selection the refinement writes, with only scale31 replaced
       (with HC_SCALE_ONLY: the input selection, with only scale31 replaced;
       out == in is allowed as before);
     - reports[i] (a DEVICE pointer, one hcScaleReport per selection: 1,
       num_groups, k or num_groups * k, in the order of out / refined) is
       written in full.  Its key is the vote's own word: the call's kernels
       zero it, so a recorded graph replays without the caller restoring anything;
     - a selection without a path (HC_SCALE_NONE) or without a voter
       (HC_SCALE_NO_VOTER) keeps scale31 as copied;
     - transfer_mask (a DEVICE pointer or NULL; hc_trifocal_pose_refine only,
       NULL in the three other calls): (num_edgels + 63) / 64 words, bit e % 64
       of word e / 64 set iff e is in the tested set and T(e, out->scale31)
       holds; the number of set bits is transfer_inliers, and the mask is a
       subset of hc_trifocal_pose_inlier_mask on out.  All words are 0
       without a fit;
     - the top-k calls fit all k refined selections; best and best_rank are
       chosen as without the mode (best then carries its fitted scale31),
       unless HC_SCALE_SELECT_BY_TRANSFER is set: then the selection with a
       path and the largest key transfer_inliers << 32 | path wins, and among
       equal keys the larger joint key.
   A NULL reports, a mode bit that is not defined or does not apply to the call,
   HC_SCALE_ONLY with head.iterations != 0, or a transfer_mask where it does not
   apply returns HC_ERROR_INVALID_VALUE before anything is enqueued.  No
   allocation, copy or synchronisation, as in every stream call. */
typedef struct {
    hcRefineSettings head;      /* offset 0; head.pad[0] == HC_REFINE_SCALE31 */
    hcScaleReport *reports;     /* device */
    uint64_t *transfer_mask;    /* device, or NULL */
} hcRefineScaleSettings;        /* 32 bytes */

#ifdef __cplusplus
}
#endif
#endif /* HC_POSE_SCALE_H */
