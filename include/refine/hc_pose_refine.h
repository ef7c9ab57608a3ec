/*
 * hc_pose_refine.h -- refinement of a selected trifocal pose on its joint
 * inliers, on the device (not in the reference).
 *
 * hc_trifocal_pose_support_joint ends at the minimal solver's exact solution
 * for three noisy edgels.  The calls below fit that one pose to the edgels it
 * explains: Gauss-Newton on the pixel reprojection residuals of the joint
 * inliers, with the inlier set recomputed at every iterate, and the iterate
 * with the most joint inliers returned.  They take a joint selection and a
 * triplet's edgels, no tracks, so the result of hc_pose_merge_joint can be
 * uploaded and refined.
 *
 * A header of its own, beside hc_pose.h (same conventions: caller-owned device
 * buffers, asynchronous on the caller's stream and current device, no
 * allocation, copy or synchronisation, hcStatus errors): no struct of
 * hc_pose.h or hc_trifocal.h changes for it, and the ABI version stays 2.
 *
 * Method.  Each view (1-2, 1-3) has a state R (3x3) and unit t in double;
 * iterate 0 is the input selection's floats widened.  For k = 0, 1, ...:
 *   1. the state is rounded to float, element by element, and all E edgels
 *      are scored with the 2 px test of the pose-support calls (the same
 *      device function): the joint mask m_k and the counts (joint, 21, 31);
 *   2. the iterate with the largest joint count is remembered, the later one
 *      on a tie; the output pose is exactly the floats that were scored, so
 *      out->inliers is the number of set bits of hc_trifocal_pose_inlier_mask
 *      on out, and when iterate 0 wins the pose is the input's bit for bit;
 *   3. the loop ends after iterate `iterations` was scored, or earlier with
 *      HC_REFINE_TOO_FEW when the joint count is below min_inliers;
 *   4. over the edgels of m_k and per view, in double at the double state: the
 *      2-vector pixel residual r (reprojected minus observed, as the 2 px test
 *      forms it) and its 2x5 Jacobian J in the local parameters
 *        w in R^3:  R <- Exp(w) R
 *        u in R^2:  t <- normalize(t + u0 b1 + u1 b2),  b1 = normalize(t x e_i)
 *                   with i the axis of smallest |t_i| (the lowest on a tie),
 *                   b2 = t x b1
 *      are summed into A = sum J'J, g = sum J'r and the squared error.  The
 *      views share only the mask.  Every thread sums a fixed set of edgels and
 *      the reduction tree is fixed: two calls give the same bits;
 *   5. per view (A + 1e-9 diag(A)) d = -g is solved by Cholesky in double and
 *      d is applied.  A pivot that is not positive or a value that is not
 *      finite, in either view, ends the loop with HC_REFINE_SINGULAR.
 */
#ifndef HC_POSE_REFINE_H
#define HC_POSE_REFINE_H

#include "../hc_pose.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HC_REFINE_MAX_ITERATIONS 32

/* hcRefineReport::status bits */
#define HC_REFINE_NONE     1   /* the input had no path (path < 0): copied to out unchanged    */
#define HC_REFINE_TOO_FEW  2   /* an iterate had fewer than min_inliers joint inliers           */
#define HC_REFINE_SINGULAR 4   /* a pivot was not positive, or a value not finite               */

typedef struct {
    int32_t iterations;    /* Gauss-Newton steps, 1..HC_REFINE_MAX_ITERATIONS; 0: the default, 10 */
    int32_t min_inliers;   /* >= 6; 0: the default, 16                                            */
    int32_t pad[2];
} hcRefineSettings;        /* 16 bytes */

/* What one refinement did (device memory, written by the entry point). */
typedef struct {
    int32_t status;           /* HC_REFINE_* bits, 0: the loop ran to its end                    */
    int32_t iterations_run;   /* steps applied = the index of the last iterate scored            */
    int32_t best_iteration;   /* the iterate returned                                            */
    int32_t joint_history[HC_REFINE_MAX_ITERATIONS + 1];   /* joint count of iterate k, -1 beyond the last scored */
    double rms_px_in[2];      /* RMS residual (px) of view 1-2, 1-3 over iterate 0's own mask    */
    double rms_px_out[2];     /* the same of the best iterate over its own mask (0 without inliers) */
} hcRefineReport;             /* 176 bytes */

/* Refines one joint selection on a triplet's edgels.
 *   in          one hcTrifocalSelection, DEVICE pointer (the output of the joint
 *               calls, or an uploaded hc_pose_merge_joint result)
 *   locations   E x 6 floats, K 9 floats: the scene of the pose-support calls
 *   settings    HOST pointer, read before the call returns; NULL: the defaults
 *   out         one hcTrifocalSelection; out == in is allowed.  The pose is the
 *               best iterate's; inliers, inliers21, inliers31 and key are its
 *               counts on this scene; path, num_candidates, scale31 and the
 *               padding are copied.  out->inliers >= the input pose's count on
 *               this scene.  An input without a path, and one with fewer than
 *               min_inliers joint inliers, is copied unchanged.
 *   report      one hcRefineReport, or NULL
 * A NULL in, locations, K or out, num_edgels <= 0, or a setting out of range
 * returns HC_ERROR_INVALID_VALUE before anything is enqueued. */
hcStatus hc_trifocal_pose_refine(const hcTrifocalSelection *in, int num_edgels, const float *locations,
                                 const float *K, const hcRefineSettings *settings, hcTrifocalSelection *out,
                                 hcRefineReport *report, hcStream stream);

/* The same for the selections of several triplets in one launch: in[t] is
 * refined on groups[t] (a device array of num_groups, as for
 * hc_trifocal_pose_support_joint_grouped) into out[t], reports[t]; each is what
 * the call above gives on that triplet alone, bit for bit.  reports may be
 * NULL.  A NULL groups, in or out, or num_groups <= 0, returns
 * HC_ERROR_INVALID_VALUE. */
hcStatus hc_trifocal_pose_refine_grouped(int num_groups, const hcTripletGroup *groups,
                                         const hcTrifocalSelection *in, const hcRefineSettings *settings,
                                         hcTrifocalSelection *out, hcRefineReport *reports, hcStream stream);

#ifdef __cplusplus
}
#endif
#endif /* HC_POSE_REFINE_H */
