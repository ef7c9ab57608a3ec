/*
 * hc_pose_topk.h -- the k best joint candidates of a tracking launch, their
 * refinement on one scene and the selection among the refined ones, on the
 * device (not in the reference).
 *
 * hc_trifocal_pose_support_joint selects the candidate with the most joint
 * inliers, and hc_trifocal_pose_refine fits that one pose to the edgels it
 * explains.  On noisy edgels the winner by count can sit in a wrong basin, from
 * which no iterate gains an inlier, while a candidate ranked below it refines
 * to several times its count.  The calls below rank the k best candidates from
 * the per-path counts the joint call has written, refine all k in one launch
 * and return the refined selection with the most joint inliers.  Nothing
 * touches the host between the tracking launch and the final pose.
 *
 * A header of its own, beside hc_pose.h and refine/hc_pose_refine.h (same
 * conventions: caller-owned device buffers, asynchronous on the caller's stream
 * and current device, no allocation, copy or synchronisation, hcStatus errors
 * returned before anything is enqueued): no struct of the other headers
 * changes, and the ABI version stays 2.
 */
#ifndef HC_POSE_TOPK_H
#define HC_POSE_TOPK_H

#include "../refine/hc_pose_refine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HC_TOPK_MAX 32

/* The k candidates with the largest key = joint << 32 | b, in descending key order.
 *   tracks      (num_paths) x 31 complex, the tracker's output
 *   inliers     the 3 x num_paths counts written by hc_trifocal_pose_support_joint(_grouped);
 *               a path is a candidate iff inliers[3b] >= 0 (converge is not needed)
 *   candidates  k hcTrifocalSelection out.  candidates[r] is exactly what the joint call would
 *               have selected had the r better candidates not existed: path, the three counts,
 *               key, pose bits and scale31 as the joint call gives them, num_candidates = the number
 *               of candidates of the call, padding 0.  So candidates[0] equals the joint call's
 *               selection byte for byte (136 bytes).  Ranks at or beyond the number of candidates
 *               hold the "none" selection (path -1, counts -1, zero pose, scale31 0, key 0),
 *               with num_candidates still the call's.
 * k outside 1..HC_TOPK_MAX, num_paths < 0, a NULL candidates, or with num_paths > 0 a NULL tracks
 * or inliers, returns HC_ERROR_INVALID_VALUE.  num_paths == 0 writes k "none" selections with
 * num_candidates 0.  Two calls on the same input write the same bytes. */
hcStatus hc_trifocal_pose_topk_joint(int num_paths, const hcComplex *tracks, const int32_t *inliers,
                                     int k, hcTrifocalSelection *candidates, hcStream stream);

/* Per triplet: candidates[t * k + r] over the samples s with sample_group[s] == t (batch ids of
 * the call; the layout of hc_trifocal_pose_support_joint_grouped).  num_paths must be a multiple
 * of 312 and num_groups >= 1; group ids outside [0, num_groups) are a contract violation. */
hcStatus hc_trifocal_pose_topk_joint_grouped(int num_paths, const hcComplex *tracks, const int32_t *inliers,
                                             int num_groups, const int32_t *sample_group, int k,
                                             hcTrifocalSelection *candidates, hcStream stream);

/* Refines the k candidates on one scene, then selects.
 *   candidates  k hcTrifocalSelection, DEVICE pointer (the output of the calls above, or an
 *               uploaded hc_pose_merge_topk result)
 *   settings    HOST pointer as for hc_trifocal_pose_refine; NULL: the defaults
 *   refined[r], reports[r]   what hc_trifocal_pose_refine gives on candidates[r], bit for bit
 *                            (reports may be NULL; refined may alias candidates)
 *   best        the refined selection with the largest key (inliers << 32 | path: most joint
 *               inliers, ties -> the larger batch id); "none" candidates never win; all none -> none
 *               (with refined[0]'s num_candidates).  best may not overlap refined.
 *   best_rank   one int32: the rank r that won, -1 for none
 * A NULL candidates, locations, K, refined, best or best_rank, num_edgels <= 0, k outside
 * 1..HC_TOPK_MAX, or a setting out of range returns HC_ERROR_INVALID_VALUE. */
hcStatus hc_trifocal_pose_refine_topk(int k, const hcTrifocalSelection *candidates, int num_edgels,
                                      const float *locations, const float *K, const hcRefineSettings *settings,
                                      hcTrifocalSelection *refined, hcRefineReport *reports,
                                      hcTrifocalSelection *best, int32_t *best_rank, hcStream stream);

/* The same for num_groups triplets: candidates / refined / reports are [t * k + r] on groups[t];
 * best and best_rank have num_groups entries.  Each group's result is the call above on that
 * triplet alone, bit for bit. */
hcStatus hc_trifocal_pose_refine_topk_grouped(int num_groups, const hcTripletGroup *groups, int k,
                                              const hcTrifocalSelection *candidates,
                                              const hcRefineSettings *settings, hcTrifocalSelection *refined,
                                              hcRefineReport *reports, hcTrifocalSelection *best,
                                              int32_t *best_rank, hcStream stream);

/* Host: the top-k lists of n launches / GPUs (parts[i * k + r], batch ids starting at path_offsets[i])
 * -> the k largest re-based keys, descending, as if one launch had covered all paths;
 * num_candidates is the sum of the parts'.  n = 0 -> k none selections.  parts are host copies;
 * a k outside 1..HC_TOPK_MAX writes nothing. */
void hc_pose_merge_topk(int n, int k, const hcTrifocalSelection *parts, const int32_t *path_offsets,
                        hcTrifocalSelection *out);

#ifdef __cplusplus
}
#endif
#endif /* HC_POSE_TOPK_H */
