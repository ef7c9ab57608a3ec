/*
 * hc_trifocal_adaptive.h -- the adaptive sample limit of the gated abort launch:
 * a triplet's RANSAC stops on the device at the standard rule's sample count.
 *
 * After a hypothesis with inlier share w = cJ / E, at most
 *     n(w) = ceil(log(1 - p) / log(1 - w^3))
 * samples (three edgels each) are needed for confidence p.  The best hypothesis
 * scored so far sets a triplet's limit; a sample whose index among its triplet's
 * samples has reached the limit is not tracked.  A weak hypothesis only trims the
 * budget, a strong one ends the run, and one wrong hypothesis no longer decides
 * a trial as it does with a hand-tuned hcJointGate::min_joint_ratio alone.
 *
 * A header of its own, beside hc_trifocal.h (same rules of the boundary).  It
 * declares no launch: the adaptive limit is a mode of
 * hc_trifocal_2op1p_30x30_track_abort_gated, selected by hcJointGate::pad, and no
 * struct of hc_trifocal.h changes for it (the ABI version stays 2).
 */
#ifndef HC_TRIFOCAL_ADAPTIVE_H
#define HC_TRIFOCAL_ADAPTIVE_H

#include "../hc_trifocal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hcJointGate::pad of a gate that is the head of an hcAdaptiveGate ("ADP1").
   Any other value of pad -- 0, or whatever a caller left there -- is the gated
   launch as hc_trifocal.h describes it. */
#define HC_GATE_ADAPTIVE 0x41445031

/* The gate of the adaptive mode.  The caller sets head.pad = HC_GATE_ADAPTIVE
   and passes (const hcJointGate *)&gate to
   hc_trifocal_2op1p_30x30_track_abort_gated:

       hcAdaptiveGate ag = {{2.0f, HC_GATE_ADAPTIVE, joint_inliers},
                            need, need_offset, sample_ordinal, group_limit};
       hc_trifocal_2op1p_30x30_track_abort_gated(&args, &grouped, (const hcJointGate *)&ag,
                                                 workspace, workspace_bytes, stream);

   Semantics, for a path of sample s of group t = sample_group[s]:
     - it is skipped at dequeue iff group_found[t] is set or
       sample_ordinal[s] >= group_limit[t]; with inflight_stop it also stops at
       its next step boundary under the same condition; a skipped or stopped
       path reports as in the gated launch (track untouched, converge = 0,
       infinity = 0, zero stats, joint_inliers not written);
     - a scored path reports as in the gated launch (joint_inliers, the two
       counts in stats) and, in addition, lowers its triplet's limit:
           atomicMin(&group_limit[t], need[need_offset[t] + cJ]);
     - head.min_joint_ratio keeps its role: a count of at least ratio * E still
       raises group_found[t]; a ratio > 1 never fires ("limit only");
     - group_limit is in/out, the carry-over between chunked launches as
       group_found is: the caller sets it to the triplet's budget for a fresh
       run, and sample_ordinal counts over the whole run, chunks included;
     - the dequeue order, the ticks and batch_index are unchanged.
   With pad == HC_GATE_ADAPTIVE a NULL need, need_offset, sample_ordinal or
   group_limit returns HC_ERROR_INVALID_VALUE before anything is enqueued.  The
   tables' contents are a contract like group ids (not validated on the device):
   need_offset[t] + E_t is the last entry read of group t, ordinals are >= 0.
   Several GPUs: each rank's group_limit is its own; a min-reduce of the words
   between chunks shares a limit across ranks. */
typedef struct {
    hcJointGate head;              /* offset 0; head.pad == HC_GATE_ADAPTIVE */
    const int32_t *need;           /* device: the groups' tables, concatenated */
    const int64_t *need_offset;    /* device, T: where group t's E_t + 1 entries start */
    const int32_t *sample_ordinal; /* device, one per sample of the launch: its index among
                                      its own triplet's samples, counted over the whole run
                                      (chunks included) */
    uint32_t      *group_limit;    /* device, T words, in/out */
} hcAdaptiveGate;                  /* 48 bytes */

/* Host: the table of the rule for a triplet of num_edgels = E edgels,
   need[c] for c = 0..E joint inliers, everything in double:
       w = c / E,  q = 1 - w w w,
       n = 0 if q <= 0; max_samples if q >= 1 or log(1 - p) / log(q) is not finite;
           otherwise ceil(log(1 - p) / log(q)),
       need[c] = clamp(n, min_samples, max_samples).
   Built on the host and read on the device on purpose: a device log would not
   be reproducible against the host's, and one int load costs nothing beside a
   path.  HC_ERROR_INVALID_VALUE for E <= 0, a confidence outside (0, 1),
   min_samples < 1, max_samples < min_samples or a NULL need. */
hcStatus hc_ransac_need_table(int num_edgels, double confidence, int min_samples, int max_samples,
                              int32_t *need /* E + 1 */);

#ifdef __cplusplus
}
#endif
#endif /* HC_TRIFOCAL_ADAPTIVE_H */
