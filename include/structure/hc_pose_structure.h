/*
 * hc_pose_structure.h -- the 3D edgels a trifocal pose explains, reconstructed
 * on the device (not in the reference).
 *
 * The refinement, the scale vote and the three-view stage triangulate every
 * joint inlier from views 1-2 and keep only counts and masks.  The mode below
 * keeps the structure: for the pose that goes out, one record per three-view
 * (transfer) inlier, in edgel order -- the triangulated point, the 3D tangent in
 * which the tangent planes of views 1 and 2 meet, and how well that tangent,
 * reprojected, lines up with the tangent observed in view 3.  No stage fits to
 * the tangents, so the last figure checks the pose on data it has not seen.
 *
 * A header of its own, beside threeview/hc_pose_threeview.h (same rules of the
 * boundary).  It declares no function: the stage is a mode of the four refine
 * calls (hc_trifocal_pose_refine, _grouped, hc_trifocal_pose_refine_topk,
 * _topk_grouped), selected by hcRefineSettings::pad, and no struct of the other
 * headers changes for it (the ABI version stays 2).
 *
 * The rule.  All arithmetic is float32, no contraction, IEEE division and
 * square root; a matrix-vector product accumulates its row from 0.0f, as
 * ((0.0f + r0 x0) + r1 x1) + r2 x2.  Tangents are metric image vectors like the
 * locations (x2 = R21 x1 + t21); the sign of a tangent is not consistent
 * between the views, so the residual of step 5 is unsigned.  Given the
 * selection's floats (R21, t21, R31, t31, s = scale31), the scene (E edgels
 * g = (g0 g1), h = (h0 h1), q = (q0 q1), and K) and the tangents (E rows
 * a = (a0 a1), b = (b0 b1), c = (c0 c1) of views 1, 2, 3):
 *   1. The set.  W: the edgels e of the tested set of scale/hc_pose_scale.h
 *      (step 2: joint inlier and rho > 0) for which its T(e, s) holds (step 3).
 *      After the three-view stage this is the transfer mask of the pose that
 *      went out.  Entry j of the output is the j-th edgel of W in increasing e.
 *   2. The point.  X = (rho g0, rho g1, rho) with rho of that header's step 2,
 *      and err3_px = sqrt((d0 d0 + d1 d1) + 0.0f 0.0f) of its step 3, the value
 *      that is compared with 2.0f.
 *   3. The tangent planes.
 *        n1   = (-a1, a0, g0 a1 - g1 a0)                          gamma1 x (a, 0)
 *        m    = (-b1, b0, h0 b1 - h1 b0)                          gamma2 x (b, 0)
 *        n2_i = ((0.0f + R21[i] m0) + R21[3+i] m1) + R21[6+i] m2,  i = 0, 1, 2   (R21' m)
 *        n1 and n2 are each divided, component by component, by their length
 *        sqrt((x x + y y) + z z)
 *        D    = (n1_1 n2_2 - n1_2 n2_1,  n1_2 n2_0 - n1_0 n2_2,  n1_0 n2_1 - n1_1 n2_0)
 *        sin_plane = sqrt((D0 D0 + D1 D1) + D2 D2)
 *   4. Validity.  The tangent is defined iff sin_plane is finite and
 *      >= min_sin_plane.  Then T = D / sin_plane (component by component),
 *      negated when (T0 - T2 g0) a0 + (T1 - T2 g1) a1 < 0.0f, so that its image
 *      in view 1 points as a does.  Otherwise T = 0, sin3 = 1.0f and
 *      HC_EDGEL3D_TANGENT is clear.
 *   5. The view-3 residual, for a defined tangent.
 *        V_i  = ((0.0f + R31[3i] T0) + R31[3i+1] T1) + R31[3i+2] T2
 *        Z    = step 3's of scale/hc_pose_scale.h, Z_i = Y_i + s t31[i]
 *        p    = ((V0 Z2 - Z0 V2) K0,  (V1 Z2 - Z1 V2) K4)
 *        o    = (c0 K0, c1 K4)
 *        sin3 = |p0 o1 - p1 o0| / (sqrt(p0 p0 + p1 p1) * sqrt(o0 o0 + o1 o1))
 *      HC_EDGEL3D_ORIENTED iff the tangent is defined and sin3 < max_sin3 (a
 *      NaN compares false).
 *   6. The report.  count = |W|, tangents and oriented the numbers of entries
 *      with each bit, scale31 the scale used.  For a selection without a path,
 *      or one for which stage 2 reported HC_SCALE_NONE or HC_SCALE_NO_VOTER:
 *      status HC_STRUCTURE_NONE and all counts 0.  Entries at and beyond count
 *      are not written: the caller's bytes stay.
 * Every integer is a function of the inputs and every float is defined to the
 * bit; there is no sum over a set and no atomic.
 */
#ifndef HC_POSE_STRUCTURE_H
#define HC_POSE_STRUCTURE_H

#include "../threeview/hc_pose_threeview.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hcRefineSettings::pad[0] of settings that are the head of an
   hcRefineStructureSettings ("ST3D"). */
#define HC_REFINE_STRUCTURE 0x53543344

/* hcRefineSettings::pad[1] in that mode: mode bits (any other bit is refused).
   Bit 2 stays HC_THREEVIEW_SELECT_BY_TRANSFER (the top-k calls only). */
#define HC_STRUCTURE_ONLY   1   /* no refinement, no vote, no three-view stage: the input's own pose and scale31 */

/* hcEdgel3D::flags */
#define HC_EDGEL3D_TANGENT  1   /* T is defined                        */
#define HC_EDGEL3D_ORIENTED 2   /* ... and sin3 < max_sin3             */

/* hcStructureReport::status */
#define HC_STRUCTURE_NONE   1   /* no path, or stage 2 fitted no scale: nothing was reconstructed */

/* One reconstructed edgel (device memory, written by the entry point). */
typedef struct {
    float X[3];          /* the point, in view 1's frame, in units of |t21|          */
    float T[3];          /* the unit tangent there, or 0                             */
    float err3_px;       /* the transfer error in view 3 (px), < 2                   */
    float sin_plane;     /* the sine of the angle between the two tangent planes     */
    float sin3;          /* the sine between reprojected and observed view-3 tangent */
    int32_t edgel;       /* e                                                        */
    int32_t flags;       /* HC_EDGEL3D_* bits                                        */
    int32_t pad;         /* 0                                                        */
} hcEdgel3D;             /* 48 bytes */

/* What one reconstruction did (device memory, written by the entry point). */
typedef struct {
    int32_t status;      /* 0, or HC_STRUCTURE_NONE        */
    int32_t count;       /* |W|: the entries written       */
    int32_t tangents;    /* entries with HC_EDGEL3D_TANGENT  */
    int32_t oriented;    /* entries with HC_EDGEL3D_ORIENTED */
    float scale31;       /* the scale used                 */
    int32_t pad[3];      /* 0                              */
} hcStructureReport;     /* 32 bytes */

/* The settings of the mode.  The caller sets tv.head.pad[0] =
   HC_REFINE_STRUCTURE, tv.head.pad[1] to the mode bits, and passes
   (const hcRefineSettings *)&settings (a HOST pointer, read before the call
   returns) to a refine call.
   Without HC_STRUCTURE_ONLY the call runs the three stages exactly as
   threeview/hc_pose_threeview.h says, with the embedded tv (the same checks,
   the same outputs: a call with HC_REFINE_THREEVIEW and the same inputs writes
   the same bytes), and then, on the same stream, the rule above on the
   selection that went out: out[t] of the two refine calls, best[t] of the two
   top-k calls (after the selection among the k; its stage-2 report is that of
   rank best_rank[t]).
   With HC_STRUCTURE_ONLY (hc_trifocal_pose_refine and _grouped only;
   head.iterations == 0, tv.scale_reports, tv.reports and tv.transfer_mask NULL,
   tv.iterations3 == 0) nothing is refined or voted: out is in bit for bit, no
   other report is written, and the rule runs on in's own pose floats and
   scale31 (HC_STRUCTURE_NONE only without a path).
   tangents: E x 6 floats (tx1 ty1 tx2 ty2 tx3 ty3) beside locations; in a
   grouped call the groups' rows concatenated, group t's E_t rows from row
   edgel_offsets[t].  edgels3d: E entries; grouped: group t's from entry
   edgel_offsets[t], so sum E entries when the offsets are the running sums.
   edgel_offsets: num_groups int32 on the device, required in the grouped calls
   and NULL in the two others.  reports: one per group (1 or num_groups).
   min_sin_plane, max_sin3: 0 selects the default, 0.05 for both.
   A NULL tangents, edgels3d or reports, edgel_offsets given to a single call
   or missing in a grouped one, a threshold that is not finite or outside
   [0, 1], a mode bit that is not defined or does not apply to the call, or
   anything the three-view header refuses returns HC_ERROR_INVALID_VALUE before
   anything is enqueued.  No allocation, copy or synchronisation, as in every
   stream call; the stage accumulates nothing across launches, so a recorded
   graph replays as it is. */
typedef struct {
    hcRefineThreeViewSettings tv;   /* offset 0; tv.head.pad[0] == HC_REFINE_STRUCTURE */
    const float *tangents;          /* device */
    const int32_t *edgel_offsets;   /* device, or NULL */
    hcEdgel3D *edgels3d;            /* device */
    hcStructureReport *reports;     /* device */
    float min_sin_plane, max_sin3;  /* 0: the defaults, 0.05 and 0.05 */
} hcRefineStructureSettings;        /* 88 bytes */

#ifdef __cplusplus
}
#endif
#endif /* HC_POSE_STRUCTURE_H */
