// What the abort-mode tracker kernels score a converged path with (PH_FINISH,
// hc_track_body.inc).
#pragma once

#include "hc_pose_device.hpp"

namespace hc {

// Abort-mode scoring of one half's converged path (dev-trifocal_2op1p-eval.cuh:
// 28-250, 32 lanes per path): inlier counts of views 2 and 3 over all triplet
// edgels.
template <int VIEW>   // 0: view 2 (edgel columns 2, 3), 1: view 3 (columns 4, 5)
__device__ __forceinline__ int score_view(const float *R, float da, float db, float dc, const float *edgels,
                                          int num_edgels, float fx, float fy, float cx, float cy, int r) {
    int c = 0;
    for (int e = r; e < num_edgels; e += 32) {
        const float *g = edgels + (size_t)e * 6;
        const float g0 = g[0], g1 = g[1], gu = g[2 + 2 * VIEW], gv = g[3 + 2 * VIEW];
        const float num = dc * (R[2] * gu + R[5] * gv + R[8]) - (R[2] * da + R[5] * db + R[8] * dc);
        const float den = 1.0f - (R[6] * g0 + R[7] * g1 + R[8]) * (R[2] * gu + R[5] * gv + R[8]);
        const float v2 = num * (R[6] * g0 + R[7] * g1 + R[8]) + den * dc;
        const float v0 = (num * (R[0] * g0 + R[1] * g1 + R[2]) + den * da) / v2;
        const float v1 = (num * (R[3] * g0 + R[4] * g1 + R[5]) + den * db) / v2;
        const float ex = (v0 * fx + cx) - (gu * fx + cx);
        const float ey = (v1 * fy + cy) - (gv * fy + cy);
        c += (__builtin_sqrtf(ex * ex + ey * ey) < 2.0f) ? 1 : 0;
    }
    return c;
}
// The two views are scored in separate passes, each from its own evaluation
// of the hypothesis (12 live values instead of 24): the abort kernel's register
// allocation is otherwise set by this cold path.
__device__ __forceinline__ int2 score_half(const cf *sx, const float *edgels, int num_edgels,
                                           const float *K, int r) {
    const float fx = K[0], fy = K[4], cx = K[3] /* eval quirk, SURVEY Appendix C.4 */, cy = K[5];
    int c21, c31;
    {
        Hyp hy;
        make_hypothesis(sx, hy);
        c21 = score_view<0>(hy.R, hy.T[0], hy.T[1], hy.T[2], edgels, num_edgels, fx, fy, cx, cy, r);
    }
    {
        const cf *sx2 = sx;
        asm volatile("" : "+v"(sx2));   // a second evaluation, not the first one kept live
        Hyp hy;
        make_hypothesis(sx2, hy);
        c31 = score_view<1>(hy.R + 9, hy.T[3], hy.T[4], hy.T[5], edgels, num_edgels, fx, fy, cx, cy, r);
    }
    return make_int2(half_sum_i(c21), half_sum_i(c31));
}

// Gated abort launches (k_track_gated): the pose-support counts of one half's
// converged candidate -- make_pose and the per-edgel test of hc_pose_device.hpp,
// so the three counts are those of k_pose_support<true, *> for the same track
// and scene (integer sums: the order of summation is free).  32 lanes over the
// triplet's edgels.  Both views of an edgel need 24 pose values; held live they
// would set the kernel's register allocation (as score_half's note says), so
// the edgels go in chunks of 2048, 64 per lane: a first pass keeps the lane's
// view-1-2 verdicts as bits, a second one the view-1-3 verdicts, each from its
// own evaluation of the pose (12 live values); the joint verdicts are the AND.
struct JointCounts { int cJ, c21, c31; };
__device__ __forceinline__ JointCounts score_joint_half(const cf *sx, const Scene sc, int r) {
    constexpr unsigned CHUNK = 64u * 32u;
    const unsigned E = sc.E > 0 ? (unsigned)sc.E : 0u;
    int cJ = 0, c21 = 0, c31 = 0;
    for (unsigned base = 0u; base < E; base += CHUNK) {
        unsigned long long m21 = 0ull, m31 = 0ull;
        {
            const cf *s1 = sx;
            asm volatile("" : "+v"(s1));   // evaluated here, per chunk and pass: not kept live
            Pose P;
            make_pose(s1, P);
            unsigned e = base + (unsigned)r;
            for (int j = 0; j < 64 && e < E; j++, e += 32u)
                m21 |= (unsigned long long)(edgel_view<0>(sc, (int)e, P.R, P.t) ? 1u : 0u) << j;
        }
        {
            const cf *s2 = sx;
            asm volatile("" : "+v"(s2));
            Pose P;
            make_pose(s2, P);
            unsigned e = base + (unsigned)r;
            for (int j = 0; j < 64 && e < E; j++, e += 32u)
                m31 |= (unsigned long long)(edgel_view<1>(sc, (int)e, P.R + 9, P.t + 3) ? 1u : 0u) << j;
        }
        c21 += __builtin_popcountll(m21);
        c31 += __builtin_popcountll(m31);
        cJ += __builtin_popcountll(m21 & m31);
    }
    return JointCounts{half_sum_i(cJ), half_sum_i(c21), half_sum_i(c31)};
}

}  // namespace hc
