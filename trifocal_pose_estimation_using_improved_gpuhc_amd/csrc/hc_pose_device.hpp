// hc_pose_device.hpp -- the pose-support test on the device: candidate filter,
// pose recovery and the 2 px reprojection test of one edgel.
//
// Shared by the pose-support kernels (hc_pose.hip) and the gated abort kernel
// (hc_kernels.hip k_track_gated), so that a path scored by either gets the same
// counts bit for bit.  The multiview helpers of magmaHC/util.hpp restated op
// for op (FP32, no contraction: -ffp-contract=off; IEEE division and sqrt).
#pragma once

#include "hc_device.hpp"

namespace hc {

struct Pose {
    float R[18];   // R21 row-major, R31 row-major
    float t[6];    // unit t21, unit t31
};

// util.hpp:31-66: Cayley_To_Rotation_Matrix + Normalize_Rotation_Matrix
// (all three column norms first, then the divisions)
__device__ __forceinline__ void cayley_unit(float a, float b, float c, float *R) {
    R[0] = (1.0f + a * a) - (b * b + c * c);
    R[1] = 2.0f * (a * b - c);
    R[2] = 2.0f * (a * c + b);
    R[3] = 2.0f * (a * b + c);
    R[4] = (1.0f + b * b) - (a * a + c * c);
    R[5] = 2.0f * (b * c - a);
    R[6] = 2.0f * (a * c - b);
    R[7] = 2.0f * (b * c + a);
    R[8] = (1.0f + c * c) - (a * a + b * b);
    const float n0 = __builtin_sqrtf((R[0] * R[0] + R[3] * R[3]) + R[6] * R[6]);
    const float n1 = __builtin_sqrtf((R[1] * R[1] + R[4] * R[4]) + R[7] * R[7]);
    const float n2 = __builtin_sqrtf((R[2] * R[2] + R[5] * R[5]) + R[8] * R[8]);
    R[0] /= n0; R[3] /= n0; R[6] /= n0;
    R[1] /= n1; R[4] /= n1; R[7] /= n1;
    R[2] /= n2; R[5] /= n2; R[8] /= n2;
}

// util.hpp:69-78: Normalize_Translation_Vector
__device__ __forceinline__ void unit3(float *t) {
    const float n = __builtin_sqrtf((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    t[0] /= n; t[1] /= n; t[2] /= n;
}

// Evaluations.cpp:235-265 (Convert_Trifocal_Translation / _Rotation) from x = 31 complex
__device__ __forceinline__ void make_pose(const cf *__restrict__ x, Pose &P) {
#pragma unroll
    for (int i = 0; i < 6; i++) P.t[i] = x[18 + i].x;
    unit3(P.t);
    unit3(P.t + 3);
    cayley_unit(x[24].x, x[25].x, x[26].x, P.R);
    cayley_unit(x[27].x, x[28].x, x[29].x, P.R + 9);
}

// util.hpp:169-209 for one view pair: depth rho of gamma1 (get_depth_rho), then
// the pixel reprojection error of gamma2 (get_Reprojection_Pixels_Error).
// gamma = (g.x, g.y, 1); matrix-vector products accumulate from 0.0f as the
// reference's get_Matrix_Vector_Product does.
__device__ __forceinline__ bool reproj_inlier(float g0, float g1, float h0, float h1, const float *R, const float *T,
                                              float K0, float K2, float K4, float K5) {
    const float Rg2_2 = ((0.0f + R[2] * h0) + R[5] * h1) + R[8] * 1.0f;   // (R' gamma2)_2
    float rho = T[2] * Rg2_2;
    const float RtT_2 = ((0.0f + R[2] * T[0]) + R[5] * T[1]) + R[8] * T[2];   // (R' T)_2
    rho -= RtT_2;
    float m0 = ((0.0f + R[0] * g0) + R[1] * g1) + R[2] * 1.0f;            // R gamma1
    float m1 = ((0.0f + R[3] * g0) + R[4] * g1) + R[5] * 1.0f;
    float m2 = ((0.0f + R[6] * g0) + R[7] * g1) + R[8] * 1.0f;
    rho /= (1.0f - m2 * Rg2_2);
    m0 *= rho; m0 += T[0];
    m1 *= rho; m1 += T[1];
    m2 *= rho; m2 += T[2];
    m0 /= m2;
    m1 /= m2;
    m0 = m0 * K0 + K2;
    m1 = m1 * K4 + K5;
    const float p0 = h0 * K0 + K2, p1 = h1 * K4 + K5;
    m0 -= p0;
    m1 -= p1;
    const float err = __builtin_sqrtf((m0 * m0 + m1 * m1) + 0.0f * 0.0f);
    return err < 2.0f;   // REPROJ_ERROR_INLIER_THRESH (definitions.hpp:17)
}

// One triplet's scoring set: E edgels of 6 floats and the four intrinsics used.
struct Scene {
    int E;
    const float *loc;
    float K0, K2, K4, K5;
};

__device__ __forceinline__ Scene load_scene(int E, const float *__restrict__ loc, const float *__restrict__ K) {
    return Scene{E, loc, K[0], K[2], K[4], K[5]};
}

// Edgel e of a scene under one pose: inlier in view 1-2, inlier in view 1-3.
__device__ __forceinline__ void edgel_views(const Scene &sc, int e, const float *R21, const float *t21,
                                            const float *R31, const float *t31, bool &in21, bool &in31) {
    const float2 g01 = *reinterpret_cast<const float2 *>(sc.loc + (size_t)e * 6);
    const float2 g23 = *reinterpret_cast<const float2 *>(sc.loc + (size_t)e * 6 + 2);
    const float2 g45 = *reinterpret_cast<const float2 *>(sc.loc + (size_t)e * 6 + 4);
    in21 = reproj_inlier(g01.x, g01.y, g23.x, g23.y, R21, t21, sc.K0, sc.K2, sc.K4, sc.K5);
    in31 = reproj_inlier(g01.x, g01.y, g45.x, g45.y, R31, t31, sc.K0, sc.K2, sc.K4, sc.K5);
}

// One view of edgel_views (VIEW 0: view 1-2 with R21 | t21, 1: view 1-3 with
// R31 | t31): the same loads and the same reproj_inlier call.
template <int VIEW>
__device__ __forceinline__ bool edgel_view(const Scene &sc, int e, const float *R, const float *t) {
    const float2 g01 = *reinterpret_cast<const float2 *>(sc.loc + (size_t)e * 6);
    const float2 h = *reinterpret_cast<const float2 *>(sc.loc + (size_t)e * 6 + 2 + 2 * VIEW);
    return reproj_inlier(g01.x, g01.y, h.x, h.y, R, t, sc.K0, sc.K2, sc.K4, sc.K5);
}

// ---- three-view transfer (include/scale/hc_pose_scale.h: the operation order
// is the header's, steps 2 and 3) -----------------------------------------------

// The depth of gamma1 from views 1-2, the value reproj_inlier forms before it
// reprojects (the same operations on the same floats).
__device__ __forceinline__ float depth_rho(float g0, float g1, float h0, float h1, const float *R, const float *T) {
    const float a = ((0.0f + R[2] * h0) + R[5] * h1) + R[8] * 1.0f;
    float rho = T[2] * a;
    const float RtT_2 = ((0.0f + R[2] * T[0]) + R[5] * T[1]) + R[8] * T[2];
    rho -= RtT_2;
    const float m2 = ((0.0f + R[6] * g0) + R[7] * g1) + R[8] * 1.0f;
    rho /= (1.0f - m2 * a);
    return rho;
}

// What the transfer test needs of one edgel: Y = R31 X of the triangulated
// point and the view-3 observation in pixels; tested = joint inlier with rho > 0.
struct TransferEdgel {
    float Y0, Y1, Y2;
    float p0, p1;      // q0 K0 + K2, q1 K4 + K5
    bool joint, tested;
};

// Step 2 for edgel e; s is the edgel's candidate scale (meaningful when tested).
__device__ __forceinline__ TransferEdgel transfer_edgel(const Scene &sc, int e, const float *R21, const float *t21,
                                                        const float *R31, const float *t31, float &s) {
    TransferEdgel r;
    bool in21, in31;
    edgel_views(sc, e, R21, t21, R31, t31, in21, in31);
    const float2 g = *reinterpret_cast<const float2 *>(sc.loc + (size_t)e * 6);
    const float2 h = *reinterpret_cast<const float2 *>(sc.loc + (size_t)e * 6 + 2);
    const float2 q = *reinterpret_cast<const float2 *>(sc.loc + (size_t)e * 6 + 4);
    const float rho = depth_rho(g.x, g.y, h.x, h.y, R21, t21);
    const float X0 = rho * g.x, X1 = rho * g.y, X2 = rho;
    r.Y0 = ((0.0f + R31[0] * X0) + R31[1] * X1) + R31[2] * X2;
    r.Y1 = ((0.0f + R31[3] * X0) + R31[4] * X1) + R31[5] * X2;
    r.Y2 = ((0.0f + R31[6] * X0) + R31[7] * X1) + R31[8] * X2;
    const float a0 = q.y * r.Y2 - 1.0f * r.Y1, a1 = 1.0f * r.Y0 - q.x * r.Y2, a2 = q.x * r.Y1 - q.y * r.Y0;
    const float b0 = q.y * t31[2] - 1.0f * t31[1], b1 = 1.0f * t31[0] - q.x * t31[2], b2 = q.x * t31[1] - q.y * t31[0];
    s = -(((a0 * b0 + a1 * b1) + a2 * b2) / ((b0 * b0 + b1 * b1) + b2 * b2));
    r.p0 = q.x * sc.K0 + sc.K2;
    r.p1 = q.y * sc.K4 + sc.K5;
    r.joint = in21 && in31;
    r.tested = r.joint && rho > 0.0f;
    return r;
}

__device__ __forceinline__ bool is_voter(bool tested, float s) { return tested && __builtin_isfinite(s) && s > 0.0f; }

// Step 3, T(e, s) for a tested edgel: within 2 px of the view-3 observation,
// the error formed as reproj_inlier forms it.
__device__ __forceinline__ bool transfer_inlier(float Y0, float Y1, float Y2, float p0, float p1, float s,
                                                const float *t31, float K0, float K2, float K4, float K5) {
    const float Z0 = Y0 + s * t31[0], Z1 = Y1 + s * t31[1], Z2 = Y2 + s * t31[2];
    float m0 = Z0 / Z2, m1 = Z1 / Z2;
    m0 = m0 * K0 + K2;
    m1 = m1 * K4 + K5;
    m0 -= p0;
    m1 -= p1;
    const float err = __builtin_sqrtf((m0 * m0 + m1 * m1) + 0.0f * 0.0f);
    return Z2 > 0.0f && err < 2.0f;
}

// x[0..30] of a converged path: Evaluations.cpp:322-331, |Im x[24..29]| <
// IMAG_PART_TOL and Re x[0..7] >= 0 (wave-uniform result)
__device__ __forceinline__ bool is_candidate(const cf *__restrict__ x, int lane) {
    const cf xv = lane < NV ? x[lane] : cmk(0.0f, 0.0f);
    const unsigned long long im = __ballot(lane >= 24 && lane < NV && (double)__builtin_fabsf(xv.y) < 1e-5);
    const unsigned long long dp = __ballot(lane < 8 && xv.x >= 0.0f);
    return (im & 0x3F000000ull) == 0x3F000000ull && (dp & 0xFFull) == 0xFFull;
}

// The same filter where a path lives in one 32-lane half of a wave (the
// tracker): lane r of the half at bit offset hb holds xv = x[r] (r < NV).
// Uniform within the half.
__device__ __forceinline__ bool is_candidate_half(cf xv, int r, int hb) {
    const unsigned long long im = __ballot(r >= 24 && r < NV && (double)__builtin_fabsf(xv.y) < 1e-5);
    const unsigned long long dp = __ballot(r < 8 && xv.x >= 0.0f);
    return ((unsigned)(im >> hb) & 0x3F000000u) == 0x3F000000u && ((unsigned)(dp >> hb) & 0xFFu) == 0xFFu;
}

}  // namespace hc
