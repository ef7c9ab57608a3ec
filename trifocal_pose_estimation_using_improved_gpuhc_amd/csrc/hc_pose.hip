// hc_pose.hip -- device pose recovery + maximal-support selection (include/hc_pose.h).
//
// Replaces the host post-processing of every RANSAC round
// (magmaHC/GPU_HC_Solver.cpp:526-527):
//   Evaluations::Transform_GPUHC_Sols_to_Trifocal_Relative_Pose (Evaluations.cpp:298-358)
//   Evaluations::get_Solution_with_Maximal_Support              (Evaluations.cpp:382-504)
// with the multiview helpers of magmaHC/util.hpp restated op for op (FP32,
// no contraction: -ffp-contract=off; IEEE division and sqrt).
//
// One support kernel, k_pose_support<JOINT, GROUPED>, serves the four entry
// points.  Layout: one wavefront per batch id b (grid-stride).  Non-converged
// paths cost one byte load.  A candidate's pose is computed redundantly by
// every lane (uniform loads of x[18..29]), then the 64 lanes stride over the
// triplet edgels (E x 24 B, L2-resident after the first candidate), evaluate
// both views of an edgel (edgel_views) and the inlier counts are wave-reduced.
// Selection is a 64-bit atomicMax on key = count << 32 | b (largest count,
// ties -> largest b = the last candidate attaining the maximum, the rule of
// Evaluations.cpp:460,466); k_pose_final decodes the keys, one thread per
// selection, and writes the selected poses.
//   GROUPED: the samples of several triplets at once; a candidate is scored on
//            its own triplet's scene and published to its triplet's selection.
//   JOINT:   ONE candidate for both views, by the number of edgels that are
//            inliers in both (hcTrifocalSelection, one key); otherwise one key
//            per view (hcPoseSelection).
// The switches choose the scene, a third count and the key; the converged test,
// the candidate filter, make_pose and the edgel loop exist once, so a path's
// counts and pose bits are the same in every form.  k_pose_inlier_mask lists a
// joint selection's inlier edgels as a bit mask, through the same edgel_views.
// k_pose_refine<GROUPED> (include/refine/hc_pose_refine.h, described where it
// is defined below) refines a joint selection on the edgels edgel_views accepts.
// k_pose_topk<GROUPED>, k_pose_topk_final and k_pose_topk_select
// (include/topk/hc_pose_topk.h, described below the refinement) rank the k best
// joint candidates and select among their refinements.
// k_scale_vote<GROUPED> and k_scale_final<GROUPED> (include/scale/hc_pose_scale.h,
// described below the top-k) fit a refined selection's scale31 by three-view transfer.
// k_pose_refine3<GROUPED> (include/threeview/hc_pose_threeview.h, described at the
// end) then refines both views and the scale jointly on the three-view transfer.
// k_pose_structure<GROUPED> (include/structure/hc_pose_structure.h, in
// hc_structure.hpp) reconstructs the 3D edgels of the pose that goes out.
#include <type_traits>

#include "../../include/hc_pose.h"
#include "../../include/refine/hc_pose_refine.h"
#include "../../include/topk/hc_pose_topk.h"
#include "../../include/scale/hc_pose_scale.h"
#include "../../include/threeview/hc_pose_threeview.h"
#include "../../include/structure/hc_pose_structure.h"
#include "hc_device.hpp"
#include "hc_pose_device.hpp"   // make_pose, reproj_inlier, edgel_views, is_candidate: shared with the gated tracker

namespace hc {

extern thread_local hipError_t g_last_hip_error;   // hc_kernels.hip

namespace {

__device__ __forceinline__ bool is_converged(const uint8_t *conv, int b, int num_paths, bool quirks) {
    if (!quirks) return conv[b] != 0;
    const long long ci = (long long)b + (long long)NTRK * (b / NTRK);   // Evaluations.cpp:317
    return ci < num_paths && conv[ci] != 0;
}

__device__ __forceinline__ uint64_t sel_key(int count, int b, bool quirks) {
    return quirks ? (uint64_t)(0xFFFFFFFFu - (uint32_t)b) : (((uint64_t)(uint32_t)count << 32) | (uint32_t)b);
}

__device__ __forceinline__ void key_max(uint64_t *key, uint64_t v) {
    atomicMax(reinterpret_cast<unsigned long long *>(key), (unsigned long long)v);
}

template <bool JOINT>
using Selection = std::conditional_t<JOINT, hcTrifocalSelection, hcPoseSelection>;

// Arguments of a pose-support call, by value to both kernels.
template <bool JOINT>
struct PoseArgs {
    int num_paths;
    const cf *tracks;
    const uint8_t *conv;
    // the scene: (E, loc, K), or with GROUPED that of groups[sample_group[b / NTRK]]
    int E;
    const float *loc;
    const float *K;
    const hcTripletGroup *groups;
    const int32_t *sample_group;
    int flags;             // HC_POSE_REFERENCE_QUIRKS: <false, false> only
    int32_t *inl;          // per path (c21, c31), or with JOINT (joint, c21, c31); -1 for non-candidates
    Selection<JOINT> *sels;
    int num_sel;           // 1, or with GROUPED the number of triplets
};

template <bool JOINT, bool GROUPED>
__global__ void __launch_bounds__(256) k_pose_support(const PoseArgs<JOINT> a) {
    const int lane = lane_id();
    const int nw = gridDim.x * (blockDim.x / WAVE);
    const bool quirks = !JOINT && !GROUPED && (a.flags & HC_POSE_REFERENCE_QUIRKS) != 0;
    Scene sc{};
    if constexpr (!GROUPED) sc = load_scene(a.E, a.loc, a.K);
    for (int b = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE; b < a.num_paths; b += nw) {
        int c21 = -1, c31 = -1, cJ = -1;
        const cf *x = a.tracks + (size_t)b * (NV + 1);
        if (is_converged(a.conv, b, a.num_paths, quirks) && is_candidate(x, lane)) {
            Selection<JOINT> *sel = a.sels;
            if constexpr (GROUPED) {
                const int t = __builtin_amdgcn_readfirstlane(a.sample_group[b / NTRK]);   // wave-uniform
                const hcTripletGroup g = a.groups[t];
                sc = load_scene(g.num_edgels, g.locations, g.K);
                sel += t;
            }
            Pose P;
            make_pose(quirks ? a.tracks : x, P);   // quirk: converted from the base pointer (:334-341)
            int a21 = 0, a31 = 0, aJ = 0;
            for (int e = lane; e < sc.E; e += WAVE) {
                bool in21, in31;
                edgel_views(sc, e, P.R, P.t, P.R + 9, P.t + 3, in21, in31);
                a21 += in21 ? 1 : 0;
                a31 += in31 ? 1 : 0;
                if constexpr (JOINT) aJ += (in21 && in31) ? 1 : 0;
            }
            c21 = wave_sum_i(a21);
            c31 = wave_sum_i(a31);
            if constexpr (JOINT) cJ = wave_sum_i(aJ);
            if (lane == 0) {
                atomicAdd(&sel->num_candidates, 1);
                if constexpr (JOINT) {
                    key_max(&sel->key, sel_key(cJ, b, false));
                } else {
                    key_max(&sel->key21, sel_key(c21, b, quirks));
                    key_max(&sel->key31, sel_key(c31, b, quirks));
                }
            }
        }
        if (lane == 0) {
            if constexpr (JOINT) {
                a.inl[3 * (size_t)b] = cJ;
                a.inl[3 * (size_t)b + 1] = c21;
                a.inl[3 * (size_t)b + 2] = c31;
            } else {
                a.inl[2 * (size_t)b] = c21;
                a.inl[2 * (size_t)b + 1] = c31;
            }
        }
    }
}

// decode the keys of one selection; pose of the selected path (Evaluations.cpp:496-501)
__device__ __forceinline__ void decode_selection(int num_paths, const cf *__restrict__ tracks,
                                                 const int32_t *__restrict__ inl, bool quirks, hcPoseSelection *sel) {
    const bool any = sel->num_candidates > 0;
    for (int v = 0; v < 2; v++) {
        const uint64_t key = v == 0 ? sel->key21 : sel->key31;
        int b = -1, cnt = -1;
        if (any) {
            b = quirks ? (int)(0xFFFFFFFFu - (uint32_t)key) : (int)(uint32_t)key;
            cnt = (b >= 0 && b < num_paths) ? inl[2 * (size_t)b + v] : -1;
        }
        Pose P;
        for (int i = 0; i < 18; i++) P.R[i] = 0.0f;
        for (int i = 0; i < 6; i++) P.t[i] = 0.0f;
        if (b >= 0 && b < num_paths) make_pose(quirks ? tracks : tracks + (size_t)b * (NV + 1), P);
        float *R = v == 0 ? sel->R21 : sel->R31;
        float *t = v == 0 ? sel->t21 : sel->t31;
        for (int i = 0; i < 9; i++) R[i] = P.R[v * 9 + i];
        for (int i = 0; i < 3; i++) t[i] = P.t[v * 3 + i];
        if (v == 0) { sel->path21 = b; sel->inliers21 = cnt; }
        else { sel->path31 = b; sel->inliers31 = cnt; }
    }
}

// the joint selection of path b (-1: none): its counts, its pose for both views
// and |Re x[21..23]| / |Re x[18..20]| (the norms unit3 divides by).  num_candidates,
// key and the padding are not written: they are the launch's zeroes and atomics.
__device__ __forceinline__ void write_joint_path(int b, const cf *__restrict__ tracks, const int32_t *__restrict__ inl,
                                                 hcTrifocalSelection *sel) {
    Pose P;
    for (int i = 0; i < 18; i++) P.R[i] = 0.0f;
    for (int i = 0; i < 6; i++) P.t[i] = 0.0f;
    float scale = 0.0f;
    int cJ = -1, c21 = -1, c31 = -1;
    if (b >= 0) {
        const cf *x = tracks + (size_t)b * (NV + 1);
        make_pose(x, P);
        const float n21 = __builtin_sqrtf((x[18].x * x[18].x + x[19].x * x[19].x) + x[20].x * x[20].x);
        const float n31 = __builtin_sqrtf((x[21].x * x[21].x + x[22].x * x[22].x) + x[23].x * x[23].x);
        scale = n31 / n21;
        cJ = inl[3 * (size_t)b];
        c21 = inl[3 * (size_t)b + 1];
        c31 = inl[3 * (size_t)b + 2];
    }
    for (int i = 0; i < 9; i++) { sel->R21[i] = P.R[i]; sel->R31[i] = P.R[9 + i]; }
    for (int i = 0; i < 3; i++) { sel->t21[i] = P.t[i]; sel->t31[i] = P.t[3 + i]; }
    sel->path = b;
    sel->inliers = cJ;
    sel->inliers21 = c21;
    sel->inliers31 = c31;
    sel->scale31 = scale;
}

// decode the key of one joint selection
__device__ __forceinline__ void decode_joint(int num_paths, const cf *__restrict__ tracks,
                                             const int32_t *__restrict__ inl, hcTrifocalSelection *sel) {
    int b = -1;
    if (sel->num_candidates > 0) b = (int)(uint32_t)sel->key;
    if (b >= num_paths) b = -1;
    write_joint_path(b, tracks, inl, sel);
}

// one thread per selection (num_sel = 1 for the single-triplet calls)
template <bool JOINT>
__global__ void __launch_bounds__(64) k_pose_final(const PoseArgs<JOINT> a) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.num_sel) return;
    if constexpr (JOINT) decode_joint(a.num_paths, a.tracks, a.inl, a.sels + t);
    else decode_selection(a.num_paths, a.tracks, a.inl, (a.flags & HC_POSE_REFERENCE_QUIRKS) != 0, a.sels + t);
}

// Inlier mask of a device-resident selection: one wave per 64-bit word, lane l
// tests edgel 64w + l in both views with the selection's own R and t (the
// floats make_pose produced, so the bits are those counted in sel->inliers);
// the ballot is the word, written by lane 0.  Lanes at or beyond E and a
// selection without a path contribute 0.
__global__ void __launch_bounds__(256) k_pose_inlier_mask(const hcTrifocalSelection *__restrict__ sel, int E,
                                                          const float *__restrict__ loc, const float *__restrict__ K,
                                                          int num_words, unsigned long long *__restrict__ mask) {
    const int lane = lane_id();
    const int nw = gridDim.x * (blockDim.x / WAVE);
    const Scene sc = load_scene(E, loc, K);
    const bool have = sel->path >= 0;
    float R21[9], t21[3], R31[9], t31[3];
#pragma unroll
    for (int i = 0; i < 9; i++) { R21[i] = sel->R21[i]; R31[i] = sel->R31[i]; }
#pragma unroll
    for (int i = 0; i < 3; i++) { t21[i] = sel->t21[i]; t31[i] = sel->t31[i]; }
    for (int w = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE; w < num_words; w += nw) {
        const int e = w * WAVE + lane;
        bool in21 = false, in31 = false;
        if (have && e < E) edgel_views(sc, e, R21, t21, R31, t31, in21, in31);
        const unsigned long long word = __ballot(in21 && in31);
        if (lane == 0) mask[w] = word;
    }
}

// The zeroed selections every launch sequence below starts from (their keys and
// counts are atomics' targets).  A kernel of this library, not hipMemsetAsync:
// recorded in a graph, the runtime's memset node filled a selection with stale
// bytes at a later replay (tests/test_gpu_graph_replay.py), while a kernel node
// carries all it needs in its own arguments.
__global__ void __launch_bounds__(256) k_zero_words(uint32_t *__restrict__ p, unsigned n) {
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = 0u;
}

template <typename S>
hcStatus zero_selections(S *sels, size_t count, hipStream_t s) {
    static_assert(sizeof(S) % sizeof(uint32_t) == 0 && alignof(S) >= alignof(uint32_t), "whole 32-bit words");
    const size_t words = count * (sizeof(S) / sizeof(uint32_t));
    if (words == 0) return HC_SUCCESS;
    if (words > 0xFFFFFFFFull) return HC_ERROR_INVALID_VALUE;
    const size_t blocks = (words + 255) / 256;
    hipLaunchKernelGGL(k_zero_words, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s,
                       reinterpret_cast<uint32_t *>(sels), (unsigned)words);
    if ((g_last_hip_error = hipGetLastError()) != hipSuccess) return HC_ERROR_LAUNCH;
    return HC_SUCCESS;
}

// grid of the one-wave-per-path kernels: up to 32 waves per CU, 4 per block
inline hcStatus path_grid(int num_paths, int &blocks) {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess) return HC_ERROR_DEVICE;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return HC_ERROR_DEVICE;
    const long long waves = num_paths < cus * 32 ? num_paths : (long long)cus * 32;
    blocks = (int)((waves + 3) / 4);
    return HC_SUCCESS;
}

// The launch sequence of the four entry points (arguments already validated):
// zeroed selections, the support kernel over the paths, the decoding epilogue.
// Without paths there is no device query and no support launch, and the
// epilogue writes the "none" selections.
template <bool JOINT, bool GROUPED>
hcStatus launch_pose_support(const PoseArgs<JOINT> &a, hcStream stream) {
    hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
    const hcStatus zs = zero_selections(a.sels, (size_t)a.num_sel, s);
    if (zs != HC_SUCCESS) return zs;
    if (a.num_paths > 0) {
        int blocks = 0;
        const hcStatus st = path_grid(a.num_paths, blocks);
        if (st != HC_SUCCESS) return st;
        hipLaunchKernelGGL((k_pose_support<JOINT, GROUPED>), dim3(blocks), dim3(256), 0, s, a);
        if ((g_last_hip_error = hipGetLastError()) != hipSuccess) return HC_ERROR_LAUNCH;
    }
    hipLaunchKernelGGL(k_pose_final<JOINT>, dim3((a.num_sel + 63) / 64), dim3(64), 0, s, a);
    if ((g_last_hip_error = hipGetLastError()) != hipSuccess) return HC_ERROR_LAUNCH;
    return HC_SUCCESS;
}

template <bool JOINT>
hcStatus pose_support_single(int num_paths, const hcComplex *tracks, const uint8_t *converge, int num_edgels,
                             const float *locations, const float *K, int flags, int32_t *inliers,
                             Selection<JOINT> *selection, hcStream stream) {
    constexpr int allowed_flags = JOINT ? 0 : HC_POSE_REFERENCE_QUIRKS;
    if (num_paths < 0 || num_edgels < 0 || !selection || (flags & ~allowed_flags) != 0) return HC_ERROR_INVALID_VALUE;
    if (num_paths > 0 && (!tracks || !converge || !inliers || !K || (num_edgels > 0 && !locations)))
        return HC_ERROR_INVALID_VALUE;
    const PoseArgs<JOINT> a{num_paths, (const cf *)tracks, converge, num_edgels, locations, K, nullptr, nullptr,
                            flags, inliers, selection, 1};
    return launch_pose_support<JOINT, false>(a, stream);
}

// (the quirks flag's literal indexing has no per-group meaning: no flag is accepted)
template <bool JOINT>
hcStatus pose_support_grouped(int num_paths, const hcComplex *tracks, const uint8_t *converge, int num_groups,
                              const hcTripletGroup *groups, const int32_t *sample_group, int flags, int32_t *inliers,
                              Selection<JOINT> *selections, hcStream stream) {
    if (num_paths < 0 || num_paths % NTRK != 0 || num_groups < 1 || !groups || !selections || flags != 0)
        return HC_ERROR_INVALID_VALUE;
    if (num_paths > 0 && (!tracks || !converge || !inliers || !sample_group)) return HC_ERROR_INVALID_VALUE;
    const PoseArgs<JOINT> a{num_paths, (const cf *)tracks, converge, 0, nullptr, nullptr, groups, sample_group,
                            0, inliers, selections, num_groups};
    return launch_pose_support<JOINT, true>(a, stream);
}

// ---- refinement of a joint selection (include/refine/hc_pose_refine.h) ------
//
// k_pose_refine<GROUPED>: one workgroup of 256 threads per selection, the whole
// Gauss-Newton loop in one launch.  An iterate is one pass over the edgels:
// thread i takes edgels i, i + 256, ..., scores each with edgel_views on the
// state rounded to float (the bits k_pose_inlier_mask and the support kernel
// test) and, for a joint inlier, adds the residual and its 2x5 Jacobian of both
// views, in double at the double state, to its 2 x (15 + 5 + 1) sums.  The sums
// go through a butterfly over the wave's lanes, then through LDS over the four
// waves as (w0 + w1) + (w2 + w3): a fixed tree, no floating-point atomics.
// Lanes 0 and 1 solve the two 5x5 systems and write the new state to LDS, from
// where every thread reads it.  Nothing waits on another workgroup.
constexpr int RF_THREADS = 256, RF_WAVES = RF_THREADS / WAVE;
constexpr int RF_SYS = 21;   // per view: the 15 upper entries of A = sum J'J, the 5 of g = sum J'r, sum r'r

struct RefineArgs {
    const hcTrifocalSelection *in;
    hcTrifocalSelection *out;   // may be in
    hcRefineReport *rep;        // or nullptr
    int E;                      // the scene, or with GROUPED that of groups[blockIdx.x / per_group]
    const float *loc;
    const float *K;
    const hcTripletGroup *groups;
    int iterations, min_inliers;
    int per_group;              // GROUPED: selections per triplet (1, or the k of the top-k call)
};

__device__ __forceinline__ double wave_sum_d(double v) {
    v += __shfl_xor(v, 32);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    return v;   // the same bits in every lane: each step adds the same pair on both sides
}

// b[0..2] = b1 = normalize(t x e_i), i the axis of smallest |t_i| (the lowest on a tie); b[3..5] = b2 = t x b1
__device__ __forceinline__ void tangent_basis(const double *t, double *b) {
    int i = 0;
    double m = __builtin_fabs(t[0]);
    if (__builtin_fabs(t[1]) < m) { i = 1; m = __builtin_fabs(t[1]); }
    if (__builtin_fabs(t[2]) < m) i = 2;
    b[0] = i == 0 ? 0.0 : (i == 1 ? -t[2] : t[1]);
    b[1] = i == 0 ? t[2] : (i == 1 ? 0.0 : -t[0]);
    b[2] = i == 0 ? -t[1] : (i == 1 ? t[0] : 0.0);
    const double n = __builtin_sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
    b[0] /= n; b[1] /= n; b[2] /= n;
    b[3] = t[1] * b[2] - t[2] * b[1];
    b[4] = t[2] * b[0] - t[0] * b[2];
    b[5] = t[0] * b[1] - t[1] * b[0];
}

// One view of one edgel: reproj_inlier's m - p in double, its derivative along
// the five local directions (w = e0, e1, e2 with dR = [w]x R; dt = b1, b2), and
// the sums.  c = R e3, a = c.h, m = R g, rho = (t2 a - c.t) / (1 - m2 a), q = m rho + t.
__device__ __forceinline__ void view_accumulate(double g0, double g1, double h0, double h1, const double *R,
                                                const double *t, const double *b, double K0, double K2, double K4,
                                                double K5, double *acc) {
    const double c[3] = {R[2], R[5], R[8]};
    const double a = (c[0] * h0 + c[1] * h1) + c[2];
    const double ct = (c[0] * t[0] + c[1] * t[1]) + c[2] * t[2];
    const double m[3] = {(R[0] * g0 + R[1] * g1) + R[2], (R[3] * g0 + R[4] * g1) + R[5], (R[6] * g0 + R[7] * g1) + R[8]};
    const double den = 1.0 - m[2] * a;
    const double rho = (t[2] * a - ct) / den;
    const double q[3] = {m[0] * rho + t[0], m[1] * rho + t[1], m[2] * rho + t[2]};
    const double x = q[0] / q[2], y = q[1] / q[2];
    const double r0 = (x * K0 + K2) - (h0 * K0 + K2), r1 = (y * K4 + K5) - (h1 * K4 + K5);
    const double iden = 1.0 / den, iq2 = 1.0 / q[2];   // the derivatives multiply by the reciprocals: 5 divisions, not 18
    double J0[5], J1[5];
#pragma unroll
    for (int d = 0; d < 5; d++) {
        double dc[3] = {0.0, 0.0, 0.0}, dm[3] = {0.0, 0.0, 0.0}, dt[3] = {0.0, 0.0, 0.0};
        if (d == 0) { dc[1] = -c[2]; dc[2] = c[1]; dm[1] = -m[2]; dm[2] = m[1]; }        // e0 x v = (0, -v2, v1)
        else if (d == 1) { dc[0] = c[2]; dc[2] = -c[0]; dm[0] = m[2]; dm[2] = -m[0]; }   // e1 x v = (v2, 0, -v0)
        else if (d == 2) { dc[0] = -c[1]; dc[1] = c[0]; dm[0] = -m[1]; dm[1] = m[0]; }   // e2 x v = (-v1, v0, 0)
        else { dt[0] = b[3 * (d - 3)]; dt[1] = b[3 * (d - 3) + 1]; dt[2] = b[3 * (d - 3) + 2]; }
        const double da = (dc[0] * h0 + dc[1] * h1) + dc[2];
        const double dct = ((dc[0] * t[0] + dc[1] * t[1]) + dc[2] * t[2]) + ((c[0] * dt[0] + c[1] * dt[1]) + c[2] * dt[2]);
        const double dnum = (dt[2] * a + t[2] * da) - dct;
        const double dden = -(dm[2] * a + m[2] * da);
        const double drho = (dnum - rho * dden) * iden;
        const double dq0 = (dm[0] * rho + m[0] * drho) + dt[0];
        const double dq1 = (dm[1] * rho + m[1] * drho) + dt[1];
        const double dq2 = (dm[2] * rho + m[2] * drho) + dt[2];
        J0[d] = K0 * ((dq0 - x * dq2) * iq2);
        J1[d] = K4 * ((dq1 - y * dq2) * iq2);
    }
    int n = 0;
#pragma unroll
    for (int i = 0; i < 5; i++)
#pragma unroll
        for (int j = i; j < 5; j++) acc[n++] += J0[i] * J0[j] + J1[i] * J1[j];
#pragma unroll
    for (int i = 0; i < 5; i++) acc[15 + i] += J0[i] * r0 + J1[i] * r1;
    acc[20] += r0 * r0 + r1 * r1;
}

// (A + 1e-9 diag A) d = -g by Cholesky, s = one view's sums; false when a pivot
// is not positive or a value is not finite
__device__ __forceinline__ bool refine_solve(const double *s, double *d) {
    double M[5][5], L[5][5];
    int n = 0;
#pragma unroll
    for (int i = 0; i < 5; i++)
#pragma unroll
        for (int j = i; j < 5; j++) { M[i][j] = M[j][i] = s[n]; n++; }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 5; i++) {
        M[i][i] = M[i][i] + 1e-9 * M[i][i];
        ok = ok && __builtin_isfinite(s[15 + i]);
#pragma unroll
        for (int j = 0; j < 5; j++) ok = ok && __builtin_isfinite(M[i][j]);
    }
#pragma unroll
    for (int j = 0; j < 5; j++) {
        double p = M[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) p -= L[j][k] * L[j][k];
        ok = ok && p > 0.0;
        L[j][j] = __builtin_sqrt(p);
#pragma unroll
        for (int i = j + 1; i < 5; i++) {
            double v = M[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    double y[5];
#pragma unroll
    for (int i = 0; i < 5; i++) {
        double v = -s[15 + i];
#pragma unroll
        for (int k = 0; k < i; k++) v -= L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = 4; i >= 0; i--) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < 5; k++) v -= L[k][i] * d[k];
        d[i] = v / L[i][i];
        ok = ok && __builtin_isfinite(d[i]);
    }
    return ok;
}

// st = R (9, row-major) | t (3) of one view in LDS: R <- Exp(w) R by Rodrigues'
// formula, column by column; t <- normalize(t + u0 b1 + u1 b2).  d = (w, u).
__device__ __forceinline__ void refine_apply(double *st, const double *d) {
    const double th2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    double A = 1.0 - th2 / 6.0, B = 0.5 - th2 / 24.0;
    if (th2 >= 1e-16) {
        const double th = __builtin_sqrt(th2), sh = sin(0.5 * th);
        A = sin(th) / th;
        B = 2.0 * sh * sh / th2;
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const double c0 = st[j], c1 = st[3 + j], c2 = st[6 + j];
        const double w0 = d[1] * c2 - d[2] * c1, w1 = d[2] * c0 - d[0] * c2, w2 = d[0] * c1 - d[1] * c0;   // w x c
        const double v0 = d[1] * w2 - d[2] * w1, v1 = d[2] * w0 - d[0] * w2, v2 = d[0] * w1 - d[1] * w0;   // w x (w x c)
        st[j] = c0 + (A * w0 + B * v0);
        st[3 + j] = c1 + (A * w1 + B * v1);
        st[6 + j] = c2 + (A * w2 + B * v2);
    }
    double t[3] = {st[9], st[10], st[11]}, b[6];
    tangent_basis(t, b);
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = t[i] + (d[3] * b[i] + d[4] * b[3 + i]);
    const double n = __builtin_sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
#pragma unroll
    for (int i = 0; i < 3; i++) st[9 + i] = t[i] / n;
}

template <bool GROUPED>
__global__ void __launch_bounds__(RF_THREADS) k_pose_refine(const RefineArgs a) {
    __shared__ double s_sum[RF_WAVES][2 * RF_SYS];
    __shared__ double s_state[2][12];   // per view R | t, the double state
    __shared__ float s_best[24];        // the best iterate's scored floats: R21 | t21 | R31 | t31
    __shared__ int s_cnt[RF_WAVES][3];
    __shared__ int s_singular;
    const int tid = threadIdx.x, lane = lane_id(), wave = tid / WAVE, sel = blockIdx.x;
    Scene sc;
    if constexpr (GROUPED) {
        const hcTripletGroup g = a.groups[sel / a.per_group];
        sc = load_scene(g.num_edgels, g.locations, g.K);
    } else {
        sc = load_scene(a.E, a.loc, a.K);
    }
    // every thread reads the input here, before the first barrier; thread 0
    // writes the output after the last one (out may be in; a workgroup touches
    // no other selection than its own)
    const hcTrifocalSelection keep = a.in[sel];
    hcRefineReport *rep = a.rep ? a.rep + sel : nullptr;
    if (keep.path < 0) {
        if (tid == 0) {
            a.out[sel] = keep;
            if (rep) {
                rep->status = HC_REFINE_NONE;
                rep->iterations_run = rep->best_iteration = 0;
                for (int i = 0; i <= HC_REFINE_MAX_ITERATIONS; i++) rep->joint_history[i] = -1;
                rep->rms_px_in[0] = rep->rms_px_in[1] = rep->rms_px_out[0] = rep->rms_px_out[1] = 0.0;
            }
        }
        return;
    }
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 9; i++) { s_state[0][i] = (double)keep.R21[i]; s_state[1][i] = (double)keep.R31[i]; }
#pragma unroll
        for (int i = 0; i < 3; i++) { s_state[0][9 + i] = (double)keep.t21[i]; s_state[1][9 + i] = (double)keep.t31[i]; }
    }
    __syncthreads();
    const double K0 = (double)sc.K0, K2 = (double)sc.K2, K4 = (double)sc.K4, K5 = (double)sc.K5;
    int status = 0, k = 0, bestJ = -1, best21 = 0, best31 = 0, bestK = 0;
    double rms_in[2] = {0.0, 0.0}, rms_out[2] = {0.0, 0.0};
    for (;;) {
        double R[18], T[6], B[12];
        float Rf[18], Tf[6];
#pragma unroll
        for (int i = 0; i < 9; i++) { R[i] = s_state[0][i]; R[9 + i] = s_state[1][i]; }
#pragma unroll
        for (int i = 0; i < 3; i++) { T[i] = s_state[0][9 + i]; T[3 + i] = s_state[1][9 + i]; }
#pragma unroll
        for (int i = 0; i < 18; i++) Rf[i] = (float)R[i];
#pragma unroll
        for (int i = 0; i < 6; i++) Tf[i] = (float)T[i];
        tangent_basis(T, B);
        tangent_basis(T + 3, B + 6);
        double acc[2 * RF_SYS];
#pragma unroll
        for (int i = 0; i < 2 * RF_SYS; i++) acc[i] = 0.0;
        int c21 = 0, c31 = 0, cJ = 0;
        for (int e = tid; e < sc.E; e += RF_THREADS) {
            bool in21, in31;
            edgel_views(sc, e, Rf, Tf, Rf + 9, Tf + 3, in21, in31);
            c21 += in21 ? 1 : 0;
            c31 += in31 ? 1 : 0;
            if (in21 && in31) {
                cJ++;
                const float *p = sc.loc + (size_t)e * 6;
                const double g0 = (double)p[0], g1 = (double)p[1];
                view_accumulate(g0, g1, (double)p[2], (double)p[3], R, T, B, K0, K2, K4, K5, acc);
                view_accumulate(g0, g1, (double)p[4], (double)p[5], R + 9, T + 3, B + 6, K0, K2, K4, K5, acc + RF_SYS);
            }
        }
#pragma unroll
        for (int i = 0; i < 2 * RF_SYS; i++) acc[i] = wave_sum_d(acc[i]);
        c21 = wave_sum_i(c21);
        c31 = wave_sum_i(c31);
        cJ = wave_sum_i(cJ);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 2 * RF_SYS; i++) s_sum[wave][i] = acc[i];
            s_cnt[wave][0] = cJ;
            s_cnt[wave][1] = c21;
            s_cnt[wave][2] = c31;
        }
        __syncthreads();
        // the totals, the same in every thread
        cJ = (s_cnt[0][0] + s_cnt[1][0]) + (s_cnt[2][0] + s_cnt[3][0]);
        c21 = (s_cnt[0][1] + s_cnt[1][1]) + (s_cnt[2][1] + s_cnt[3][1]);
        c31 = (s_cnt[0][2] + s_cnt[1][2]) + (s_cnt[2][2] + s_cnt[3][2]);
        double rms[2];
#pragma unroll
        for (int v = 0; v < 2; v++) {
            const int i = v * RF_SYS + 20;
            const double sse = (s_sum[0][i] + s_sum[1][i]) + (s_sum[2][i] + s_sum[3][i]);
            rms[v] = cJ > 0 ? __builtin_sqrt(sse / (double)cJ) : 0.0;
        }
        if (k == 0) { rms_in[0] = rms[0]; rms_in[1] = rms[1]; }
        if (tid == 0 && rep) rep->joint_history[k] = cJ;
        if (cJ >= bestJ) {   // a tie goes to the later iterate
            bestJ = cJ; best21 = c21; best31 = c31; bestK = k;
            rms_out[0] = rms[0]; rms_out[1] = rms[1];
            if (tid == 0) {
#pragma unroll
                for (int i = 0; i < 9; i++) { s_best[i] = Rf[i]; s_best[12 + i] = Rf[9 + i]; }
#pragma unroll
                for (int i = 0; i < 3; i++) { s_best[9 + i] = Tf[i]; s_best[21 + i] = Tf[3 + i]; }
            }
        }
        if (cJ < a.min_inliers) { status |= HC_REFINE_TOO_FEW; break; }
        if (k == a.iterations) break;
        if (wave == 0) {
            bool ok = true;
            double d[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
            if (lane < 2) {
                double s[RF_SYS];
#pragma unroll
                for (int i = 0; i < RF_SYS; i++) {
                    const int j = lane * RF_SYS + i;
                    s[i] = (s_sum[0][j] + s_sum[1][j]) + (s_sum[2][j] + s_sum[3][j]);
                }
                ok = refine_solve(s, d);
            }
            const bool bad = __ballot(!ok) != 0;
            if (lane == 0) s_singular = bad ? 1 : 0;
            if (!bad && lane < 2) refine_apply(s_state[lane], d);
        }
        __syncthreads();
        if (s_singular) { status |= HC_REFINE_SINGULAR; break; }
        k++;
    }
    if (tid != 0) return;
    hcTrifocalSelection o = keep;
    if (bestJ >= a.min_inliers || bestK > 0) {   // otherwise iterate 0 had too few: the input, unchanged
        o.inliers = bestJ;
        o.inliers21 = best21;
        o.inliers31 = best31;
        o.key = ((uint64_t)(uint32_t)bestJ << 32) | (uint32_t)keep.path;
#pragma unroll
        for (int i = 0; i < 9; i++) { o.R21[i] = s_best[i]; o.R31[i] = s_best[12 + i]; }
#pragma unroll
        for (int i = 0; i < 3; i++) { o.t21[i] = s_best[9 + i]; o.t31[i] = s_best[21 + i]; }
    }
    a.out[sel] = o;
    if (rep) {
        rep->status = status;
        rep->iterations_run = k;
        rep->best_iteration = bestK;
        for (int i = k + 1; i <= HC_REFINE_MAX_ITERATIONS; i++) rep->joint_history[i] = -1;
        rep->rms_px_in[0] = rms_in[0]; rep->rms_px_in[1] = rms_in[1];
        rep->rms_px_out[0] = rms_out[0]; rep->rms_px_out[1] = rms_out[1];
    }
}

// settings (a host pointer or nullptr) -> the values the kernel runs with; false when out of range
inline bool refine_settings(const hcRefineSettings *s, int &iterations, int &min_inliers) {
    iterations = 10;
    min_inliers = 16;
    if (!s) return true;
    if (s->iterations < 0 || s->iterations > HC_REFINE_MAX_ITERATIONS) return false;
    if (s->min_inliers < 0 || (s->min_inliers > 0 && s->min_inliers < 6)) return false;
    if (s->iterations > 0) iterations = s->iterations;
    if (s->min_inliers > 0) min_inliers = s->min_inliers;
    return true;
}

template <bool GROUPED>
hcStatus launch_pose_refine(const RefineArgs &a, int num_selections, hcStream stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_pose_refine<GROUPED>, dim3(num_selections), dim3(RF_THREADS), 0, (hipStream_t)stream, a);
    if ((g_last_hip_error = hipGetLastError()) != hipSuccess) return HC_ERROR_LAUNCH;
    return HC_SUCCESS;
}

// ---- the k best joint candidates (include/topk/hc_pose_topk.h) ---------------
//
// k_pose_topk<GROUPED>: one pass over the per-path joint counts, one thread per
// batch id (grid-stride).  The k output slots of a group are the data structure:
// a candidate offers its key v = joint << 32 | b to slot 0 with a 64-bit
// atomicMax, carries the smaller of (old, v) to slot 1, and so on; a value that
// is 0 or falls off the end is dropped.  Slot i ends with the i-th largest key:
// every key is offered to slot 0, which ends with the maximum; every key that
// does not end in slot 0 is at some moment carried to slot 1; and so on down.
// The keys are distinct (b is in them), so the final state does not depend on
// the order of arrival: two runs write the same bytes.  A slot's value only
// grows, so a key below what slot k-1 holds at any moment can be skipped.
// Candidates are about 0.1 % of the paths: no pre-reduction.  The group's
// candidates are counted in slot 0's num_candidates, as k_pose_support does.
// The key 0 (no joint inlier, batch id 0) is never inserted and needs not be:
// it is the smallest key, and the zeroed slot that it would end in holds it.
struct TopkArgs {
    int num_paths;
    const cf *tracks;
    const int32_t *inl;            // (joint, c21, c31) per path, joint < 0: no candidate
    const int32_t *sample_group;   // GROUPED
    int k;
    hcTrifocalSelection *cand;     // num_groups x k
    int num_groups;
};

template <bool GROUPED>
__global__ void __launch_bounds__(256) k_pose_topk(const TopkArgs a) {
    const int stride = gridDim.x * blockDim.x;
    for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < a.num_paths; b += stride) {
        const int cJ = a.inl[3 * (size_t)b];
        if (cJ < 0) continue;
        hcTrifocalSelection *slots = a.cand;
        if constexpr (GROUPED) slots += (size_t)a.sample_group[b / NTRK] * a.k;
        atomicAdd(&slots[0].num_candidates, 1);
        unsigned long long v = sel_key(cJ, b, false);
        const unsigned long long last =
            __atomic_load_n(reinterpret_cast<unsigned long long *>(&slots[a.k - 1].key), __ATOMIC_RELAXED);
        if (v < last) continue;   // a stale value only skips less
        for (int i = 0; i < a.k && v != 0; i++) {
            const unsigned long long old = atomicMax(reinterpret_cast<unsigned long long *>(&slots[i].key), v);
            if (old < v) v = old;
        }
    }
}

// one thread per (group, rank): the selection of the rank's key, "none" at or
// beyond the number of candidates.  Slot 0's num_candidates is the pass's
// counter and is only read here; the other ranks copy it.
__global__ void __launch_bounds__(64) k_pose_topk_final(const TopkArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.num_groups * a.k) return;
    const int r = i % a.k;
    hcTrifocalSelection *sel = a.cand + i;
    const int nc = a.cand[i - r].num_candidates;
    int b = -1;
    if (r < nc) b = (int)(uint32_t)sel->key;
    if (b >= a.num_paths) b = -1;
    write_joint_path(b, a.tracks, a.inl, sel);
    if (r > 0) sel->num_candidates = nc;
}

// one thread per group: the refined selection with the largest key among those
// with a path, or "none" with rank -1
__global__ void __launch_bounds__(64) k_pose_topk_select(int num_groups, int k,
                                                         const hcTrifocalSelection *__restrict__ refined,
                                                         hcTrifocalSelection *__restrict__ best,
                                                         int32_t *__restrict__ best_rank) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= num_groups) return;
    const hcTrifocalSelection *in = refined + (size_t)t * k;
    int rank = -1;
    uint64_t key = 0;
    for (int r = 0; r < k; r++) {
        if (in[r].path < 0) continue;
        if (rank < 0 || in[r].key > key) { rank = r; key = in[r].key; }
    }
    hcTrifocalSelection o;
    if (rank >= 0) {
        o = in[rank];
    } else {
        o.num_candidates = in[0].num_candidates;
        o.path = o.inliers = o.inliers21 = o.inliers31 = -1;
        o.pad = 0;
        o.key = 0;
        for (int i = 0; i < 9; i++) o.R21[i] = o.R31[i] = 0.0f;
        for (int i = 0; i < 3; i++) o.t21[i] = o.t31[i] = 0.0f;
        o.scale31 = o.pad2 = 0.0f;
    }
    best[t] = o;
    best_rank[t] = rank;
}

// zeroed slots, the pass over the paths, the decoding epilogue (arguments validated)
template <bool GROUPED>
hcStatus launch_pose_topk(const TopkArgs &a, hcStream stream) {
    hipStream_t s = (hipStream_t)stream;
    const int slots = a.num_groups * a.k;
    (void)hipGetLastError();
    const hcStatus zs = zero_selections(a.cand, (size_t)slots, s);
    if (zs != HC_SUCCESS) return zs;
    if (a.num_paths > 0) {
        const int want = (a.num_paths + 255) / 256;
        hipLaunchKernelGGL(k_pose_topk<GROUPED>, dim3(want < 2048 ? want : 2048), dim3(256), 0, s, a);
        if ((g_last_hip_error = hipGetLastError()) != hipSuccess) return HC_ERROR_LAUNCH;
    }
    hipLaunchKernelGGL(k_pose_topk_final, dim3((slots + 63) / 64), dim3(64), 0, s, a);
    if ((g_last_hip_error = hipGetLastError()) != hipSuccess) return HC_ERROR_LAUNCH;
    return HC_SUCCESS;
}

// ---- the relative scale by three-view transfer (include/scale/hc_pose_scale.h) ----
//
// A mode of the four refine calls: after k_pose_refine (or instead of it, with
// HC_SCALE_ONLY) every selection's scale31 is fitted by the vote the header
// describes, |tested| transfer tests per voter.
//
// k_scale_vote<GROUPED>: grid (selections, voter tiles), a tile of 64 voters
// per workgroup of 8 waves.  Lane l of every wave holds voter v = 64 j + l of
// tile j: it forms the edgel's candidate scale s_v once and keeps it in a
// register.  The workgroup then stages the edgels in chunks of SV_CHUNK into
// LDS -- per edgel Y = R31 X, the tested flag and the view-3 pixel, 24 bytes,
// recomputed by every workgroup (E^2 / 64 edgel evaluations beside E^2 transfer
// tests: no scratch buffer, so no allocation) -- and wave w walks entries w,
// w + 8, ... of the chunk: all lanes read the same address (a broadcast), an
// edgel outside the tested set is skipped by a scalar branch on its flag, and
// the lane counts T(e, s_v).  The eight waves' counts of a voter are integers
// summed through LDS (any order gives the same number); wave 0 forms the keys
// c_v << 32 | v and reduces them by a butterfly over its lanes; one 64-bit
// atomicMax and one atomicAdd (the voters) per workgroup go to the selection's
// hcScaleReport, which k_zero_words has zeroed on the same stream.  Splitting
// the edgels over the waves, not only the voters over the lanes, is what fills
// the device: a scene of 5117 edgels gives 80 workgroups of 8 waves, where one
// voter per thread of a 256-thread workgroup gave 80 waves in all and the walk
// of 3640 tests per lane, a dependent chain of two divisions and a square root
// each, took 0.9 ms.  A grouped call does not know its triplets' E on the host:
// its grid has SV_TILES tiles and a workgroup strides over the voter tiles of
// its own triplet.
//
// k_scale_final<GROUPED>: one workgroup per selection.  It decodes the key,
// re-evaluates T(e, scale31) of every edgel with the same device functions, one
// wave per 64 edgels -- the ballot is the transfer mask's word -- counts the
// tested set and the joint inliers, and writes out (src with only scale31
// replaced) and the report.
constexpr int SV_THREADS = 512, SV_WAVES = SV_THREADS / WAVE;   // the vote: 64 voters x 8 slices of the edgels
constexpr int SV_CHUNK = 2048;   // edgels per LDS stage: 48 KiB
constexpr int SV_TILES = 128;    // grid.y of a grouped call: 8192 voters without a second pass
constexpr int SF_THREADS = 256, SF_WAVES = SF_THREADS / WAVE;   // the epilogue

struct ScaleArgs {
    const hcTrifocalSelection *src;   // the poses to fit: the refinement's out, or with HC_SCALE_ONLY its in
    hcTrifocalSelection *out;         // may be src
    hcScaleReport *rep;
    unsigned long long *mask;         // or nullptr; the single call only
    int E;                            // the scene, or with GROUPED that of groups[selection / per_group]
    const float *loc;
    const float *K;
    const hcTripletGroup *groups;
    int per_group;
};

template <bool GROUPED>
__device__ __forceinline__ Scene scale_scene(const ScaleArgs &a, int sel) {
    if constexpr (GROUPED) {
        const hcTripletGroup g = a.groups[sel / a.per_group];
        return load_scene(g.num_edgels, g.locations, g.K);
    } else {
        return load_scene(a.E, a.loc, a.K);
    }
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;   // the same in every lane
}

template <bool GROUPED>
__global__ void __launch_bounds__(SV_THREADS) k_scale_vote(const ScaleArgs a) {
    __shared__ float4 s_Y[SV_CHUNK];   // Y0 Y1 Y2 | tested (1.0f or 0.0f)
    __shared__ float2 s_p[SV_CHUNK];   // the view-3 observation in pixels
    __shared__ int s_c[SV_WAVES][WAVE];
    const int tid = threadIdx.x, lane = lane_id(), wave = tid / WAVE, sel = blockIdx.x;
    const Scene sc = scale_scene<GROUPED>(a, sel);
    const int tiles = (sc.E + WAVE - 1) / WAVE;
    const hcTrifocalSelection *S = a.src + sel;
    if ((int)blockIdx.y >= tiles || S->path < 0) return;   // the whole workgroup
    float R21[9], t21[3], R31[9], t31[3];
#pragma unroll
    for (int i = 0; i < 9; i++) { R21[i] = S->R21[i]; R31[i] = S->R31[i]; }
#pragma unroll
    for (int i = 0; i < 3; i++) { t21[i] = S->t21[i]; t31[i] = S->t31[i]; }
    unsigned long long best = 0;   // wave 0 only
    int nv = 0;
    for (int tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
        const int v = tile * WAVE + lane;   // the same 64 voters in every wave
        float s_v = 0.0f;
        bool voter = false;
        if (v < sc.E) {
            const TransferEdgel te = transfer_edgel(sc, v, R21, t21, R31, t31, s_v);
            voter = is_voter(te.tested, s_v);
        }
        const bool tile_votes = __ballot(voter) != 0;   // the same in every wave
        int c = 0;
        for (int c0 = 0; c0 < sc.E; c0 += SV_CHUNK) {
            const int n = sc.E - c0 < SV_CHUNK ? sc.E - c0 : SV_CHUNK;
            __syncthreads();   // the previous stage has been walked, the previous tile's counts read
            for (int i = tid; i < n; i += SV_THREADS) {
                float s;
                const TransferEdgel te = transfer_edgel(sc, c0 + i, R21, t21, R31, t31, s);
                s_Y[i] = make_float4(te.Y0, te.Y1, te.Y2, te.tested ? 1.0f : 0.0f);
                s_p[i] = make_float2(te.p0, te.p1);
            }
            __syncthreads();
            if (!tile_votes) continue;
            for (int i = wave; i < n; i += SV_WAVES) {
                const float4 Y = s_Y[i];
                if (__builtin_amdgcn_readfirstlane(__float_as_int(Y.w)) == 0) continue;   // not tested: the same for all lanes
                const float2 p = s_p[i];
                c += transfer_inlier(Y.x, Y.y, Y.z, p.x, p.y, s_v, t31, sc.K0, sc.K2, sc.K4, sc.K5) ? 1 : 0;
            }
        }
        s_c[wave][lane] = c;
        __syncthreads();
        if (wave == 0 && voter) {
            int cv = 0;
#pragma unroll
            for (int w = 0; w < SV_WAVES; w++) cv += s_c[w][lane];
            nv++;
            const unsigned long long key = ((unsigned long long)(uint32_t)cv << 32) | (uint32_t)v;
            best = key > best ? key : best;
        }
    }
    if (wave != 0) return;
    best = wave_max_u64(best);
    nv = wave_sum_i(nv);
    if (lane == 0 && nv > 0) {
        atomicAdd(&a.rep[sel].num_voters, nv);
        key_max(&a.rep[sel].key, best);
    }
}

template <bool GROUPED>
__global__ void __launch_bounds__(SF_THREADS) k_scale_final(const ScaleArgs a) {
    __shared__ int s_cnt[SF_WAVES][2];
    const int tid = threadIdx.x, lane = lane_id(), wave = tid / WAVE, sel = blockIdx.x;
    const Scene sc = scale_scene<GROUPED>(a, sel);
    // every thread reads src and the vote's words here, before the barrier;
    // thread 0 writes out and the report after it (out may be src)
    const hcTrifocalSelection keep = a.src[sel];
    hcScaleReport *rep = a.rep + sel;
    const int num_voters = rep->num_voters;
    const uint64_t key = rep->key;
    const bool have = keep.path >= 0, fitted = have && num_voters > 0 && (uint32_t)key < (uint32_t)sc.E;
    const int voter = fitted ? (int)(uint32_t)key : -1;
    float scale = keep.scale31;
    if (fitted) {
        (void)transfer_edgel(sc, voter, keep.R21, keep.t21, keep.R31, keep.t31, scale);   // s_v again, the same bits
    }
    const int words = (sc.E + WAVE - 1) / WAVE;
    int tested = 0, joint = 0;
    for (int w = wave; w < words; w += SF_WAVES) {
        const int e = w * WAVE + lane;
        bool in = false;
        if (have && e < sc.E) {
            float s;
            const TransferEdgel te = transfer_edgel(sc, e, keep.R21, keep.t21, keep.R31, keep.t31, s);
            tested += te.tested ? 1 : 0;
            joint += te.joint ? 1 : 0;
            in = fitted && te.tested &&
                 transfer_inlier(te.Y0, te.Y1, te.Y2, te.p0, te.p1, scale, keep.t31, sc.K0, sc.K2, sc.K4, sc.K5);
        }
        const unsigned long long word = __ballot(in);
        if (a.mask && lane == 0) a.mask[w] = word;
    }
    tested = wave_sum_i(tested);
    joint = wave_sum_i(joint);
    if (lane == 0) { s_cnt[wave][0] = tested; s_cnt[wave][1] = joint; }
    __syncthreads();
    if (tid != 0) return;
    tested = joint = 0;
#pragma unroll
    for (int w = 0; w < SF_WAVES; w++) { tested += s_cnt[w][0]; joint += s_cnt[w][1]; }
    hcTrifocalSelection o = keep;
    o.scale31 = scale;
    a.out[sel] = o;
    rep->status = !have ? HC_SCALE_NONE : (fitted ? 0 : HC_SCALE_NO_VOTER);
    rep->num_voters = have ? num_voters : 0;
    rep->voter = voter;
    rep->transfer_inliers = fitted ? (int)(key >> 32) : 0;
    rep->tested = tested;
    rep->joint = joint;
    rep->scale_in = keep.scale31;
    rep->scale31 = scale;
    rep->key = fitted ? key : 0;
}

// HC_SCALE_SELECT_BY_TRANSFER: k_pose_topk_select with the transfer key first.
// One thread per group: among the fitted selections with a path the largest
// transfer_inliers << 32 | path, among equal keys the larger joint key; "none"
// with rank -1 as k_pose_topk_select writes it.
__global__ void __launch_bounds__(64) k_pose_topk_select_transfer(int num_groups, int k,
                                                                  const hcTrifocalSelection *__restrict__ refined,
                                                                  const hcScaleReport *__restrict__ reports,
                                                                  hcTrifocalSelection *__restrict__ best,
                                                                  int32_t *__restrict__ best_rank) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= num_groups) return;
    const hcTrifocalSelection *in = refined + (size_t)t * k;
    const hcScaleReport *rp = reports + (size_t)t * k;
    int rank = -1;
    uint64_t tkey = 0, jkey = 0;
    for (int r = 0; r < k; r++) {
        if (in[r].path < 0) continue;
        const uint64_t tk = ((uint64_t)(uint32_t)rp[r].transfer_inliers << 32) | (uint32_t)in[r].path;
        if (rank < 0 || tk > tkey || (tk == tkey && in[r].key > jkey)) { rank = r; tkey = tk; jkey = in[r].key; }
    }
    hcTrifocalSelection o;
    if (rank >= 0) {
        o = in[rank];
    } else {
        o.num_candidates = in[0].num_candidates;
        o.path = o.inliers = o.inliers21 = o.inliers31 = -1;
        o.pad = 0;
        o.key = 0;
        for (int i = 0; i < 9; i++) o.R21[i] = o.R31[i] = 0.0f;
        for (int i = 0; i < 3; i++) o.t21[i] = o.t31[i] = 0.0f;
        o.scale31 = o.pad2 = 0.0f;
    }
    best[t] = o;
    best_rank[t] = rank;
}

// What a refine call's settings ask of the scale mode (off: the call as it was).
struct ScaleMode {
    bool on = false;
    int bits = 0;
    hcScaleReport *reports = nullptr;
    uint64_t *mask = nullptr;
};

// settings (a host pointer or nullptr) -> the mode; false when the mode is
// selected and its fields are not valid for this call
inline bool scale_mode(const hcRefineSettings *s, bool topk, bool mask_allowed, ScaleMode &m) {
    if (!s || s->pad[0] != HC_REFINE_SCALE31) return true;
    const hcRefineScaleSettings *ss = reinterpret_cast<const hcRefineScaleSettings *>(s);
    m.on = true;
    m.bits = s->pad[1];
    m.reports = ss->reports;
    m.mask = ss->transfer_mask;
    const int allowed = HC_SCALE_ONLY | (topk ? HC_SCALE_SELECT_BY_TRANSFER : 0);
    if (!m.reports || (m.bits & ~allowed) != 0) return false;
    if ((m.bits & HC_SCALE_ONLY) != 0 && s->iterations != 0) return false;
    if (m.mask && !mask_allowed) return false;
    return true;
}

// zeroed reports (the vote's atomics' targets), the vote, the epilogue
template <bool GROUPED>
hcStatus launch_scale_fit(const ScaleArgs &a, int num_selections, hcStream stream) {
    hipStream_t s = (hipStream_t)stream;
    const hcStatus zs = zero_selections(a.rep, (size_t)num_selections, s);
    if (zs != HC_SUCCESS) return zs;
    int tiles = GROUPED ? SV_TILES : (a.E + WAVE - 1) / WAVE;
    if (tiles > 65535) tiles = 65535;   // grid.y's limit: the workgroups stride over the rest
    hipLaunchKernelGGL(k_scale_vote<GROUPED>, dim3(num_selections, tiles), dim3(SV_THREADS), 0, s, a);
    if ((g_last_hip_error = hipGetLastError()) != hipSuccess) return HC_ERROR_LAUNCH;
    hipLaunchKernelGGL(k_scale_final<GROUPED>, dim3(num_selections), dim3(SF_THREADS), 0, s, a);
    if ((g_last_hip_error = hipGetLastError()) != hipSuccess) return HC_ERROR_LAUNCH;
    return HC_SUCCESS;
}

// A refine call (per_group = 1) or a refine-and-select call (best != nullptr)
// with its scale mode: the refinement unless HC_SCALE_ONLY, the fit of every
// selection when the mode is on, then the selection among a group's k.
template <bool GROUPED>
hcStatus launch_refine_scaled(const RefineArgs &a, const ScaleMode &m, int num_groups, hcTrifocalSelection *best,
                              int32_t *best_rank, hcStream stream) {
    const int n = num_groups * a.per_group;
    const bool only = m.on && (m.bits & HC_SCALE_ONLY) != 0;
    if (!only) {
        const hcStatus st = launch_pose_refine<GROUPED>(a, n, stream);
        if (st != HC_SUCCESS) return st;
    } else {
        (void)hipGetLastError();
    }
    if (m.on) {
        const ScaleArgs sa{only ? a.in : a.out, a.out, m.reports, reinterpret_cast<unsigned long long *>(m.mask),
                           a.E, a.loc, a.K, a.groups, a.per_group};
        const hcStatus st = launch_scale_fit<GROUPED>(sa, n, stream);
        if (st != HC_SUCCESS) return st;
    }
    if (!best) return HC_SUCCESS;
    if (m.on && (m.bits & HC_SCALE_SELECT_BY_TRANSFER) != 0)
        hipLaunchKernelGGL(k_pose_topk_select_transfer, dim3((num_groups + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                           num_groups, a.per_group, a.out, m.reports, best, best_rank);
    else
        hipLaunchKernelGGL(k_pose_topk_select, dim3((num_groups + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                           num_groups, a.per_group, a.out, best, best_rank);
    if ((g_last_hip_error = hipGetLastError()) != hipSuccess) return HC_ERROR_LAUNCH;
    return HC_SUCCESS;
}

// ---- the three-view refinement (include/threeview/hc_pose_threeview.h) --------
//
// The third stage of a refine call: after k_pose_refine and the scale fit,
// k_pose_refine3<GROUPED> refines both views and the scale jointly, in place on
// the selections the fit has written.  One workgroup of 256 threads per
// selection, the whole Gauss-Newton loop in one launch, laid out as
// k_pose_refine: an iterate is one pass over the edgels, thread i takes edgels
// i, i + 256, ...; it counts each with edgel_views, transfer_edgel and
// transfer_inlier on the state rounded to float (the functions the vote and the
// masks use) and, for an edgel of the fit set, adds the four residual rows and
// their derivatives along the eleven local directions, in double at the double
// state, to its 79 sums (66 of A, 11 of g, the squared error of each row pair).
// The sums go through a butterfly over the wave's lanes, then through LDS over
// the four waves as (w0 + w1) + (w2 + w3).  Wave 0 solves the 11 x 11 system, a
// row per lane (refine3_solve), and lanes 0, 1 and 2 write view 2's, view 3's
// and the scale's new state to LDS.  Nothing waits on another
// workgroup.  After the loop the four waves write the transfer mask of the best
// iterate, one ballot per word.
constexpr int R3_THREADS = 256, R3_WAVES = R3_THREADS / WAVE;
constexpr int R3_N = 11, R3_A = R3_N * (R3_N + 1) / 2;
constexpr int R3_SUMS = R3_A + R3_N + 2;   // A | g | sum r'r of the view-2 rows, of the transfer rows

struct Refine3Args {
    hcTrifocalSelection *sels;      // stage 2's out, refined in place
    const hcScaleReport *scale;     // stage 2's reports: a status other than 0 skips the stage
    hcThreeViewReport *rep;
    unsigned long long *mask;       // or nullptr; the single call only
    int E;                          // the scene, or with GROUPED that of groups[blockIdx.x / per_group]
    const float *loc;
    const float *K;
    const hcTripletGroup *groups;
    int iterations, min_inliers;
    int per_group;
};

// One edgel of the fit set: rows 0, 1 are view_accumulate's residual and its
// derivatives along view 2's five directions; rows 2, 3 the pixel error of
// Z = R31 (rho gamma1) + s t31 against (q0, q1), along all eleven: view 2's
// through rho alone (dZ = R31 gamma1 drho), w3 = e_i (dZ = e_i x Y), u3 (dZ =
// s b), sigma (dZ = s t31).
__device__ __forceinline__ void threeview_accumulate(double g0, double g1, double h0, double h1, double q0, double q1,
                                                     const double *R, const double *t, const double *b,
                                                     const double *R3, const double *t3, const double *b3, double s,
                                                     double K0, double K2, double K4, double K5, double *acc) {
    const double c[3] = {R[2], R[5], R[8]};
    const double a = (c[0] * h0 + c[1] * h1) + c[2];
    const double ct = (c[0] * t[0] + c[1] * t[1]) + c[2] * t[2];
    const double m[3] = {(R[0] * g0 + R[1] * g1) + R[2], (R[3] * g0 + R[4] * g1) + R[5], (R[6] * g0 + R[7] * g1) + R[8]};
    const double den = 1.0 - m[2] * a;
    const double rho = (t[2] * a - ct) / den;
    const double q[3] = {m[0] * rho + t[0], m[1] * rho + t[1], m[2] * rho + t[2]};
    const double x = q[0] / q[2], y = q[1] / q[2];
    const double r0 = (x * K0 + K2) - (h0 * K0 + K2), r1 = (y * K4 + K5) - (h1 * K4 + K5);
    const double iden = 1.0 / den, iq2 = 1.0 / q[2];
    const double M3[3] = {(R3[0] * g0 + R3[1] * g1) + R3[2], (R3[3] * g0 + R3[4] * g1) + R3[5],
                          (R3[6] * g0 + R3[7] * g1) + R3[8]};
    const double Y[3] = {M3[0] * rho, M3[1] * rho, M3[2] * rho};
    const double Z[3] = {Y[0] + s * t3[0], Y[1] + s * t3[1], Y[2] + s * t3[2]};
    const double iz = 1.0 / Z[2];
    const double xz = Z[0] * iz, yz = Z[1] * iz;
    const double r2 = ((Z[0] / Z[2]) * K0 + K2) - (q0 * K0 + K2), r3 = ((Z[1] / Z[2]) * K4 + K5) - (q1 * K4 + K5);
    double J0[5], J1[5], T0[R3_N], T1[R3_N];
#pragma unroll
    for (int d = 0; d < 5; d++) {
        double dc[3] = {0.0, 0.0, 0.0}, dm[3] = {0.0, 0.0, 0.0}, dt[3] = {0.0, 0.0, 0.0};
        if (d == 0) { dc[1] = -c[2]; dc[2] = c[1]; dm[1] = -m[2]; dm[2] = m[1]; }
        else if (d == 1) { dc[0] = c[2]; dc[2] = -c[0]; dm[0] = m[2]; dm[2] = -m[0]; }
        else if (d == 2) { dc[0] = -c[1]; dc[1] = c[0]; dm[0] = -m[1]; dm[1] = m[0]; }
        else { dt[0] = b[3 * (d - 3)]; dt[1] = b[3 * (d - 3) + 1]; dt[2] = b[3 * (d - 3) + 2]; }
        const double da = (dc[0] * h0 + dc[1] * h1) + dc[2];
        const double dct = ((dc[0] * t[0] + dc[1] * t[1]) + dc[2] * t[2]) + ((c[0] * dt[0] + c[1] * dt[1]) + c[2] * dt[2]);
        const double dnum = (dt[2] * a + t[2] * da) - dct;
        const double dden = -(dm[2] * a + m[2] * da);
        const double drho = (dnum - rho * dden) * iden;
        const double dq0 = (dm[0] * rho + m[0] * drho) + dt[0];
        const double dq1 = (dm[1] * rho + m[1] * drho) + dt[1];
        const double dq2 = (dm[2] * rho + m[2] * drho) + dt[2];
        J0[d] = K0 * ((dq0 - x * dq2) * iq2);
        J1[d] = K4 * ((dq1 - y * dq2) * iq2);
        T0[d] = K0 * (((M3[0] - xz * M3[2]) * drho) * iz);
        T1[d] = K4 * (((M3[1] - yz * M3[2]) * drho) * iz);
    }
#pragma unroll
    for (int d = 5; d < R3_N; d++) {
        double dZ[3];
        if (d == 5) { dZ[0] = 0.0; dZ[1] = -Y[2]; dZ[2] = Y[1]; }
        else if (d == 6) { dZ[0] = Y[2]; dZ[1] = 0.0; dZ[2] = -Y[0]; }
        else if (d == 7) { dZ[0] = -Y[1]; dZ[1] = Y[0]; dZ[2] = 0.0; }
        else if (d < 10) { dZ[0] = s * b3[3 * (d - 8)]; dZ[1] = s * b3[3 * (d - 8) + 1]; dZ[2] = s * b3[3 * (d - 8) + 2]; }
        else { dZ[0] = s * t3[0]; dZ[1] = s * t3[1]; dZ[2] = s * t3[2]; }
        T0[d] = K0 * ((dZ[0] - xz * dZ[2]) * iz);
        T1[d] = K4 * ((dZ[1] - yz * dZ[2]) * iz);
    }
    int n = 0;
#pragma unroll
    for (int i = 0; i < R3_N; i++)
#pragma unroll
        for (int j = i; j < R3_N; j++) {
            double v = T0[i] * T0[j] + T1[i] * T1[j];
            if (j < 5) v += J0[i] * J0[j] + J1[i] * J1[j];
            acc[n++] += v;
        }
#pragma unroll
    for (int i = 0; i < R3_N; i++) {
        double v = T0[i] * r2 + T1[i] * r3;
        if (i < 5) v += J0[i] * r0 + J1[i] * r1;
        acc[R3_A + i] += v;
    }
    acc[R3_A + R3_N] += r0 * r0 + r1 * r1;
    acc[R3_A + R3_N + 1] += r2 * r2 + r3 * r3;
}

// Entry (i, j), i <= j, of the packed upper triangle (row by row).
__host__ __device__ constexpr int r3_at(int i, int j) { return i * R3_N - i * (i - 1) / 2 + (j - i); }

// refine_solve at size 11, by the 64 lanes of one wave: (A + 1e-9 diag A) d = -g
// by Cholesky, the operations of refine_solve in its order.  Lane i < 11 owns
// row i of A and of the factor L (the lanes above repeat row 10, unused); what a
// step needs of another row comes by a shuffle from a fixed lane: the pivot of
// column j and L[j][0..j-1] from lane j.  The substitutions run in every lane on
// broadcast entries, so d comes out the same in all of them.  tot(n) is total n
// of the workgroup's sums.  False when a pivot is not positive or a value is not
// finite; the same in every lane.
template <typename Tot>
__device__ __forceinline__ bool refine3_solve(Tot tot, int lane, double *d) {
    const int row = lane < R3_N ? lane : R3_N - 1;
    double M[R3_N], L[R3_N], g[R3_N], y[R3_N];
    bool fin = true;
#pragma unroll
    for (int j = 0; j < R3_N; j++) {
        M[j] = tot(row <= j ? row * R3_N - row * (row - 1) / 2 + (j - row) : j * R3_N - j * (j - 1) / 2 + (row - j));
        if (j == row) M[j] = M[j] + 1e-9 * M[j];
        g[j] = tot(R3_A + j);
        fin = fin && __builtin_isfinite(M[j]) && __builtin_isfinite(g[j]);
        L[j] = 0.0;
    }
    bool ok = __ballot(!fin) == 0;
#pragma unroll
    for (int j = 0; j < R3_N; j++) {
        double v = M[j];
#pragma unroll
        for (int k = 0; k < j; k++) v -= L[k] * __shfl(L[k], j);   // lane j: M[j][j] - sum L[j][k]^2
        const double p = __shfl(v, j);
        ok = ok && p > 0.0;
        const double ljj = __builtin_sqrt(p);
        L[j] = row == j ? ljj : v / ljj;   // rows above j hold no entry of this column: never read
    }
#pragma unroll
    for (int i = 0; i < R3_N; i++) {
        double v = -g[i];
#pragma unroll
        for (int k = 0; k < i; k++) v -= __shfl(L[k], i) * y[k];
        y[i] = v / __shfl(L[i], i);
    }
#pragma unroll
    for (int i = R3_N - 1; i >= 0; i--) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < R3_N; k++) v -= __shfl(L[i], k) * d[k];
        d[i] = v / __shfl(L[i], i);
        ok = ok && __builtin_isfinite(d[i]);
    }
    return ok;
}

template <bool GROUPED>
__global__ void __launch_bounds__(R3_THREADS) k_pose_refine3(const Refine3Args a) {
    __shared__ double s_sum[R3_WAVES][R3_SUMS];
    __shared__ double s_state[2][12];   // per view R | t, the double state
    __shared__ double s_scale;          // s
    __shared__ float s_best[25];        // the best iterate's scored floats: R21 | t21 | R31 | t31 | s
    __shared__ int s_cnt[R3_WAVES][5];
    __shared__ int s_singular;
    const int tid = threadIdx.x, lane = lane_id(), wave = tid / WAVE, sel = blockIdx.x;
    Scene sc;
    if constexpr (GROUPED) {
        const hcTripletGroup g = a.groups[sel / a.per_group];
        sc = load_scene(g.num_edgels, g.locations, g.K);
    } else {
        sc = load_scene(a.E, a.loc, a.K);
    }
    const int words = (sc.E + WAVE - 1) / WAVE;
    // every thread reads the selection here, before the first barrier; thread 0
    // writes it after the last one
    const hcTrifocalSelection keep = a.sels[sel];
    hcThreeViewReport *rep = a.rep + sel;
    if (keep.path < 0 || a.scale[sel].status != 0) {   // stage 2 fitted nothing: its output stands
        if (a.mask)
            for (int w = tid; w < words; w += R3_THREADS) a.mask[w] = 0ull;
        if (tid == 0) {
            rep->status = HC_THREEVIEW_SKIPPED | (keep.path < 0 ? HC_THREEVIEW_NONE : 0);
            rep->iterations_run = rep->best_iteration = 0;
            for (int i = 0; i <= HC_REFINE_MAX_ITERATIONS; i++) rep->transfer_history[i] = rep->joint_history[i] = -1;
            rep->fit_set = rep->transfer_inliers = 0;
            rep->scale_in = rep->scale_out = keep.scale31;
            rep->pad = 0;
            rep->rms_px_in[0] = rep->rms_px_in[1] = rep->rms_px_out[0] = rep->rms_px_out[1] = 0.0;
        }
        return;
    }
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 9; i++) { s_state[0][i] = (double)keep.R21[i]; s_state[1][i] = (double)keep.R31[i]; }
#pragma unroll
        for (int i = 0; i < 3; i++) { s_state[0][9 + i] = (double)keep.t21[i]; s_state[1][9 + i] = (double)keep.t31[i]; }
        s_scale = (double)keep.scale31;
    }
    __syncthreads();
    const double K0 = (double)sc.K0, K2 = (double)sc.K2, K4 = (double)sc.K4, K5 = (double)sc.K5;
    int status = 0, k = 0, bestT = -1, bestF = 0, bestJ = 0, best21 = 0, best31 = 0, bestK = 0;
    double rms_in[2] = {0.0, 0.0}, rms_out[2] = {0.0, 0.0};
    for (;;) {
        double R[18], T[6], B[12];
        float Rf[18], Tf[6];
#pragma unroll
        for (int i = 0; i < 9; i++) { R[i] = s_state[0][i]; R[9 + i] = s_state[1][i]; }
#pragma unroll
        for (int i = 0; i < 3; i++) { T[i] = s_state[0][9 + i]; T[3 + i] = s_state[1][9 + i]; }
        const double s = s_scale;
        const float sf = (float)s;
#pragma unroll
        for (int i = 0; i < 18; i++) Rf[i] = (float)R[i];
#pragma unroll
        for (int i = 0; i < 6; i++) Tf[i] = (float)T[i];
        tangent_basis(T, B);
        tangent_basis(T + 3, B + 6);
        double acc[R3_SUMS];
#pragma unroll
        for (int i = 0; i < R3_SUMS; i++) acc[i] = 0.0;
        int c21 = 0, c31 = 0, cJ = 0, cF = 0, cT = 0;
        for (int e = tid; e < sc.E; e += R3_THREADS) {
            bool in21, in31;
            edgel_views(sc, e, Rf, Tf, Rf + 9, Tf + 3, in21, in31);
            float se;
            const TransferEdgel te = transfer_edgel(sc, e, Rf, Tf, Rf + 9, Tf + 3, se);
            const float Z2 = te.Y2 + sf * Tf[5];   // transfer_inlier's own Z2
            const bool inF = te.tested && Z2 > 0.0f;
            const bool inT = inF && transfer_inlier(te.Y0, te.Y1, te.Y2, te.p0, te.p1, sf, Tf + 3, sc.K0, sc.K2, sc.K4, sc.K5);
            c21 += in21 ? 1 : 0;
            c31 += in31 ? 1 : 0;
            cJ += te.joint ? 1 : 0;
            cF += inF ? 1 : 0;
            cT += inT ? 1 : 0;
            if (inF) {
                const float *p = sc.loc + (size_t)e * 6;
                threeview_accumulate((double)p[0], (double)p[1], (double)p[2], (double)p[3], (double)p[4], (double)p[5],
                                     R, T, B, R + 9, T + 3, B + 6, s, K0, K2, K4, K5, acc);
            }
        }
#pragma unroll
        for (int i = 0; i < R3_SUMS; i++) acc[i] = wave_sum_d(acc[i]);
        c21 = wave_sum_i(c21);
        c31 = wave_sum_i(c31);
        cJ = wave_sum_i(cJ);
        cF = wave_sum_i(cF);
        cT = wave_sum_i(cT);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < R3_SUMS; i++) s_sum[wave][i] = acc[i];
            s_cnt[wave][0] = cJ;
            s_cnt[wave][1] = c21;
            s_cnt[wave][2] = c31;
            s_cnt[wave][3] = cF;
            s_cnt[wave][4] = cT;
        }
        __syncthreads();
        // the totals, the same in every thread
        cJ = (s_cnt[0][0] + s_cnt[1][0]) + (s_cnt[2][0] + s_cnt[3][0]);
        c21 = (s_cnt[0][1] + s_cnt[1][1]) + (s_cnt[2][1] + s_cnt[3][1]);
        c31 = (s_cnt[0][2] + s_cnt[1][2]) + (s_cnt[2][2] + s_cnt[3][2]);
        cF = (s_cnt[0][3] + s_cnt[1][3]) + (s_cnt[2][3] + s_cnt[3][3]);
        cT = (s_cnt[0][4] + s_cnt[1][4]) + (s_cnt[2][4] + s_cnt[3][4]);
        double rms[2];
#pragma unroll
        for (int v = 0; v < 2; v++) {
            const int i = R3_A + R3_N + v;
            const double sse = (s_sum[0][i] + s_sum[1][i]) + (s_sum[2][i] + s_sum[3][i]);
            rms[v] = cF > 0 ? __builtin_sqrt(sse / (double)cF) : 0.0;
        }
        if (k == 0) { rms_in[0] = rms[0]; rms_in[1] = rms[1]; }
        if (tid == 0) { rep->transfer_history[k] = cT; rep->joint_history[k] = cJ; }
        if (cT >= bestT) {   // a tie goes to the later iterate
            bestT = cT; bestF = cF; bestJ = cJ; best21 = c21; best31 = c31; bestK = k;
            rms_out[0] = rms[0]; rms_out[1] = rms[1];
            if (tid == 0) {
#pragma unroll
                for (int i = 0; i < 9; i++) { s_best[i] = Rf[i]; s_best[12 + i] = Rf[9 + i]; }
#pragma unroll
                for (int i = 0; i < 3; i++) { s_best[9 + i] = Tf[i]; s_best[21 + i] = Tf[3 + i]; }
                s_best[24] = sf;
            }
        }
        if (cF < a.min_inliers) { status |= HC_THREEVIEW_TOO_FEW; break; }
        if (k == a.iterations) break;
        if (wave == 0) {   // the whole wave: the solve shuffles between its lanes
            double d[R3_N];
            const bool ok = refine3_solve(
                [&](int n) { return (s_sum[0][n] + s_sum[1][n]) + (s_sum[2][n] + s_sum[3][n]); }, lane, d);
            if (lane == 0) s_singular = ok ? 0 : 1;
            if (ok) {
                if (lane == 0) refine_apply(s_state[0], d);
                if (lane == 1) refine_apply(s_state[1], d + 5);
                if (lane == 2) s_scale = s * exp(d[10]);
            }
        }
        __syncthreads();
        if (s_singular) { status |= HC_THREEVIEW_SINGULAR; break; }
        k++;
    }
    __syncthreads();   // thread 0's last write of s_best
    if (a.mask) {
        float Rf[18], Tf[6];
#pragma unroll
        for (int i = 0; i < 9; i++) { Rf[i] = s_best[i]; Rf[9 + i] = s_best[12 + i]; }
#pragma unroll
        for (int i = 0; i < 3; i++) { Tf[i] = s_best[9 + i]; Tf[3 + i] = s_best[21 + i]; }
        const float sf = s_best[24];
        for (int w = wave; w < words; w += R3_WAVES) {
            const int e = w * WAVE + lane;
            bool in = false;
            if (e < sc.E) {
                float se;
                const TransferEdgel te = transfer_edgel(sc, e, Rf, Tf, Rf + 9, Tf + 3, se);
                in = te.tested && transfer_inlier(te.Y0, te.Y1, te.Y2, te.p0, te.p1, sf, Tf + 3, sc.K0, sc.K2, sc.K4, sc.K5);
            }
            const unsigned long long word = __ballot(in);
            if (lane == 0) a.mask[w] = word;
        }
    }
    if (tid != 0) return;
    if (bestK > 0) {   // otherwise the values it came in with, bit for bit
        hcTrifocalSelection o = keep;
        o.inliers = bestJ;
        o.inliers21 = best21;
        o.inliers31 = best31;
        o.key = ((uint64_t)(uint32_t)bestJ << 32) | (uint32_t)keep.path;
#pragma unroll
        for (int i = 0; i < 9; i++) { o.R21[i] = s_best[i]; o.R31[i] = s_best[12 + i]; }
#pragma unroll
        for (int i = 0; i < 3; i++) { o.t21[i] = s_best[9 + i]; o.t31[i] = s_best[21 + i]; }
        o.scale31 = s_best[24];
        a.sels[sel] = o;
    }
    rep->status = status;
    rep->iterations_run = k;
    rep->best_iteration = bestK;
    for (int i = k + 1; i <= HC_REFINE_MAX_ITERATIONS; i++) rep->transfer_history[i] = rep->joint_history[i] = -1;
    rep->fit_set = bestF;
    rep->transfer_inliers = bestT;
    rep->scale_in = keep.scale31;
    rep->scale_out = s_best[24];
    rep->pad = 0;
    rep->rms_px_in[0] = rms_in[0]; rep->rms_px_in[1] = rms_in[1];
    rep->rms_px_out[0] = rms_out[0]; rep->rms_px_out[1] = rms_out[1];
}

// HC_THREEVIEW_SELECT_BY_TRANSFER: k_pose_topk_select_transfer with the
// three-view reports' final transfer counts.
__global__ void __launch_bounds__(64) k_pose_topk_select_transfer3(int num_groups, int k,
                                                                   const hcTrifocalSelection *__restrict__ refined,
                                                                   const hcThreeViewReport *__restrict__ reports,
                                                                   hcTrifocalSelection *__restrict__ best,
                                                                   int32_t *__restrict__ best_rank) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= num_groups) return;
    const hcTrifocalSelection *in = refined + (size_t)t * k;
    const hcThreeViewReport *rp = reports + (size_t)t * k;
    int rank = -1;
    uint64_t tkey = 0, jkey = 0;
    for (int r = 0; r < k; r++) {
        if (in[r].path < 0) continue;
        const uint64_t tk = ((uint64_t)(uint32_t)rp[r].transfer_inliers << 32) | (uint32_t)in[r].path;
        if (rank < 0 || tk > tkey || (tk == tkey && in[r].key > jkey)) { rank = r; tkey = tk; jkey = in[r].key; }
    }
    hcTrifocalSelection o;
    if (rank >= 0) {
        o = in[rank];
    } else {
        o.num_candidates = in[0].num_candidates;
        o.path = o.inliers = o.inliers21 = o.inliers31 = -1;
        o.pad = 0;
        o.key = 0;
        for (int i = 0; i < 9; i++) o.R21[i] = o.R31[i] = 0.0f;
        for (int i = 0; i < 3; i++) o.t21[i] = o.t31[i] = 0.0f;
        o.scale31 = o.pad2 = 0.0f;
    }
    best[t] = o;
    best_rank[t] = rank;
}

// What a refine call's settings ask of the three-view mode (off: the call as it was).
struct ThreeViewMode {
    bool on = false;
    int bits = 0, iterations = 10;
    hcScaleReport *scale_reports = nullptr;
    hcThreeViewReport *reports = nullptr;
    uint64_t *mask = nullptr;
};

// The fields of a three-view settings block with the mode bits `bits` -> the
// mode; false when they are not valid for this call
inline bool threeview_fields(const hcRefineThreeViewSettings *ts, int bits, bool topk, bool mask_allowed,
                             ThreeViewMode &m) {
    m.on = true;
    m.bits = bits;
    m.scale_reports = ts->scale_reports;
    m.reports = ts->reports;
    m.mask = ts->transfer_mask;
    if (!m.scale_reports || !m.reports || (m.bits & ~(topk ? HC_THREEVIEW_SELECT_BY_TRANSFER : 0)) != 0) return false;
    if (ts->iterations3 < 0 || ts->iterations3 > HC_REFINE_MAX_ITERATIONS || ts->pad != 0) return false;
    if (m.mask && !mask_allowed) return false;
    if (ts->iterations3 > 0) m.iterations = ts->iterations3;
    return true;
}

// settings (a host pointer or nullptr) -> the mode; false when the mode is
// selected and its fields are not valid for this call
inline bool threeview_mode(const hcRefineSettings *s, bool topk, bool mask_allowed, ThreeViewMode &m) {
    if (!s || s->pad[0] != HC_REFINE_THREEVIEW) return true;
    return threeview_fields(reinterpret_cast<const hcRefineThreeViewSettings *>(s), s->pad[1], topk, mask_allowed, m);
}

// ---- the structure stage (include/structure/hc_pose_structure.h) ---------------
#include "hc_structure.hpp"

// A refine or refine-and-select call with its modes.  Three-view: the
// refinement, the scale fit of every selection (reports as in the scale mode, no
// mask), the three-view stage in place on out, then the selection among a
// group's k.  Structure: the same (its settings embed the three-view mode's),
// then the structure stage on out, or on best after the selection; with
// HC_STRUCTURE_ONLY that stage alone, on in.
template <bool GROUPED>
hcStatus launch_refine_modes(const RefineArgs &a, const ScaleMode &m, const ThreeViewMode &tv, const StructureMode &sm,
                             int num_groups, hcTrifocalSelection *best, int32_t *best_rank, hcStream stream) {
    if (sm.only) {
        (void)hipGetLastError();
        return launch_structure<GROUPED>(a, sm, a.in, a.out != a.in ? a.out : nullptr, nullptr, nullptr, num_groups,
                                         stream);
    }
    if (!tv.on) return launch_refine_scaled<GROUPED>(a, m, num_groups, best, best_rank, stream);
    ScaleMode fit;
    fit.on = true;
    fit.reports = tv.scale_reports;
    const hcStatus st = launch_refine_scaled<GROUPED>(a, fit, num_groups, nullptr, nullptr, stream);
    if (st != HC_SUCCESS) return st;
    const int n = num_groups * a.per_group;
    const Refine3Args ra{a.out, tv.scale_reports, tv.reports, reinterpret_cast<unsigned long long *>(tv.mask),
                         a.E, a.loc, a.K, a.groups, tv.iterations, a.min_inliers, a.per_group};
    hipLaunchKernelGGL(k_pose_refine3<GROUPED>, dim3(n), dim3(R3_THREADS), 0, (hipStream_t)stream, ra);
    if ((g_last_hip_error = hipGetLastError()) != hipSuccess) return HC_ERROR_LAUNCH;
    if (best) {
        if ((tv.bits & HC_THREEVIEW_SELECT_BY_TRANSFER) != 0)
            hipLaunchKernelGGL(k_pose_topk_select_transfer3, dim3((num_groups + 63) / 64), dim3(64), 0,
                               (hipStream_t)stream, num_groups, a.per_group, a.out, tv.reports, best, best_rank);
        else
            hipLaunchKernelGGL(k_pose_topk_select, dim3((num_groups + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                               num_groups, a.per_group, a.out, best, best_rank);
        if ((g_last_hip_error = hipGetLastError()) != hipSuccess) return HC_ERROR_LAUNCH;
    }
    if (!sm.on) return HC_SUCCESS;
    return launch_structure<GROUPED>(a, sm, best ? best : a.out, nullptr, tv.scale_reports, best ? best_rank : nullptr,
                                     num_groups, stream);
}

}  // namespace

}  // namespace hc

extern "C" hcStatus hc_trifocal_pose_support(int num_paths, const hcComplex *tracks, const uint8_t *converge,
                                             int num_edgels, const float *locations, const float *K, int flags,
                                             int32_t *inliers, hcPoseSelection *selection, hcStream stream) {
    return hc::pose_support_single<false>(num_paths, tracks, converge, num_edgels, locations, K, flags, inliers,
                                          selection, stream);
}

extern "C" hcStatus hc_trifocal_pose_support_joint(int num_paths, const hcComplex *tracks, const uint8_t *converge,
                                                   int num_edgels, const float *locations, const float *K, int flags,
                                                   int32_t *inliers, hcTrifocalSelection *selection,
                                                   hcStream stream) {
    return hc::pose_support_single<true>(num_paths, tracks, converge, num_edgels, locations, K, flags, inliers,
                                         selection, stream);
}

extern "C" hcStatus hc_trifocal_pose_support_grouped(int num_paths, const hcComplex *tracks, const uint8_t *converge,
                                                     int num_groups, const hcTripletGroup *groups,
                                                     const int32_t *sample_group, int flags, int32_t *inliers,
                                                     hcPoseSelection *selections, hcStream stream) {
    return hc::pose_support_grouped<false>(num_paths, tracks, converge, num_groups, groups, sample_group, flags,
                                           inliers, selections, stream);
}

extern "C" hcStatus hc_trifocal_pose_support_joint_grouped(int num_paths, const hcComplex *tracks,
                                                           const uint8_t *converge, int num_groups,
                                                           const hcTripletGroup *groups, const int32_t *sample_group,
                                                           int flags, int32_t *inliers,
                                                           hcTrifocalSelection *selections, hcStream stream) {
    return hc::pose_support_grouped<true>(num_paths, tracks, converge, num_groups, groups, sample_group, flags,
                                          inliers, selections, stream);
}

extern "C" hcStatus hc_trifocal_pose_inlier_mask(const hcTrifocalSelection *selection, int num_edgels,
                                                 const float *locations, const float *K, uint64_t *mask,
                                                 hcStream stream) {
    using namespace hc;
    if (!selection || num_edgels < 0) return HC_ERROR_INVALID_VALUE;
    if (num_edgels > 0 && (!locations || !K || !mask)) return HC_ERROR_INVALID_VALUE;
    if (num_edgels == 0) return HC_SUCCESS;   // no word to write
    const int words = (int)(((long long)num_edgels + WAVE - 1) / WAVE);
    int blocks = 0;
    const hcStatus st = path_grid(words, blocks);
    if (st != HC_SUCCESS) return st;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_pose_inlier_mask, dim3(blocks), dim3(256), 0, (hipStream_t)stream, selection, num_edgels,
                       locations, K, words, reinterpret_cast<unsigned long long *>(mask));
    if ((g_last_hip_error = hipGetLastError()) != hipSuccess) return HC_ERROR_LAUNCH;
    return HC_SUCCESS;
}

extern "C" hcStatus hc_trifocal_pose_refine(const hcTrifocalSelection *in, int num_edgels, const float *locations,
                                            const float *K, const hcRefineSettings *settings,
                                            hcTrifocalSelection *out, hcRefineReport *report, hcStream stream) {
    using namespace hc;
    int iterations, min_inliers;
    ScaleMode m;
    ThreeViewMode tv;
    StructureMode sm;
    if (!in || num_edgels <= 0 || !locations || !K || !out || !refine_settings(settings, iterations, min_inliers) ||
        !scale_mode(settings, false, true, m) || !threeview_mode(settings, false, true, tv) ||
        !structure_mode(settings, false, false, sm, tv))
        return HC_ERROR_INVALID_VALUE;
    const RefineArgs a{in, out, report, num_edgels, locations, K, nullptr, iterations, min_inliers, 1};
    return launch_refine_modes<false>(a, m, tv, sm, 1, nullptr, nullptr, stream);
}

extern "C" hcStatus hc_trifocal_pose_refine_grouped(int num_groups, const hcTripletGroup *groups,
                                                    const hcTrifocalSelection *in, const hcRefineSettings *settings,
                                                    hcTrifocalSelection *out, hcRefineReport *reports,
                                                    hcStream stream) {
    using namespace hc;
    int iterations, min_inliers;
    ScaleMode m;
    ThreeViewMode tv;
    StructureMode sm;
    if (num_groups <= 0 || !groups || !in || !out || !refine_settings(settings, iterations, min_inliers) ||
        !scale_mode(settings, false, false, m) || !threeview_mode(settings, false, false, tv) ||
        !structure_mode(settings, false, true, sm, tv))
        return HC_ERROR_INVALID_VALUE;
    const RefineArgs a{in, out, reports, 0, nullptr, nullptr, groups, iterations, min_inliers, 1};
    return launch_refine_modes<true>(a, m, tv, sm, num_groups, nullptr, nullptr, stream);
}

extern "C" hcStatus hc_trifocal_pose_topk_joint(int num_paths, const hcComplex *tracks, const int32_t *inliers, int k,
                                                hcTrifocalSelection *candidates, hcStream stream) {
    using namespace hc;
    if (k < 1 || k > HC_TOPK_MAX || num_paths < 0 || !candidates) return HC_ERROR_INVALID_VALUE;
    if (num_paths > 0 && (!tracks || !inliers)) return HC_ERROR_INVALID_VALUE;
    const TopkArgs a{num_paths, (const cf *)tracks, inliers, nullptr, k, candidates, 1};
    return launch_pose_topk<false>(a, stream);
}

extern "C" hcStatus hc_trifocal_pose_topk_joint_grouped(int num_paths, const hcComplex *tracks,
                                                        const int32_t *inliers, int num_groups,
                                                        const int32_t *sample_group, int k,
                                                        hcTrifocalSelection *candidates, hcStream stream) {
    using namespace hc;
    if (k < 1 || k > HC_TOPK_MAX || num_paths < 0 || num_paths % NTRK != 0 || num_groups < 1 || !candidates)
        return HC_ERROR_INVALID_VALUE;
    if (num_groups > 0x7FFFFFFF / HC_TOPK_MAX) return HC_ERROR_INVALID_VALUE;
    if (num_paths > 0 && (!tracks || !inliers || !sample_group)) return HC_ERROR_INVALID_VALUE;
    const TopkArgs a{num_paths, (const cf *)tracks, inliers, sample_group, k, candidates, num_groups};
    return launch_pose_topk<true>(a, stream);
}

extern "C" hcStatus hc_trifocal_pose_refine_topk(int k, const hcTrifocalSelection *candidates, int num_edgels,
                                                 const float *locations, const float *K,
                                                 const hcRefineSettings *settings, hcTrifocalSelection *refined,
                                                 hcRefineReport *reports, hcTrifocalSelection *best,
                                                 int32_t *best_rank, hcStream stream) {
    using namespace hc;
    int iterations, min_inliers;
    ScaleMode m;
    ThreeViewMode tv;
    StructureMode sm;
    if (k < 1 || k > HC_TOPK_MAX || !candidates || num_edgels <= 0 || !locations || !K || !refined || !best ||
        !best_rank || !refine_settings(settings, iterations, min_inliers) || !scale_mode(settings, true, false, m) ||
        !threeview_mode(settings, true, false, tv) || !structure_mode(settings, true, false, sm, tv))
        return HC_ERROR_INVALID_VALUE;
    const RefineArgs a{candidates, refined, reports, num_edgels, locations, K, nullptr, iterations, min_inliers, k};
    return launch_refine_modes<false>(a, m, tv, sm, 1, best, best_rank, stream);
}

extern "C" hcStatus hc_trifocal_pose_refine_topk_grouped(int num_groups, const hcTripletGroup *groups, int k,
                                                         const hcTrifocalSelection *candidates,
                                                         const hcRefineSettings *settings,
                                                         hcTrifocalSelection *refined, hcRefineReport *reports,
                                                         hcTrifocalSelection *best, int32_t *best_rank,
                                                         hcStream stream) {
    using namespace hc;
    int iterations, min_inliers;
    ScaleMode m;
    ThreeViewMode tv;
    StructureMode sm;
    if (num_groups < 1 || num_groups > 0x7FFFFFFF / HC_TOPK_MAX || !groups || k < 1 || k > HC_TOPK_MAX ||
        !candidates || !refined || !best || !best_rank || !refine_settings(settings, iterations, min_inliers) ||
        !scale_mode(settings, true, false, m) || !threeview_mode(settings, true, false, tv) ||
        !structure_mode(settings, true, true, sm, tv))
        return HC_ERROR_INVALID_VALUE;
    const RefineArgs a{candidates, refined, reports, 0, nullptr, nullptr, groups, iterations, min_inliers, k};
    return launch_refine_modes<true>(a, m, tv, sm, num_groups, best, best_rank, stream);
}
