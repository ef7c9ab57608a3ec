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
#include <type_traits>

#include "../../include/hc_pose.h"
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

// decode the key of one joint selection: the selected path's counts, its pose
// for both views and |Re x[21..23]| / |Re x[18..20]| (the norms unit3 divides by)
__device__ __forceinline__ void decode_joint(int num_paths, const cf *__restrict__ tracks,
                                             const int32_t *__restrict__ inl, hcTrifocalSelection *sel) {
    int b = -1;
    if (sel->num_candidates > 0) b = (int)(uint32_t)sel->key;
    if (b >= num_paths) b = -1;
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
    if ((g_last_hip_error = hipMemsetAsync(a.sels, 0, sizeof(Selection<JOINT>) * (size_t)a.num_sel, s)) != hipSuccess)
        return HC_ERROR_LAUNCH;
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
