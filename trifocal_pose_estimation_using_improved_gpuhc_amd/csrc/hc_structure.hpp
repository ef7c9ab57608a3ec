// hc_structure.hpp -- the structure stage of a refine call
// (include/structure/hc_pose_structure.h): the 3D edgels, point and tangent,
// that the pose that goes out explains in all three views.
//
// Included by hc_pose.hip inside its namespace, below the three-view stage whose
// ThreeViewMode it embeds, and dispatched from launch_refine_modes.
//
// k_pose_structure<GROUPED>: one workgroup of 256 threads per selection, as
// k_pose_refine3.  It walks the scene in tiles of 256 edgels with a running
// base.  A thread decides its edgel with transfer_edgel and transfer_inlier --
// the functions the vote, the three-view stage and the masks use, so W cannot
// drift from them -- and its entry index is base + the inliers of the waves
// before it in the tile (their ballots' popcounts, through LDS) + the inliers of
// the lanes before it in its own ballot: entry order is edgel order by
// construction, without an atomic.  Every float of a record is one thread's
// arithmetic in the header's operation order.  One thread writes the report at
// the end.  Nothing is accumulated across launches.
#pragma once

constexpr int ST_THREADS = 256, ST_WAVES = ST_THREADS / WAVE;

struct StructureArgs {
    const hcTrifocalSelection *sels;   // one per group: out of the refine calls (HC_STRUCTURE_ONLY: in), best of the top-k calls
    hcTrifocalSelection *copy_to;      // HC_STRUCTURE_ONLY with out != in: out, else nullptr
    const hcScaleReport *scale;        // stage 2's reports, nullptr with HC_STRUCTURE_ONLY
    const int32_t *best_rank;          // the top-k calls: sels[t]'s report is scale[t * k + best_rank[t]]; else nullptr
    int k;
    int E;                             // the scene, or with GROUPED that of groups[blockIdx.x]
    const float *loc;
    const float *K;
    const hcTripletGroup *groups;
    const float *tangents;
    const int32_t *offsets;            // GROUPED: the first row of tangents and entry of out of every group
    hcEdgel3D *out;
    hcStructureReport *rep;
    float min_sin_plane, max_sin3;
};

// Steps 2 to 5 of the rule for an edgel of W.  te: transfer_edgel's result for
// it under the same floats; tan: its row of the tangents.
__device__ __forceinline__ hcEdgel3D structure_edgel(const Scene &sc, int e, const float *tan,
                                                     const hcTrifocalSelection &S, const TransferEdgel &te,
                                                     float min_sin_plane, float max_sin3) {
    const float2 g = *reinterpret_cast<const float2 *>(sc.loc + (size_t)e * 6);
    const float2 h = *reinterpret_cast<const float2 *>(sc.loc + (size_t)e * 6 + 2);
    const float2 ta = *reinterpret_cast<const float2 *>(tan);
    const float2 tb = *reinterpret_cast<const float2 *>(tan + 2);
    const float2 tc = *reinterpret_cast<const float2 *>(tan + 4);
    const float *R21 = S.R21, *R31 = S.R31, *t31 = S.t31;
    const float s = S.scale31;
    hcEdgel3D r;
    // the point: depth_rho forms the bits transfer_edgel triangulated with
    const float rho = depth_rho(g.x, g.y, h.x, h.y, R21, S.t21);
    r.X[0] = rho * g.x;
    r.X[1] = rho * g.y;
    r.X[2] = rho;
    // transfer_inlier's error, kept
    const float Z0 = te.Y0 + s * t31[0], Z1 = te.Y1 + s * t31[1], Z2 = te.Y2 + s * t31[2];
    float d0 = Z0 / Z2, d1 = Z1 / Z2;
    d0 = d0 * sc.K0 + sc.K2;
    d1 = d1 * sc.K4 + sc.K5;
    d0 -= te.p0;
    d1 -= te.p1;
    r.err3_px = __builtin_sqrtf((d0 * d0 + d1 * d1) + 0.0f * 0.0f);
    // the tangent planes of views 1 and 2, both in view 1's frame
    float n1[3] = {-ta.y, ta.x, g.x * ta.y - g.y * ta.x};
    const float m[3] = {-tb.y, tb.x, h.x * tb.y - h.y * tb.x};
    float n2[3];
#pragma unroll
    for (int i = 0; i < 3; i++) n2[i] = ((0.0f + R21[i] * m[0]) + R21[3 + i] * m[1]) + R21[6 + i] * m[2];
    const float l1 = __builtin_sqrtf((n1[0] * n1[0] + n1[1] * n1[1]) + n1[2] * n1[2]);
    const float l2 = __builtin_sqrtf((n2[0] * n2[0] + n2[1] * n2[1]) + n2[2] * n2[2]);
#pragma unroll
    for (int i = 0; i < 3; i++) { n1[i] /= l1; n2[i] /= l2; }
    const float D[3] = {n1[1] * n2[2] - n1[2] * n2[1], n1[2] * n2[0] - n1[0] * n2[2], n1[0] * n2[1] - n1[1] * n2[0]};
    const float sp = __builtin_sqrtf((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]);
    r.sin_plane = sp;
    r.edgel = e;
    r.pad = 0;
    if (!(__builtin_isfinite(sp) && sp >= min_sin_plane)) {
        r.T[0] = r.T[1] = r.T[2] = 0.0f;
        r.sin3 = 1.0f;
        r.flags = 0;
        return r;
    }
    float T[3] = {D[0] / sp, D[1] / sp, D[2] / sp};
    if ((T[0] - T[2] * g.x) * ta.x + (T[1] - T[2] * g.y) * ta.y < 0.0f) { T[0] = -T[0]; T[1] = -T[1]; T[2] = -T[2]; }
    r.T[0] = T[0];
    r.T[1] = T[1];
    r.T[2] = T[2];
    // its image in view 3 against the observed tangent
    float V[3];
#pragma unroll
    for (int i = 0; i < 3; i++) V[i] = ((0.0f + R31[3 * i] * T[0]) + R31[3 * i + 1] * T[1]) + R31[3 * i + 2] * T[2];
    const float p0 = (V[0] * Z2 - Z0 * V[2]) * sc.K0, p1 = (V[1] * Z2 - Z1 * V[2]) * sc.K4;
    const float o0 = tc.x * sc.K0, o1 = tc.y * sc.K4;
    r.sin3 = __builtin_fabsf(p0 * o1 - p1 * o0) /
             (__builtin_sqrtf(p0 * p0 + p1 * p1) * __builtin_sqrtf(o0 * o0 + o1 * o1));
    r.flags = HC_EDGEL3D_TANGENT | (r.sin3 < max_sin3 ? HC_EDGEL3D_ORIENTED : 0);
    return r;
}

template <bool GROUPED>
__global__ void __launch_bounds__(ST_THREADS) k_pose_structure(const StructureArgs a) {
    __shared__ int s_tile[2][ST_WAVES];   // the waves' inliers of a tile; two tiles in flight, one barrier each
    __shared__ int s_bits[ST_WAVES][2];   // the waves' tangent and oriented counts
    const int tid = threadIdx.x, lane = lane_id(), wave = tid / WAVE, sel = blockIdx.x;
    Scene sc;
    const float *tangents = a.tangents;
    hcEdgel3D *out = a.out;
    if constexpr (GROUPED) {
        const hcTripletGroup g = a.groups[sel];
        sc = load_scene(g.num_edgels, g.locations, g.K);
        const size_t first = (size_t)a.offsets[sel];
        tangents += first * 6;
        out += first;
    } else {
        sc = load_scene(a.E, a.loc, a.K);
    }
    // every thread reads the selection here; thread 0 copies it at the end
    // (copy_to is never the buffer it was read from)
    const hcTrifocalSelection keep = a.sels[sel];
    hcStructureReport *rep = a.rep + sel;
    bool none = keep.path < 0;
    if (a.scale && !none) {
        int r = sel;
        if (a.best_rank) {
            const int rank = a.best_rank[sel];
            r = rank < 0 ? -1 : sel * a.k + rank;
        }
        none = r < 0 || a.scale[r].status != 0;   // stage 2 fitted no scale
    }
    if (none) {   // the whole workgroup
        if (tid == 0) {
            if (a.copy_to) a.copy_to[sel] = keep;
            rep->status = HC_STRUCTURE_NONE;
            rep->count = rep->tangents = rep->oriented = 0;
            rep->scale31 = keep.scale31;
            rep->pad[0] = rep->pad[1] = rep->pad[2] = 0;
        }
        return;
    }
    int base = 0, n_tan = 0, n_ori = 0;
    for (int first = 0, it = 0; first < sc.E; first += ST_THREADS, it ^= 1) {
        const int e = first + tid;
        bool in = false;
        TransferEdgel te;
        if (e < sc.E) {
            float se;
            te = transfer_edgel(sc, e, keep.R21, keep.t21, keep.R31, keep.t31, se);
            in = te.tested &&
                 transfer_inlier(te.Y0, te.Y1, te.Y2, te.p0, te.p1, keep.scale31, keep.t31, sc.K0, sc.K2, sc.K4, sc.K5);
        }
        const unsigned long long word = __ballot(in);
        if (lane == 0) s_tile[it][wave] = __popcll(word);
        __syncthreads();   // the one barrier of a tile: the next tile writes the other half of s_tile
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < ST_WAVES; w++) {
            const int c = s_tile[it][w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (in) {
            const int j = base + before + __popcll(word & ((1ull << lane) - 1ull));   // < E: one entry per edgel at most
            const hcEdgel3D r = structure_edgel(sc, e, tangents + (size_t)e * 6, keep, te, a.min_sin_plane, a.max_sin3);
            out[j] = r;
            n_tan += (r.flags & HC_EDGEL3D_TANGENT) != 0 ? 1 : 0;
            n_ori += (r.flags & HC_EDGEL3D_ORIENTED) != 0 ? 1 : 0;
        }
        base += total;
    }
    n_tan = wave_sum_i(n_tan);
    n_ori = wave_sum_i(n_ori);
    if (lane == 0) { s_bits[wave][0] = n_tan; s_bits[wave][1] = n_ori; }
    __syncthreads();
    if (tid != 0) return;
    n_tan = n_ori = 0;
#pragma unroll
    for (int w = 0; w < ST_WAVES; w++) { n_tan += s_bits[w][0]; n_ori += s_bits[w][1]; }
    if (a.copy_to) a.copy_to[sel] = keep;
    rep->status = 0;
    rep->count = base;
    rep->tangents = n_tan;
    rep->oriented = n_ori;
    rep->scale31 = keep.scale31;
    rep->pad[0] = rep->pad[1] = rep->pad[2] = 0;
}

// What a refine call's settings ask of the structure mode (off: the call as it was).
struct StructureMode {
    bool on = false, only = false;
    const float *tangents = nullptr;
    const int32_t *offsets = nullptr;
    hcEdgel3D *edgels3d = nullptr;
    hcStructureReport *reports = nullptr;
    float min_sin_plane = 0.05f, max_sin3 = 0.05f;
};

inline bool structure_threshold(float v, float &out) {
    if (!(v >= 0.0f && v <= 1.0f)) return false;   // a NaN or an infinity fails here too
    if (v > 0.0f) out = v;
    return true;
}

// settings (a host pointer or nullptr) -> the mode and, unless
// HC_STRUCTURE_ONLY, the three-view mode of its embedded settings; false when
// the mode is selected and its fields are not valid for this call
inline bool structure_mode(const hcRefineSettings *s, bool topk, bool grouped, StructureMode &m, ThreeViewMode &tv) {
    if (!s || s->pad[0] != HC_REFINE_STRUCTURE) return true;
    const hcRefineStructureSettings *ss = reinterpret_cast<const hcRefineStructureSettings *>(s);
    const int bits = s->pad[1];
    m.on = true;
    m.only = (bits & HC_STRUCTURE_ONLY) != 0;
    m.tangents = ss->tangents;
    m.offsets = ss->edgel_offsets;
    m.edgels3d = ss->edgels3d;
    m.reports = ss->reports;
    if (!m.tangents || !m.edgels3d || !m.reports || (m.offsets != nullptr) != grouped) return false;
    if (!structure_threshold(ss->min_sin_plane, m.min_sin_plane) || !structure_threshold(ss->max_sin3, m.max_sin3))
        return false;
    if (m.only) {
        if (topk || bits != HC_STRUCTURE_ONLY || s->iterations != 0) return false;
        return !ss->tv.scale_reports && !ss->tv.reports && !ss->tv.transfer_mask && ss->tv.iterations3 == 0 &&
               ss->tv.pad == 0;
    }
    return threeview_fields(&ss->tv, bits, topk, !topk && !grouped, tv);
}

// The stage on the num_groups selections at sels, after whatever wrote them on
// the same stream.
template <bool GROUPED>
hcStatus launch_structure(const RefineArgs &a, const StructureMode &m, const hcTrifocalSelection *sels,
                          hcTrifocalSelection *copy_to, const hcScaleReport *scale, const int32_t *best_rank,
                          int num_groups, hcStream stream) {
    const StructureArgs sa{sels, copy_to, scale, best_rank, a.per_group, a.E, a.loc, a.K, a.groups, m.tangents,
                           m.offsets, m.edgels3d, m.reports, m.min_sin_plane, m.max_sin3};
    hipLaunchKernelGGL(k_pose_structure<GROUPED>, dim3(num_groups), dim3(ST_THREADS), 0, (hipStream_t)stream, sa);
    if ((g_last_hip_error = hipGetLastError()) != hipSuccess) return HC_ERROR_LAUNCH;
    return HC_SUCCESS;
}
