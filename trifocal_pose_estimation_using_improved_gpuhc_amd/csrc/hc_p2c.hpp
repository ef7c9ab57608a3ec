// The plain kernels of the P2C mode (include/p2c/hc_trifocal_p2c.h): the table
// compaction for the P2C layout and the component evaluation.  The tracker is
// k_track_p2c (hc_track.hpp).  Both are templates (instantiated with `true`
// only) although neither needs a parameter: the device compiler emits plain
// kernels first and instantiations in the order the host code first names
// them, so these two come after every kernel that existed before them, which
// all keep their order in the code object (emitted as plain kernels they
// moved the tracker kernels by 68 KB, and that build's config-2 launch came
// out 0.01 ms outside the parent's spread: profiles/r14a_ab_p2c_plain_kernels.jsonl).
#pragma once

#include "hc_prep.hpp"

namespace hc {

// k_prep_tables for the P2C layout (hc_prep_body.inc with P2C on): pa.U is the
// dH/dx table, ht the dH/dt table.  The same workspace tables, with the prefix
// build jobs of build_prefix_rounds_p2c; the hash it keeps differs from that of
// any unified table, so a workspace that changes format rebuilds.
template <bool P2C>
__global__ void __launch_bounds__(PREP_THREADS) k_prep_tables_p2c(PrepArgs pa, const int32_t *ht) {
    static_assert(P2C, "the P2C layout's compaction");
    const int32_t *__restrict__ D_in = ht;
#include "hc_prep_body.inc"
}

// k_eval (hc_components.hpp) for the P2C mode: dH/dx, dH/dt, H at n points, one
// point per half-wave, each from its own coefficient blocks at its own t
template <bool P2C>
__global__ void __launch_bounds__(WG_THREADS) k_eval_p2c(int n, const Workspace *ws, const cf *__restrict__ X,
                                                         const cf *__restrict__ CHX, const cf *__restrict__ CHT,
                                                         const float *__restrict__ TT, cf *__restrict__ HX,
                                                         cf *__restrict__ HT, cf *__restrict__ H) {
    __shared__ uint32_t s_hx[HX_SLOT_CAP * 32];
    __shared__ uint2 s_ht[HT_TERMS * 32];
    __shared__ uint32_t s_hxd[HX_NSLOT / 2 * 32];
    __shared__ SlotLDS s_slot[2 * WAVES_PER_WG];
    static_assert(P2C, "the P2C evaluation");
    const EvalTables *T = &ws->tab;
    if (ws->status != 0u) return;
    for (int i = threadIdx.x; i < HX_SLOT_CAP * 32; i += WG_THREADS) s_hx[i] = T->hx[i];
    for (int i = threadIdx.x; i < HT_TERMS * 32; i += WG_THREADS) s_ht[i] = T->ht[i];
    for (int i = threadIdx.x; i < HX_NSLOT / 2 * 32; i += WG_THREADS) s_hxd[i] = (&T->hxd[0][0])[i];
    {
        float *z = reinterpret_cast<float *>(s_slot);
        for (int i = threadIdx.x; i < (int)(sizeof(s_slot) / 4); i += WG_THREADS) z[i] = 0.0f;
    }
    __syncthreads();
    const int lane = lane_id();
    const int r = lane & 31;
    const int sys = (blockIdx.x * WAVES_PER_WG + threadIdx.x / WAVE) * 2 + (lane >> 5);
    SlotLDS &S = s_slot[(threadIdx.x / WAVE) * 2 + (lane >> 5)];
    const bool ok = sys < n;
    if (ok && r < 31) S.x[r] = X[(size_t)sys * 31 + r];
    if (ok) p2c_stage(S, r, CHX + (size_t)sys * P2C_NK * 3, CHT + (size_t)sys * P2C_NK * 2, TT[sys]);
    __shared__ uint32_t s_gm[GM_WORDS][32];
    if (threadIdx.x < 32)
        for (int q = 0; q < GM_WORDS; q++) s_gm[q][threadIdx.x] = T->gm[q][threadIdx.x];
    __syncthreads();
    build_prefix_rounds_p2c(S, r, &T->pre[0][0]);
    cf rA[NV];
    eval_hx(rA, s_hx, s_hxd, &s_gm[0][0], S, r);
    const cf ht = eval_rhs<RHS_HT>(s_ht, S, r, true, rhs_masks(T));
    const cf h = eval_rhs<RHS_H>(s_ht, S, r, false, rhs_masks(T));
    if (ok && r < NV) {
#pragma unroll
        for (int c = 0; c < NV; c++) HX[((size_t)sys * NV + r) * NV + c] = rA[c];
        HT[(size_t)sys * NV + r] = ht;
        H[(size_t)sys * NV + r] = h;
    }
}

}  // namespace hc
