// The component kernels k_cgesv and k_eval.
#pragma once

#include "hc_layout.hpp"

namespace hc {

// The tracker's building blocks alone, from HBM operands (component ABI entry
// points; parity tests of dev-cgesv-batched-small.cuh and the index evals).

// LU: two systems per wave; a row's structural pattern is its non-zero entries
__global__ void __launch_bounds__(WG_THREADS) k_cgesv(int n, const cf *__restrict__ A, const cf *__restrict__ B,
                                                      cf *__restrict__ X) {
    __shared__ LUBuf s_lu[2 * WAVES_PER_WG];
    __shared__ __attribute__((aligned(16))) cf s_scr[2 * WAVES_PER_WG][LU_SCRATCH_CF];
    const int lane = lane_id();
    const int r = lane & 31;
    const int sys = (blockIdx.x * WAVES_PER_WG + threadIdx.x / WAVE) * 2 + (lane >> 5);
    const bool ok = sys < n && r < NV;
    cf rA[NV];
    uint32_t pat = 0;
#pragma unroll
    for (int c = 0; c < NV; c++) {
        rA[c] = ok ? A[((size_t)sys * NV + r) * NV + c] : cmk(0.0f, 0.0f);
        if (rA[c].x != 0.0f || rA[c].y != 0.0f) pat |= 1u << c;   // NaN counts as non-zero
    }
    const cf rB = ok ? B[(size_t)sys * NV + r] : cmk(0.0f, 0.0f);
    LUBuf &LB = s_lu[(threadIdx.x / WAVE) * 2 + (lane >> 5)];
    cf *scr = s_scr[(threadIdx.x / WAVE) * 2 + (lane >> 5)];
    bool redo;
    cf x = lu_solve<false>(rA, rB, lane, pat, LB, scr, redo, __ballot(sys < n));
    if (__builtin_expect(redo, 0)) {   // solved again densely from the original system
#pragma unroll
        for (int c = 0; c < NV; c++) rA[c] = ok ? A[((size_t)sys * NV + r) * NV + c] : cmk(0.0f, 0.0f);
        x = lu_solve<true>(rA, rB, lane, pat, LB, scr, redo);
    }
    if (ok) X[(size_t)sys * NV + r] = x;
}

// Any of the tracker's solves alone (include/lu/hc_lu_testing.h,
// hc_cgesv_30x30_variant_batched): lu_solve<false, LAT, STRUCT, ENTCHK, FUSE>
// with the template arguments one of the tracking kernels passes (lu_mode,
// hc_lu.hpp; the host side derives them from the kernel's parameters), and on `redo` the tracker's fallback: the system loaded
// again and solved densely.  STRUCT: the row patterns are LU_STRUCT_PAT, and
// every entry outside them must be zero: k_cgesv_struct_check sets *bad
// otherwise, and the host launches the solve only when it stays 0.  !STRUCT
// (the twins that track a table of another structure): a row's pattern is its
// non-zero entries, as in k_cgesv, and any matrix is accepted.  ENTCHK: the
// finiteness verdict is taken here, on the entries' sums of squares, as
// eval_hx_terms_abs takes it.  <0, true, true, true> is the throughput tracker's.
__global__ void __launch_bounds__(WG_THREADS) k_cgesv_struct_check(int n, const cf *__restrict__ A,
                                                                   unsigned *__restrict__ bad) {
    const size_t i = (size_t)blockIdx.x * WG_THREADS + threadIdx.x;   // one thread per row
    if (i >= (size_t)n * NV) return;
    const uint32_t pat = LU_STRUCT_PAT[i % NV];
    bool out = false;
    for (int c = 0; c < NV; c++) {
        const cf a = A[i * NV + c];
        // NaN counts as non-zero
        if (!((pat >> c) & 1u) && (a.x != 0.0f || a.y != 0.0f)) out = true;
    }
    if (out) *bad = 1u;
}
template <int LAT, bool STRUCT, bool ENTCHK, bool FUSE>
__global__ void __launch_bounds__(WG_THREADS) k_cgesv_variant(int n, const cf *__restrict__ A,
                                                              const cf *__restrict__ B, cf *__restrict__ X) {
    __shared__ LUBuf s_lu[2 * WAVES_PER_WG];
    __shared__ __attribute__((aligned(16))) cf s_scr[2 * WAVES_PER_WG][FUSE ? LU_SCRATCH_FUSED_CF : LU_SCRATCH_CF];
    const int lane = lane_id();
    const int r = lane & 31;
    const int sys = (blockIdx.x * WAVES_PER_WG + threadIdx.x / WAVE) * 2 + (lane >> 5);
    const bool ok = sys < n && r < NV;
    cf rA[NV];
    uint32_t nz = 0;
    pf2 sq = {0.0f, 0.0f};   // the entries' sums of squares, as eval_hx_terms_abs takes them
#pragma unroll
    for (int c = 0; c < NV; c++) {
        rA[c] = ok ? A[((size_t)sys * NV + r) * NV + c] : cmk(0.0f, 0.0f);
        if constexpr (!STRUCT) {
            if (rA[c].x != 0.0f || rA[c].y != 0.0f) nz |= 1u << c;   // NaN counts as non-zero
        }
        if constexpr (ENTCHK) {
            sq.x = __builtin_fmaf(rA[c].x, rA[c].x, sq.x);
            sq.y = __builtin_fmaf(rA[c].y, rA[c].y, sq.y);
        }
    }
    bool ent_bad = false;
    if constexpr (ENTCHK) ent_bad = __ballot(!(sq.x + sq.y < __builtin_inff())) != 0ull;
    const uint32_t pat = STRUCT ? (r < NV ? LU_STRUCT_PAT[r] : 0u) : nz;
    const cf rB = ok ? B[(size_t)sys * NV + r] : cmk(0.0f, 0.0f);
    LUBuf &LB = s_lu[(threadIdx.x / WAVE) * 2 + (lane >> 5)];
    cf *scr = s_scr[(threadIdx.x / WAVE) * 2 + (lane >> 5)];
    bool redo;
    cf x = lu_solve<false, LAT, STRUCT, ENTCHK, FUSE>(rA, rB, lane, pat, LB, scr, redo, __ballot(sys < n), ent_bad);
    if (__builtin_expect(redo, 0)) {
#pragma unroll
        for (int c = 0; c < NV; c++) rA[c] = ok ? A[((size_t)sys * NV + r) * NV + c] : cmk(0.0f, 0.0f);
        x = lu_solve<true>(rA, rB, lane, pat, LB, scr, redo);
    }
    if (ok) X[(size_t)sys * NV + r] = x;
}


// dH/dx, dH/dt, H at n points: one point per half-wave
__global__ void __launch_bounds__(WG_THREADS) k_eval(int n, const Workspace *ws, const cf *__restrict__ X,
                                                     const cf *__restrict__ P, const cf *__restrict__ D,
                                                     cf *__restrict__ HX, cf *__restrict__ HT, cf *__restrict__ H) {
    __shared__ uint32_t s_hx[HX_SLOT_CAP * 32];
    __shared__ uint2 s_ht[HT_TERMS * 32];
    __shared__ uint32_t s_hxd[HX_NSLOT / 2 * 32];
    __shared__ SlotLDS s_slot[2 * WAVES_PER_WG];
    const EvalTables *T = &ws->tab;
    if (ws->status != 0u) return;
    for (int i = threadIdx.x; i < HX_SLOT_CAP * 32; i += WG_THREADS) s_hx[i] = T->hx[i];   // padded table
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
    if (ok) {   // the point's p and d, staged for the prefix tables
        S.ent[r] = P[(size_t)sys * NPP + r];
        S.ent[NPP + r] = D[(size_t)sys * NPP + r];
        if (r < NPP - 32) {
            S.ent[r + 32] = P[(size_t)sys * NPP + r + 32];
            S.ent[NPP + r + 32] = D[(size_t)sys * NPP + r + 32];
        }
    }
    __shared__ uint32_t s_gm[GM_WORDS][32];
    if (threadIdx.x < 32)
        for (int q = 0; q < GM_WORDS; q++) s_gm[q][threadIdx.x] = T->gm[q][threadIdx.x];
    __syncthreads();
    build_prefix_rounds(S, r, &T->pre[0][0]);
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
