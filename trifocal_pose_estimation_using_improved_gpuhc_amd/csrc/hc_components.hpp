// The component kernels k_cgesv and k_eval, and the test hooks' k_cgesv_variant and k_eval_variant.
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
    if constexpr (FUSE) {   // the fused levels' row records (hc_lu_levels.hpp)
        lu_rowtab_fill(threadIdx.x);
        __syncthreads();
    }
    const int lane = lane_id();
    const int r = lane & 31;
    const int sys = (blockIdx.x * WAVES_PER_WG + threadIdx.x / WAVE) * 2 + (lane >> 5);
    const bool ok = sys < n && r < NV;
    // FUSE: the row in its compact form (LuRowForm<true>, hc_lu_struct.hpp), as the tracker's gather
    // leaves it: slot L takes A[r][the member the row's record names at level L] (a zero without
    // one), columns 18..29 stand behind the slots.  The verdict is still taken on all 30 entries.
    cf rA[LuRowForm<FUSE>::W];
    uint32_t nz = 0;
    pf2 sq = {0.0f, 0.0f};   // the entries' sums of squares, as eval_hx_terms_abs takes them
    if constexpr (!FUSE) {
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
    } else {
        static_assert(STRUCT && ENTCHK, "the fused solve's mode");
#pragma unroll
        for (int c = 0; c < NV; c++) {
            const cf a = ok ? A[((size_t)sys * NV + r) * NV + c] : cmk(0.0f, 0.0f);
            if (c >= lu_first_unfused_step()) rA[LuRowForm<FUSE>::pos(c)] = a;
            sq.x = __builtin_fmaf(a.x, a.x, sq.x);
            sq.y = __builtin_fmaf(a.y, a.y, sq.y);
        }
#pragma unroll
        for (int lv = 0; lv < LU_SLOTS; lv++) {
            const int mem = (int)((lu_rowtab_lds()[lv * LU_REC_ROWS + r] >> LU_REC_MEMBER_AT) & 31u);
            rA[lv] = ok && mem != LU_REC_NO_MEMBER ? A[((size_t)sys * NV + r) * NV + mem] : cmk(0.0f, 0.0f);
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
        if constexpr (!FUSE) {
#pragma unroll
            for (int c = 0; c < NV; c++) rA[c] = ok ? A[((size_t)sys * NV + r) * NV + c] : cmk(0.0f, 0.0f);
            x = lu_solve<true>(rA, rB, lane, pat, LB, scr, redo);
        } else {
            cf rD[NV];   // (the dense solve takes the 30 columns)
#pragma unroll
            for (int c = 0; c < NV; c++) rD[c] = ok ? A[((size_t)sys * NV + r) * NV + c] : cmk(0.0f, 0.0f);
            x = lu_solve<true>(rD, rB, lane, pat, LB, scr, redo);
        }
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

// One stage's evaluations as the tracking kernels run them
// (include/eval/hc_eval_testing.h, hc_trifocal_eval_variant_batched): k_eval
// above builds the prefixes from a staged p and reads LDS copies of the packed
// tables, which no tracking kernel does.  This kernel restates
// hc_track_body.inc's sequence call for call, by hand (that file is included
// textually into the trackers and cannot be called): keep the two in step; the
// numbers below are that file's lines.  ABSTAB as there: the throughput
// kernel's slot-absolute tables and its verdict on the dH/dx entries; else the
// packed tables, read from the workspace.  Point i is served by path slot i % 8
// of workgroup i / 8, the slot a path of that wave half has in a tracker, so
// the absolute offsets count from s_slot as they do there.  kind: 0 a
// predictor stage (pred), 1 the corrector; a half without a point is not `act`.
// redo: the values of the evaluations before the dense re-solve (:607-636),
// after the entry block was overwritten as the sparse solve's scratch use may.
// CROW (hc_trifocal_compact_rows_batched, include/lu/hc_lu_compact_testing.h;
// with ABSTAB): the stage's gather as the kernel with the fused solve runs it,
// LUFUSE there: HX takes the rows in their compact form, n x 30 x
// LU_COMPACT_W.  The dense re-solve's gather is the 30-column one in that
// kernel too, which CROW = false returns; redo_vals is not read.
template <bool ABSTAB, bool CROW = false>
__global__ void __launch_bounds__(WG_THREADS) k_eval_variant(int n, int redo_vals, const Workspace *ws,
                                                             const cf *__restrict__ X, const cf *__restrict__ TGT,
                                                             const cf *__restrict__ DIF, const cf *__restrict__ SP,
                                                             const float *__restrict__ T0,
                                                             const uint8_t *__restrict__ KIND, cf *__restrict__ HX,
                                                             cf *__restrict__ RHS, uint8_t *__restrict__ ENT_OK) {
    __shared__ cf s_sp[NPP];                                                      // :35-36
    __shared__ SlotLDS s_slot[2 * WAVES_PER_WG];
    const EvalTables *T = &ws->tab;                                               // :38-39
    if (ws->status != 0u) return;
    const uint2 *s_ht = T->ht;                                                    // :44-46
    const uint32_t *s_hx = T->hx;
    const uint32_t *s_hxd = &T->hxd[0][0];
    if (threadIdx.x < NPP) s_sp[threadIdx.x] = SP[threadIdx.x];                   // :49-54
    {
        float *z = reinterpret_cast<float *>(s_slot);
        for (int i = threadIdx.x; i < (int)(sizeof(s_slot) / 4); i += WG_THREADS) z[i] = 0.0f;
    }
    __syncthreads();
    const int lane = lane_id();                                                   // :56-60
    const int r = lane & 31, hb = lane & 32;
    const int wid = threadIdx.x / WAVE;
    SlotLDS &S = s_slot[wid * 2 + (hb >> 5)];
    if (r == 30) S.x[30] = cmk(1.0f, 0.0f);
    __shared__ uint32_t s_rowc[GM_WORDS + 1][32];                                 // :64-69
    if (threadIdx.x < 32) {
        for (int q = 0; q < GM_WORDS; q++) s_rowc[q][threadIdx.x] = T->gm[q][threadIdx.x];
        s_rowc[GM_WORDS][threadIdx.x] = T->pat[threadIdx.x];
    }
    __syncthreads();
    const bool rl = r < NV;                                                       // :70-75
    wave_lds_sync();
    const AbsTables *AT = &ws->abs;
    const int wv = ABSTAB ? __builtin_amdgcn_readfirstlane(wid) : 0;
    char *const l0 = reinterpret_cast<char *>(s_slot);

    // the slot's point: its x, and its prefix tables from its own target, diff and t (a half
    // without a point stages the last point's parameters, as an idle tracker slot stages sample 0's)
    const int pt = (blockIdx.x * WAVES_PER_WG + wid) * 2 + (hb >> 5);
    const size_t pi = (size_t)(pt < n ? pt : n - 1);
    const unsigned kd = KIND[pi];
    const bool act = pt < n && kd < 2u;   // (2: HC_EVAL_KIND_IDLE)
    const bool pred = act && kd == 0u;
    if (act && rl) S.x[r] = X[pi * (NV + 1) + r];                                 // :518
    build_prefixes(S, r, &T->pre[0][0], TGT + pi * NPP, DIF + pi * NPP, s_sp, T0[pi]);   // :532
    wave_lds_sync();                                                              // :535
    const int lane_v = lane_fresh();                                              // :540-542
    const int r_v = lane_v & 31;
    const uint32_t l16 = (uint32_t)lane_v << 4;
    cf rB = cmk(0.0f, 0.0f);                                                      // :550-573
    {
        const bool any_p = __ballot(pred) != 0ull, any_c = __ballot(act && !pred) != 0ull;
        const RhsMasks mk = rhs_masks(T);
        if (any_p && any_c) {
            if constexpr (ABSTAB) rB = eval_rhs_abs<RHS_MIXED>(AT->ht[wv], AT->htq[wv], l0, l16, pred, mk);
            else rB = eval_rhs<RHS_MIXED>(s_ht, S, r_v, pred, mk);
        } else if (any_p) {
            const cf t = ABSTAB ? eval_rhs_abs<RHS_HT>(AT->ht[wv], AT->htq[wv], l0, l16, true, mk)
                                : eval_rhs<RHS_HT>(s_ht, S, r_v, true, mk);
            if (pred) rB = t;
        } else if (any_c) {
            const cf t = ABSTAB ? eval_rhs_abs<RHS_H>(AT->ht[wv], AT->htq[wv], l0, l16, false, mk)
                                : eval_rhs<RHS_H>(s_ht, S, r_v, false, mk);
            if (!pred) rB = t;
        }
    }
    static_assert(ABSTAB || !CROW, "the compact row is gathered through the absolute tables");
    cf rA[LuRowForm<CROW>::W];                                                    // :576-588
    if constexpr (ABSTAB) {
        uint4 gmv[CROW ? ABS_GMC_Q : ABS_GM_Q];
        const bool ent_ok = eval_hx_terms_abs(AT->hx[wv], l0, l16, CROW ? AT->gmc[wv] : AT->gm[wv], gmv);
        if (act) ENT_OK[pi * 32 + r] = ent_ok ? 1 : 0;   // the lane's own verdict, before the tracker's ballot (:588)
        wave_lds_sync();
        gather_hx_abs(rA, l0, gmv);
    } else {
        eval_hx(rA, s_hx, s_hxd, &s_rowc[0][0], S, r_v);
    }
    wave_lds_sync();
    if constexpr (CROW) {
        if (act && rl) {
#pragma unroll
            for (int c = 0; c < LU_COMPACT_W; c++) HX[(pi * NV + r) * LU_COMPACT_W + c] = rA[c];
            RHS[pi * NV + r] = rB;
        }
    } else {
    if (redo_vals) {
        // what lu_solve<false> may leave of the entry block (hc_slot.hpp): everything but the structural zero
        for (int k = r; k < ENT_CAP - 1; k += 32) S.ent[k] = cmk(__builtin_nanf(""), __builtin_nanf(""));
        wave_lds_sync();
        const bool act_r = act, pred_r = pred;                                    // :606-634
        const int l_r = lane_fresh(), r_r = l_r & 31;
        const uint32_t l16_r = (uint32_t)l_r << 4;
        cf rb = cmk(0.0f, 0.0f);
        if (__ballot(pred_r) != 0ull) {
            const cf t = ABSTAB ? eval_rhs_abs<RHS_HT>(AT->ht[wv], AT->htq[wv], l0, l16_r, true, rhs_masks(T))
                                : eval_rhs<RHS_HT>(s_ht, S, r_r, true, rhs_masks(T));
            if (pred_r) rb = t;
        }
        if (__ballot(act_r && !pred_r) != 0ull) {
            const cf t = ABSTAB ? eval_rhs_abs<RHS_H>(AT->ht[wv], AT->htq[wv], l0, l16_r, false, rhs_masks(T))
                                : eval_rhs<RHS_H>(s_ht, S, r_r, false, rhs_masks(T));
            if (!pred_r) rb = t;
        }
        if constexpr (ABSTAB) {
            uint4 gmv[ABS_GM_Q];
            eval_hx_terms_abs(AT->hx[wv], l0, l16_r, AT->gm[wv], gmv);
            wave_lds_sync();
            gather_hx_abs(rA, l0, gmv);
        } else {
            eval_hx_terms(s_hx, s_hxd, reinterpret_cast<char *>(&S), r_r);
            wave_lds_sync();
            gather_hx(rA, &s_rowc[0][0], S, r_r);
        }
        wave_lds_sync();
        rB = rb;
    }
    if (act && rl) {
#pragma unroll
        for (int c = 0; c < NV; c++) HX[(pi * NV + r) * NV + c] = rA[c];
        RHS[pi * NV + r] = rB;
    }
    }
}

}  // namespace hc
