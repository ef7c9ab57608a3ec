// hc_lu.hpp -- the tracker's batched 30x30 complex LU solve, two systems per
// wavefront (one per 32-lane half; lane r owns row r in 60 VGPRs, the fused
// solve in the 32 of its compact form).
//
// The LU's headers, all part of this one:
//   hc_lu_struct.hpp  what is known at compile time: column groups, the fill-in
//                     bound and group classes, search spans, the levels of
//                     independent steps, the scratch layout, the fused solve's
//                     compact row form (no device code)
//   hc_lu_diag.hpp    the counters of the diagnostic builds (HC_LU_WORK*, ...)
//   hc_lu.hpp         the primitives, one column group's store / load / update,
//                     the three pivot steps (batched, tested, dense), the pivot
//                     search (lu_forward), the back substitution, lu_solve and
//                     which solve each tracking kernel runs (lu_mode)
//   hc_lu_levels.hpp  the fused levels (lu_level, lu_back_level), included below the primitives
//
// Semantics: magmaHC/dev-cgesv-batched-small.cuh:38-107 -- partial pivoting
// on cabs1 = |re| + |im| with first-maximum ties (the pivot search scans the
// eligible positions in order with a strict '>'), rows relabelled through
// rowid instead of moved, a zero pivot skips the elimination with recip = 1,
// back substitution with cuCdivf.  Op for op the spec of DESIGN.md §4, up to
// the sign of exact zeros (the equivalence class DESIGN.md §4 documents).
//
// How one pivot step I runs (common path, both halves at once):
//  * search: key = bits of |re|+|im| (non-negative floats order like ints),
//    max over the half with 4 DPP steps + v_permlane16_swap, ballot of the
//    maxima.  NaN keys take part (positive NaN bits order above every finite
//    value); a maximum outside the fast reciprocal range (NaN, inf, zero,
//    tiny, huge) or a tie in either half sends the step to the exact rare
//    path (NaN at position I wins, first position among ties);
//  * 1/pivot: every lane computes cuCdivf(1, a_rI) of its own candidate
//    while the search runs (round 4: off the step's critical path), with
//    v_rcp_f32 + one Newton step, which is the IEEE quotient for s in
//    [2^-90, 2^120) (exhaustively verified, scripts/rcp_check.hip,
//    profiles/r1_rcp_check.json); the pivot lane's is the step's 1/pivot, and
//    it keeps the factors (o1, o2) for the back substitution;
//  * broadcast: the pivot lane writes 1/pivot (in the pivot element's slot),
//    rhs and rowid into its half's LDS buffer, every lane reads them back;
//  * one exec region of the eligible rows (the rows below and the pivot row,
//    whose multiplier is zero; round 5): multiplier, right-hand side and
//    fill-in pattern, then per column group (one uniform test) every eligible
//    lane writes the group of its row (ds_write_b128; the pivot lane to the
//    buffer, the others to their own scratch window) and reads the pivot
//    row's group back (broadcast ds_read_b128) and updates, 2 v_pk_fma_f32 per
//    element (lu_step_tested).  The latency mode (LAT > 0: the abort and
//    small-launch kernels) makes one LDS round trip per step instead: every
//    lane writes 1/pivot, rhs, rowid and every column group the fill-in bound
//    leaves alive, none of them tested (lu_step_batched).  Their
//    structure-agnostic twins test the groups as above, and write 1/pivot, rhs
//    and rowid from every lane (no exec region for the broadcast: lu_step_tested's X1).
//
// A column group is LU_CHUNK = 2 columns everywhere (the scratch windows are
// 16 B); only a group's length N (1 for a leading single column) is generic.
//
// Structural sparsity.  The trifocal Jacobian is sparse (170 of 900 entries
// carry terms) and partial-pivot elimination fills it in only partly: on
// tracker Jacobians 64 % of the pivot-row entries a step broadcasts are exact
// zeros.  Each lane keeps the structural pattern of its row (bit c: column c
// may be non-zero) -- initially the columns with index terms, then OR-ed with
// the pivot rows' patterns whenever the row takes a multiple of one
// (fill-in).  A chunk of columns that is zero in both pivot rows of the wave
// is neither written, read nor used in the update (one uniform branch).
// Exactness: a structurally zero entry holds an exact zero while no product
// is infinite or NaN, and a - l*0 == a up to the sign of a zero.  Guarantees:
//  * the solve runs sparse only if every entry is finite with |re|, |im| <
//    2^64 (wave-uniform check on sums of squares; the argument below needs
//    2^88).  Pivoting on |re|+|im| bounds every multiplier by sqrt(2) and the
//    element growth by (1+sqrt(2))^29 < 2^37, so no intermediate can overflow;
//  * and only while every 1/pivot stays in the fast range (|pivot| < 2^-90:
//    1/pivot may overflow; zero or NaN pivot).
// Otherwise the sparse solve reports `redo` and the caller solves the rebuilt
// system with the dense instantiation (every column, the IEEE reciprocal):
// the reference algorithm step for step.  So the sparse steps carry no dense
// tests at all (a per-step `dense` flag cost ~12 SALU and 3 branches a step).
//
// The buffer is the path slot's SlotLDS::lu; the scratch windows are the dH/dx
// entry block (SlotLDS::ent), dead once gathered into the registers (a dense
// re-solve evaluates dH/dx again).
#pragma once

#include "hc_eval.hpp"
#include "hc_lu_struct.hpp"
#include "hc_lu_diag.hpp"

namespace hc {

typedef float f4v __attribute__((ext_vector_type(4)));

struct alignas(16) LUBuf {
    cf row[32];    // current pivot row: [0..29] A, [30] rhs, [31].x = rowid (int bits); x in the back sub
};
static_assert(sizeof(LUBuf) == sizeof(SlotLDS::lu), "LUBuf is SlotLDS::lu");
static_assert(offsetof(SlotLDS, lu) % 16 == 0, "SlotLDS::lu must be 16-B aligned");

// Correctly rounded 1/s for s in [2^-90, 2^120): v_rcp_f32 plus one Newton
// step (bit-identical to hipcc's div_scale / div_fmas / div_fixup sequence
// for every float in that range).
__device__ __forceinline__ float rcp_rn(float s) {
    const float r0 = __builtin_amdgcn_rcpf(s);
    const float e0 = __builtin_fmaf(-s, r0, 1.0f);
    return __builtin_fmaf(e0, r0, r0);
}
// s in the fast reciprocal range, on the bit pattern of a non-negative float
// (NaN and the -1 "no candidate" key fall outside)
__device__ __forceinline__ bool rcp_fast_bits(int bits) {
    return (uint32_t)(bits - 0x12800000) < (uint32_t)(0x7B800000 - 0x12800000);
}

__device__ __forceinline__ void st4(cf *p, cf a, cf b) {
    f4v v = {a.x, a.y, b.x, b.y};
    *reinterpret_cast<f4v *>(p) = v;
}
__device__ __forceinline__ void ld4(const cf *p, cf &a, cf &b) {
    const f4v v = *reinterpret_cast<const f4v *>(p);
    a = cmk(v.x, v.y);
    b = cmk(v.z, v.w);
}

// max over each 32-lane half: DPP inside 16-lane rows, then v_permlane16_swap
// across the row pair (VALU; no LDS round trip unlike ds_swizzle)
__device__ __forceinline__ int half_max_int_p16(int v) {
    v = max(v, dpp_i<DPP_QP_1032>(v));
    v = max(v, dpp_i<DPP_QP_2301>(v));
    v = max(v, dpp_i<DPP_ROW_HALF_MIRROR>(v));
    v = max(v, dpp_i<DPP_ROW_MIRROR>(v));
    const auto sw = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
    return max((int)sw[0], (int)sw[1]);
}

// x & (c | c << 32) as two s_and_b32 with a literal (no 64-bit constant
// materialised in SGPRs)
template <uint32_t C>
__device__ __forceinline__ unsigned long long and_halves(unsigned long long x) {
    uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    asm("s_and_b32 %0, %0, %2\n\ts_and_b32 %1, %1, %2" : "+s"(lo), "+s"(hi) : "i"(C) : "scc");
    return (unsigned long long)lo | ((unsigned long long)hi << 32);
}
// max over the DPP span of lu_search_span (4: half_max_int_p16)
template <int SPAN>
__device__ __forceinline__ int half_max_int_span(int v) {
    if constexpr (SPAN >= 4) {
        return half_max_int_p16(v);
    } else {
        v = max(v, dpp_i<DPP_QP_1032>(v));
        v = max(v, dpp_i<DPP_QP_2301>(v));
        if constexpr (SPAN >= 2) v = max(v, dpp_i<DPP_ROW_HALF_MIRROR>(v));
        if constexpr (SPAN >= 3) v = max(v, dpp_i<DPP_ROW_MIRROR>(v));
        return v;
    }
}

__device__ __forceinline__ int half_min_int_p16(int v) {
    v = min(v, dpp_i<DPP_QP_1032>(v));
    v = min(v, dpp_i<DPP_QP_2301>(v));
    v = min(v, dpp_i<DPP_ROW_HALF_MIRROR>(v));
    v = min(v, dpp_i<DPP_ROW_MIRROR>(v));
    const auto sw = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
    return min((int)sw[0], (int)sw[1]);
}

// reciprocals (o1, o2) of the cuCdivf factors of the pivot a lane owns, kept
// from the forward step that chose it (brs, bis = pivot * o1 are recomputed
// from the pivot element, which stays in the owner's rA)
struct PivF { pf2 oo; };

// cuCdivf(1, y) for s = |y.re| + |y.im| in the fast range, in packed FP32 with
// the spec's ops: o1 = 1/s, (brs, bis) = y*o1, o2 = 1/(brs*brs + bis*bis),
// 1/y = ((o1*brs)*o2, (-(o1*bis))*o2); -(o1*bis) is computed as o1*(-bis)
// (IEEE: the same value).  oo returns (o1, o2).  (Computing o2 straight into
// the high half of o1's pair saves the pivot lane one move per step but
// raised the tracking kernel's spills from 11 to 53 VGPRs; round 6.)
__device__ __forceinline__ pf2 recip_fast(pf2 y, float s, pf2 &oo) {
    // o1 and o2 each in a pair of their own (low half), broadcast by op_sel:
    // no copy to place them side by side
    pf2 o1p, o2p, bb, sq, q, r;
    o1p.x = rcp_rn(s);
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(bb) : "v"(y), "v"(o1p));
    asm("v_pk_mul_f32 %0, %1, %1" : "=v"(sq) : "v"(bb));
    o2p.x = rcp_rn(sq.x + sq.y);
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1] neg_hi:[0,1]" : "=v"(q) : "v"(o1p), "v"(bb));
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(r) : "v"(q), "v"(o2p));
    oo.x = o1p.x;
    oo.y = o2p.x;
    return r;
}

// cdiv_apply(b, f) = cuCdivf(b, pivot) in packed FP32, op for op:
// (brs, bis) = pivot*o1; (ars, ais) = b*o1; re = (ars*brs + ais*bis)*o2; im = (ais*brs - ars*bis)*o2
__device__ __forceinline__ pf2 pcdiv_apply(pf2 b, pf2 piv, const PivF &f) {
    pf2 bb, a, t1, t2, s, q;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(bb) : "v"(piv), "v"(f.oo));
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(a) : "v"(b), "v"(f.oo));
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(t1) : "v"(a), "v"(bb));
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[0,1]" : "=v"(t2) : "v"(a), "v"(bb));
    asm("v_pk_add_f32 %0, %1, %2 neg_hi:[0,1]" : "=v"(s) : "v"(t1), "v"(t2));
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(q) : "v"(s), "v"(f.oo));
    return q;
}

// Group tests on one bit: gbits = pmw | pmw >> 1 | pmw >> 2 | pmw >> 3, so bit J
// says "some column of J..J+3 may be non-zero" and a group test is s_bitcmp1
// + s_cbranch (the compiler keeps an s_cmp after a multi-bit s_and).
__device__ __forceinline__ uint32_t group_bits(uint32_t pmw) {
    uint32_t t = pmw;
#pragma unroll
    for (int k = 1; k < LU_CHUNK; k++) t |= pmw >> k;
    return t;
}
template <int I, int K>
__device__ __forceinline__ bool group_live(uint32_t pmw, uint32_t gb) {
    using C = LuChunks;
    constexpr int J = C::start(I, K), N = C::len(I, K);
    if constexpr (N == 1) return (pmw >> J) & 1u;
    else return (gb >> J) & 1u;
}

// One column group, columns J .. J + N - 1 (N = 1 or 2), of every mode: a lane
// writes its row's group to a row buffer or scratch window w, reads the pivot
// row's group from p into u, and takes a_j -= l * u_j.
// (P: the register position of column J, LuRowForm::pos; the buffer and the
// windows are indexed by J in every row form)
template <int J, int N, int P = J, int W>
__device__ __forceinline__ void grp_store(cf *w, const cf (&rA)[W]) {
    static_assert(P >= 0 && P + N <= W, "the group lies inside the row");
    if constexpr (N == 1) w[J] = rA[P];
    else st4(&w[J], rA[P], rA[P + 1]);
}
template <int J, int N>
__device__ __forceinline__ void grp_load(const cf *p, cf *u) {
    if constexpr (N == 1) u[0] = p[J];
    else ld4(&p[J], u[0], u[1]);
}
template <int J, int N, int P = J, int W>
__device__ __forceinline__ void grp_update(cf (&rA)[W], const pf2 &l, const cf *u) {
    static_assert(P >= 0 && P + N <= W, "the group lies inside the row");
#pragma unroll
    for (int q = 0; q < N; q++) {
        const pf2 v = pcmsub(pf2{rA[P + q].x, rA[P + q].y}, l, pf2{u[q].x, u[q].y});
        rA[P + q] = cmk(v.x, v.y);
    }
}

// After a step's broadcast: 1/pivot, the pivot row's rhs and (returned) the
// pivot lane's old label, from the half's buffer.
template <int I>
__device__ __forceinline__ int lu_read_pivot(const LUBuf &L, cf &reg, cf &sB0) {
    reg = L.row[I];
    cf pr;
    ld4(&L.row[30], sB0, pr);
    return __float_as_int(pr.x);
}
// (The relabel that follows it in every step -- the pivot lane takes label I,
// the lane that held I the pivot lane's old label, :70-82, and the pivot lane
// keeps the factors of its 1/pivot -- is written out in each: as a helper it
// reordered two instructions of the tested step in the HC_DIAG_LIVE build.  Its
// closing asm is opaque on purpose: the select chain must be resolved there, not
// carried as 30 per-step factor pairs into the back substitution.)

// ------------------------------------------------------- the batched step
// Batched latency mode (round 6; LAT > 0 && STRUCT: the abort and small-launch
// kernels with the problem's structure, whose time to the first pose is a lone
// path's latency).  Every column group the fill-in bound leaves alive (124 of
// 225 per solve) runs without a test --
// a group that happens to be zero in the pivot row is exact, as for the
// always-live groups -- so a pivot step needs no pattern bookkeeping, and it
// makes ONE LDS round trip instead of one per live group: every lane writes
// 1/pivot, rhs, rowid and all those groups (the pivot lane into the buffer,
// the others into their scratch windows), then every lane reads them back
// together, then the eligible rows update.  Before it, this mode paired
// always-live groups under one wait (profiles/r5lp_ttfp_lat_pairs.jsonl; the
// code is in 12ddb46).
struct LatCols {   // the columns of step I's live-able groups, packed in group order
    static constexpr int off(int I, int K) {
        int n = 0;
        for (int k = 0; k < K; k++)
            if (lu_group_class(I, k) != GRP_DEAD) n += LuChunks::len(I, k);
        return n;
    }
    static constexpr int total(int I) { return off(I, LuChunks::count(I)); }
};
template <int I, int K>
__device__ __forceinline__ void lat_store(const cf (&rA)[NV], cf *wrow) {
    using C = LuChunks;
    if constexpr (K < C::count(I)) {
        if constexpr (lu_group_class(I, K) != GRP_DEAD) grp_store<C::start(I, K), C::len(I, K)>(wrow, rA);
        lat_store<I, K + 1>(rA, wrow);
    }
}
// the groups whose packed columns start in [LO, HI) (a batch: its reads are
// issued together, its updates follow)
template <int I, int K, int LO, int HI, int M>
__device__ __forceinline__ void lat_load(cf (&u)[M], const LUBuf &L) {
    using C = LuChunks;
    if constexpr (K < C::count(I)) {
        constexpr int O = LatCols::off(I, K);
        if constexpr (lu_group_class(I, K) != GRP_DEAD && O >= LO && O < HI)
            grp_load<C::start(I, K), C::len(I, K)>(L.row, &u[O - LO]);
        lat_load<I, K + 1, LO, HI>(u, L);
    }
}
template <int I, int K, int LO, int HI, int M>
__device__ __forceinline__ void lat_fma(cf (&rA)[NV], const pf2 &l, const cf (&u)[M]) {
    using C = LuChunks;
    if constexpr (K < C::count(I)) {
        constexpr int O = LatCols::off(I, K);
        if constexpr (lu_group_class(I, K) != GRP_DEAD && O >= LO && O < HI)
            grp_update<C::start(I, K), C::len(I, K)>(rA, l, &u[O - LO]);
        lat_fma<I, K + 1, LO, HI>(rA, l, u);
    }
}
// columns read in the step's first batch (with 1/pivot and rhs); the rest
// follow in batches of the same size: the lu_solve template parameter LAT
// (the abort kernel has 128 VGPRs: 8, profiles/r6c_ttfp_ab_latb_cols.jsonl)
#ifndef HC_LU_LATB_COLS
#define HC_LU_LATB_COLS 8
#endif
template <int I, int LO, int B>
__device__ __forceinline__ void lat_batches(cf (&rA)[NV], const pf2 &l, const LUBuf &L) {
    constexpr int T = LatCols::total(I);
    if constexpr (LO < T) {
        constexpr int HI = LO + B;
        cf u[B + 1];
        lat_load<I, 0, LO, HI>(u, L);
        lat_fma<I, 0, LO, HI>(rA, l, u);
        lat_batches<I, HI, B>(rA, l, L);
    }
}
// A step function is the rest of pivot step I once lu_forward has chosen the
// pivots: broadcast, relabel, 1/pivot, update.  This is the batched mode's.
template <int I, int LAT>
__device__ __forceinline__ void lu_step_batched(cf (&rA)[NV], cf &rB, int &rowid, PivF &my, LUBuf &L, cf *scr,
                                                bool is_piv, pf2 reg_s, pf2 oo_s, bool elig) {
    HC_ISA_MARK_I("lu_store", I);
    cf *wrow = is_piv ? L.row : scr;
    wrow[I] = cmk(reg_s.x, reg_s.y);
    st4(&wrow[30], rB, cmk(__int_as_float(rowid), 0.0f));
    lat_store<I, 0>(rA, wrow);
    wave_lds_sync();
    HC_ISA_MARK_I("lu_rcp", I);
    // (the pivot lane reading an exact zero from a zero slot instead, so that
    // its multiplier needs no selects, issued fewer instructions and measured
    // no faster: profiles/r6f_ttfp_ab_zero_slot.jsonl)
    cf reg, sB0;
    const int piv_pos = lu_read_pivot<I>(L, reg, sB0);
    cf u[LAT + 1];
    lat_load<I, 0, 0, LAT>(u, L);
    rowid = is_piv ? I : (rowid == I ? piv_pos : rowid);
    my.oo.x = is_piv ? oo_s.x : my.oo.x;
    my.oo.y = is_piv ? oo_s.y : my.oo.y;
    asm volatile("" : "+v"(my.oo));
    HC_ISA_MARK_I("lu_update", I);
    if (elig) {   // the rows below and the pivot row (multiplier 0: unchanged up to the sign of zeros)
        HC_ISA_MARK_I("lu_mult", I);
        const pf2 lq = pcmul(pf2{rA[I].x, rA[I].y}, pf2{reg.x, reg.y});
        const pf2 lp = {is_piv ? 0.0f : lq.x, is_piv ? 0.0f : lq.y};
        const pf2 bp = pcmsub(pf2{rB.x, rB.y}, lp, pf2{sB0.x, sB0.y});
        rB = cmk(bp.x, bp.y);
        lat_fma<I, 0, 0, LAT>(rA, lp, u);
        lat_batches<I, LAT, LAT>(rA, lp, L);
    }
}

// -------------------------------------------------------- the tested step
// The column groups K.. of step I inside the eligible rows' exec region (the
// rows below and the pivot row; round 5): one uniform test per group, then
// every eligible lane writes the group of its row -- the pivot lane to the
// pivot-row buffer, the others to their own 16-B window of a scratch area
// (wrow, chosen per step: row r's window for group J is scratch[2r + J], so
// one instruction's windows are disjoint), so the store needs no exec switch
// -- reads the pivot row's group back and takes a_j -= l * u_j.  The pivot
// lane has l = 0: its row is unchanged up to the sign of zeros (sparse solves
// only: every entry is finite there, so 0 * u is a zero).  A live group is
// one SALU test and one branch besides its store, read and FMAs; the round-4
// group (the pivot lane's store and the update of the rows below, each in its
// own exec region) took four more SALU and one more branch.
// (profiles/r5c_ab_lu_elig_groups.jsonl: config-2 launch -2.0 %, lone sample
// -5 %; a variant whose pivot row also went through a window, its address
// exchanged with 1/pivot, issued fewer instructions and ran 1 % slower,
// profiles/r5h_ab_lu_windows.jsonl.)
template <int I, int K, bool STRUCT, bool COMPACT>
__device__ __forceinline__ void lu_group_elig(cf (&rA)[LuRowForm<COMPACT>::W], const pf2 &l, uint32_t pmw, uint32_t gb,
                                              cf *wrow, const LUBuf &L HC_LU_WORK_ARG) {
    using C = LuChunks;
    if constexpr (K < C::count(I)) {
        constexpr int J = C::start(I, K), N = C::len(I, K), P = LuRowForm<COMPACT>::pos(J);
        constexpr int CLS = STRUCT ? lu_group_class(I, K) : GRP_TESTED;
        if (CLS != GRP_DEAD && (CLS == GRP_ALWAYS || __builtin_expect(group_live<I, K>(pmw, gb), 1))) {
            grp_store<J, N, P>(wrow, rA);
            wave_lds_sync();
            HC_LU_WORK(N);
            HC_DIAG_LIVE_HIT(I, K);
            HC_LU_WORK_GROUP();
            cf u[N];
            grp_load<J, N>(L.row, u);
            grp_update<J, N, P>(rA, l, u);
        }
        __builtin_amdgcn_sched_barrier(0);
        lu_group_elig<I, K + 1, STRUCT, COMPACT>(rA, l, pmw, gb, wrow, L HC_LU_WORK_PASS);
    }
}
// The sparse step that tests its column groups: the throughput tracker's
// sequential steps, the archived kernels' and every structure-agnostic twin's.
// X1, the latency mode without the problem's structure (LAT > 0, !STRUCT: the
// twins of the abort and small-launch kernels): every lane writes 1/pivot, rhs
// and rowid, the pivot lane to the buffer, the others to their scratch windows
// -- no exec region, at the price of LDS bandwidth
// (profiles/r5m_ab_lu_x.jsonl: lone sample -2 %, loaded launch +0.8 %).
template <int I, bool X1, bool STRUCT, bool COMPACT>
__device__ __forceinline__ void lu_step_tested(cf (&rA)[LuRowForm<COMPACT>::W], cf &rB, int &rowid, uint32_t &pat, PivF &my, LUBuf &L,
                                               cf *scr, bool is_piv, int pl0, int pl1, pf2 reg_s, pf2 oo_s,
                                               bool elig HC_LU_WORK_ARG) {
    // structural patterns of the two pivot rows (wave-uniform)
    const uint32_t pp0 = (uint32_t)__builtin_amdgcn_readlane((int)pat, pl0);
    const uint32_t pp1 = (uint32_t)__builtin_amdgcn_readlane((int)pat, pl1);
    const uint32_t pmw = (pp0 | pp1) & (0xFFFFFFFFu << (I + 1));
    const uint32_t gb = group_bits(pmw);
    HC_ISA_MARK_I("lu_store", I);
    cf *wrow;
    if constexpr (X1) {
        wrow = is_piv ? L.row : scr;
        wrow[I] = cmk(reg_s.x, reg_s.y);
        st4(&wrow[30], rB, cmk(__int_as_float(rowid), 0.0f));
    } else if (is_piv) {                                   // pivot row -> buffer, 1/pivot in the pivot's slot
        L.row[I] = cmk(reg_s.x, reg_s.y);
        L.row[30] = rB;
        L.row[31].x = __int_as_float(rowid);
    }
    wave_lds_sync();
    HC_ISA_MARK_I("lu_rcp", I);
    cf reg, sB0;
    const int piv_pos = lu_read_pivot<I>(L, reg, sB0);
    if constexpr (X1) {
        rowid = is_piv ? I : (rowid == I ? piv_pos : rowid);
        my.oo.x = is_piv ? oo_s.x : my.oo.x;
        my.oo.y = is_piv ? oo_s.y : my.oo.y;
    } else {
        if (is_piv) rowid = I;
        else if (rowid == I) rowid = piv_pos;
        if (is_piv) my.oo = oo_s;
    }
    asm volatile("" : "+v"(my.oo));
    // one exec-masked region per step: multiplier, right-hand side, fill-in
    // pattern (branch-free) and the rank-1 update, in the eligible rows' region
    // (:86-93: eligible is known from the search, so the region does not wait
    // for the read-back; the pivot lane's multiplier is zeroed: its rhs and row
    // stay, up to the sign of zeros; profiles/r5m_ab_lu_x.jsonl: -0.4 %, lone
    // sample -1.5 %).  Fill-in: a row whose column I may be non-zero takes the
    // pivot patterns (both halves': a superset of its own pivot row's).
    HC_ISA_MARK_I("lu_update", I);
    if constexpr (!X1) wrow = is_piv ? L.row : scr;
#ifdef HC_DIAG_LUWORK
    lu_work_acc.excl = __builtin_amdgcn_ballot_w64(is_piv);
#endif
    HC_DIAG_LIVE_HIT(I, LIVE_SOLVES);
    if (elig) {
        HC_ISA_MARK_I("lu_mult", I);
        // (the pivot lane's multiplier is zeroed by two selects: reading an
        // exact zero from a zero slot instead held one more address in a VGPR
        // across the solve: 11 -> 20 spills; round 6)
        constexpr int PI = LuRowForm<COMPACT>::pos(I);
        const pf2 lq = pcmul(pf2{rA[PI].x, rA[PI].y}, pf2{reg.x, reg.y});
        const pf2 lp = {is_piv ? 0.0f : lq.x, is_piv ? 0.0f : lq.y};
        const pf2 bp = pcmsub(pf2{rB.x, rB.y}, lp, pf2{sB0.x, sB0.y});
        rB = cmk(bp.x, bp.y);
        pat |= (uint32_t)__builtin_amdgcn_sbfe((int)pat, I, 1) & pmw;   // v_bfe_i32 + v_and_or_b32
        lu_group_elig<I, 0, STRUCT, COMPACT>(rA, lp, pmw, gb, wrow, L HC_LU_WORK_PASS);
    }
}

// --------------------------------------------------------- the dense step
// The column groups K.. of a dense step, every one of them: the pivot lane
// writes the group, the rows below read it back and take a_j -= l * u_j (one
// exec region each; the dense steps may hold inf and NaN, so the pivot row
// cannot take a zero multiplier there).
template <int I, int K>
__device__ __forceinline__ void lu_group_dense(cf (&rA)[NV], const pf2 &l, LUBuf &L, bool is_piv,
                                               bool below HC_LU_WORK_ARG) {
    using C = LuChunks;
    if constexpr (K < C::count(I)) {
        constexpr int J = C::start(I, K), N = C::len(I, K);
        if (is_piv) grp_store<J, N>(L.row, rA);
        wave_lds_sync();
        if (below) {
            HC_LU_WORK(N);
            HC_LU_WORK_GROUP();
            cf u[N];
            grp_load<J, N>(L.row, u);
            grp_update<J, N>(rA, l, u);
        }
        __builtin_amdgcn_sched_barrier(0);
        lu_group_dense<I, K + 1>(rA, l, L, is_piv, below HC_LU_WORK_PASS);
    }
}
// DENSE (the whole solve of a matrix that is not provably finite or that met a
// pivot outside the fast reciprocal range): every column group and the IEEE
// reciprocal, the reference algorithm step for step.
template <int I>
__device__ __forceinline__ void lu_step_dense(cf (&rA)[NV], cf &rB, int &rowid, PivF &my, LUBuf &L, bool is_piv,
                                              pf2 reg_s, pf2 oo_s, bool elig HC_LU_WORK_ARG) {
    HC_ISA_MARK_I("lu_store", I);
    if (is_piv) {                                          // pivot row -> buffer, 1/pivot in the pivot's slot
        L.row[I] = cmk(reg_s.x, reg_s.y);
        L.row[30] = rB;
        L.row[31].x = __int_as_float(rowid);
    }
    wave_lds_sync();
    HC_ISA_MARK_I("lu_rcp", I);
    cf reg, sB0;
    const int piv_pos = lu_read_pivot<I>(L, reg, sB0);
    if (is_piv) rowid = I;
    else if (rowid == I) rowid = piv_pos;
    if (is_piv) my.oo = oo_s;
    asm volatile("" : "+v"(my.oo));
    // :86-93: rowid > I after the relabel, i.e. an eligible row that is not the
    // pivot (the displaced row takes the pivot's old id > I); known from the
    // search, so the exec region does not wait for the read-back (padding lanes,
    // never eligible, stay out: their rows are not part of the system)
    const bool below = elig && !is_piv;
    pf2 lp = {0.0f, 0.0f};
    if (below) {
        HC_ISA_MARK_I("lu_mult", I);
        lp = pcmul(pf2{rA[I].x, rA[I].y}, pf2{reg.x, reg.y});
        const pf2 bp = pcmsub(pf2{rB.x, rB.y}, lp, pf2{sB0.x, sB0.y});
        rB = cmk(bp.x, bp.y);
    }
    HC_ISA_MARK_I("lu_update", I);
    lu_group_dense<I, 0>(rA, lp, L, is_piv, below HC_LU_WORK_PASS);
}

}  // namespace hc

#include "hc_lu_levels.hpp"   // the fused levels: lu_level, on the primitives above

namespace hc {

// ------------------------------------------------------ forward elimination
// Pivot steps I .. NV - 1, one after the other: the pivot search, then the
// step of the solve's mode.  !DENSE: a pivot outside the fast reciprocal range
// sets `redo` (the solve goes on with garbage, the caller discards it and
// solves densely).  COMPACT: the row form (LuRowForm, hc_lu_struct.hpp; the
// fused solve's sequential steps, whose columns all lie behind the slots).
template <int I, bool DENSE, int LAT, bool STRUCT, bool COMPACT = false>
__device__ __forceinline__ void lu_forward(cf (&rA)[LuRowForm<COMPACT>::W], cf &rB, int &rowid, uint32_t &pat, int lane, int r, int hb,
                                           bool row_lane, PivF &my, LUBuf &L, cf *scr, bool &redo,
                                           unsigned long long elig_m HC_LU_WORK_ARG) {
    static_assert(!COMPACT || (!DENSE && LAT == 0 && STRUCT && I >= lu_first_unfused_step()),
                  "the compact row is the fused solve's");
    if constexpr (I < NV) {
        HC_ISA_MARK_I("lu_search", I);
        constexpr int PI = LuRowForm<COMPACT>::pos(I);
        const float v = __builtin_fabsf(rA[PI].x) + __builtin_fabsf(rA[PI].y);          // :55
        // 1 / own candidate as cuCdivf(1, a_rI) (:66, :84), off the step's critical path:
        // the pivot lane's is the step's 1/pivot (same ops on the same value)
        pf2 reg_s, oo_s;
        if constexpr (!DENSE) {
            reg_s = recip_fast(pf2{rA[PI].x, rA[PI].y}, v, oo_s);
        } else {
            const divf f = cdiv_factors(rA[PI]);
            const cf rg = (v == 0.0f) ? cmk(1.0f, 0.0f) : cdiv_apply(cmk(1.0f, 0.0f), f);
            reg_s = pf2{rg.x, rg.y};
            oo_s = pf2{f.o1, f.o2};
        }
        // eligible rows (not pivoted yet; :86-93), carried from the previous
        // step as a lane mask, elig & ~pivots (SALU), instead of a rowid
        // compare after the relabel (profiles/r5e1_ab_lu_elig_carry.jsonl: -0.6 %)
        const bool elig = __builtin_amdgcn_inverse_ballot_w64(elig_m);
        bool is_piv;
        float piv_abs;
        int pl0, pl1;   // pivot lanes of the two halves
        unsigned long long piv_m;   // the two pivot lanes
        // the tracker's steps 0..17 reduce over the candidate rows' quad,
        // half-row or row only (lu_search_span): every other row's entry is an
        // exact zero (key 0, or -1 when not eligible), so the candidates'
        // group holds the maximum whenever it is a fast-range (positive) key,
        // and the ballots keep the candidate lanes only (other groups match
        // their own maxima).  bad == 0 then means each half's maximum is a
        // candidate's, so popcount(m) == 2 is still one pivot per half.
        constexpr int SPAN = (STRUCT && !DENSE) ? lu_search_span(I) : 4;
        const int key = elig ? __float_as_int(v) : -1;
        const int mx = half_max_int_span<SPAN>(key);
        unsigned long long m = __builtin_amdgcn_ballot_w64(key == mx);
        unsigned long long bad = __builtin_amdgcn_ballot_w64(!rcp_fast_bits(mx));
        if constexpr (SPAN < 4) {
            m = and_halves<LU_BOUND.cand[I]>(m);
            bad = and_halves<LU_BOUND.cand[I]>(bad);
        }
        const unsigned mlo = (unsigned)m, mhi = (unsigned)(m >> 32);
        // common: one maximum per half (two in the wave; s_bcnt1, where the
        // per-half m & (m - 1) tests took six SALU), both in the fast range
        // the pivot steps where exact ties are frequent on this problem's Jacobians
        // (steps 18, 19, 21, 22: 79, 29, 51, 32 % of solves) resolve them inline
        // with one more half-wave min reduction (lowest row id among the maxima)
        // instead of taking the rare path (profiles/r4f_ab_trims.jsonl)
        constexpr bool TIE = I == 18 || I == 19 || I == 21 || I == 22;
        const bool rare = DENSE || (TIE ? (bad != 0ull) : ((__builtin_popcountll(m) != 2) | (bad != 0ull)));
        if (__builtin_expect(rare, 0)) {
            HC_ISA_MARK_I("lu_rare", I);
#ifdef HC_DIAG_LUWORK
            lu_work_acc.rare++;
            if constexpr (!DENSE) {
                if (lane == 0) atomicAdd(&g_diag_luwork[DIAG_LUWORK_RARE_AT + I], 1ull);
                if (lu_step_fusable(I)) lu_work_acc.rare_fusable = 1ull;
            }
#endif
            // rare: NaN at position I wins (:57-64); exact ties: first position wins
            const bool isn = v != v;
            const unsigned long long nanb = __builtin_amdgcn_ballot_w64(isn);
            // the maximum over the non-NaN candidates: the first search's unless
            // some lane holds a NaN (ties and out-of-range pivots need no second
            // reduction) or the search was narrowed to the candidate rows
            int mx2 = mx;
            unsigned long long m2 = m;
            if constexpr (SPAN < 4) {
                mx2 = half_max_int_p16(key);
                m2 = __builtin_amdgcn_ballot_w64(key == mx2);
            }
            if (__builtin_expect(nanb != 0ull, 0)) {
                const int key2 = (elig && !isn) ? __float_as_int(v) : -1;
                mx2 = half_max_int_p16(key2);
                m2 = __builtin_amdgcn_ballot_w64(key2 == mx2);
            }
            const unsigned long long nanm = nanb & __builtin_amdgcn_ballot_w64(rowid == I);
            const unsigned nlo = (unsigned)nanm, nhi = (unsigned)(nanm >> 32);
            const unsigned mine_m = hb ? (unsigned)(m2 >> 32) : (unsigned)m2, mine_n = hb ? nhi : nlo;
            const int c2 = ((mine_m >> r) & 1u) ? rowid : (1 << 20);
            const int mn = half_min_int_p16(c2);
            const unsigned long long w = __builtin_amdgcn_ballot_w64(row_lane && rowid == mn);
            const unsigned wm = hb ? (unsigned)(w >> 32) : (unsigned)w;
            const int pl = mine_n ? hb + __builtin_ctz(mine_n) : hb + (wm ? __builtin_ctz(wm) : 0);
            is_piv = lane == pl;
            piv_abs = mine_n ? __builtin_nanf("") : __int_as_float(mx2);
            const unsigned long long pm = __builtin_amdgcn_ballot_w64(is_piv);
            piv_m = pm;
            pl0 = __builtin_ctz((unsigned)pm | 0x80000000u);
            pl1 = 32 + __builtin_ctz((unsigned)(pm >> 32) | 0x80000000u);
            if constexpr (!DENSE)
                redo = redo || __builtin_amdgcn_ballot_w64(!rcp_fast_bits(__float_as_int(piv_abs))) != 0ull;
        } else if constexpr (TIE) {
            // first position (lowest row id) among each half's maxima
            const int c2 = key == mx ? rowid : (1 << 20);
            const int mn = half_min_int_p16(c2);
            is_piv = key == mx && rowid == mn;
            piv_abs = __int_as_float(mx);
            const unsigned long long w = __builtin_amdgcn_ballot_w64(is_piv);
            piv_m = w;
            pl0 = __builtin_ctz((unsigned)w);
            pl1 = 32 + __builtin_ctz((unsigned)(w >> 32));
        } else {
            // (the narrowed search: only the candidate lanes' matches count)
            is_piv = __builtin_amdgcn_inverse_ballot_w64(m);   // (one bit per half: m is the pivot mask)
            piv_m = m;
            piv_abs = __int_as_float(mx);
            pl0 = __builtin_ctz(mlo);        // exactly one bit per half here
            pl1 = 32 + __builtin_ctz(mhi);
        }
        HC_ISA_MARK_I("lu_pattern", I);
        if constexpr (DENSE) lu_step_dense<I>(rA, rB, rowid, my, L, is_piv, reg_s, oo_s, elig HC_LU_WORK_PASS);
        else if constexpr (LAT > 0 && STRUCT) lu_step_batched<I, LAT>(rA, rB, rowid, my, L, scr, is_piv, reg_s, oo_s, elig);
        else lu_step_tested<I, (LAT > 0), STRUCT, COMPACT>(rA, rB, rowid, pat, my, L, scr, is_piv, pl0, pl1, reg_s, oo_s,
                                                           elig HC_LU_WORK_PASS);
        lu_forward<I + 1, DENSE, LAT, STRUCT, COMPACT>(rA, rB, rowid, pat, lane, r, hb, row_lane, my, L, scr, redo,
                                              elig_m & ~piv_m HC_LU_WORK_PASS);
    }
}
// The forward elimination of lu_solve<..., FUSE>: the fused levels LV ..
// LU_LEVELS.nlevels - 1 (hc_lu_levels.hpp), then the sequential steps from the
// first step no level holds.  A rare condition inside a level sets `redo` and
// ends the elimination.
template <int LV>
__device__ __forceinline__ void lu_forward_fused(cf (&rA)[LU_COMPACT_W], cf &rB, int &rowid, uint32_t &pat, int lane, int r, int hb,
                                                 bool row_lane, PivF &my, LUBuf &L, cf *scr, bool &redo,
                                                 unsigned long long elig_m HC_LU_WORK_ARG) {
    if constexpr (LV < LU_LEVELS.nlevels) {
        if (!lu_level<LV>(rA, rB, rowid, pat, r, hb, my, L, scr, elig_m HC_LU_WORK_PASS)) {
#ifdef HC_DIAG_LUWORK
            lu_work_acc.rare++;
            lu_work_acc.rare_fusable = 1ull;
#endif
            redo = true;
            return;
        }
        lu_forward_fused<LV + 1>(rA, rB, rowid, pat, lane, r, hb, row_lane, my, L, scr, redo, elig_m HC_LU_WORK_PASS);
    } else {
        lu_forward<lu_first_unfused_step(), false, 0, true, true>(rA, rB, rowid, pat, lane, r, hb, row_lane, my, L, scr, redo,
                                                           elig_m HC_LU_WORK_PASS);
    }
}

// back substitution (:97-106): the lane whose final rowid is I owns position I
// and divides with the factors it kept from the forward step; x_I reaches the
// lanes of its half with v_readlane (owner lane of each half found by a
// ballot of the final row ids), and lanes I and 32 + I -- which return x_I --
// capture it with one exec-masked move (static lanes: no compare, no select,
// no LDS redistribution at the end).  The owner's rB is final at its step
// (every step J > I has updated it) and dead after it, so the later steps
// J < I may update it unmasked.
// LAST: the position the walk ends with (18 in lu_solve<..., FUSE>, whose
// positions 17..0 run level by level: lu_backward_fused, hc_lu_levels.hpp).
template <int I, int LAST = 0, bool COMPACT = false>
__device__ __forceinline__ void lu_backward(const cf (&rA)[LuRowForm<COMPACT>::W], cf &rB, int rowid, const PivF &my,
                                            pf2 &res) {
    static_assert(!COMPACT || LAST >= lu_first_unfused_step(), "the compact row's low positions run level by level");
    if constexpr (I >= LAST) {
        HC_ISA_MARK_I("lu_back", I);
        constexpr int PI = LuRowForm<COMPACT>::pos(I);
        const unsigned long long own = __builtin_amdgcn_ballot_w64(rowid == I);
        const int o0 = __builtin_ctz((unsigned)own);          // one owner per half
        const int o1 = 32 + __builtin_ctz((unsigned)(own >> 32));
        const pf2 q = pcdiv_apply(pf2{rB.x, rB.y}, pf2{rA[PI].x, rA[PI].y}, my);
        const float x0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q.x), o0));
        const float y0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q.y), o0));
        const float x1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q.x), o1));
        const float y1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q.y), o1));
        // x_I of each half from its SGPR pair: one v_mov_b64 for all lanes, one
        // more with the low half masked off, one into res of lanes I, 32 + I
        // (exec saved and restored)
        const pf2 xs0 = {x0, y0}, xs1 = {x1, y1};
        pf2 xv;
        unsigned long long tmp;
        asm volatile("s_nop 1\n\ts_mov_b64 %2, exec\n\tv_mov_b64 %0, %3\n\ts_mov_b32 exec_lo, 0\n\t"
                     "v_mov_b64 %0, %4\n\ts_mov_b32 exec_lo, %5\n\ts_mov_b32 exec_hi, %5\n\t"
                     "v_mov_b64 %1, %0\n\ts_mov_b64 exec, %2"
                     : "=&v"(xv), "+v"(res), "=&s"(tmp) : "s"(xs0), "s"(xs1), "i"(1u << I));
        // rows above position I take b -= x_I * a_I; the update runs unmasked
        // (no compare, no exec region): the rows at or below I are solved, so
        // their rB is dead (profiles/r3aa_ab_backsub_unmasked.jsonl)
        if constexpr (I > 0) {
            const pf2 w = pcmsub(pf2{rB.x, rB.y}, xv, pf2{rA[PI].x, rA[PI].y});
            rB = cmk(w.x, w.y);
        }
        lu_backward<I - 1, LAST, COMPACT>(rA, rB, rowid, my, res);
    }
}

// Which sparse solve a tracking kernel runs, lu_solve<false, lat, strct,
// entchk, fuse>, from what the kernel knows (hc_track.hpp: ABORT, ARCH, LULAT,
// LUS).  The one statement of it: hc_track_body.inc and the test hook of each
// solve alone (hc_cgesv_30x30_variant_batched) both read it here.
//  * entchk: the throughput tracking kernel (neither abort nor archived
//    semantics, no latency mode) checks finiteness on the dH/dx entries it
//    gathers the rows from (eval_hx_terms_abs);
//  * fuse: of those, the instantiation with the problem's structure runs its
//    independent pivot steps level by level; its structure-agnostic twin has no
//    levels to fuse.
struct LuMode { int lat; bool strct, entchk, fuse; };
constexpr LuMode lu_mode(bool ABORT, bool ARCH, int LULAT, bool LUS) {
    const bool entchk = !ABORT && !ARCH && LULAT == 0;
    return LuMode{LULAT, LUS, entchk, entchk && LUS};
}

// Solves the system of each half: lane r holds row r of A in rA and b_r in
// rB; pattern = the structural pattern of row r.  Returns x_r in lane r.  L is
// this half's buffer (16-B aligned).  DENSE = false: the structurally sparse
// solve, which sets `redo` (wave-uniform) instead of handling a matrix that is
// not provably finite or a pivot outside the fast reciprocal range: the
// caller then rebuilds the system and calls the DENSE solve, the reference
// algorithm step for step (both exact).
// scratch: this half's LU_SCRATCH_CF entries (hc_lu_struct.hpp) that the
// sparse solve may overwrite.
// ENTCHK: the caller has made the finiteness check on the entries it gathered
// the rows from (eval_hx_terms_abs) and passes the wave-uniform verdict in
// ent_bad; the row loop below is left out.
// FUSE (the throughput tracker's solve): the row comes in its compact form,
// LU_COMPACT_W positions (LuRowForm<true>, hc_lu_struct.hpp: the row's column
// of each level, then columns 18..29; every other instantiation takes the 30
// columns in place, and `pattern` keeps true column numbers in both); the
// fusable steps run level by level
// (lu_forward_fused), and so do their positions of the back substitution
// (lu_backward_fused); scratch then has LU_SCRATCH_FUSED_CF entries, and a
// rare condition inside a level or a solution that is not finite reports
// `redo` as well.
// count_mask: diagnostic builds (HC_DIAG_LUWORK), the lanes whose executed
// work is counted; call sites pass HC_LU_COUNT(mask).
template <bool DENSE, int LAT = 0, bool STRUCT = false, bool ENTCHK = false, bool FUSE = false>
__device__ __forceinline__ cf lu_solve(cf (&rA)[LuRowForm<FUSE>::W], cf rB, int lane, uint32_t pattern, LUBuf &L, cf *scratch,
                                      bool &redo, unsigned long long count_mask = ~0ull, bool ent_bad = false) {
    static_assert(!FUSE || (!DENSE && LAT == 0 && STRUCT && ENTCHK), "the fused levels belong to the throughput tracker's solve");
    (void)count_mask;
    const int r = lane & 31, hb = lane & 32;
    const bool row_lane = r < NV;
    redo = false;
    if constexpr (DENSE) HC_ISA_MARK("lu_dense");   // (scripts/isa_phases.py: the dense re-solve's copy)
    else HC_ISA_MARK("lu_sparse");
    HC_ISA_MARK("lu_finite");
    if constexpr (!DENSE && ENTCHK) {
        if (__builtin_expect(ent_bad, 0)) {
            redo = true;
            return cmk(0.0f, 0.0f);
        }
    } else if constexpr (!DENSE) {
        // every entry finite and below 2^64 in magnitude (inside the 2^88 the
        // sparse path needs): the per-component sums of squares (v_pk_fma_f32, 30
        // VALU) stay finite only then -- NaN propagates, an inf or |entry| >= 2^64
        // makes a square overflow.  A sum that overflows from many entries below
        // 2^64 only sends the solve to the dense path, which is exact as well.
        pf2 sq = {0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < NV; c++) {
            const pf2 e = {rA[c].x, rA[c].y};
            asm("v_pk_fma_f32 %0, %1, %1, %0" : "+v"(sq) : "v"(e));
        }
        const bool ok = sq.x + sq.y < __builtin_inff();
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(!ok) != 0ull, 0)) {
            redo = true;
            return cmk(0.0f, 0.0f);
        }
    }
    // padding lanes never pivot (FUSE: a label is an index into the levels' label table, row[0..31])
    int rowid = row_lane ? r : FUSE ? NV : 99;
    uint32_t pat = row_lane ? pattern : 0u;
    PivF my{pf2{0.0f, 0.0f}};
#ifdef HC_DIAG_LUWORK
    LuWork lu_work_acc{0ull, count_mask, 0ull, 0ull, 0ull, 0ull};
#endif
    if constexpr (FUSE)
        lu_forward_fused<0>(rA, rB, rowid, pat, lane, r, hb, row_lane, my, L, scratch + 2 * r, redo,
                            __builtin_amdgcn_ballot_w64(row_lane) HC_LU_WORK_PASS);
    else
        lu_forward<0, DENSE, LAT, STRUCT>(rA, rB, rowid, pat, lane, r, hb, row_lane, my, L, scratch + 2 * r, redo,
                                          __builtin_amdgcn_ballot_w64(row_lane) HC_LU_WORK_PASS);
#ifdef HC_DIAG_LUWORK
    const unsigned long long solves = (unsigned long long)__builtin_popcountll(count_mask & __builtin_amdgcn_ballot_w64(row_lane)) / NV;
    if (lane == 0 && !DENSE && !redo) {   // sparse solves that completed, and their work
        atomicAdd(&g_diag_luwork[0], lu_work_acc.acc);
        atomicAdd(&g_diag_luwork[1], solves);
        atomicAdd(&g_diag_luwork[3], 1ull);
        atomicAdd(&g_diag_luwork[4], lu_work_acc.groups);
        atomicAdd(&g_diag_luwork[5], lu_work_acc.rare);
    }
    if (lane == 0 && DENSE) atomicAdd(&g_diag_luwork[2], solves);   // dense (re-)solves
    if (lane == 0 && !DENSE) atomicAdd(&g_diag_luwork[DIAG_LUWORK_RARE_FUSABLE], lu_work_acc.rare_fusable);
#endif
    if constexpr (FUSE) {   // (wave-uniform: the caller solves the system again)
        if (__builtin_expect(redo, 0)) return cmk(0.0f, 0.0f);
    }
#ifdef HC_DIAG_PHASES
    // diagnostic build: the forward / back-substitution boundary of this wave's
    // solve (s_memtime), read by k_track after the solve (g_diag_lu_mid)
    if ((lane & 63) == 0 && blockIdx.x < 16384u) g_diag_lu_mid[blockIdx.x * 4 + (threadIdx.x >> 6)] = __builtin_amdgcn_s_memtime();
#endif
    // lane r returns x_r (captured at back-substitution step r; padding lanes 0)
    HC_ISA_MARK("lu_back_init");
    pf2 res = {0.0f, 0.0f};
    if constexpr (FUSE) {
        lu_backward<NV - 1, lu_first_unfused_step(), true>(rA, rB, rowid, my, res);
        lu_backward_fused<LU_LEVELS.nlevels - 1>(rA, rB, rowid, my, L, r, res);
        // the levels skip the rows that take x_J * 0, which is a zero only for
        // a finite x_J: a solve with a non-finite x goes to the dense one
        // (padding lanes return 0)
        const float nf = __builtin_fmaf(res.y, 0.0f, res.x * 0.0f);   // NaN unless both parts are finite
        redo = __builtin_amdgcn_ballot_w64(nf != nf) != 0ull;
#ifdef HC_DIAG_LUWORK
        if (lane == 0 && redo) {   // not a completed sparse solve after all: its counts are taken back
            atomicAdd(&g_diag_luwork[0], 0ull - lu_work_acc.acc);
            atomicAdd(&g_diag_luwork[1], 0ull - solves);
            atomicAdd(&g_diag_luwork[3], 0ull - 1ull);
            atomicAdd(&g_diag_luwork[4], 0ull - lu_work_acc.groups);
            atomicAdd(&g_diag_luwork[5], 0ull - lu_work_acc.rare);
        }
#endif
    } else {
        lu_backward<NV - 1>(rA, rB, rowid, my, res);
    }
    return cmk(res.x, res.y);
}

}  // namespace hc
