// hc_lu_levels.hpp -- the fused levels of the tracker LU.  A part of hc_lu.hpp,
// which includes it between its primitives (which this file uses) and the
// forward elimination (which calls lu_level); not a header to include alone.
//
// One step for all the fusable steps of a level (LU_LEVELS, hc_lu_struct.hpp;
// the throughput tracker's solve only: lu_solve<..., FUSE>).  The steps'
// candidate sets are pairwise disjoint "chains" of one or two lane triples, and
// every lane of a chain does for its own chain's column what a step does for
// column I:
//  * candidate: the lane's entry in its chain's column (a select over the
//    level's members on static lane masks); 1 / candidate once;
//  * search: the maximum key over the lane's own chain -- inside the triple
//    with four DPP wave shifts masked by the lane's place in it, across the two
//    triples of a 6-row chain with one ds_bpermute (rows 15..17 cross the
//    16-lane DPP row).  One maximum per chain and half, all in the fast
//    reciprocal range, or the solve leaves the fused path: `redo` (the labels
//    inside a level are not sequential, so the rare path's first-position rule
//    cannot be applied here; the dense re-solve is exact);
//  * broadcast and update: chain k of the level owns a pivot-row window
//    scratch[LU_CHAIN_WIN0 + 2k + J] for column pair J; its pivot lane writes
//    there, every other eligible lane to its own window scratch[2r + J] as in a
//    single step (so the store needs no exec switch), and every lane reads its
//    own chain's window.  1/pivot and the rhs travel in pair 0.  The column
//    pairs are those that hold a column of LU_LEVELS.cols, untested: where a
//    chain's pivot row has no such column it holds an exact zero (equivalence
//    3 of DESIGN.md §4).  A pair may hold a member's own pivot column: the
//    rows below then take a_I - l * pivot there, a value nothing reads (column
//    I of a row that is not step I's pivot row is dead after the multiplier;
//    the back substitution's unmasked update only feeds right-hand sides that
//    are dead as well);
//  * pattern: a row that holds its chain's column takes the member's bound
//    LU_BOUND.s (a superset of the pivot rows' patterns);
//  * row labels: the members' relabels one after the other in increasing I,
//    from the pivot ballot (v_readlane of the pivot lanes' labels).
#pragma once

namespace hc {

constexpr int DPP_WAVE_SHL1 = 0x130, DPP_WAVE_SHR1 = 0x138;   // lane i takes lane i + 1 / i - 1 (GFX9)

// each lane's candidate, its member's bound and its chain's window offset
template <int LV, int K>
__device__ __forceinline__ void lvl_pick(const cf (&rA)[NV], pf2 &c, uint32_t &bnd, int &cwo) {
    if constexpr (K < lu_level_count(LV)) {
        constexpr int I = lu_level_member(LV, K);
        const bool in = __builtin_amdgcn_inverse_ballot_w64(lu_both(LU_BOUND.cand[I]));
        c.x = in ? rA[I].x : c.x;
        c.y = in ? rA[I].y : c.y;
        bnd = in ? LU_BOUND.s[I] : bnd;
        cwo = in ? LU_CHAIN_WIN0 + 2 * K : cwo;
        lvl_pick<LV, K + 1>(rA, c, bnd, cwo);
    }
}
// the members' relabels in increasing I (:70-82): the pivot lane takes label
// I, the lane that held I takes the pivot lane's old label.  Over the whole
// solve the order is level by level (0, 1, 2, 5, 8..11, then 3, 4, 12, 15, ...),
// not 0..17, and the labels before step 18 are still exactly the sequential
// ones: a relabel exchanges the label values I and label(p_I), the pivot lanes
// p_I are chosen from the entries, never from the labels, and two relabels with
// different pivot lanes p, q commute -- both orders end with p at I, q at J,
// and the former holders of I and J (where they are not p or q) at the old
// labels of p and q; if p held J, the holder of I ends with q's old label
// either way.  So any order of the 18 relabels gives the same labels.
template <int LV, int K>
__device__ __forceinline__ void lvl_relabel(int &rowid, unsigned long long m, int hb) {
    if constexpr (K < lu_level_count(LV)) {
        constexpr int I = lu_level_member(LV, K);
        const unsigned long long mi = and_halves<LU_BOUND.cand[I]>(m);
        const int p0 = __builtin_amdgcn_readlane(rowid, __builtin_ctz((unsigned)mi));
        const int p1 = __builtin_amdgcn_readlane(rowid, 32 + __builtin_ctz((unsigned)(mi >> 32)));
        const int piv_pos = hb ? p1 : p0;
        const bool is_p = __builtin_amdgcn_inverse_ballot_w64(mi);
        rowid = is_p ? I : (rowid == I ? piv_pos : rowid);
        lvl_relabel<LV, K + 1>(rowid, m, hb);
    }
}
// the level's column pairs J, J + 1 (J even) inside the eligible rows' region
template <int LV, int J>
__device__ __forceinline__ void lvl_groups(cf (&rA)[NV], const pf2 &l, cf *wrow, const cf *cw) {
    if constexpr (J < NV) {
        if constexpr (((LU_LEVELS.cols[LV] >> J) & 3u) != 0u) {
            grp_store<J, 2>(wrow, rA);
            wave_lds_sync();
            cf u[2];
            grp_load<J, 2>(cw, u);
            grp_update<J, 2>(rA, l, u);
            __builtin_amdgcn_sched_barrier(0);
        }
        lvl_groups<LV, J + 2>(rA, l, wrow, cw);
    }
}
// returns false when the level met a rare condition (nothing is changed then)
template <int LV>
__device__ __forceinline__ bool lu_level(cf (&rA)[NV], cf &rB, int &rowid, uint32_t &pat, int lane, int r, int hb,
                                         PivF &my, cf *scr, unsigned long long &elig_m HC_LU_WORK_ARG) {
    constexpr int CNT = lu_level_count(LV), I0 = lu_level_member(LV, 0);
    constexpr uint32_t ROWS = LU_LEVELS.rows[LV];
    HC_ISA_MARK_I("lu_search", I0);
    pf2 c = {0.0f, 0.0f};
    uint32_t bnd = 0u;
    int cwo = 0;
    lvl_pick<LV, 0>(rA, c, bnd, cwo);
    const float v = __builtin_fabsf(c.x) + __builtin_fabsf(c.y);          // :55
    pf2 oo_s;
    const pf2 reg_s = recip_fast(c, v, oo_s);
    const unsigned long long lv_elig = and_halves<ROWS>(elig_m);
    const bool elig = __builtin_amdgcn_inverse_ballot_w64(lv_elig);
    const int key = elig ? __float_as_int(v) : -1;
    // the maximum over the lane's triple: the neighbours one and two lanes up
    // and down, each only where it lies in the same triple
    int mx;
    {
        const int u1 = dpp_i<DPP_WAVE_SHL1>(key), u2 = dpp_i<DPP_WAVE_SHL1>(u1);
        const int d1 = dpp_i<DPP_WAVE_SHR1>(key), d2 = dpp_i<DPP_WAVE_SHR1>(d1);
        const int a = __builtin_amdgcn_inverse_ballot_w64(lu_both(LU_TRI0 | LU_TRI1)) ? u1 : -1;
        const int b = __builtin_amdgcn_inverse_ballot_w64(lu_both(LU_TRI0)) ? u2 : -1;
        const int e = __builtin_amdgcn_inverse_ballot_w64(lu_both(LU_TRI1 | LU_TRI2)) ? d1 : -1;
        const int f = __builtin_amdgcn_inverse_ballot_w64(lu_both(LU_TRI2)) ? d2 : -1;
        mx = max(max(key, a), max(b, max(e, f)));
    }
    // ... and over the partner triple of a 6-row chain
    constexpr uint32_t UP9 = lu_partner_rows(LV, 9), DN9 = lu_partner_rows(LV, -9), UP6 = lu_partner_rows(LV, 6),
                       DN6 = lu_partner_rows(LV, -6);
    static_assert((UP9 | DN9 | UP6 | DN6 | lu_partner_rows(LV, 0)) == (1u << NV) - 1u, "partner triples 6 or 9 lanes away");
    if constexpr ((UP9 | DN9 | UP6 | DN6) != 0u) {
        int pl = lane;
        if constexpr (UP9 != 0u) pl = __builtin_amdgcn_inverse_ballot_w64(lu_both(UP9)) ? lane + 9 : pl;
        if constexpr (DN9 != 0u) pl = __builtin_amdgcn_inverse_ballot_w64(lu_both(DN9)) ? lane - 9 : pl;
        if constexpr (UP6 != 0u) pl = __builtin_amdgcn_inverse_ballot_w64(lu_both(UP6)) ? lane + 6 : pl;
        if constexpr (DN6 != 0u) pl = __builtin_amdgcn_inverse_ballot_w64(lu_both(DN6)) ? lane - 6 : pl;
        mx = max(mx, __builtin_amdgcn_ds_bpermute(pl << 2, mx));
    }
    // one maximum per chain and half, every one in the fast reciprocal range
    // (a lane outside the level's rows matches its own key: masked off)
    const unsigned long long m = and_halves<ROWS>(__builtin_amdgcn_ballot_w64(key == mx));
    const unsigned long long bad = and_halves<ROWS>(__builtin_amdgcn_ballot_w64(!rcp_fast_bits(mx)));
    if (__builtin_expect((__builtin_popcountll(m) != 2 * CNT) | (bad != 0ull), 0)) return false;
    const bool is_piv = __builtin_amdgcn_inverse_ballot_w64(m);
    HC_ISA_MARK_I("lu_store", I0);
    const cf *cw = scr + (cwo - 2 * r);
    cf *wrow = is_piv ? const_cast<cf *>(cw) : scr;
    st4(&wrow[0], cmk(reg_s.x, reg_s.y), rB);
    wave_lds_sync();
    HC_ISA_MARK_I("lu_rcp", I0);
    cf reg, sB0;
    ld4(&cw[0], reg, sB0);
    if (is_piv) my.oo = oo_s;
    asm volatile("" : "+v"(my.oo));
    lvl_relabel<LV, 0>(rowid, m, hb);
    HC_ISA_MARK_I("lu_update", I0);
#ifdef HC_DIAG_LUWORK
    {   // the level's column pairs x the eligible rows below the pivots (wave-uniform)
        int pairs = 0;
        for (int j = 0; j < NV; j += 2) pairs += ((LU_LEVELS.cols[LV] >> j) & 3u) != 0u;
        lu_work_acc.acc += 2ull * (unsigned long long)pairs *
                           (unsigned long long)__builtin_popcountll(lv_elig & lu_work_acc.mask & ~m);
        lu_work_acc.groups += (unsigned long long)pairs;
    }
#endif
    if (elig) {
        HC_ISA_MARK_I("lu_mult", I0);
        const pf2 lq = pcmul(c, pf2{reg.x, reg.y});
        const pf2 lp = {is_piv ? 0.0f : lq.x, is_piv ? 0.0f : lq.y};
        const pf2 bp = pcmsub(pf2{rB.x, rB.y}, lp, pf2{sB0.x, sB0.y});
        rB = cmk(bp.x, bp.y);
        pat |= (pat & lu_member_cols(LV)) != 0u ? bnd : 0u;
        lvl_groups<LV, 0>(rA, lp, wrow, cw);
    }
    elig_m &= ~m;
    return true;
}

// ---------------------------------------------- the back substitution by level
// Positions 0..17 of the back substitution, one step per level, from the top
// level down (lu_solve<..., FUSE>, after the sequential positions 29..18).  A
// row pivoted at a fused step I holds a non-zero in a column J, I < J <= 17, only
// where J is an ancestor of I in the forest (lu_back_chains_nested,
// hc_lu_struct.hpp), and every lane has at most one member per level, so a lane
// does for its own chain's column what lu_backward<I> does for column I:
//  * select: its entry in the member's column, on the static lane masks of
//    lvl_pick, and the member's position;
//  * divide: cuCdivf(b, pivot) with the factors it kept, once per level; the
//    owner's (the lane whose label is its member: its b is final, every
//    position above 17 and every ancestor has updated it) is x_I;
//  * broadcast: the owner writes x_I into its half's buffer at row[I] (free
//    since the forward elimination ended);
//  * update: every lane of the level's rows reads the x of its own member and
//    takes b -= x * a.  Rows at later positions are solved, so they update
//    unmasked as in lu_backward; lanes without a member at the level keep their
//    b (it may still be waiting for a lower level).  The rows outside the
//    member's chain, which the sequential substitution updates with x_I * 0, are
//    skipped: equal up to the sign of a zero while x_I is finite, and lu_solve
//    hands a solve with a non-finite x to the dense one (equivalence 5 of
//    DESIGN.md §4).  Along a row's ancestors the column rises with the level
//    (lu_back_order_kept), so its non-zero updates keep the descending order.
// Level 0 has nothing left to update: after its broadcast the lanes r < 18 read
// the x_r they return.
template <int LV, int K>
__device__ __forceinline__ void lvl_back_pick(const cf (&rA)[NV], pf2 &c, int &mem) {
    if constexpr (K < lu_level_count(LV)) {
        constexpr int I = lu_level_member(LV, K);
        if constexpr (K == 0) {   // (lanes outside the level: never owners, masked off the update)
            c = pf2{rA[I].x, rA[I].y};
            mem = I;
        } else {
            const bool in = __builtin_amdgcn_inverse_ballot_w64(lu_both(LU_BOUND.cand[I]));
            c.x = in ? rA[I].x : c.x;
            c.y = in ? rA[I].y : c.y;
            mem = in ? I : mem;
        }
        lvl_back_pick<LV, K + 1>(rA, c, mem);
    }
}
template <int LV>
__device__ __forceinline__ void lu_back_level(const cf (&rA)[NV], cf &rB, int rowid, const PivF &my, LUBuf &L) {
    HC_ISA_MARK_I("lu_back_level", LV);
    pf2 c;
    int mem;
    lvl_back_pick<LV, 0>(rA, c, mem);
    const pf2 q = pcdiv_apply(pf2{rB.x, rB.y}, c, my);
    if (rowid == mem) L.row[mem] = cmk(q.x, q.y);   // mem is one of the level's members: inside row[0..17]
    wave_lds_sync();
    if constexpr (LV > 0) {
        if (__builtin_amdgcn_inverse_ballot_w64(lu_both(LU_LEVELS.rows[LV]))) {
            const cf x = L.row[mem];
            const pf2 w = pcmsub(pf2{rB.x, rB.y}, pf2{x.x, x.y}, c);
            rB = cmk(w.x, w.y);
        }
    }
}
// levels LV .. 0, then x_r into the lanes r < 18 (lanes 18..29 hold theirs from
// the sequential positions)
template <int LV>
__device__ __forceinline__ void lu_backward_fused(const cf (&rA)[NV], cf &rB, int rowid, const PivF &my, LUBuf &L, int r,
                                                  pf2 &res) {
    if constexpr (LV >= 0) {
        lu_back_level<LV>(rA, rB, rowid, my, L);
        lu_backward_fused<LV - 1>(rA, rB, rowid, my, L, r, res);
    } else {
        if (__builtin_amdgcn_inverse_ballot_w64(lu_both(lu_fused_steps()))) {
            const cf x = L.row[r];
            res = pf2{x.x, x.y};
        }
    }
}

}  // namespace hc
