// hc_lu_levels.hpp -- the fused levels of the tracker LU.  A part of hc_lu.hpp,
// which includes it between its primitives (which this file uses) and the
// forward elimination (which calls lu_level); not a header to include alone.
//
// One step for all the fusable steps of a level (LU_LEVELS, hc_lu_struct.hpp;
// the throughput tracker's solve only: lu_solve<..., FUSE>).  The steps'
// candidate sets are pairwise disjoint "chains" of one or two lane triples, and
// every lane of a chain does for its own chain's column what a step does for
// column I:
//  * the row's record: what the row is to the level -- its chain and member,
//    its chain's window, its partner across a 6-row chain, its place in its
//    triple -- is one word of LU_ROWTAB (hc_lu_struct.hpp), read from LDS;
//  * candidate: the lane's entry in its chain's column, which the compact row
//    (LuRowForm<true>, hc_lu_struct.hpp) keeps at position LV whatever the
//    chain (until v10.12 a select over the level's members in a 30-column
//    row, one compare with the record's chain number each); 1 / candidate once;
//  * search: the maximum key over the lane's own chain -- inside the triple
//    with four DPP wave shifts selected by the lane's place in it, across the two
//    triples of a 6-row chain with one ds_bpermute (rows 15..17 cross the
//    16-lane DPP row).  One maximum per chain and half, all in the fast
//    reciprocal range, or the solve leaves the fused path: `redo` (the labels
//    inside a level are not sequential, so the rare path's first-position rule
//    cannot be applied here; the dense re-solve is exact);
//  * broadcast and update: chain k of the level owns a pivot-row window
//    scratch[LU_CHAIN_WIN0 + 2k + J] for column pair J; its pivot lane writes
//    there, every other eligible lane to its own window scratch[2r + J] as in a
//    single step (so the store needs no exec switch), and every lane reads its
//    own chain's window.  1/pivot and the rhs travel in pair 0.  The pairs
//    are those of positions that hold a column of LU_LEVELS.cols (lvl_groups;
//    the rows of a chain name the same columns in the slots above the level, so
//    a slot pair is the same column pair to the pivot row and to the rows that
//    take it), untested: where a
//    chain's pivot row has no such column it holds an exact zero (equivalence
//    3 of DESIGN.md §4).  A pair may hold a member's own pivot column: the
//    rows below then take a_I - l * pivot there, a value nothing reads (column
//    I of a row that is not step I's pivot row is dead after the multiplier;
//    the back substitution's unmasked update only feeds right-hand sides that
//    are dead as well);
//  * pattern: a row that holds its chain's column takes the member's bound
//    LU_BOUND.s (a superset of the pivot rows' patterns);
//  * row labels: the members' relabels at once, through a table of labels in
//    the half's buffer (lvl_relabel).
#pragma once

namespace hc {

constexpr int DPP_WAVE_SHL1 = 0x130, DPP_WAVE_SHR1 = 0x138;   // lane i takes lane i + 1 / i - 1 (GFX9)

// The row records' home (LU_ROWTAB, hc_lu_struct.hpp): 640 B of the workgroup's
// LDS, in the kernels that run the fused solve only.  lu_rowtab_fill runs once
// per workgroup, before a barrier that precedes the first solve.
__device__ __forceinline__ uint32_t *lu_rowtab_lds() {
    __shared__ uint32_t t[LU_REC_WORDS];
    return t;
}
__device__ __forceinline__ void lu_rowtab_fill(int tid) {
    if (tid < LU_REC_WORDS) lu_rowtab_lds()[tid] = LU_ROWTAB.w[tid];
}

// The members' relabels (:70-82): the pivot lane takes label I, the lane that
// held I takes the pivot lane's old label.  Over the whole solve the order is
// level by level (0, 1, 2, 5, 8..11, then 3, 4, 12, 15, ...), not 0..17, and the
// labels before step 18 are still exactly the sequential ones: a relabel
// exchanges the label values I and label(p_I), the pivot lanes p_I are chosen
// from the entries, never from the labels, and two relabels with different
// pivot lanes p, q commute -- both orders end with p at I, q at J, and the
// former holders of I and J (where they are not p or q) at the old labels of p
// and q; if p held J, the holder of I ends with q's old label either way.  So
// any order of the 18 relabels gives the same labels.
// A level's relabels at once: the labels' table is row[l].x of the half's buffer
// (unused until step 18), the label a row that holds label l takes next.  It is
// the identity (lu_level<0> writes it) but at the level's members, where the
// pivot lane of member I has written its own label to row[I].x before the
// level's broadcast.  Every row not pivoted yet takes the table's label for its
// own, and again while some row has reached another member's label: that
// member's pivot lane held the label the first member's holder was due (at
// level 0, row 5 can be member 0's pivot lane), which is what the relabels one
// after the other give.  No such row enters a cycle of the table: it is
// injective on the members, and a cycle's labels are all held by pivot lanes.
// Then the pivot lanes take their members.  A pivoted row keeps its label from
// there on, so a label a row holds is a member of the level or not in the
// table's changed part: the entries of earlier levels are never read again.
// (Until v10.11 the members' relabels ran one after the other, 8 instructions
// each with two v_readlane.)
template <int LV>
__device__ __forceinline__ void lvl_relabel(int &rowid, int mem, bool is_piv, unsigned long long live_m, const LUBuf &L) {
    const bool live = __builtin_amdgcn_inverse_ballot_w64(live_m);
    for (;;) {
        const int t = __float_as_int(L.row[rowid].x);
        rowid = live ? t : rowid;
        const bool again = live && ((lu_member_cols(LV) >> rowid) & 1u) != 0u;
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(again) == 0ull, 1)) break;
    }
    rowid = is_piv ? mem : rowid;
}
// The level's pairs of positions P, P + 1 (P even) of the compact row, inside
// the eligible rows' region: the slot pairs that hold a slot the level can
// change (lu_level_slots), then the pairs of columns 18.. that hold a column of
// LU_LEVELS.cols.  A slot pair travels through entries LVL_SLOT_J0 + P of the
// windows (entry 0 holds 1/pivot and the rhs), a pair of columns J, J + 1
// through entries J as in a sequential step.
constexpr int LVL_SLOT_J0 = 2;
template <int LV, int P>
__device__ __forceinline__ void lvl_groups(cf (&rA)[LU_COMPACT_W], const pf2 &l, cf *wrow, const cf *cw) {
    if constexpr (P < LU_COMPACT_W) {
        constexpr int C0 = lu_first_unfused_step() + P - LU_SLOTS;   // (P >= LU_SLOTS: the pair's first column)
        constexpr bool RUN = P < LU_SLOTS ? ((lu_level_slots(LV) >> P) & 3u) != 0u : ((LU_LEVELS.cols[LV] >> C0) & 3u) != 0u;
        if constexpr (RUN) {
            constexpr int J = P < LU_SLOTS ? LVL_SLOT_J0 + P : C0;
            grp_store<J, 2, P>(wrow, rA);
            wave_lds_sync();
            cf u[2];
            grp_load<J, 2>(cw, u);
            grp_update<J, 2, P>(rA, l, u);
            __builtin_amdgcn_sched_barrier(0);
        }
        lvl_groups<LV, P + 2>(rA, l, wrow, cw);
    }
}
constexpr int lvl_pairs(int lv) {   // the pairs lvl_groups<lv> runs
    int n = 0;
    for (int p = 0; p < LU_SLOTS; p += 2) n += ((lu_level_slots(lv) >> p) & 3u) != 0u;
    for (int j = lu_first_unfused_step(); j < NV; j += 2) n += ((LU_LEVELS.cols[lv] >> j) & 3u) != 0u;
    return n;
}
// returns false when the level met a rare condition (nothing is changed then)
template <int LV>
__device__ __forceinline__ bool lu_level(cf (&rA)[LU_COMPACT_W], cf &rB, int &rowid, uint32_t &pat, int r, int hb, PivF &my,
                                         LUBuf &L, cf *scr, unsigned long long &elig_m HC_LU_WORK_ARG) {
    constexpr int CNT = lu_level_count(LV), I0 = lu_level_member(LV, 0);
    constexpr uint32_t ROWS = LU_LEVELS.rows[LV];
    HC_ISA_MARK_I("lu_search", I0);
    const pf2 c = {rA[LV].x, rA[LV].y};   // the row's slot of the level (a zero outside the level's rows)
    const uint32_t rec = lu_rowtab_lds()[LV * LU_REC_ROWS + r];
    const float v = __builtin_fabsf(c.x) + __builtin_fabsf(c.y);          // :55
    pf2 oo_s;
    const pf2 reg_s = recip_fast(c, v, oo_s);
    const unsigned long long lv_elig = and_halves<ROWS>(elig_m);
    const bool elig = __builtin_amdgcn_inverse_ballot_w64(lv_elig);
    const int key = elig ? __float_as_int(v) : -1;
    // the maximum over the lane's triple: the two other rows are one and two
    // lanes up from its first row, one up and one down from the middle one, one
    // and two down from the last
    int mx;
    {
        const int u1 = dpp_i<DPP_WAVE_SHL1>(key), u2 = dpp_i<DPP_WAVE_SHL1>(u1);
        const int d1 = dpp_i<DPP_WAVE_SHR1>(key), d2 = dpp_i<DPP_WAVE_SHR1>(d1);
        const int a = rec >= LU_REC_UP ? u1 : d2;
        const int b = (int)rec < 0 ? u2 : d1;
        mx = max(key, max(a, b));
    }
    // ... and over the partner triple of a 6-row chain
    if constexpr (lu_partner_rows(LV, 0) != (1u << NV) - 1u) {
        const int pl = (int)((rec >> LU_REC_PARTNER_AT) & 31u) + hb;   // (a row without a partner: itself)
        mx = max(mx, __builtin_amdgcn_ds_bpermute(pl << 2, mx));
    }
    // one maximum per chain and half, every one in the fast reciprocal range
    // (a lane outside the level's rows matches its own key: masked off)
    const unsigned long long m = and_halves<ROWS>(__builtin_amdgcn_ballot_w64(key == mx));
    const unsigned long long bad = and_halves<ROWS>(__builtin_amdgcn_ballot_w64(!rcp_fast_bits(mx)));
    if (__builtin_expect((__builtin_popcountll(m) != 2 * CNT) | (bad != 0ull), 0)) return false;
    const bool is_piv = __builtin_amdgcn_inverse_ballot_w64(m);
    HC_ISA_MARK_I("lu_store", I0);
    const cf *cw = reinterpret_cast<const cf *>(reinterpret_cast<const char *>(scr) + (rec & ((1u << LU_REC_WIN_BITS) - 1u)));
    cf *wrow = is_piv ? const_cast<cf *>(cw) : scr;
    st4(&wrow[0], cmk(reg_s.x, reg_s.y), rB);
    const int mem = (int)((rec >> LU_REC_MEMBER_AT) & 31u);
    const uint32_t bnd = lu_rowtab_lds()[LU_REC_BOUND0 + mem];   // (read back with the broadcast below)
    // the labels' table (lvl_relabel)
    if constexpr (LV == 0) L.row[r].x = __int_as_float(r);
    if (is_piv) L.row[mem].x = __int_as_float(rowid);
    wave_lds_sync();
    HC_ISA_MARK_I("lu_rcp", I0);
    cf reg, sB0;
    ld4(&cw[0], reg, sB0);
    if (is_piv) my.oo = oo_s;
    asm volatile("" : "+v"(my.oo));
    lvl_relabel<LV>(rowid, mem, is_piv, elig_m & ~m, L);
    HC_ISA_MARK_I("lu_update", I0);
#ifdef HC_DIAG_LUWORK
    {   // the level's pairs x the eligible rows below the pivots (wave-uniform)
        constexpr int pairs = lvl_pairs(LV);
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
//  * select: its entry in the member's column, slot LV of the compact row, and
//    the member's position, from the row's record as in lu_level;
//  * divide: cuCdivf(b, pivot) with the factors it kept, once per level; the
//    owner's (the lane whose label is its member, which lvl_relabel gave the
//    member's pivot lane: its b is final, every position above 17 and every
//    ancestor has updated it) is x_I;
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
template <int LV>
__device__ __forceinline__ void lu_back_level(const cf (&rA)[LU_COMPACT_W], cf &rB, int rowid, const PivF &my, LUBuf &L,
                                              int r) {
    HC_ISA_MARK_I("lu_back_level", LV);
    const pf2 c = {rA[LV].x, rA[LV].y};
    const uint32_t rec = lu_rowtab_lds()[LV * LU_REC_ROWS + r];
    const int mem = (int)((rec >> LU_REC_MEMBER_AT) & 31u);   // (LU_REC_NO_MEMBER outside the level: no row's label)
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
__device__ __forceinline__ void lu_backward_fused(const cf (&rA)[LU_COMPACT_W], cf &rB, int rowid, const PivF &my, LUBuf &L, int r,
                                                  pf2 &res) {
    if constexpr (LV >= 0) {
        lu_back_level<LV>(rA, rB, rowid, my, L, r);
        lu_backward_fused<LV - 1>(rA, rB, rowid, my, L, r, res);
    } else {
        if (__builtin_amdgcn_inverse_ballot_w64(lu_both(lu_fused_steps()))) {
            const cf x = L.row[r];
            res = pf2{x.x, x.y};
        }
    }
}

}  // namespace hc
