// hc_lu_struct.hpp -- what the tracker LU (hc_lu.hpp) knows about this problem's
// Jacobian at compile time: the column groups of a pivot step, the symbolic
// fill-in bound and the group classes it gives, the span of each step's pivot
// search, the levels of independent pivot steps with their chains, the layout
// of the solve's LDS scratch, and the row forms of the solve modes (LuRowForm).
// Host-evaluable constants and their static_asserts only, no device code: the
// hc_lu_* test exports of hc_kernels.hip and k_prep_tables' structure check
// read nothing else of the LU.
#pragma once

#include <initializer_list>

#include "hc_device.hpp"

namespace hc {

// columns per skippable group: 2, where the LDS stores of dead columns are
// what a wider group costs, and what the 16-B scratch windows hold
// (profiles/r3u_ab_oo_rz_gs_chunk2.jsonl: 33.55 -> 31.78 ms per config-2
// launch).  The abort kernel used groups of 4 in two loops until round 5, for
// its lone-wave latency; groups of 2 in the eligible rows' region are as fast
// there, and its latency mode faster (profiles/r5j_ttfp_abort_lu_variants.jsonl,
// r5n_ttfp.jsonl)
constexpr int LU_CHUNK = 2;

// Column groups of step I: a leading single column when I+1 is odd, then
// groups of LU_CHUNK (even) columns.  The pivot lanes write, and the update reads,
// exactly these groups.
struct LuChunks {
    static constexpr int single(int I) { return ((I + 1) & 1) && (I + 1 < NV) ? 1 : 0; }
    static constexpr int start(int I, int k) { return k < single(I) ? I + 1 : I + 1 + single(I) + (k - single(I)) * LU_CHUNK; }
    static constexpr int len(int I, int k) {
        return k < single(I) ? 1 : ((NV - start(I, k)) < LU_CHUNK ? (NV - start(I, k)) : LU_CHUNK);
    }
    static constexpr int count(int I) { return single(I) + (NV - (I + 1 + single(I)) + LU_CHUNK - 1) / LU_CHUNK; }
    static constexpr uint32_t mask(int I, int k) { return ((1u << len(I, k)) - 1u) << start(I, k); }
};

// The tracker's column groups by class (round 5).  The sparse LU tests a
// group live when a pivot row of the wave may be non-zero there; for this
// problem's Jacobian most outcomes are fixed in advance:
//  * dead: the symbolic fill-in bound -- at step I every row pattern is within
//    the row's bound cur[r], the pivot rows' within S_I = OR of the bounds of
//    the rows that may hold column I, and a row that may hold column I grows
//    by at most S_I -- has no column of the group: the test can never pass
//    (101 of the 225 groups of a solve);
//  * always: live in every one of the 1.2 M sampled wave-solves of datasets
//    000/001/002 (profiles/r5lv_live.jsonl; 16 of the 40 provably, from the
//    rows that must hold column I): no test, the update runs.  Running a group
//    that happens to be dead is exact: the pivot rows hold zeros there, and a
//    - l * 0 == a (up to the sign of a zero; l is finite in the sparse solve);
//  * tested: the other 84.
// Only the tracker's solves (STRUCT) use the classes: k_tables checks that the
// loaded problem's structural patterns lie within LU_STRUCT_PAT; the component
// LU (k_cgesv) takes any matrix and tests every group.
constexpr uint32_t LU_STRUCT_PAT[NV] = {
    0x7040004u, 0x7080004u, 0x7100004u, 0x7040009u, 0x7080009u, 0x7100009u, 0x7040012u, 0x7080012u,
    0x7100012u, 0x38200020u, 0x38400020u, 0x38800020u, 0x38200041u, 0x38400041u, 0x38800041u, 0x38200082u,
    0x38400082u, 0x38800082u, 0x7003100u, 0x7003100u, 0x7001100u, 0x7018400u, 0x7018400u, 0x7008400u,
    0x38005200u, 0x38005200u, 0x38001200u, 0x38028800u, 0x38028800u, 0x38008800u};
constexpr uint16_t LU_ALWAYS[NV] = {0x2000, 0x1000, 0x1800, 0xc00, 0xc00, 0xd00, 0xc00, 0x600, 0x304, 0x302,
                                    0x184,  0x182,  0x80,   0x60,  0xc0,  0x21,  0x30,  0x30,  0x18,  0,
                                    0,      0,      0,      0,     0,     0,     0,     0,     0,     0};
struct LuBound { uint32_t s[NV], cand[NV]; };   // cand[I]: the rows that may hold column I at step I
constexpr LuBound lu_struct_bound() {
    LuBound b{};
    uint32_t cur[NV] = {};
    for (int r = 0; r < NV; r++) cur[r] = LU_STRUCT_PAT[r];
    for (int i = 0; i < NV; i++) {
        const uint32_t above = (0xFFFFFFFFu << (i + 1)) & ((1u << NV) - 1u);
        uint32_t u = 0u;
        for (int r = 0; r < NV; r++)
            if ((cur[r] >> i) & 1u) { u |= cur[r]; b.cand[i] |= 1u << r; }
        b.s[i] = u & above;
        for (int r = 0; r < NV; r++)
            if ((cur[r] >> i) & 1u) cur[r] |= u & above;
    }
    return b;
}
constexpr LuBound LU_BOUND = lu_struct_bound();
enum : int { GRP_TESTED = 0, GRP_DEAD = 1, GRP_ALWAYS = 2 };
constexpr int lu_group_class(int I, int K) {
    return (LU_BOUND.s[I] & LuChunks::mask(I, K)) == 0u ? GRP_DEAD
           : ((LU_ALWAYS[I] >> K) & 1u)                     ? GRP_ALWAYS
                                                              : GRP_TESTED;
}
// The pivot search of the tracker's step I need only reduce over the lanes
// (rows) that may hold column I: every other row's entry is an exact zero.
// Span of the DPP reduction that covers them: 1 a quad (two quad_perm
// steps), 2 a half-row (+ row_half_mirror), 3 a 16-lane row (+ row_mirror),
// 4 the half-wave (+ v_permlane16_swap).  Steps 0..17 need 1 to 3.
constexpr int lu_search_span(int I) {
    const uint32_t c = LU_BOUND.cand[I];
    if (c == 0u) return 4;
    int lo = 0, hi = 31;
    while (!((c >> lo) & 1u)) lo++;
    while (!((c >> hi) & 1u)) hi--;
    return (lo >> 2) == (hi >> 2) ? 1 : (lo >> 3) == (hi >> 3) ? 2 : (lo >> 4) == (hi >> 4) ? 3 : 4;
}
constexpr bool lu_classes_consistent() {   // no measured-always group is provably dead
    for (int i = 0; i < NV - 1; i++)
        for (int k = 0; k < LuChunks::count(i); k++)
            if (((LU_ALWAYS[i] >> k) & 1u) && (LU_BOUND.s[i] & LuChunks::mask(i, k)) == 0u) return false;
    return true;
}
static_assert(lu_classes_consistent(), "LU_ALWAYS names a provably dead group");

// Independent pivot steps.  A step reads and writes only its candidate rows
// (cand[I]: every other row holds an exact zero in column I, so it neither
// wins the search nor takes a multiple of the pivot row), so two steps whose
// candidate sets are disjoint read nothing the other writes and commute
// exactly.  level[j] = 1 + max level[i] over the earlier steps i whose
// candidates meet step j's (0 without one): the steps of one level are
// pairwise independent, and a level's steps come after every step of the
// levels below that they depend on.  A step is fusable when its candidates are
// one or two triples of adjacent rows (at most LU_FUSE_ROWS rows: what a
// chain-segmented pivot search covers); a level's fusable steps can run as one
// step.  For this problem they are steps 0..17 in four levels -- a forest of
// depth 4 that the forward elimination walks as 18 serial steps; step 18 is
// on level 3 as well but reduces over 15 rows and stays sequential with 19..29.
constexpr int LU_FUSE_ROWS = 6;
struct LuLevels {
    int level[NV];          // level of step I
    int nlevels;            // levels that hold a fusable step (they are 0 .. nlevels - 1)
    uint32_t fused[NV];     // fused[l]: the fusable steps of level l (bit I)
    uint32_t rows[NV];      // rows[l]: the rows those steps work on (bit r)
    uint32_t cols[NV];      // cols[l]: the columns they can touch, OR of LU_BOUND.s
};
constexpr int lu_popcount(uint32_t x) { int n = 0; for (; x; x &= x - 1u) n++; return n; }
constexpr bool lu_step_fusable(int I) {
    const int n = lu_popcount(LU_BOUND.cand[I]);
    return n > 0 && n <= LU_FUSE_ROWS;
}
constexpr LuLevels lu_struct_levels() {
    LuLevels v{};
    for (int j = 0; j < NV; j++) {
        int l = 0;
        for (int i = 0; i < j; i++)
            if ((LU_BOUND.cand[i] & LU_BOUND.cand[j]) != 0u && v.level[i] + 1 > l) l = v.level[i] + 1;
        v.level[j] = l;
        if (lu_step_fusable(j)) {
            v.fused[l] |= 1u << j;
            v.rows[l] |= LU_BOUND.cand[j];
            v.cols[l] |= LU_BOUND.s[j];
            if (l + 1 > v.nlevels) v.nlevels = l + 1;
        }
    }
    return v;
}
constexpr LuLevels LU_LEVELS = lu_struct_levels();
constexpr bool lu_levels_disjoint() {   // the members of a level have pairwise disjoint candidates
    for (int i = 0; i < NV; i++)
        for (int j = i + 1; j < NV; j++)
            if (LU_LEVELS.level[i] == LU_LEVELS.level[j] && (LU_BOUND.cand[i] & LU_BOUND.cand[j]) != 0u) return false;
    return true;
}
constexpr bool lu_levels_ordered() {   // a fused step's dependencies are fused steps of lower levels
    for (int j = 0; j < NV; j++)
        for (int i = 0; i < j; i++)
            if (lu_step_fusable(j) && (LU_BOUND.cand[i] & LU_BOUND.cand[j]) != 0u &&
                !(lu_step_fusable(i) && LU_LEVELS.level[i] < LU_LEVELS.level[j])) return false;
    return true;
}
// The back substitution of the fused positions, level by level (lu_back_level,
// hc_lu_levels.hpp).  The row pivoted at a fused step I lies within LU_BOUND.s[I]
// above the diagonal, and a column J of that bound with J <= 17 is an ancestor
// of I: every candidate row of I is a candidate row of J, on a higher level.
// So x_J reaches every row it can change through the lanes of cand[J] alone.
constexpr bool lu_back_chains_nested() {
    for (int i = 0; i < NV; i++)
        for (int j = i + 1; j < NV; j++)
            if (lu_step_fusable(i) && lu_step_fusable(j) && ((LU_BOUND.s[i] >> j) & 1u) &&
                !((LU_BOUND.cand[i] & ~LU_BOUND.cand[j]) == 0u && LU_LEVELS.level[i] < LU_LEVELS.level[j])) return false;
    return true;
}
// Along the fused steps a row is a candidate of -- one per level
// (lu_levels_disjoint) -- the column rises with the level: walking the levels
// downwards gives a row its non-zero updates in the reference's descending order.
constexpr bool lu_back_order_kept() {
    for (int r = 0; r < NV; r++) {
        int last = -1;
        for (int l = 0; l < NV; l++)
            for (int i = 0; i < NV; i++)
                if (lu_step_fusable(i) && LU_LEVELS.level[i] == l && ((LU_BOUND.cand[i] >> r) & 1u)) {
                    if (i <= last) return false;
                    last = i;
                }
    }
    return true;
}
constexpr uint32_t lu_fused_steps() {
    uint32_t m = 0u;
    for (int l = 0; l < LU_LEVELS.nlevels; l++) m |= LU_LEVELS.fused[l];
    return m;
}
// the step the sequential elimination takes over at, once every level has run
constexpr int lu_first_unfused_step() {
    int i = 0;
    while (i < NV && ((lu_fused_steps() >> i) & 1u)) i++;
    return i;
}
constexpr uint32_t lu_bits(std::initializer_list<int> v) {
    uint32_t m = 0u;
    for (int b : v) m |= 1u << b;
    return m;
}
static_assert(lu_levels_disjoint(), "two steps of one level share a candidate row");
static_assert(lu_levels_ordered(), "a fused step depends on a step outside the lower fused levels");
static_assert(lu_back_chains_nested(), "a fused pivot row can hold a fused column outside its chain's ancestors");
static_assert(lu_back_order_kept(), "a row's ancestors do not rise in column with the level");
static_assert(lu_fused_steps() == (1u << 18) - 1u, "the fused levels cover exactly steps 0..17");
static_assert(LU_LEVELS.nlevels == 4 && LU_LEVELS.fused[0] == lu_bits({0, 1, 2, 5, 8, 9, 10, 11}) &&
              LU_LEVELS.fused[1] == lu_bits({3, 4, 12, 15}) && LU_LEVELS.fused[2] == lu_bits({6, 7, 13, 16}) &&
              LU_LEVELS.fused[3] == lu_bits({14, 17}), "the levels of DESIGN.md §3.5");
static_assert(LU_LEVELS.rows[0] == (1u << NV) - 1u && LU_LEVELS.rows[1] == (LU_LEVELS.rows[0] & ~lu_bits({0, 1, 2, 9, 10, 11})) &&
              LU_LEVELS.rows[2] == LU_LEVELS.rows[1] && LU_LEVELS.rows[3] == (0x3FFC0000u & LU_LEVELS.rows[0]),
              "the rows the levels work on");

// The chains of a level (hc_lu_levels.hpp): the candidate sets of its fusable
// steps, each one or two lane triples.
constexpr int lu_level_count(int lv) { return lu_popcount(LU_LEVELS.fused[lv]); }
constexpr int lu_level_member(int lv, int k) {   // the k-th fusable step of level lv
    for (int i = 0; i < NV; i++)
        if ((LU_LEVELS.fused[lv] >> i) & 1u) {
            if (k == 0) return i;
            k--;
        }
    return -1;
}
constexpr int lu_max_level_count() {
    int n = 0;
    for (int l = 0; l < LU_LEVELS.nlevels; l++)
        if (lu_level_count(l) > n) n = lu_level_count(l);
    return n;
}
// rows whose chain partner triple is `off` lanes away (0: rows of 3-row chains)
constexpr int lu_partner_off(int lv, int row) {
    for (int k = 0; k < lu_level_count(lv); k++) {
        const uint32_t c = LU_BOUND.cand[lu_level_member(lv, k)];
        if (!((c >> row) & 1u) || lu_popcount(c) <= 3) continue;
        int lo = 0, hi = 31;
        while (!((c >> lo) & 1u)) lo++;
        while (!((c >> hi) & 1u)) hi--;
        return row < lo + 3 ? (hi - 2) - lo : lo - (hi - 2);
    }
    return 0;
}
constexpr uint32_t lu_partner_rows(int lv, int off) {
    uint32_t m = 0u;
    for (int r = 0; r < NV; r++)
        if (lu_partner_off(lv, r) == off) m |= 1u << r;
    return m;
}
constexpr bool lu_chains_are_triples() {   // every fusable candidate set: one or two aligned lane triples
    for (int i = 0; i < NV; i++) {
        if (!lu_step_fusable(i)) continue;
        uint32_t c = LU_BOUND.cand[i], t = 0u;
        for (int q = 0; q < NV; q += 3)
            if (((c >> q) & 7u) == 7u) t |= 7u << q;
        if (t != c) return false;
    }
    return true;
}
static_assert(lu_chains_are_triples(), "a fusable step's candidates are not whole lane triples");
constexpr uint32_t lu_member_cols(int lv) { return LU_LEVELS.fused[lv]; }   // bit I: step I pivots column I
constexpr unsigned long long lu_both(uint32_t m) { return (unsigned long long)m | ((unsigned long long)m << 32); }
constexpr uint32_t LU_TRI0 = 0x09249249u, LU_TRI1 = LU_TRI0 << 1, LU_TRI2 = LU_TRI0 << 2;   // rows 3q, 3q + 1, 3q + 2 (< 30)

// The solve's LDS scratch, per half, in cf entries (16-B aligned; the caller's
// data there is lost).  The sparse solve with groups of 2 overwrites
// LU_SCRATCH_CF entries: the store windows of the eligible rows (row r writes
// column group J at scratch[2r + J]).  The fused levels need
// LU_SCRATCH_FUSED_CF: chain k of a level owns the pivot-row window
// scratch[LU_CHAIN_WIN0 + 2k ..], behind the rows' windows.
constexpr int LU_SCRATCH_CF = 2 * 31 + 32;   // 94: lane r's window scratch[2r .. 2r + 31]
constexpr int LU_CHAIN_WIN0 = LU_SCRATCH_CF;
constexpr int LU_SCRATCH_FUSED_CF = LU_CHAIN_WIN0 + 2 * (lu_max_level_count() - 1) + 32;

// What a row is to a fused level: one word per level and row, and the fill-in
// bound of each fused step (hc_lu_levels.hpp reads them from LDS, a ds_read_b32
// each, where it built the same values with selects on static lane masks).
// The headline kernel's five workgroups per CU leave less than 1 KB of LDS (an
// 8-byte record per level and row, 1 024 B, cost the fifth workgroup): the
// bound, which is a member's and not a row's, stands once per member,
// LU_REC_WORDS words in all.  A row's
// word, from bit 0:
//   10 bits  the byte offset of its chain's window from the row's own window,
//            8 * (LU_CHAIN_WIN0 + 2k - 2r)
//    5 bits  the member: the pivot step of its chain
//    5 bits  the row whose maximum it takes with ds_bpermute: the same place in
//            the other triple of a 6-row chain
//    4 bits  k, the chain's number at the level
//   bit 30   the row is not the last of its triple (it takes the row above's key)
//   bit 31   the row is the first of its triple
// A row outside the level's rows, and the pad rows 30 and 31 at every level, hold
// neutral values: its own window, member LU_REC_NO_MEMBER (whose bound is
// empty), itself as the partner, chain LU_REC_NO_CHAIN.
struct LuRowRec { uint32_t bound, word; };
constexpr int LU_REC_WIN_BITS = 10, LU_REC_MEMBER_AT = 10, LU_REC_PARTNER_AT = 15, LU_REC_CHAIN_AT = 20;
constexpr uint32_t LU_REC_UP = 1u << 30, LU_REC_FIRST = 1u << 31;
constexpr int LU_REC_NO_MEMBER = 31, LU_REC_NO_CHAIN = 15;
constexpr int LU_REC_ROWS = 32, LU_REC_LEVELS = 4;
constexpr int lu_row_chain(int lv, int row) {   // the chain of the level that holds the row, -1 without one
    if (row >= NV) return -1;
    for (int k = 0; k < lu_level_count(lv); k++)
        if ((LU_BOUND.cand[lu_level_member(lv, k)] >> row) & 1u) return k;
    return -1;
}
constexpr LuRowRec lu_row_record(int lv, int row) {
    const int k = lu_row_chain(lv, row);
    const uint32_t place = (row % 3 == 0 ? LU_REC_FIRST : 0u) | (row % 3 != 2 ? LU_REC_UP : 0u);
    if (k < 0)
        return LuRowRec{0u, place | (uint32_t)LU_REC_NO_CHAIN << LU_REC_CHAIN_AT | (uint32_t)row << LU_REC_PARTNER_AT |
                                (uint32_t)LU_REC_NO_MEMBER << LU_REC_MEMBER_AT};
    const int I = lu_level_member(lv, k);
    return LuRowRec{LU_BOUND.s[I], place | (uint32_t)k << LU_REC_CHAIN_AT |
                                       (uint32_t)(row + lu_partner_off(lv, row)) << LU_REC_PARTNER_AT |
                                       (uint32_t)I << LU_REC_MEMBER_AT | (uint32_t)(8 * (LU_CHAIN_WIN0 + 2 * k - 2 * row))};
}
// the rows' words by level, then the bounds by member (0 .. LU_REC_NO_MEMBER)
constexpr int LU_REC_BOUND0 = LU_REC_LEVELS * LU_REC_ROWS, LU_REC_WORDS = LU_REC_BOUND0 + LU_REC_NO_MEMBER + 1;
struct LuRowTab { uint32_t w[LU_REC_WORDS]; };
constexpr LuRowTab lu_row_table() {
    LuRowTab t{};
    for (int lv = 0; lv < LU_REC_LEVELS; lv++)
        for (int r = 0; r < LU_REC_ROWS; r++) {
            const LuRowRec rec = lu_row_record(lv, r);
            t.w[lv * LU_REC_ROWS + r] = rec.word;
            t.w[LU_REC_BOUND0 + (int)((rec.word >> LU_REC_MEMBER_AT) & 31u)] = rec.bound;
        }
    return t;
}
constexpr LuRowTab LU_ROWTAB = lu_row_table();
constexpr bool lu_row_fields_fit() {
    for (int lv = 0; lv < LU_REC_LEVELS; lv++)
        for (int r = 0; r < NV; r++) {
            const int k = lu_row_chain(lv, r), p = r + lu_partner_off(lv, r);
            if (k < 0) continue;
            const int win = 8 * (LU_CHAIN_WIN0 + 2 * k - 2 * r);
            if (win <= 0 || win >= (1 << LU_REC_WIN_BITS) || k >= LU_REC_NO_CHAIN || p < 0 || p >= NV) return false;
            if (lu_level_member(lv, k) >= LU_REC_NO_MEMBER || (LU_BOUND.s[lu_level_member(lv, k)] >> NV) != 0u) return false;
        }
    return true;
}
static_assert(LU_LEVELS.nlevels == LU_REC_LEVELS && lu_row_fields_fit(), "a field of the row records overflows");
// 31 120 B of the headline kernel's workgroup + the table: at 32 144 B five
// workgroups no longer share a CU (measured), at 31 760 B they do
static_assert(LU_REC_WORDS * sizeof(uint32_t) <= 640, "a larger row table may cost the headline kernel its fifth workgroup per CU: measure");

// The compact row of the fused solve (lu_solve<..., FUSE>).  Bit c < 18 of a
// row's bound can only be set before step c, so a row's bound holds column c
// exactly when the row is a candidate of step c; the candidates of a level's
// steps are disjoint, so a row holds at most one column below
// lu_first_unfused_step() per level: the member its record names.  In the
// other low columns it carries an exact zero through the whole solve.  The
// fused solve therefore keeps a row in LU_COMPACT_W positions: position L <
// LU_SLOTS is the row's level-L column (its "slot"; a zero where it has none),
// the positions behind them are the columns from lu_first_unfused_step() on
// (from an even position: their column pairs stay pairs).  The rows of a chain
// share their ancestors, so above the chain's level their slots name the same
// columns, and a pivot row's slot pair means to every row that takes it what
// it means to the pivot row.
constexpr int LU_SLOTS = LU_REC_LEVELS;
constexpr int LU_COMPACT_W = LU_SLOTS + NV - lu_first_unfused_step();
constexpr int lu_slot_col(int row, int lv) {   // the column in slot lv of the row, -1 without one
    const int k = lu_row_chain(lv, row);
    return k < 0 ? -1 : lu_level_member(lv, k);
}
constexpr int lu_compact_col(int row, int pos) {   // the column at a position of the row's compact form, -1: none
    return pos < LU_SLOTS ? lu_slot_col(row, pos) : lu_first_unfused_step() + pos - LU_SLOTS;
}
constexpr uint32_t lu_row_bound(int row) {   // everything the row can hold during the solve (lu_struct_bound's cur[row] at its end)
    uint32_t cur[NV] = {};
    for (int r = 0; r < NV; r++) cur[r] = LU_STRUCT_PAT[r];
    for (int i = 0; i < NV; i++)
        for (int r = 0; r < NV; r++)
            if ((cur[r] >> i) & 1u) cur[r] |= LU_BOUND.s[i];
    return cur[row];
}
constexpr bool lu_slots_hold_the_bound() {   // every low column of a row's bound: a fused step, the one in the slot of its level
    for (int r = 0; r < NV; r++) {
        const uint32_t low = lu_row_bound(r) & ((1u << lu_first_unfused_step()) - 1u);
        int per_level[LU_SLOTS] = {};
        for (int c = 0; c < lu_first_unfused_step(); c++) {
            if (!((low >> c) & 1u)) continue;
            const int lv = LU_LEVELS.level[c];
            if (!lu_step_fusable(c) || lv >= LU_SLOTS || ++per_level[lv] > 1 || lu_slot_col(r, lv) != c) return false;
        }
        for (int lv = 0; lv < LU_SLOTS; lv++)   // and a slot's column is in the bound
            if (lu_slot_col(r, lv) >= 0 && !((low >> lu_slot_col(r, lv)) & 1u)) return false;
    }
    return true;
}
static_assert(lu_slots_hold_the_bound(), "a row's bound holds a low column outside its level's slot");
static_assert(LU_SLOTS % 2 == 0 && lu_first_unfused_step() % 2 == 0 && LU_COMPACT_W == 16,
              "the columns behind the slots keep their pairs; 4 slots and columns 18..29");
// the slots a level's update can change: those of the columns of its members' bounds
constexpr uint32_t lu_level_slots(int lv) {
    uint32_t m = 0u;
    for (int c = 0; c < lu_first_unfused_step(); c++)
        if ((LU_LEVELS.cols[lv] >> c) & 1u) m |= 1u << LU_LEVELS.level[c];
    return m;
}
static_assert(lu_level_slots(0) == 0xEu && lu_level_slots(1) == 0xCu && lu_level_slots(2) == 0x8u && lu_level_slots(3) == 0u,
              "a level changes the slots above its own only");
// The row form of a solve mode: the compact one for the fused solve, else the
// 30 columns in place.  pos(c): the register position of column c >=
// lu_first_unfused_step() (a low column's position is its level, and depends
// on the row); W: the row's width.
template <bool COMPACT>
struct LuRowForm {
    static constexpr int W = COMPACT ? LU_COMPACT_W : NV;
    static constexpr int pos(int c) { return COMPACT ? c - (lu_first_unfused_step() - LU_SLOTS) : c; }
};

}  // namespace hc
