// The body of k_prep_tables (hc_prep.hpp: P2C = false, pa.U the unified table)
// and of k_prep_tables_p2c (hc_p2c.hpp: P2C = true, pa.U the dH/dx table, D_in
// the dH/dt table), included inside each like hc_track_body.inc: a function
// template inlined into the two kernels compiles k_prep_tables to other code.
    const int32_t *__restrict__ U = pa.U;
    Workspace *ws = pa.ws;
    EvalTables *T = &ws->tab;
    __shared__ int s_len[32];
    __shared__ int s_bad;
    __shared__ int s_nostruct;   // the dH/dx structure is not within the tracker LU's
    __shared__ unsigned long long s_h[PREP_THREADS];
    __shared__ unsigned s_cleared, s_dlo, s_dhi;
    __shared__ int s_valid;
    const int tid = threadIdx.x;
    {
        // the table's hash (a sum, so any load order gives it): 16-B loads when
        // the caller's table is 16-B aligned (the per-launch check took 40 us
        // with one int per load, a fifth of the launch overhead; round 6)
        unsigned long long h = 0;
        if constexpr (P2C) {
            for (int i = tid; i < P2C_HX_SIZE; i += PREP_THREADS)
                h += mix64(((unsigned long long)i << 32) | (unsigned)U[i]);
            for (int i = tid; i < P2C_HT_SIZE; i += PREP_THREADS)
                h += mix64(((unsigned long long)(P2C_HX_SIZE + i) << 32) | (unsigned)D_in[i]);
        } else if (((uintptr_t)U & 15u) == 0u) {
            const int4 *U4 = reinterpret_cast<const int4 *>(U);
            static_assert((HX_SIZE + HT_SIZE) % 4 == 0, "whole int4 words");
#pragma unroll 4
            for (int i = tid; i < (HX_SIZE + HT_SIZE) / 4; i += PREP_THREADS) {
                const int4 v = U4[i];
                const unsigned long long b = (unsigned long long)(4 * i) << 32;
                h += mix64(b | (unsigned)v.x) + mix64((b + (1ull << 32)) | (unsigned)v.y) +
                     mix64((b + (2ull << 32)) | (unsigned)v.z) + mix64((b + (3ull << 32)) | (unsigned)v.w);
            }
        } else {
#pragma unroll 8
            for (int i = tid; i < HX_SIZE + HT_SIZE; i += PREP_THREADS)
                h += mix64(((unsigned long long)i << 32) | (unsigned)U[i]);
        }
        s_h[tid] = h;
    }
    if (tid == 0) {
        // the launch's control block (queue, status, flag, timestamps, diagnostics)
        unsigned *cb = reinterpret_cast<unsigned *>(ws);
        for (int q = 0; q < 16; q++) cb[q] = 0u;
        s_bad = 0;
        s_nostruct = 0;
        if (pa.found_in) {
            const bool peer = pa.peer_found &&
                              __hip_atomic_load(pa.peer_found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u;
            ws->found = (pa.found_in[0] || peer) ? 1u : 0u;
        }
        const bool known = pa.rq && pa.rq[RQ_MAGIC] == RQ_MAGIC_VALUE;
        s_cleared = known ? pa.rq[RQ_CLEARED] : 0u;
        s_dlo = known ? pa.rq[RQ_DLO] : 0u;
        s_dhi = known ? pa.rq[RQ_DHI] : 0u;
    }
    __syncthreads();
    for (int w = PREP_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) s_h[tid] += s_h[tid + w];
        __syncthreads();
    }
    const unsigned long long src_hash = s_h[0] + (P2C ? P2C_HASH_TAG : 0ull);
    if (pa.rq) {
        // entries never cleared, and cleared entries an earlier launch's
        // suspend blocks overwrote (the dirty range), inside this launch's ring
        for (unsigned e = s_cleared + tid; e < pa.ring_cap; e += PREP_THREADS) pa.ring[e] = 0ull;
        const unsigned dhi = min(s_dhi, min(s_cleared, pa.ring_cap));
        for (unsigned e = s_dlo + tid; e < dhi; e += PREP_THREADS) pa.ring[e] = 0ull;
    }
    if (tid == 0) s_valid = (T->magic == TAB_MAGIC && T->src_hash == src_hash && T->status == 0) ? 1 : 0;
    __syncthreads();
    if (pa.rq && tid == 0) {
        unsigned *rq = pa.rq;
        rq[RQ_HEAD] = 0u;
        rq[RQ_TAIL] = 0u;
        rq[RQ_AVAIL] = 0u;
        const unsigned e = (rq[RQ_MAGIC] == RQ_MAGIC_VALUE) ? rq[RQ_EPOCH] + 1u : 1u;
        rq[RQ_EPOCH] = e ? e : 1u;
        // this launch's suspend blocks start right after its ring: the cleared
        // entries they may overwrite join the dirty range (one interval that
        // covers every such range not re-zeroed yet)
        const unsigned cleared = max(s_cleared, pa.ring_cap);
        unsigned lo = max(s_dlo, pa.ring_cap), hi = s_dhi;                 // what this launch did not re-zero
        const unsigned s0 = pa.susp_entry0, s1 = min(cleared, pa.susp_entry1);   // this launch's blocks
        if (s0 < s1) {
            const bool had = lo < hi;
            lo = had ? min(lo, s0) : s0;
            hi = had ? max(hi, s1) : s1;
        }
        if (hi > cleared) hi = cleared;
        if (lo >= hi) lo = hi = 0u;
        rq[RQ_CLEARED] = cleared;
        rq[RQ_DLO] = lo;
        rq[RQ_DHI] = hi;
        rq[RQ_MAGIC] = RQ_MAGIC_VALUE;
    }
    if (s_valid) return;   // tables built from this index table already
    const int r = tid;
    // dH/dx: entries bin-packed over the 32 lanes (hc_eval.hpp).  A: terms per
    // entry (rows in parallel); B: one thread places the entries, largest first,
    // each in the smallest-capacity slot class with a free lane (ties: lower
    // row, then lower column), numbering the entries 0..169 in placement order
    // (their place in the slot's packed entry block), and lists the distinct
    // prefix triples (c, a, b) of the dH/dx and H terms and pairs (a, b) of the
    // dH/dt terms (padding first: (0, 33, 33) and (33, 33)); C: rows write their
    // terms' words; D: the prefix build jobs.
    __shared__ uint8_t s_cnt[NV][NV];
    __shared__ int s_htn[32];             // dH/dt | H terms of row r (0 for lanes 30, 31)
    __shared__ uint8_t s_place[NV][NV];   // lane << 3 | slot, 0xFF: structural zero
    __shared__ uint16_t s_eoff[NV][NV];   // SlotLDS byte offset of entry (row, column)
    __shared__ uint32_t s_dst[HX_NSLOT / 2][32];
    __shared__ uint32_t s_tri[TP_CAP];    // (uint8)c | a << 8 | b << 16
    __shared__ uint32_t s_pair[QP_CAP];   // a | b << 8
    __shared__ int s_ntri, s_npair;
    __shared__ uint32_t s_th[256], s_ph[128];   // hash sets of the prefix keys (+ 1)
    // slot capacities and starts as locals (a runtime index into the
    // namespace-scope constexpr table does not reach device memory)
    int cap[HX_NSLOT], start[HX_NSLOT];
    for (int s2 = 0, acc2 = 0; s2 < HX_NSLOT; s2++) {
        cap[s2] = HX_GCAP[0] * (s2 == 0) + HX_GCAP[1] * (s2 == 1) + HX_GCAP[2] * (s2 == 2) +
                  HX_GCAP[3] * (s2 == 3) + HX_GCAP[4] * (s2 == 4) + HX_GCAP[5] * (s2 == 5);
        start[s2] = acc2;
        acc2 += cap[s2];
    }
    const int32_t *D = P2C ? D_in : U + HX_SIZE;
    // part p of dH/dx term j of entry (row, column) and of dH/dt | H term j of a row,
    // as the PH parts (c, a, b, x_u, x_v[, x_w]); a P2C coefficient outside 0..37
    // reads as a = -1, which C rejects
    auto p2c_part = [](const int32_t *e, int part) -> int {
        if (part == 0) return e[0];
        if (part >= 3) return e[part - 1];
        const int k = e[1];
        if (k < 0 || k >= P2C_NK) return -1;
        return part == 1 ? (k & 31) : (k >> 5);
    };
    auto hxp = [&](int c, int j, int part, int row) -> int {
        return p2c_part(U + ((row * NV + c) * HX_TERMS + j) * P2C_HX_PARTS, part);
    };
    auto htp = [&](int j, int part, int row) -> int {
        return p2c_part(D + (row * HT_TERMS + j) * P2C_HT_PARTS, part);
    };
    // (the PH reads below stay as they were written: k_prep_tables keeps its code)
    if (r < NV)
        for (int c = 0; c < NV; c++) {
            int n = 0;
            for (int j = 0; j < HX_TERMS; j++)
                if ((P2C ? hxp(c, j, 0, r) : U[(c * HX_TERMS + j) * HX_PARTS * NV + r]) != 0) n++;
            s_cnt[r][c] = (uint8_t)n;
            s_place[r][c] = 0xFFu;
            s_eoff[r][c] = (uint16_t)SLOT_OFF_ENTZERO;
        }
    // the distinct prefix keys of all terms, collected by every thread into LDS
    // hash sets (open addressing, atomicCAS; key + 1, 0 = empty); a term outside
    // the index ranges is left out here and rejected in C
    for (int h = tid; h < 256; h += PREP_THREADS) s_th[h] = 0u;
    for (int h = tid; h < 128; h += PREP_THREADS) s_ph[h] = 0u;
    __syncthreads();
    {
        auto hins = [&](uint32_t *tab, uint32_t mask, uint32_t key) {
            uint32_t h = (key * 2654435761u) >> 20 & mask;
            for (uint32_t probe = 0; probe <= mask; probe++) {
                const uint32_t old = atomicCAS(&tab[h], 0u, key + 1u);
                if (old == 0u || old == key + 1u) return;
                h = (h + 1u) & mask;
            }
            s_bad = 1;   // more distinct keys than the set holds
        };
        for (int i = tid; i < HX_SIZE / HX_PARTS; i += PREP_THREADS) {   // (column, term, row) of dH/dx
            const int base = (i / NV) * HX_PARTS * NV + i % NV;
            const int pc = i / NV / HX_TERMS, pj = i / NV % HX_TERMS, pr = i % NV;   // P2C: (column, term, row)
            const int co = P2C ? hxp(pc, pj, 0, pr) : U[base];
            if (co == 0) continue;
            const int a = P2C ? hxp(pc, pj, 1, pr) : U[base + NV], b = P2C ? hxp(pc, pj, 2, pr) : U[base + 2 * NV];
            if (co >= -128 && co <= 127 && a >= 0 && a < NPP && b >= 0 && b < NPP)
                hins(s_th, 255u, ((uint32_t)co & 0xFFu) | (uint32_t)a << 8 | (uint32_t)b << 16);
        }
        for (int i = tid; i < HT_SIZE / HT_PARTS; i += PREP_THREADS) {
            const int base = (i / NV) * HT_PARTS * NV + i % NV;
            const int co = P2C ? htp(i / NV, 0, i % NV) : D[base];
            if (co == 0) continue;
            const int a = P2C ? htp(i / NV, 1, i % NV) : D[base + NV], b = P2C ? htp(i / NV, 2, i % NV) : D[base + 2 * NV];
            if (co >= -128 && co <= 127 && a >= 0 && a < NPP && b >= 0 && b < NPP) {
                hins(s_th, 255u, ((uint32_t)co & 0xFFu) | (uint32_t)a << 8 | (uint32_t)b << 16);
                hins(s_ph, 127u, (uint32_t)a | (uint32_t)b << 8);
            }
        }
    }
    if (r < 32) {
        // padding words first (other lanes' rows overwrite them in C): tp[0] = 0 on unit operands
        const uint32_t x30p = (uint32_t)(SLOT_OFF_X + 8 * 30);
        for (int k2 = 0; k2 < HX_SLOT_CAP; k2++) T->hx[k2 * 32 + r] = (uint32_t)SLOT_OFF_TP | x30p << 16 | x30p << 24;
        int n = 0;
        if (r < NV)
            for (int j = 0; j < HT_TERMS; j++)
                if ((P2C ? htp(j, 0, r) : D[j * HT_PARTS * NV + r]) != 0) n++;
        s_htn[r] = n;
    }
    __syncthreads();
    if (tid == 0) {
        int used[HX_NSLOT], order[HX_NSLOT];
        for (int s2 = 0; s2 < HX_NSLOT; s2++) { used[s2] = 0; order[s2] = s2; }
        for (int i = 1; i < HX_NSLOT; i++)   // slot classes by capacity, smallest first (stable)
            for (int j2 = i; j2 > 0 && cap[order[j2 - 1]] > cap[order[j2]]; j2--) {
                const int t2 = order[j2]; order[j2] = order[j2 - 1]; order[j2 - 1] = t2;
            }
        for (int q = 0; q < 32; q++)
            for (int w2 = 0; w2 < HX_NSLOT / 2; w2++)
                s_dst[w2][q] = (uint32_t)SLOT_OFF_HXDUMMY | ((uint32_t)SLOT_OFF_HXDUMMY << 16);
        int ne[NV], nent = 0;
        for (int q = 0; q < NV; q++) ne[q] = 0;
        for (int n = HX_TERMS; n >= 1; n--)
            for (int row = 0; row < NV; row++)
                for (int c = 0; c < NV; c++) {
                    if (s_cnt[row][c] != n) continue;
                    int sl = -1;
                    for (int i = 0; i < HX_NSLOT && sl < 0; i++)
                        if (cap[order[i]] >= n && used[order[i]] < 32) sl = order[i];
                    if (sl < 0 || ne[row] >= 6 || nent >= ENT_CAP - 1) { s_bad = 1; continue; }
                    const int ln = used[sl]++;
                    ne[row]++;
                    s_place[row][c] = (uint8_t)(ln << 3 | sl);
                    const uint32_t off = (uint32_t)(SLOT_OFF_ENT + 8 * nent++);
                    s_eoff[row][c] = (uint16_t)off;
                    const int hi = (sl & 1) * 16;
                    s_dst[sl >> 1][ln] = (s_dst[sl >> 1][ln] & ~(0xFFFFu << hi)) | (off << hi);
                }
        // the distinct prefixes, from the hash sets below: (0, 33, 33) and (33, 33)
        // first (the padding words point at slot 0), the others in key order
        int nt = 1, np = 1;
        const uint32_t pad_t = 33u << 8 | 33u << 16, pad_p = 33u | 33u << 8;
        s_tri[0] = pad_t;
        s_pair[0] = pad_p;
        for (int h = 0; h < 256; h++) {
            const uint32_t k = s_th[h] - 1u;
            if (s_th[h] == 0u || k == pad_t) continue;
            if (nt < TP_CAP) s_tri[nt++] = k; else s_bad = 1;
        }
        for (int h = 0; h < 128; h++) {
            const uint32_t k = s_ph[h] - 1u;
            if (s_ph[h] == 0u || k == pad_p) continue;
            if (np < QP_CAP) s_pair[np++] = k; else s_bad = 1;
        }
        for (int i = 2; i < nt; i++)
            for (int j2 = i; j2 > 1 && s_tri[j2 - 1] > s_tri[j2]; j2--) {
                const uint32_t t2 = s_tri[j2]; s_tri[j2] = s_tri[j2 - 1]; s_tri[j2 - 1] = t2;
            }
        for (int i = 2; i < np; i++)
            for (int j2 = i; j2 > 1 && s_pair[j2 - 1] > s_pair[j2]; j2--) {
                const uint32_t t2 = s_pair[j2]; s_pair[j2] = s_pair[j2 - 1]; s_pair[j2 - 1] = t2;
            }
        s_ntri = nt;
        s_npair = np;
    }
    __syncthreads();
    // slot of a key: 0 for the padding key, else binary search in the sorted rest
    auto find = [](const uint32_t *tab, int n, uint32_t key) -> int {
        if (key == tab[0]) return 0;
        int lo = 1, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (tab[mid] < key) lo = mid + 1; else hi = mid;
        }
        return lo < n && tab[lo] == key ? lo : 0;
    };
    auto tp_off = [&](int co, int a, int b) -> uint32_t {
        return (uint32_t)(SLOT_OFF_TP +
                          8 * find(s_tri, s_ntri, ((uint32_t)co & 0xFFu) | (uint32_t)a << 8 | (uint32_t)b << 16));
    };
    auto qp_off = [&](int a, int b) -> uint32_t {
        return (uint32_t)(SLOT_OFF_QP + 8 * find(s_pair, s_npair, (uint32_t)a | (uint32_t)b << 8));
    };
    const uint32_t x30 = (uint32_t)(SLOT_OFF_X + 8 * 30);
    if (r < 32) {
        bool bad = false;
        // gather map and structural pattern of row r (padding lanes: zeros)
        uint32_t pat = 0;
        for (int q = 0; q < GM_WORDS; q++) {
            uint32_t v = 0;
            for (int k2 = 0; k2 < 2; k2++) {
                const int c = 2 * q + k2;
                const uint32_t off = r < NV ? s_eoff[r][c] : (uint32_t)SLOT_OFF_ENTZERO;
                v |= off << (16 * k2);
                if (off != (uint32_t)SLOT_OFF_ENTZERO) pat |= 1u << c;
            }
            T->gm[q][r] = v;
        }
        T->pat[r] = pat;
        // the tracker's LU skips the column groups this problem's structure
        // can never fill (hc_lu_struct.hpp LU_STRUCT_PAT); the evaluations take any
        // structure, the tracker only one within it
        if (r < NV && (pat & ~LU_STRUCT_PAT[r]) != 0u) atomicOr(&s_nostruct, 1);
        for (int q = 0; q < HX_NSLOT / 2; q++) T->hxd[q][r] = s_dst[q][r];
        if (r < NV)
            for (int c = 0; c < NV; c++) {
                if (s_place[r][c] == 0xFFu) continue;
                const int ln = s_place[r][c] >> 3, sl = s_place[r][c] & 7;
                int pos = start[sl];
                for (int j = 0; j < HX_TERMS; j++) {
                    const int base = (c * HX_TERMS + j) * HX_PARTS * NV + r;
                    const int co = P2C ? hxp(c, j, 0, r) : U[base], a = P2C ? hxp(c, j, 1, r) : U[base + NV],
                              b = P2C ? hxp(c, j, 2, r) : U[base + 2 * NV], u = P2C ? hxp(c, j, 3, r) : U[base + 3 * NV],
                              v = P2C ? hxp(c, j, 4, r) : U[base + 4 * NV];
                    if (co == 0) continue;
                    bad |= co < -128 || co > 127 || a < 0 || a >= NPP || b < 0 || b >= NPP || u < 0 || u > NV ||
                           v < 0 || v > NV;
                    if (!bad)
                        T->hx[pos * 32 + ln] = tp_off(co, a, b) | (uint32_t)(SLOT_OFF_X + 8 * u) << 16 |
                                               (uint32_t)(SLOT_OFF_X + 8 * v) << 24;
                    pos++;
                }
            }
        s_len[r] = HX_SLOT_CAP;
        // dH/dt | H (hc_eval.hpp eval_rhs): own terms at positions 0..12; a row
        // of more than 13 terms (an owner) puts its terms 14.. in its light
        // words 13.. (for x[w]) and in its helper's (lane ^ 16) words 10..; the
        // helper's own terms must end before 10 and it needs no help itself
        const int n = s_htn[r];
        const int need_o = max(0, n - HT_FULL);
        const int need_h = max(0, s_htn[r ^ 16] - HT_FULL);
        if (need_o > 0 && s_htn[r ^ 16] > HT_HELP_FIRST) bad = true;
        if (need_h > 0 && n > HT_HELP_FIRST) bad = true;
        const uint2 pad_ht = make_uint2((uint32_t)SLOT_OFF_TP | (uint32_t)SLOT_OFF_QP << 16,
                                        x30 | x30 << 8 | x30 << 16);   // tp[0], qp[0] with coef 0
        int k = 0;
        if (r < NV) {
            for (int j = 0; j < HT_TERMS; j++) {
                const int base = j * HT_PARTS * NV + r;
                const int co = P2C ? htp(j, 0, r) : D[base], a = P2C ? htp(j, 1, r) : D[base + NV],
                          b = P2C ? htp(j, 2, r) : D[base + 2 * NV], u = P2C ? htp(j, 3, r) : D[base + 3 * NV],
                          v = P2C ? htp(j, 4, r) : D[base + 4 * NV], x3 = P2C ? htp(j, 5, r) : D[base + 5 * NV];
                if (co == 0) continue;
                bad |= co < -128 || co > 127 || a < 0 || a >= NPP || b < 0 || b >= NPP || u < 0 || u > NV ||
                       v < 0 || v > NV || x3 < 0 || x3 > NV;
                if (!bad) {
                    const uint2 tw = make_uint2(tp_off(co, a, b) | qp_off(a, b) << 16,
                                                (uint32_t)(SLOT_OFF_X + 8 * u) | ((uint32_t)(SLOT_OFF_X + 8 * v) << 8) |
                                                    ((uint32_t)(SLOT_OFF_X + 8 * x3) << 16) |
                                                    (((uint32_t)co & 0xFFu) << 24));
                    T->ht[k * 32 + r] = tw;   // k < 13: a full term; k >= 13: the light word (x[w])
                    if (k >= HT_FULL) T->ht[(HT_HELP_FIRST + k - HT_FULL) * 32 + (r ^ 16)] = tw;
                }
                k++;
            }
        }
        for (int q = k; q < HT_TERMS; q++)
            if (!(q >= HT_HELP_FIRST && q < HT_HELP_FIRST + need_h)) T->ht[q * 32 + r] = pad_ht;
        if (bad) atomicOr(&s_bad, 1);
    }
    // E: bank-aware places of the (c, a, b) prefixes.  A ds_read_b64 of tp[]
    // serves 32 lanes a cycle when their indices differ mod 32 (or coincide);
    // the words of C read tp at 21 dH/dx and 13 rhs positions, and the sorted
    // numbering above costs ~64 cycles where 34 are the minimum.  Prefixes that
    // share a read position (conflict graph, s_adj) go to different residues:
    // the padding prefix first (tp[0]), then by degree, each to the residue
    // with the fewest conflicts and a free place (3 per residue, ties: fewer
    // used, then the lower residue); C's words are renumbered after it.
    // Places only: the values and their operations stay the same (bit-exact).
    __shared__ uint32_t s_adj[TP_CAP][3];
    __shared__ uint8_t s_pidx[HX_SLOT_CAP + HT_FULL][32];
    __shared__ uint8_t s_tslot[TP_CAP], s_tinv[TP_CAP], s_order[TP_CAP];
    __shared__ int s_deg[TP_CAP];
    for (int i = tid; i < TP_CAP * 3; i += PREP_THREADS) (&s_adj[0][0])[i] = 0u;
    for (int i = tid; i < TP_CAP; i += PREP_THREADS) { s_tinv[i] = 0xFFu; s_tslot[i] = 0u; }
    __syncthreads();
    const int ntri = s_ntri;
    auto tp_index = [&](uint32_t w) -> uint32_t {   // sorted index of a word's tp offset (TP_CAP: none)
        const uint32_t o = w & 0xFFFFu;
        const uint32_t i = (o - (uint32_t)SLOT_OFF_TP) / 8u;
        return o >= (uint32_t)SLOT_OFF_TP && i < (uint32_t)ntri ? i : (uint32_t)TP_CAP;
    };
    for (int i = tid; i < (HX_SLOT_CAP + HT_FULL) * 32; i += PREP_THREADS) {
        const int p = i >> 5, l = i & 31;
        const uint32_t w = p < HX_SLOT_CAP ? T->hx[p * 32 + l] : T->ht[(p - HX_SLOT_CAP) * 32 + l].x;
        s_pidx[p][l] = (uint8_t)min(tp_index(w), (uint32_t)0xFFu);
    }
    __syncthreads();
    for (int i = tid; i < (HX_SLOT_CAP + HT_FULL) * 32; i += PREP_THREADS) {
        const int p = i >> 5, l = i & 31;
        const uint32_t t = s_pidx[p][l];
        if (t >= (uint32_t)ntri) continue;
        for (int l2 = 0; l2 < 32; l2++) {
            const uint32_t u = s_pidx[p][l2];
            if (u != t && u < (uint32_t)ntri) atomicOr(&s_adj[t][u >> 5], 1u << (u & 31));
        }
    }
    __syncthreads();
    if (tid < ntri)
        s_deg[tid] = tid == 0 ? (1 << 20) : __popc(s_adj[tid][0]) + __popc(s_adj[tid][1]) + __popc(s_adj[tid][2]);
    __syncthreads();
    if (tid < ntri) {   // rank by degree, descending (ties: lower index first)
        int rk = 0;
        const int d = s_deg[tid];
        for (int u = 0; u < ntri; u++) rk += (s_deg[u] > d || (s_deg[u] == d && u < tid)) ? 1 : 0;
        s_order[rk] = (uint8_t)tid;
    }
    __syncthreads();
    if (tid < 64) {   // wave 0, lane c < 32: residue c (its members and fill)
        uint32_t m0 = 0u, m1 = 0u, m2 = 0u;
        int fill = 0;
        for (int k2 = 0; k2 < ntri; k2++) {
            const int t = s_order[k2];
            const int conf = __popc(s_adj[t][0] & m0) + __popc(s_adj[t][1] & m1) + __popc(s_adj[t][2] & m2);
            int key = (tid < 32 && fill < 3) ? ((conf * 4 + fill) << 5 | tid) : 0x7FFFFFFF;
            for (int s2 = 32; s2 > 0; s2 >>= 1) key = min(key, __shfl_xor(key, s2, 64));
            if (tid == (key & 31)) {
                const int slot = tid + 32 * fill++;
                s_tslot[t] = (uint8_t)slot;
                s_tinv[slot] = (uint8_t)t;
                if (t < 32) m0 |= 1u << t; else if (t < 64) m1 |= 1u << (t - 32); else m2 |= 1u << (t - 64);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < HX_SLOT_CAP * 32; i += PREP_THREADS) {
        const uint32_t w = T->hx[i], t = tp_index(w);
        if (t < (uint32_t)TP_CAP) T->hx[i] = (w & ~0xFFFFu) | (uint32_t)(SLOT_OFF_TP + 8 * s_tslot[t]);
    }
    for (int i = tid; i < HT_TERMS * 32; i += PREP_THREADS) {
        const uint32_t w = T->ht[i].x, t = tp_index(w);
        if (t < (uint32_t)TP_CAP) T->ht[i].x = (w & ~0xFFFFu) | (uint32_t)(SLOT_OFF_TP + 8 * s_tslot[t]);
    }
    if (r < 32) {
        // prefix build jobs of lane r (hc_eval.hpp build_prefixes): tp place i
        // holds prefix s_tinv[i], qp place i pair i
        const uint32_t p33 = (uint32_t)(SLOT_OFF_STG + 8 * 33);
        for (int q = 0; q < PRE_ROUNDS; q++) {
            const bool tpr = q < PRE_TP_ROUNDS;
            const int i = (tpr ? q : q - PRE_TP_ROUNDS) * 32 + r;
            uint2 job = make_uint2(p33 | p33 << 16, (uint32_t)SLOT_OFF_HXDUMMY);
            if (tpr && i < TP_CAP && s_tinv[i] != 0xFFu) {
                const uint32_t key = s_tri[s_tinv[i]];
                const uint32_t a = (key >> 8) & 0xFFu, b = key >> 16;
                job = make_uint2((uint32_t)(SLOT_OFF_STG + 8 * a) | (uint32_t)(SLOT_OFF_STG + 8 * b) << 16,
                                 (uint32_t)(SLOT_OFF_TP + 8 * i) | (key & 0xFFu) << 16);
                if constexpr (P2C)   // c * coefHx_k; the padding key: the constant coefficient, c = 0
                    job.x = (uint32_t)(SLOT_OFF_STG + 8 * (b > 1u ? (uint32_t)(P2C_NK - 1) : a + 32u * b));
            } else if (!tpr && i < s_npair) {
                const uint32_t a = s_pair[i] & 0xFFu, b = s_pair[i] >> 8;
                job = make_uint2((uint32_t)(SLOT_OFF_STG + 8 * a) | (uint32_t)(SLOT_OFF_STG + 8 * b) << 16,
                                 (uint32_t)(SLOT_OFF_QP + 8 * i));
                if constexpr (P2C)   // coefHt_k
                    job.x = (uint32_t)(SLOT_OFF_STG + 8 * (b > 1u ? (uint32_t)(P2C_NK - 1) : a + 32u * b));
            }
            T->pre[q][r] = job;
        }
    }
    __syncthreads();
    {
        // F: the slot-absolute address tables of the throughput tracking kernel
        // (hc_eval.hpp AbsTables), from the finished words of C and E: every
        // field of a word plus the byte offset of the lane's path slot from the
        // workgroup's first one.  Rebuilt whenever tab is (same pass, same hash).
        AbsTables *A = &ws->abs;
        auto slot_base = [](int i) -> uint32_t {   // i: (wave, lane) of a table row, wave * 64 + lane
            return (uint32_t)(((i >> 6) * 2 + ((i >> 5) & 1)) * (int)sizeof(SlotLDS));
        };
        for (int i = tid; i < ABS_WAVES * HX_SLOT_CAP * WAVE; i += PREP_THREADS) {
            const int l = i & 63, k = (i >> 6) % HX_SLOT_CAP, wv = (i >> 6) / HX_SLOT_CAP;
            const uint32_t sb = slot_base(wv * 64 + l);
            const uint32_t w = T->hx[k * 32 + (l & 31)];
            const int sl = hx_gslot(k);
            const uint32_t d = T->hxd[sl >> 1][l & 31];
            A->hx[wv][k][l] = make_uint4(sb + (w & 0xFFFFu), sb + ((w >> 16) & 0xFFu), sb + (w >> 24),
                                         sb + ((sl & 1) ? d >> 16 : d & 0xFFFFu));
        }
        for (int i = tid; i < ABS_WAVES * (HT_FULL + 1) * WAVE; i += PREP_THREADS) {
            const int l = i & 63, j = (i >> 6) % (HT_FULL + 1), wv = (i >> 6) / (HT_FULL + 1);
            const uint32_t sb = slot_base(wv * 64 + l);
            if (j < HT_FULL) {
                const uint2 w = T->ht[j * 32 + (l & 31)];
                A->ht[wv][j][l] = make_uint4(sb + (w.y & 0xFFu), sb + ((w.y >> 8) & 0xFFu), sb + ((w.y >> 16) & 0xFFu),
                                             sb + (w.x & 0xFFFFu));
                A->htq[wv][j][l] = make_uint2(sb + (w.x >> 16), __float_as_uint(coef_ht(w)));
            } else {
                uint32_t xw[3] = {sb + x30, sb + x30, sb + x30};
                for (int q = 0; q < HT_HELP; q++) xw[q] = sb + ((T->ht[(HT_FULL + q) * 32 + (l & 31)].y >> 16) & 0xFFu);
                A->ht[wv][j][l] = make_uint4(xw[0], xw[1], xw[2], sb + x30);
            }
        }
        for (int i = tid; i < ABS_WAVES * ABS_GM_Q * WAVE; i += PREP_THREADS) {
            const int l = i & 63, q = (i >> 6) % ABS_GM_Q, wv = (i >> 6) / ABS_GM_Q;
            const uint32_t sb = slot_base(wv * 64 + l);
            uint32_t g[4];
            for (int e = 0; e < 4; e++) {
                const int c = 4 * q + e;
                const uint32_t w = T->gm[min(c, NV - 1) >> 1][l & 31];   // (words past column 29: unused)
                g[e] = sb + ((c & 1) ? w >> 16 : w & 0xFFFFu);
            }
            A->gm[wv][q][l] = make_uint4(g[0], g[1], g[2], g[3]);
        }
        // the compact row's gather map: position p of row r is column lu_compact_col(r, p), the
        // structural zero where the row has no column at a level (and in the pad rows)
        for (int i = tid; i < ABS_WAVES * ABS_GMC_Q * WAVE; i += PREP_THREADS) {
            const int l = i & 63, q = (i >> 6) % ABS_GMC_Q, wv = (i >> 6) / ABS_GMC_Q;
            const uint32_t sb = slot_base(wv * 64 + l);
            const int row = l & 31;
            uint32_t g[4];
            for (int e = 0; e < 4; e++) {
                const int pos = 4 * q + e;
                int c = lu_first_unfused_step() + pos - LU_SLOTS;
                if (pos < LU_SLOTS) {   // the member the row's record names at level pos
                    const int mem = (int)((LU_ROWTAB.w[pos * LU_REC_ROWS + row] >> LU_REC_MEMBER_AT) & 31u);
                    c = mem == LU_REC_NO_MEMBER ? -1 : mem;
                }
                uint32_t off = (uint32_t)SLOT_OFF_ENTZERO;
                if (c >= 0 && row < NV) {
                    const uint32_t w = T->gm[c >> 1][row];
                    off = (c & 1) ? w >> 16 : w & 0xFFFFu;
                }
                g[e] = sb + off;
            }
            A->gmc[wv][q][l] = make_uint4(g[0], g[1], g[2], g[3]);
        }
    }
    if (r == 0) {
        // eval_rhs masks: help term q of the helpers (no accumulation), light
        // term q of the owners
        for (int q = 0; q < 4; q++) {
            uint32_t am = 0xFFFFFFFFu, lm = 0u;
            for (int l = 0; l < 32; l++)
                if (s_htn[l] - HT_FULL > q) { am &= ~(1u << (l ^ 16)); lm |= 1u << l; }
            T->ht_acc_mask[q] = am;
            T->ht_light_mask[q] = lm;
        }
        int mx = 0;
        for (int q = 0; q < 32; q++) mx = max(mx, s_len[q]);
        T->hx_len = mx;
        T->status = s_bad ? HC_ERROR_TABLE : 0;
        T->lu_struct = s_nostruct ? 0u : 1u;
        T->src_hash = src_hash;
        T->magic = TAB_MAGIC;
        if (s_bad) ws->status = HC_ERROR_TABLE;
    }
