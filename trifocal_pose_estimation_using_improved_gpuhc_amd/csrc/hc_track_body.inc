// The body of the tracker kernels k_track, k_track_small, k_track_grouped, k_track_gated,
// k_track_p2c and k_track_adaptive (hc_track.hpp),
// included inside each: ABORT, GROUPED, GATED, P2C, ADAPT, ARCH, LUS and LULAT are their
// template parameters or constants, `a` their argument block.  GATED
// (k_track_gated) replaces the scoring block of PH_FINISH and nothing else; P2C
// (k_track_p2c) the source of the prefix tables and the first step size; ADAPT
// (k_track_adaptive) adds the sample limit's two tests and its atomicMin.
// Included textually on purpose (DESIGN.md §3.2): a change here is a codegen
// change of all sixteen instantiations.  The other names it takes from its
// surroundings:
//   hc_layout.hpp  KArgs, Workspace, WG_THREADS, WAVES_PER_WG, PRIO_TENTHS,
//                  path_of_queue_pos, SLICE_Q, SLICE_QBIG, SUSP_WORDS, RQ_*
//   hc_ring.hpp    ld_rlx, ld_cf_rlx, st_u64_h, ld_u64_h, pack2, drain_stores,
//                  ring_push, ring_pop, ring_pop_paired, ring_wait_ticks
//   hc_score.hpp   score_half, JointCounts, score_joint_half
//   hc_track.hpp   PH_*, HC_ABORT_PRIO_DIV, the HC_DIAG_* globals
//   hc_device.hpp, hc_slot.hpp, hc_eval.hpp, hc_lu.hpp, hc_pose_device.hpp
//                  the arithmetic, SlotLDS, the evaluations, lu_mode / lu_solve, scenes
// kernel_GPUHC_trifocal_pose_PH_CodeOpt_TrunPaths (..._TrunPaths.cu:45-290) and,
// with ABORT, ..._TrunPaths_TrunRANSAC (..._TrunRANSAC.cu:45-327).
    // the sparse solve this kernel runs (hc_lu.hpp lu_mode: the one place that says so)
    constexpr LuMode LUM = lu_mode(ABORT, ARCH, LULAT, LUS);
    constexpr bool LUSTRUCT = LUM.strct;
    // The throughput tracking kernel reads its evaluations' operand addresses
    // complete, from the slot-absolute tables (hc_eval.hpp AbsTables), and checks
    // finiteness on the dH/dx entries instead of the gathered rows (the solve's
    // ENTCHK, which is therefore this flag).  The latency-critical kernels keep the
    // L1-resident packed tables.
    // (The variant builds that measured the four parts apart are not kept; DESIGN.md section 3.6
    // says how each ABSTAB site below was switched.)
    constexpr bool ABSTAB = LUM.entchk;
    // the LU's independent pivot steps fused level by level (hc_lu_levels.hpp): the
    // headline kernel only; false here gives its unfused solve
    constexpr bool LUFUSE = LUM.fuse;
    __shared__ cf s_sp[NPP];
    __shared__ SlotLDS s_slot[2 * WAVES_PER_WG];
    Workspace *ws = a.ws;
    const EvalTables *T = &ws->tab;
    if (ws->status != 0u) return;
    if ((T->lu_struct == 1u) != LUSTRUCT) return;   // the other instantiation tracks this table
    // time slicing: this launch's ring epoch (bumped by k_prep_tables)
    const unsigned epoch = (!ABORT && a.slice_q > 0) ? ld_rlx(&a.rq[RQ_EPOCH]) : 0u;
    // the term tables, read from the workspace (L1/L2-resident)
    const uint2 *s_ht = T->ht;
    const uint32_t *s_hx = T->hx;
    const uint32_t *s_hxd = &T->hxd[0][0];
    // (P2C, k_track_p2c: no parameters; a.target_params / a.diff_params are the
    // samples' coefficient blocks, 38 x 3 and 38 x 2 each)
    if (!P2C && threadIdx.x < NPP) s_sp[threadIdx.x] = a.start_params[threadIdx.x];
    {
        float *z = reinterpret_cast<float *>(s_slot);
        for (int i = threadIdx.x; i < (int)(sizeof(s_slot) / 4); i += WG_THREADS) z[i] = 0.0f;
    }
    __syncthreads();
    if (ABORT && threadIdx.x == 0) atomicCAS(&ws->t_start, 0ull, (unsigned long long)__builtin_amdgcn_s_memrealtime());
    const int lane = lane_id();
    const int r = lane & 31, hb = lane & 32;
    const int wid = threadIdx.x / WAVE;
    SlotLDS &S = s_slot[wid * 2 + (hb >> 5)];
    if (r == 30) S.x[30] = cmk(1.0f, 0.0f);
    if (r == 0) S.st.pre_smp = -2;   // no prefix tables yet
    // per-row constants (gather map, structural pattern) live in LDS and are
    // re-read every stage: held in VGPRs across the loop they spill (abort mode)
    __shared__ uint32_t s_rowc[GM_WORDS + 1][32];   // [0..14] gather map (hc_eval.hpp), [15] structural pattern
    if (threadIdx.x < 32) {
        for (int q = 0; q < GM_WORDS; q++) s_rowc[q][threadIdx.x] = T->gm[q][threadIdx.x];
        s_rowc[GM_WORDS][threadIdx.x] = T->pat[threadIdx.x];
    }
    if constexpr (LUFUSE) lu_rowtab_fill(threadIdx.x);   // the fused levels' row records (hc_lu_levels.hpp)
    __syncthreads();
    const bool rl = r < NV;
    wave_lds_sync();
    // ABSTAB: the wave's blocks of the absolute tables (uniform) and the first slot they count from
    const AbsTables *AT = &ws->abs;
    const int wv = ABSTAB ? __builtin_amdgcn_readfirstlane(wid) : 0;
    char *const l0 = reinterpret_cast<char *>(s_slot);

    // per-slot state (uniform within a half)
    int ph = PH_DEQ, b = -1, smp_loaded = -1;
    int qpos = 0;   // queue position of the slot's path (issue priority)
    unsigned found_seen = 0u;   // abort mode: the found flag as of the last stage
#ifdef HC_DIAG_TIMES
    int diag_t0 = 0;
    const unsigned long long diag_w0 = __builtin_amdgcn_s_memrealtime();
    if (lane == 0) atomicMin(&g_diag_span[0], diag_w0);
#endif
    int s = 0, stepidx = 0, coef = 1, succ = 0, nsteps = 0, ncorr = 0;
    int piece = 0;   // steps since the path (re)started on this slot (time slicing)
    float t0 = 0.0f, t_step = 0.0f, dt = 0.01f, h2 = 0.0f, scale = 0.0f;
    bool end_zone = false, check = true, isSucc = false, isInf = false;
    cf x = cmk(0.0f, 0.0f), xl = x, sols = x;
    // Retry reuse (sliced tracking launches): a rejected step's retry starts from
    // the same x, t and sample as the step it repeats, so its stage 0 would solve
    // the same system for the same slope k1.  Every stage 0 leaves k1 in words
    // 0..29 of the path's own suspend block, which is unused while the path runs;
    // k1v: the block holds the k1 of the step that starts next.  Set by a
    // rejection and consumed by the PH_BEGIN that follows it before any other
    // stage runs, so it is not parked with the slot state; a new path and a
    // resume clear it.
    constexpr bool REUSE = !ABORT && !ARCH;
    bool k1v = false;

#ifdef HC_DIAG_PHASES
    uint64_t dg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t dt_ = __builtin_amdgcn_s_memtime(), dt0_ = dt_;
#define HC_DIAG_MARK(k) do { const uint64_t n_ = __builtin_amdgcn_s_memtime(); dg[k] += n_ - dt_; dt_ = n_; } while (0)
#else
#define HC_DIAG_MARK(k) do { } while (0)
#endif
    for (;;) {
        HC_DIAG_MARK(6);
        HC_ISA_MARK("ctl_slots");
        // ---------------- resolve slot phases until every slot is at a stage or idle
        // next dequeue (time slicing): -1 normal, -2 swap with a suspended path,
        // >= 0 a new-path ticket the suspension claimed (set and used within this phase)
        int deq_hint = -1;
        for (;;) {
            if (ph == PH_FINISH) {                                            // :282-286
                const bool conv = ((double)t0 >= 1.0 || (1.0 - (double)t0 <= 0.0000001));
                cf *dtrack = a.track_array ? a.track_array[b] : a.tracks + (size_t)b * (NV + 1);
                if (rl) dtrack[r] = x;
                int in21 = 0, in31 = 0;
                if (ABORT && conv) {                                          // TrunRANSAC.cu:312-322
                    if (rl) S.x[r] = x;
                    wave_lds_sync();
                    if constexpr (GATED) {
                        // the stop rule of the gated launch: the pose-support candidate filter
                        // and counts (hc_pose_device.hpp) on the path's own triplet, the gate on
                        // the joint count
                        if (is_candidate_half(x, r, hb)) {
                            const int grp = a.sample_group[smp_loaded];
                            const hcTripletGroup g = a.groups[grp];
                            const JointCounts c = score_joint_half(S.x, load_scene(g.num_edgels, g.locations, g.K), r);
                            in21 = c.c21;
                            in31 = c.c31;
                            if (r == 0) {
                                if (a.joint_inliers) a.joint_inliers[b] = c.cJ;
                                if constexpr (ADAPT) {
                                    // the samples this count still asks for (the caller's table of the
                                    // triplet): the best hypothesis so far sets the triplet's limit
                                    __hip_atomic_fetch_min(&a.group_limit[grp],
                                                           (unsigned)a.need[a.need_offset[grp] + (long long)c.cJ],
                                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                }
                                if ((double)c.cJ >= (double)a.gate_ratio * (double)g.num_edgels) {
                                    __hip_atomic_store(&a.group_found[grp], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                    a.batch_index[b] = b;
                                    if (a.group_ticks)
                                        atomicCAS(&a.group_ticks[grp], 0ull,
                                                  (unsigned long long)__builtin_amdgcn_s_memrealtime());
                                }
                            }
                        }
                    } else {
                        const unsigned long long im = __ballot(r >= 18 && rl && (double)__builtin_fabsf(x.y) < 1e-5);
                        if constexpr (GROUPED) {
                            if (((unsigned)(im >> hb) & 0x3FFC0000u) == 0x3FFC0000u) {
                                // the path's own triplet: its scoring set, its K, its flag
                                const int grp = a.sample_group[smp_loaded];
                                const hcTripletGroup g = a.groups[grp];
                                const int2 c = score_half(S.x, g.locations, g.num_edgels, g.K, r);
                                in21 = c.x;
                                in31 = c.y;
                                const float r21 = (float)in21 / (float)g.num_edgels, r31 = (float)in31 / (float)g.num_edgels;
                                if ((double)r21 >= 0.90 && (double)r31 >= 0.90 && r == 0) {
                                    __hip_atomic_store(&a.group_found[grp], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                    a.batch_index[b] = b;
                                    if (a.group_ticks)
                                        atomicCAS(&a.group_ticks[grp], 0ull,
                                                  (unsigned long long)__builtin_amdgcn_s_memrealtime());
                                }
                            }
                        } else if (((unsigned)(im >> hb) & 0x3FFC0000u) == 0x3FFC0000u) {   // eval.cuh:46-53
                            const int2 c = score_half(S.x, a.edgels, a.num_edgels, a.K, r);
                            in21 = c.x;
                            in31 = c.y;
                            const float r21 = (float)in21 / (float)a.num_edgels, r31 = (float)in31 / (float)a.num_edgels;
                            if ((double)r21 >= 0.90 && (double)r31 >= 0.90 && r == 0) {   // eval.cuh:241-246
                                __hip_atomic_store(&ws->found, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                a.found_flag[0] = 1;
                                // the other GPUs' launches poll this (system scope: written
                                // through to the owner's memory over xGMI)
                                if (a.peer_found)
                                    __hip_atomic_store(a.peer_found, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                                a.batch_index[b] = b;
                                atomicCAS(&ws->t_found, 0ull, (unsigned long long)__builtin_amdgcn_s_memrealtime());
                            }
                        }
                    }
                }
                if (r == 0) {
                    a.conv[b] = conv ? 1 : 0;
                    a.inf[b] = isInf ? 1 : 0;
#ifdef HC_DIAG_TIMES
                    // diagnostic build: dequeue / finish device timestamps (s_memrealtime) of each path
                    in21 = diag_t0;
                    in31 = (int)__builtin_amdgcn_s_memrealtime();
#endif
                    if (a.stats) a.stats[b] = hcPathStats{nsteps, ncorr, in21, in31};
                }
                ph = PH_DEQ;
            }
            if (ph == PH_DEQ) {
                int nb = 0, rb = -1;   // new-path ticket; else a suspended path id (time slicing)
                if (r == 0) {
                    if (!ABORT && deq_hint >= 0) {
                        nb = deq_hint;                       // claimed by the suspension
                    } else if (!ABORT && deq_hint == -2) {
                        nb = a.num_paths;                    // swap: the oldest suspended path
                        rb = ring_pop_paired(a.rq, a.ring, a.ring_cap, epoch, ws, a.num_paths, ring_wait_ticks(a.ring_test));
                    } else {
                        nb = (ABORT || a.slice_q == 0 || ld_rlx(&ws->queue) < (unsigned)a.num_paths)
                                 ? (int)atomicAdd(&ws->queue, 1u) : a.num_paths;
                        if (!ABORT && nb >= a.num_paths && a.slice_q > 0) rb = ring_pop(a.rq, a.ring, a.ring_cap, epoch, ws, a.num_paths, ring_wait_ticks(a.ring_test));
                    }
                }
                deq_hint = -1;
                nb = bcast_half0(nb);
                if (!ABORT) rb = bcast_half0(rb);
                if (!ABORT && rb >= 0) {
                    // resume a suspended path at its step boundary from its
                    // suspend block (x in words 0..29, the scalars in 30, 31)
                    b = rb;
                    qpos = 0;
                    smp_loaded = b / NTRK;   // (its target / diff params are read where the prefixes are built)
                    const unsigned long long *blk = a.susp + (size_t)b * SUSP_WORDS;
                    x = rl ? ld_cf_rlx(reinterpret_cast<const cf *>(blk + r)) : cmk(0.0f, 0.0f);
                    xl = x;
                    sols = x;
                    const unsigned long long q0 = ld_u64_h(blk + 30), q1 = ld_u64_h(blk + 31);
                    t0 = __uint_as_float((unsigned)q0);
                    dt = __uint_as_float((unsigned)(q0 >> 32));
                    stepidx = (int)((unsigned)q1 & 0xFFFFu);
                    nsteps = (int)((unsigned)q1 >> 16);
                    const unsigned w3 = (unsigned)(q1 >> 32);
                    ncorr = (int)(w3 & 0xFFFFu);
                    succ = (int)((w3 >> 16) & 0x3FFFu);
                    end_zone = (w3 >> 30) & 1u; check = (w3 >> 31) & 1u; isSucc = false; isInf = false;
                    t_step = 0.0f;
                    piece = 0;
                    k1v = false;   // the block held x: a k1 kept before the suspension is gone
                    ph = PH_BEGIN;
                } else if (nb >= a.num_paths) {
                    ph = PH_IDLE;
                    b = -1;
                } else {
                    b = path_of_queue_pos(nb, a.num_paths, a.ordered);
                    qpos = nb;
                    bool skip = false;
                    if constexpr (GROUPED) {
                        // the flag of the path's own triplet (set by this launch, or by
                        // the caller: the carry-over of an earlier launch's find)
                        skip = __hip_atomic_load(&a.group_found[a.sample_group[b / NTRK]], __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT) != 0u;
                        if constexpr (ADAPT) {
                            // the triplet's sample limit (lowered by this launch's scored paths, or
                            // preset by the caller): samples from the limit on are not tracked
                            const int sq = b / NTRK;
                            skip = skip || (unsigned)a.sample_ordinal[sq] >=
                                               __hip_atomic_load(&a.group_limit[a.sample_group[sq]], __ATOMIC_RELAXED,
                                                                 __HIP_MEMORY_SCOPE_AGENT);
                        }
                        skip = bcast_half0((int)skip) != 0;
                        if (skip && r == 0) {
                            a.conv[b] = 0;
                            a.inf[b] = 0;
                            if (a.stats) a.stats[b] = hcPathStats{0, 0, 0, 0};
                        }
                    } else if (ABORT) {                                       // TrunRANSAC.cu:152
                        skip = __hip_atomic_load(&ws->found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
                        if (!skip && a.peer_found &&
                            __hip_atomic_load(a.peer_found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) {
                            // another GPU found a pose: stop here too, and let the rest of
                            // this launch see it without crossing xGMI
                            skip = true;
                            __hip_atomic_store(&ws->found, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                        skip = bcast_half0((int)skip) != 0;
                        if (skip && r == 0) {
                            a.conv[b] = 0;
                            a.inf[b] = 0;
                            if (a.stats) a.stats[b] = hcPathStats{0, 0, 0, 0};
                        }
                    }
                    if (!skip) {
                        const int trk = b % NTRK;                            // :67-69
                        smp_loaded = b / NTRK;
#ifdef HC_DIAG_TIMES
                        diag_t0 = (int)__builtin_amdgcn_s_memrealtime();
#endif
                        const cf *dtrack = a.track_array ? a.track_array[b] : a.tracks + (size_t)b * (NV + 1);
                        const cf *dstart = a.start_sols_array ? a.start_sols_array[trk]
                                                              : a.start_sols + (size_t)trk * (NV + 1);
                        x = rl ? dtrack[r] : cmk(0.0f, 0.0f);                 // :101-103
                        sols = rl ? dstart[r] : cmk(0.0f, 0.0f);
                        xl = x;
                        t0 = 0.0f; t_step = 0.0f; dt = P2C ? 0.05f : 0.01f;   // :80 (..._P2C.cu:75)
                        end_zone = false; check = !ARCH || a.truncate != 0; isSucc = false; isInf = false;
                        succ = 0; nsteps = 0; ncorr = 0; stepidx = 0; piece = 0;
                        k1v = false;
                        ph = PH_BEGIN;
                    }
                }
            }
            if (ABORT && ph == PH_BEGIN && stepidx > 0 && found_seen != 0u) {
                // inflight_stop: a pose was found, a path in flight stops at its
                // step boundary and reports like a skipped one (track untouched,
                // conv = 0).  Without it (the reference's semantics) in-flight
                // paths run to completion (..._TrunRANSAC.cu:152 only gates the start).
                if (r == 0) {
                    a.conv[b] = 0;
                    a.inf[b] = 0;
                    if (a.stats) a.stats[b] = hcPathStats{0, 0, 0, 0};
                }
                ph = PH_DEQ;
            }
            if (ph == PH_BEGIN) {                                             // :138-165
                bool done = stepidx > a.max_steps;
                if (!done) done = !((double)t0 < 1.0 && (1.0 - (double)t0 > 0.0000001));
                if (!done) {
                    if (!end_zone && (double)__builtin_fabsf(1.0f - t0) <= 0.0500001) end_zone = true;
                    if (check) {
                        const unsigned long long pos = __ballot(r < 8 && x.x > 0.0f);
                        const bool allpos = ((unsigned)(pos >> hb) & 0xFFu) == 0xFFu;
                        if (t0 > 0.0f) check = !allpos;
                    }
                    done = (double)t0 > 0.95 && check;
                }
                bool suspend = false;
                // (every path stays suspendable: long paths keeping their slots
                // measured 5-20 % slower, DESIGN.md section 3.6; that A/B switch
                // and the issue-priority ones below are in commit 02bc69d)
                // (a half about to retry with a kept k1 is not suspended, the block
                // would be overwritten with x: it runs the retry first and is
                // suspendable at the next boundary.  Suspending it like any other and
                // recomputing the slope after the resume measured 0.06-0.17 ms slower
                // per config-2 launch: DESIGN.md, retry reuse with plain invalidation)
                if (!ABORT && !done && a.slice_q > 0 && piece >= a.slice_q && !(REUSE && k1v)) {
                    // time slice used up: suspend for a new path (its ticket
                    // claimed here), else swap with a suspended path, else
                    // keep running
                    int hint = -1;
                    if (r == 0) {
                        if (ld_rlx(&ws->queue) < (unsigned)a.num_paths) {
                            const int t = (int)atomicAdd(&ws->queue, 1u);
                            if (t < a.num_paths) hint = t;
                        }
                        if (hint < 0) {
                            // -3: suspended paths wait, but more than one per path
                            // slot and this slice is shorter than SLICE_QBIG: go on
                            const int av = ld_i_rlx(reinterpret_cast<const int *>(&a.rq[RQ_AVAIL]));
                            const int slots = (int)(gridDim.x * (WG_THREADS / WAVE) * 2u);
                            if (av > 0) hint = (piece >= SLICE_QBIG || av <= slots) ? -2 : -3;
                        }
                    }
                    hint = bcast_half0(hint);
                    if (hint >= 0 || hint == -2) {
                        // the whole state in one 256-B block, one store per half:
                        // lanes 0..29 x, lane 30 (t0, dt), lane 31 the counters
                        const unsigned w2 = (unsigned)stepidx | ((unsigned)nsteps << 16);
                        const unsigned w3 = (unsigned)ncorr | ((unsigned)succ << 16) | (end_zone ? 1u << 30 : 0u) |
                                            (check ? 1u << 31 : 0u);
                        const unsigned long long word =
                            rl ? pack2(__float_as_uint(x.x), __float_as_uint(x.y))
                               : (r == 30 ? pack2(__float_as_uint(t0), __float_as_uint(dt)) : pack2(w2, w3));
                        st_u64_h(a.susp + (size_t)b * SUSP_WORDS + r, word);
                        drain_stores();
                        if (r == 0) ring_push(a.rq, a.ring, a.ring_cap, epoch, b, hint >= 0, ws, a.ring_test);
                        deq_hint = hint;
                        suspend = true;
                    } else if (hint == -1) {
                        piece = 0;
                    }
                }
                if (!done && !suspend) {
                    if (end_zone) {
                        if (dt > __builtin_fabsf(1.0f - t0)) dt = __builtin_fabsf(1.0f - t0);
                    } else if ((double)dt > __builtin_fabs(0.95 - (double)t0)) {
                        dt = (float)__builtin_fabs(0.95 - (double)t0);
                    }
                    t_step = t0;
                    h2 = (float)(0.5 * (double)dt);
                    scale = 0.0f;
                    coef = 1;
                    s = 0;
                    nsteps++;
                    piece++;
                    if constexpr (REUSE) {
                        if (k1v) {
                            // The retry of a rejected step: stage 0 is taken from the kept k1,
                            // with the s == 0 update of the stage machine below, op for op
                            // (dt enters only here, k1 does not depend on it).  The k1 was
                            // stored by these lanes several stages ago; the wait for
                            // every store of the wave to be acknowledged orders this load
                            // after it (same address, same device-coherent level).
                            drain_stores();
                            const cf k1 = rl ? ld_cf_rlx(reinterpret_cast<const cf *>(a.susp + (size_t)b * SUSP_WORDS + r))
                                             : cmk(0.0f, 0.0f);
                            sols = cadd(sols, cscale(cscale(k1, dt), (float)(1.0 / 6.0)));
                            scale += h2;
                            coef <<= 1;
                            x = cadd(x, cscale(k1, scale));
                            t0 += h2;
                            s = 1;
#ifdef HC_DIAG_LUWORK
                            if (r == 0) atomicAdd(&g_diag_luwork[10], 1ull);
#endif
                        }
                    }
                }
                k1v = false;   // used, or lost to the end of the path or to a suspension
                ph = suspend ? PH_DEQ : done ? PH_FINISH : PH_STAGE;
            }
            if (__ballot(ph == PH_FINISH || ph == PH_DEQ || ph == PH_BEGIN) == 0ull) break;
        }
        if (__ballot(ph == PH_STAGE) == 0ull) break;
#ifdef HC_DIAG_UTIL
        {
            const unsigned long long bs = __ballot(ph == PH_STAGE);
            if (lane == 0) {
                const unsigned bin = (unsigned)(__builtin_amdgcn_s_memrealtime() >> 10) & (UTIL_BINS - 1);
                unsigned long long *u = g_diag_util[blockIdx.x % UTIL_COPIES][bin];
                atomicAdd(&u[0], (unsigned long long)((bs & 1ull) + ((bs >> 32) & 1ull)));
                atomicAdd(&u[1], 1ull);
            }
        }
#endif
        if (ABORT) {
            // Abort mode: first come, first served.  The queue is sample-major,
            // so the waves holding the earliest hypotheses get the higher issue
            // priority (the first sixteenth of the launch's paths at 3, the next
            // at 2, the next at 1) and whole early hypotheses complete -- and are
            // scored -- sooner, instead of every hypothesis in flight
            // progressing at the same rate.  Which paths are tracked, and their
            // results, do not depend on it (only on when the pose flag is set).
            const int qp = (ph == PH_STAGE) ? qpos : 0x7FFFFFFF;
            const int m = min(__builtin_amdgcn_readlane(qp, 0), __builtin_amdgcn_readlane(qp, 32));
            const int lvl = (int)((long long)m * HC_ABORT_PRIO_DIV / a.num_paths);
            if (lvl <= 0) __builtin_amdgcn_s_setprio(3);
            else if (lvl == 1) __builtin_amdgcn_s_setprio(2);
            else if (lvl == 2) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
        }
        if (!ABORT && a.ordered && a.slice_q == 0) {
            // Without time slicing: issue priority by queue position (s_setprio,
            // arbitration among the waves of a SIMD): the last tenth of the
            // queue at 3, the tenth before at 2, the one before that at 1.
            // Paths dequeued late decide when the launch ends; the earlier
            // ones have slack (DESIGN.md §3, profiles/r2_ab_priority.jsonl:
            // -1.8 %).  With slicing it is neutral (profiles/r2n_ab_slice2.jsonl).
            const int qp = (ph == PH_STAGE) ? qpos : 0;
            const int m = max(__builtin_amdgcn_readlane(qp, 0), __builtin_amdgcn_readlane(qp, 32));
            const int lvl = (int)((long long)m * PRIO_TENTHS / a.num_paths);
            if (lvl >= PRIO_TENTHS - 1) __builtin_amdgcn_s_setprio(3);
            else if (lvl >= PRIO_TENTHS - 2) __builtin_amdgcn_s_setprio(2);
            else if (lvl >= PRIO_TENTHS - 3) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
        }
        if (!ABORT && a.slice_q > 0) {
            // With time slicing: issue priority to the wave whose paths have
            // run the fewest steps (least attained service): a path's remaining
            // steps are bounded by max_steps - stepidx, so the paths that can
            // still run longest get the larger share of their SIMD, and the
            // launch ends with evenly short remainders.
            // (measured against: no priority +3 %, most attained service first
            // +5 %, longest estimated remaining work first +2.5 %, levels 8-60
            // steps wide equal or slower; DESIGN.md section 3.6)
            const int si = (ph == PH_STAGE) ? stepidx : (1 << 20);
            const int m = min(__builtin_amdgcn_readlane(si, 0), __builtin_amdgcn_readlane(si, 32));
            const int q4 = (int)((long long)m * 4 / (a.max_steps + 1));
            if (q4 <= 0) __builtin_amdgcn_s_setprio(3);
            else if (q4 == 1) __builtin_amdgcn_s_setprio(2);
            else if (q4 == 2) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
        }
        HC_DIAG_MARK(0);
        // the found flag for the next step boundary: read now, used after the stage
        if constexpr (GROUPED) {
            // (the group id re-derived from the slot's sample: not held across the stage)
            if (a.inflight_stop)
                found_seen = ph == PH_STAGE ? __hip_atomic_load(&a.group_found[a.sample_group[smp_loaded]],
                                                                __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                            : 0u;
            if constexpr (ADAPT) {
                // ... or the triplet's sample limit has come down to this path's sample
                if (a.inflight_stop && ph == PH_STAGE)
                    found_seen |= (unsigned)a.sample_ordinal[smp_loaded] >=
                                          __hip_atomic_load(&a.group_limit[a.sample_group[smp_loaded]], __ATOMIC_RELAXED,
                                                            __HIP_MEMORY_SCOPE_AGENT)
                                      ? 1u : 0u;
            }
        } else if (ABORT && a.inflight_stop) {
            found_seen = __hip_atomic_load(&ws->found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // (the peer flag's xGMI round trip is hidden by the stage that follows)
            if (a.peer_found) found_seen |= __hip_atomic_load(a.peer_found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }

        // ---------------- one stage for both slots
        // park the slot state in LDS so it does not occupy VGPRs across eval + LU
        HC_ISA_MARK("ctl_park");
        // the slot's prefix tables follow its p(t): rebuilt when t or the
        // sample changed (about 0.4 times per stage and path; both halves of
        // the wave rebuild when either needs it, each from its own t and sample)
        const float pre_t = S.st.pre_t;
        const int pre_smp = S.st.pre_smp;
        const bool rebuild = __ballot(ph == PH_STAGE && (__float_as_uint(t0) != __float_as_uint(pre_t) ||
                                                         smp_loaded != pre_smp)) != 0ull;
        if (r == 0) {
            SlotState q;
            q.t0 = t0; q.t_step = t_step; q.dt = dt; q.h2 = h2; q.scale = scale;
            q.s = s; q.stepidx = stepidx; q.coef = coef; q.succ = succ; q.nsteps = nsteps; q.ncorr = ncorr;
            q.b = b; q.smp = smp_loaded; q.ph = ph;
            q.flags = (end_zone ? 1 : 0) | (check ? 2 : 0) | (isSucc ? 4 : 0) | (isInf ? 8 : 0) | (piece << 4);
            q.pad = qpos;
            q.pre_t = rebuild ? t0 : pre_t;
            q.pre_smp = rebuild ? smp_loaded : pre_smp;
            S.st = q;
        }
        if (rl) { S.x[r] = x; S.xl[r] = xl; S.sols[r] = sols; }
        if (rebuild) {
            HC_ISA_MARK("ctl_prefix");
#ifdef HC_DIAG_LUWORK
            if (lane_fresh() == 0) atomicAdd(&g_diag_luwork[9], 1ull);
#endif
            const int rs = lane_fresh() & 31;   // == r; the LDS addresses are not hoisted and held across the loop
            const size_t so = (size_t)(smp_loaded > 0 ? smp_loaded : 0) * NPP;
            if constexpr (P2C) {
                // the coefficients at the slot's t (..._P2C.cu:133, :147, :172; its third stage
                // and its corrector keep the last ones, which are this t's: no rebuild there)
                const size_t sk = (size_t)(smp_loaded > 0 ? smp_loaded : 0) * P2C_NK;
                build_prefixes_p2c(S, rs, &T->pre[0][0], a.target_params + sk * 3, a.diff_params + sk * 2, t0);
            } else {
                build_prefixes(S, rs, &T->pre[0][0], a.target_params + so, a.diff_params + so, s_sp, t0);
            }
        }
        wave_lds_sync();
        const int s_in = s, ph_in = ph;
        asm volatile("" :: "v"(s_in), "v"(ph_in));
        // opaque lane id: keeps LICM from hoisting ~30 lane-derived per-pivot
        // constants (bpermute addresses, r == i masks) out of the path loop
        const int lane_v = lane_fresh();   // recomputed (2 VALU), not held across the loop
        const int r_v = lane_v & 31;
        const uint32_t l16 = (uint32_t)lane_v << 4;   // ABSTAB: the lane's byte offset in a table row
        const uint32_t row_pat = s_rowc[GM_WORDS][r_v];
        const bool act = ph_in == PH_STAGE;
        const bool pred = act && s_in < 4;
        HC_DIAG_MARK(1);
        // the stage's linear system: right-hand side first (dH/dt | H need no
        // Jacobian registers, so their LDS gathers can run many terms ahead),
        // then dH/dx into rA
        cf rB = cmk(0.0f, 0.0f);
        HC_ISA_MARK("ev_rhs");
        {
            const bool any_p = __ballot(pred) != 0ull, any_c = __ballot(act && !pred) != 0ull;
            const RhsMasks mk = rhs_masks(T);
#ifdef HC_DIAG_LUWORK
            if (lane_v == 0) atomicAdd(&g_diag_luwork[any_p && any_c ? 6 : any_p ? 7 : 8], 1ull);
#endif
            if (any_p && any_c) {                                            // :185 | :221, one pass
                HC_ISA_MARK("ev_rhs_mixed");
                if constexpr (ABSTAB) rB = eval_rhs_abs<RHS_MIXED>(AT->ht[wv], AT->htq[wv], l0, l16, pred, mk);
                else rB = eval_rhs<RHS_MIXED>(s_ht, S, r_v, pred, mk);
            } else if (any_p) {                                              // :185
                HC_ISA_MARK("ev_rhs_ht");
                const cf t = ABSTAB ? eval_rhs_abs<RHS_HT>(AT->ht[wv], AT->htq[wv], l0, l16, true, mk)
                                    : eval_rhs<RHS_HT>(s_ht, S, r_v, true, mk);
                if (pred) rB = t;
            } else if (any_c) {                                              // :221
                HC_ISA_MARK("ev_rhs_h");
                const cf t = ABSTAB ? eval_rhs_abs<RHS_H>(AT->ht[wv], AT->htq[wv], l0, l16, false, mk)
                                    : eval_rhs<RHS_H>(s_ht, S, r_v, false, mk);
                if (!pred) rB = t;
            }
        }
        HC_DIAG_MARK(3);
        // (LUFUSE: the row in its compact form, LuRowForm<true> of hc_lu_struct.hpp, through gmc's words)
        cf rA[LuRowForm<LUFUSE>::W];
        HC_ISA_MARK("ev_hx");
        bool ent_ok = true;   // ABSTAB: the entries' sums of squares are finite
        if constexpr (ABSTAB) {
            uint4 gmv[LUFUSE ? ABS_GMC_Q : ABS_GM_Q];
            ent_ok = eval_hx_terms_abs(AT->hx[wv], l0, l16, LUFUSE ? AT->gmc[wv] : AT->gm[wv], gmv);
            wave_lds_sync();
            HC_ISA_MARK("ev_gather");
            gather_hx_abs(rA, l0, gmv);
        } else {
            eval_hx(rA, s_hx, s_hxd, &s_rowc[0][0], S, r_v);                 // :184 / :220
        }
        wave_lds_sync();
        const bool ent_bad = ABSTAB && __ballot(!ent_ok) != 0ull;
        HC_DIAG_MARK(2);
        bool redo;
        LUBuf &LB = *reinterpret_cast<LUBuf *>(S.lu);
        // the LU's scratch: the dH/dx entry block, dead once gathered into rA
        // (a dense re-solve evaluates dH/dx again)
        static_assert(ENT_CAP - 1 >= LU_SCRATCH_FUSED_CF && offsetof(SlotLDS, ent) % 16 == 0, "LU scratch in SlotLDS::ent");
        cf k = lu_solve<false, LUM.lat, LUSTRUCT, ABSTAB, LUFUSE>(rA, rB, lane_v, row_pat, LB, S.ent, redo,
                                                                  HC_LU_COUNT(__ballot(act)), ent_bad);   // :188 / :224
        HC_ISA_MARK("ctl_redo");
        if (__builtin_expect(redo, 0)) {
            // a system the sparse solve cannot take exactly (an entry not provably
            // finite, a pivot outside the fast reciprocal range): dH/dx and the
            // right-hand side are evaluated again (the sparse solve used the
            // entry block as its scratch), and the system solved densely
            // (the stage kind re-read from the parked slot state: held across the
            // LU, act / pred would be spilled)
            HC_ISA_MARK("redo_evals");
            const bool act_r = S.st.ph == PH_STAGE, pred_r = act_r && S.st.s < 4;
            // a fresh lane id: the table addresses of the stage's evaluations
            // are not shared with (and held across the LU for) this rare path
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
            // (eval_hx without its phase marker: the ISA phase count keeps this rare
            // copy under redo_evals)
            // (the dense solve takes the 30 columns, whatever form the sparse one's row had)
            cf rD[NV];
            if constexpr (ABSTAB) {
                uint4 gmv[ABS_GM_Q];
                eval_hx_terms_abs(AT->hx[wv], l0, l16_r, AT->gm[wv], gmv);
                wave_lds_sync();
                gather_hx_abs(rD, l0, gmv);
            } else {
                eval_hx_terms(s_hx, s_hxd, reinterpret_cast<char *>(&S), r_r);
                wave_lds_sync();
                gather_hx(rD, &s_rowc[0][0], S, r_r);
            }
            wave_lds_sync();
            k = lu_solve<true>(rD, rb, lane_v, row_pat, LB, S.ent, redo, HC_LU_COUNT(__ballot(act_r)));
        }
        wave_lds_sync();
#ifdef HC_DIAG_PHASES
        {   // [4] forward elimination up to the solve's boundary stamp, [5] the rest of the LU
            const uint64_t mid = g_diag_lu_mid[blockIdx.x * 4 + wid];
            const uint64_t n_ = __builtin_amdgcn_s_memtime();
            if (mid > dt_ && mid < n_) { dg[4] += mid - dt_; dt_ = mid; }
        }
#endif
        HC_DIAG_MARK(5);
        HC_ISA_MARK("ctl_update");
        {
            const SlotState q = S.st;
            t0 = q.t0; t_step = q.t_step; dt = q.dt; h2 = q.h2; scale = q.scale;
            s = q.s; stepidx = q.stepidx; coef = q.coef; succ = q.succ; nsteps = q.nsteps; ncorr = q.ncorr;
            b = q.b; smp_loaded = q.smp; ph = q.ph;
            end_zone = q.flags & 1; check = q.flags & 2; isSucc = q.flags & 4; isInf = q.flags & 8;
            piece = q.flags >> 4;
            qpos = q.pad;
            k1v = false;   // (never set across a stage)
            x = rl ? S.x[r] : cmk(0.0f, 0.0f);
            xl = rl ? S.xl[r] : cmk(0.0f, 0.0f);
            sols = rl ? S.sols[r] : cmk(0.0f, 0.0f);
        }
        // act / pred of this stage, from the reloaded state
        const bool act_q = ph == PH_STAGE, pred_q = act_q && s < 4;
        if (act_q) {
            bool step_end = false;
            if (pred_q) {
                if (ARCH && s < 3 && a.explicit_rk) {
                    // archived ..._PH.cu with dev-get-new-data.cuh:37-71, gc = MAGMA_C_ONE:
                    // s += ((k*dt)*gc*1.0)/(6|3); x = (s ? x_last : x) + k*((h2|dt)*gc)
                    const cf kd = cmul(cscale(k, dt), cmk(1.0f, 0.0f));
                    sols = cadd(sols, cdivs(cscale(kd, 1.0f), s == 0 ? 6.0f : 3.0f));
                    if (s > 0) x = xl;
                    x = cadd(x, cmul(k, cmk(s == 2 ? dt : h2, 0.0f)));
                    if (s != 1) t0 += h2;
                } else if (s < 3) {                                          // :191-205
                    // (double)coef * 1.0 / 6.0 rounded to float; coef is 1 or 2 here
                    // (it doubles after s = 0 and s = 2): a constant each, so no f64 division
                    const float w = coef == 1   ? (float)(1.0 / 6.0)
                                    : coef == 2 ? (float)(2.0 / 6.0)
                                                : (float)((double)coef * 1.0 / 6.0);
                    sols = cadd(sols, cscale(cscale(k, dt), w));
                    if (coef > 1) x = xl;
                    const int sc = (s == 1) ? 0 : 1;
                    scale += (float)sc * h2;
                    coef <<= sc;
                    x = cadd(x, cscale(k, scale));
                    t0 += (float)sc * h2;
                    if constexpr (REUSE) {
                        // keep k1 for a retry of this step (PH_BEGIN)
                        if (s == 0 && rl && a.slice_q > 0 && a.retry_reuse)
                            st_cf_rlx(reinterpret_cast<cf *>(a.susp + (size_t)b * SUSP_WORDS + r), k);
                    }
                } else {                                                     // :209-210
                    sols = cadd(sols, cdivs(cscale(cscale(k, dt), 1.0f), 6.0f));
                    x = sols;
                }
                s++;
                if (s == 4 && a.max_corr <= 0) step_end = true;
            } else {                                                         // :228-249
                x = csub(x, k);
                ncorr++;
                const float vs = rl ? k.x * k.x + k.y * k.y : 0.0f;
                const float vc = rl ? x.x * x.x + x.y * x.y : 0.0f;
                const float ns = tree_sum_half(vs), nc = tree_sum_half(vc);
                isSucc = (double)ns < 0.000001 * (double)nc;
                isInf = (double)nc > 1e14;
                if (isInf || isSucc || (s - 4) + 1 >= a.max_corr) step_end = true;
                else s++;
            }
            if (step_end) {
                if (isInf) {                                                 // :252
                    ph = PH_FINISH;
                } else {
                    if (!isSucc) {                                           // :257-265
                        dt = (float)((double)dt * 0.5);
                        x = xl;
                        sols = xl;
                        succ = 0;
                        t0 = t_step;
                        // the retry starts where this step started: its k1 is this step's
                        if constexpr (REUSE) k1v = a.slice_q > 0 && a.retry_reuse;
                    } else {                                                 // :266-275
                        succ++;
                        xl = x;
                        sols = x;
                        if (succ >= a.inc_steps) { succ = 0; dt *= 2.0f; }
                    }
                    stepidx++;
                    ph = PH_BEGIN;
                }
            }
        }
    }
#ifdef HC_DIAG_TIMES
    if (lane == 0) {
        const unsigned long long w1 = __builtin_amdgcn_s_memrealtime();
        atomicMax(&g_diag_span[1], w1);
        atomicAdd(&g_diag_span[2], w1 - diag_w0);
        atomicAdd(&g_diag_span[3], 1ull);
    }
#endif
#ifdef HC_DIAG_PHASES
    HC_DIAG_MARK(0);
    if (lane == 0) {
        dg[7] = __builtin_amdgcn_s_memtime() - dt0_;
        for (int q = 0; q < 8; q++) atomicAdd(&g_diag_phase[q], (unsigned long long)dg[q]);
        atomicAdd(&g_diag_phase[8], 1ull);
    }
#endif
#undef HC_DIAG_MARK
