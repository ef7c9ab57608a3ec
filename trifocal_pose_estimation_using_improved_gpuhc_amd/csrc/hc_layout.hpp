// What the host side and the kernels of hc_kernels.hip must agree on: the
// caller-owned workspace, the kernels' argument blocks, the time-slicing area's
// counters and sizes, the dequeue order and the workgroup shape.
#pragma once

#include <stddef.h>

#include "hc_lu.hpp"
#include "../../include/hc_trifocal.h"

namespace hc {

// Longest-processing-time-first dequeue order (scripts/make_track_order.py):
// queue position q -> track c_track_order[q / N], sample q % N.  Results are
// per batch id, so the order only changes when a path runs, not what it computes.
__constant__ int c_track_order[NTRK] = {
#include "hc_track_order.inc"
};
__device__ __forceinline__ int path_of_queue_pos(int q, int num_paths, int ordered) {
    if (!ordered) return q;
    const int n = num_paths / NTRK;          // samples in this launch
    const int rank = q / n;
    return (q - rank * n) * NTRK + c_track_order[rank];
}

constexpr int PRIO_TENTHS = 10;   // issue-priority levels over the queue (k_track)
constexpr int WG_THREADS = 256;
constexpr int WAVES_PER_WG = WG_THREADS / WAVE;

// The caller-owned workspace (hc_trifocal_workspace_size()).
struct Workspace {
    // control block, zeroed by k_prep_tables every launch (first 64 bytes)
    unsigned queue;          // path work queue
    unsigned status;         // HC_ERROR_TABLE if the index table does not fit the compaction
    unsigned found;          // device-side "good hypothesis found" flag
    unsigned pad0;
    unsigned long long t_start;   // s_memrealtime when the first workgroup started (abort mode)
    unsigned long long t_found;   // s_memrealtime of the first good hypothesis
    unsigned ring_fail[4];   // time slicing: ticket, tag seen, tail, head of a ring entry that never came (diagnostics)
    unsigned abandoned;      // time slicing: ring tickets abandoned by their consumers (re-pushed; diagnostics)
    unsigned pad1[3];
    // written by k_prep_tables
    EvalTables tab;
    // the throughput tracking kernel's operand addresses (hc_eval.hpp), built with tab and valid with it
    AbsTables abs;
};
static_assert(offsetof(Workspace, tab) == 64, "control block is 64 bytes");
static_assert(ABS_WAVES == WAVES_PER_WG && offsetof(Workspace, abs) % 16 == 0, "one table block per wave, 16-B words");
static_assert(sizeof(Workspace) < (1u << 20), "the base workspace stays below 1 MiB");

// Time slicing (hc_ring.hpp).  Suspend block of path b (32 x 8 B): words 0..29 = x, word 30 = (t0, dt),
// word 31 = (stepidx | nsteps << 16, ncorr | succ << 16 | flags << 30); the
// launcher enables slicing only where these fields fit (slice_fits).  While its
// path runs on a slot, words 0..29 hold the first RK4 slope of the path's
// current step (retry reuse, hc_track_body.inc).
constexpr int SUSP_WORDS = 32;
// Steps per time slice: SLICE_Q while at most one suspended path per path slot
// waits (the launch's end, where the rotation's granularity sets the tail;
// profiles/r2n_ab_slice*.jsonl, r3d_ab_lu_slicing.jsonl), SLICE_QBIG while
// more wait (round 3: as fair a rotation with fewer hand-overs, 239 vs 339 MB
// of HBM traffic per config-2 launch at the same launch time;
// profiles/r3g_ab_quantum.jsonl, r3h_ab_quantum.jsonl).
constexpr int SLICE_Q = 3;
constexpr int SLICE_QBIG = 8;
__host__ __device__ constexpr bool slice_fits(int max_steps, int max_corr, int inc_steps) {
    return max_steps >= 0 && max_steps < 16000 && inc_steps >= 0 && inc_steps < 16384 && max_corr >= 0 &&
           (long long)max_corr * (max_steps + 2) < 65536;
}
// Ring: one entry per ticket, never reused within a launch.  A path is
// suspended only after running SLICE_Q steps since it (re)started and runs at
// most max_steps + 1 steps, so a launch pushes at most
// paths * ((max_steps + 1) / SLICE_Q) entries.  (A reused slot is not safe: a
// wave can be paused for hundreds of ms between taking a ticket and reading
// its entry while the rest of its kernel runs on -- seen when another stream's
// first launch created its hardware queue -- and a slot reused meanwhile would
// lose the suspended path; profiles/r2zb_stress*.jsonl.)
// RING_SLACK more entries absorb the re-pushes of abandoned tickets (below).
constexpr unsigned long long RING_SLACK = 4096ull;
__host__ __device__ constexpr unsigned long long ring_entries(long long paths, int max_steps) {
    return (unsigned long long)paths * (unsigned long long)((max_steps + 1) / (SLICE_Q > 0 ? SLICE_Q : 1) + 1) +
           RING_SLACK;
}

struct KArgs {
    int num_paths;
    int ordered;        // dequeue track-major in c_track_order (abort mode off)
    int truncate;       // depth-sign path truncation (..._TrunPaths.cu:148-155); 0 = PH_CodeOpt
    int explicit_rk;    // archived ..._PH: explicit RK helpers (dev-get-new-data.cuh:37-71)
    int max_steps, max_corr, inc_steps;
    const cf *start_sols;
    const cf *const *start_sols_array;
    cf *tracks;
    cf *const *track_array;
    const cf *start_params;
    const cf *target_params;
    const cf *diff_params;
    uint8_t *conv;
    uint8_t *inf;
    hcPathStats *stats;
    Workspace *ws;
    // abort mode
    int num_edgels;
    int inflight_stop;  // paths in flight stop at their next step boundary once a pose is found
    const float *edgels;
    const float *K;
    uint8_t *found_flag;
    unsigned *peer_found;           // cross-process flag of a multi-GPU run (hcAbortArgs::peer_found), or null
    int32_t *batch_index;
    // time slicing (slice_q > 0; tracking without abort only)
    int slice_q;
    int ring_test;                  // tests only (hc_trifocal_set_ring_test): pusher delay in ticks, else 0
    unsigned ring_cap;
    int retry_reuse;                // a rejected step's retry takes its first RK4 slope from the suspend block
                                    // (hc_track_body.inc; off: tests only, hc_trifocal_set_retry_reuse)
    unsigned *rq;                  // ring counters, one 256-B line each: [0] head, [64] tail, [128] avail, [192] meta
    unsigned long long *susp;       // suspend blocks, SUSP_WORDS per path id
    unsigned long long *ring;       // ring_tag(epoch, ticket) << 32 | path id
    // grouped abort mode (hcGroupedAbortArgs): the scene and the found flag of
    // a path's own triplet instead of edgels / K / ws->found / found_flag
    const hcTripletGroup *groups;
    const int32_t *sample_group;
    unsigned *group_found;
    unsigned long long *group_ticks;   // or null
    // gated abort mode (hcJointGate; k_track_gated only)
    float gate_ratio;
    int32_t *joint_inliers;            // or null
    // adaptive sample limit (hcAdaptiveGate; k_track_adaptive only): a path of sample s of group t is
    // not tracked once sample_ordinal[s] >= group_limit[t]; a scored path lowers the limit to
    // need[need_offset[t] + cJ]
    const int32_t *need;
    const long long *need_offset;
    const int32_t *sample_ordinal;
    unsigned *group_limit;
};
// rq layout: counters zeroed by k_prep_tables every launch; meta: the launch
// epoch, a magic word and the ring entries already cleared (persist)
constexpr int RQ_HEAD = 0, RQ_TAIL = 64, RQ_AVAIL = 128, RQ_EPOCH = 192, RQ_MAGIC = 193, RQ_CLEARED = 194,
              RQ_DLO = 195, RQ_DHI = 196,
              RQ_WORDS = 256;
constexpr unsigned RQ_MAGIC_VALUE = 0x48435432u;   // "HCT2" (the ring-first layout of round 4)

struct PrepArgs {
    const int32_t *U;
    Workspace *ws;
    const uint8_t *found_in;     // abort mode: the (cross-rank reduced) found flag, else null
    const unsigned *peer_found;  // abort mode: the cross-process flag, or null
    unsigned *rq;                // time slicing, else null
    unsigned long long *ring;
    unsigned ring_cap;
    unsigned susp_entry0, susp_entry1;   // the suspend blocks' span in ring-entry units (from the ring's start)
};

}  // namespace hc
