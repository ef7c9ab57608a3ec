// The tracker kernels: six __global__ wrappers around one textually included
// body (hc_track_body.inc; DESIGN.md §3 on why it is no function template).
#pragma once

#include "hc_layout.hpp"
#include "hc_ring.hpp"
#include "hc_score.hpp"

namespace hc {

// Phases of a path slot (one per half-wave):
enum : int { PH_DEQ = 0, PH_BEGIN = 1, PH_STAGE = 2, PH_FINISH = 3, PH_IDLE = 4 };

#ifdef HC_DIAG_TIMES
// diagnostic build: [0] first wave start, [1] last wave exit (s_memrealtime),
// [2] summed wave lifetimes, [3] waves
__device__ unsigned long long g_diag_span[4] = {~0ull, 0ull, 0ull, 0ull};
#ifdef HC_DIAG_UTIL
// diagnostic build (with HC_DIAG_TIMES): per 10.24-us bin of s_memrealtime
// (modulo 8192 bins = 84 ms), the path-stages and the wave-stages started
// (64 copies of each bin, picked by workgroup, so the atomics do not serialise)
constexpr int UTIL_BINS = 8192, UTIL_COPIES = 64;
__device__ unsigned long long g_diag_util[UTIL_COPIES][UTIL_BINS][2];
#endif
#endif
#ifdef HC_DIAG_PHASES
// diagnostic build: per-phase shader cycles summed over waves (k_track):
// [0] slot phases, [1] park + p(t), [2] dH/dx, [3] dH/dt | H, [5] LU,
// [6] stage update, [7] wave lifetime, [8] waves
__device__ unsigned long long g_diag_phase[13];
#endif

// Tuning defaults (a variant build overrides them with -D, scripts/build_variant.sh).
// The small-launch kernels (k_track_small): such a launch needs few waves, so
// the registers go to 3 waves/SIMD: no spills and 16 columns per LU batch
// (profiles/r7g_ab_small_occupancy.jsonl: a further -5 % at 1-4 samples,
// -4..-7 % at 8-16; 6144 path slots)
#ifndef HC_SMALL_MINW
#define HC_SMALL_MINW 3
#endif
#ifndef HC_SMALL_LAT
#define HC_SMALL_LAT 16
#endif
// The abort kernels (k_track<true, ...>, k_track_grouped, k_track_gated, k_track_adaptive):
// 4 waves/SIMD (the scoring path needs the registers).  Their term tables left
// the LDS in round 5, where the other waves' LDS traffic was delaying the
// earliest hypotheses (time to the first pose -2.8 %,
// profiles/r5q_ttfp_probe.jsonl); no kernel stages them there any more
#ifndef HC_ABORT_MINW
#define HC_ABORT_MINW 4
#endif
// Abort mode's issue priority falls by one level per 1 / HC_ABORT_PRIO_DIV of
// the launch's paths in queue order (hc_track_body.inc, "first come, first served")
#ifndef HC_ABORT_PRIO_DIV
#define HC_ABORT_PRIO_DIV 16
#endif

// kernel_GPUHC_trifocal_pose_PH_CodeOpt_TrunPaths (..._TrunPaths.cu:45-290) and,
// with ABORT, ..._TrunPaths_TrunRANSAC (..._TrunRANSAC.cu:45-327).
// MINW: waves per SIMD the register allocation targets.  The term tables are
// read from the workspace (global, L1/L2-resident), which leaves 27.6 KB LDS
// per workgroup (5 workgroups per CU); GTAB once chose between that and a
// staging copy in LDS, and is always true.
// ARCH: the archived ablation semantics (KArgs::truncate / explicit_rk read at
// run time); a separate instantiation so the headline kernel carries neither
// switch and the two show up under their own names in a kernel trace.
// LUS: the LU's column groups classed by this problem's dH/dx structure
// (hc_lu_struct.hpp LU_STRUCT_PAT / LU_BOUND: never-fillable groups untested,
// always-live groups unconditional, narrowed pivot search).  Every launch
// enqueues both instantiations; k_prep_tables decides on the device which one
// tracks (EvalTables::lu_struct) and the other returns at once, so a table of
// any structure the reference kernel takes (e.g. the same system with its
// equations permuted) tracks, through the structure-agnostic LU.
template <bool ABORT, int MINW, bool GTAB, bool ARCH = false, bool LUS = true>
__global__ void __launch_bounds__(WG_THREADS, MINW) k_track(KArgs a) {
    // GTAB remains only for the kernel's name (traces, scripts/isa_phases.py),
    // until a version that moves the build id anyway
    static_assert(GTAB, "the term tables are read from the workspace");
    constexpr bool GROUPED = false, GATED = false;   // (k_track_grouped, k_track_gated below)
    constexpr bool P2C = false;                      // (k_track_p2c below)
    constexpr bool ADAPT = false;                    // (k_track_adaptive below)
    // LU (hc_lu.hpp): the abort kernel's time to the first pose is a lone
    // path's latency, so it runs the latency mode (one LDS round trip per pivot
    // step, in batches of HC_LU_LATB_COLS columns); the tracking kernel the
    // throughput mode (profiles/r6x_ab_track_latency_lu.jsonl: the latency mode
    // is 9 % slower per config-2 launch there)
    constexpr int LULAT = ABORT ? HC_LU_LATB_COLS : 0;
#include "hc_track_body.inc"
}

// Tracking launches that fill at most half of the path slots: the SIMDs are
// short of waves, a path's latency sets the launch time, and the latency-mode
// LU is faster (profiles/r6y_ab_small_launch.jsonl: 1-8 samples -16..-19 %,
// 16 samples -5 %, 24 equal, 100 +9 %).  The same body as k_track, at
// HC_SMALL_MINW waves/SIMD and HC_SMALL_LAT columns per LU batch (above).
template <bool LUS>
__global__ void __launch_bounds__(WG_THREADS, HC_SMALL_MINW) k_track_small(KArgs a) {
    constexpr bool ABORT = false, ARCH = false, GROUPED = false, GATED = false, P2C = false, ADAPT = false;
    constexpr int LULAT = HC_SMALL_LAT;
#include "hc_track_body.inc"
}

// Grouped (multi-triplet) abort launches (hcGroupedAbortArgs): the abort
// instantiation's body and configuration (k_track<true, HC_ABORT_MINW, true>)
// with GROUPED on: the scoring set, K and the found flag are those of the
// path's own triplet, looked up from the slot's sample where they are used
// (nothing of a group is carried across the stage loop).  A kernel of its own
// rather than one more template parameter of k_track, so the existing
// instantiations keep their code and their names in kernel traces.
template <bool LUS>
__global__ void __launch_bounds__(WG_THREADS, HC_ABORT_MINW) k_track_grouped(KArgs a) {
    constexpr bool ABORT = true, ARCH = false, GROUPED = true, GATED = false, P2C = false, ADAPT = false;
    constexpr int LULAT = HC_LU_LATB_COLS;
#include "hc_track_body.inc"
}

// Gated abort launches (hcJointGate): k_track_grouped's configuration and body
// with GATED on, which replaces the scoring block alone: the candidate filter
// and the counts are the pose-support ones (score_joint_half), and a triplet's
// flag is raised by the joint count against KArgs::gate_ratio.  Again a kernel
// of its own, so the grouped instantiations keep their code.
template <bool LUS>
__global__ void __launch_bounds__(WG_THREADS, HC_ABORT_MINW) k_track_gated(KArgs a) {
    constexpr bool ABORT = true, ARCH = false, GROUPED = true, GATED = true, P2C = false, ADAPT = false;
    constexpr int LULAT = HC_LU_LATB_COLS;
#include "hc_track_body.inc"
}

// The archived parameter-to-coefficient tracker (include/p2c/hc_trifocal_p2c.h;
// kernel_GPUHC_trifocal_pose_P2C, arxived ..._P2C.cu:56-263): the archived ..._PH
// instantiation's body and configuration (k_track<false, 5, true, true>: ARCH,
// launched with truncate = 0 and explicit_rk = 1, throughput LU, 5 waves/SIMD)
// with P2C on, which starts a path at a step of 0.05 and builds the slot's
// prefix tables from the sample's coefficient blocks, interpolated at the
// slot's t (hc_eval.hpp build_prefixes_p2c), instead of from p(t).  The
// archived kernel's other differences from ..._PH follow from that: its clamp
// 1 - 0.05 - t0 is PH's 0.95 - t0 in double, its third stage keeps the second's
// coefficients (the same t), and its corrector evaluates H from the Hx
// coefficients of the fourth stage (tp at the step's last t).  No time slicing
// and no small-launch variant.  Again a kernel of its own, so the existing
// instantiations keep their code.
template <bool LUS>
__global__ void __launch_bounds__(WG_THREADS, 5) k_track_p2c(KArgs a) {
    constexpr bool ABORT = false, ARCH = true, GROUPED = false, GATED = false, P2C = true, ADAPT = false;
    constexpr int LULAT = 0;
#include "hc_track_body.inc"
}

// The gated launch with an adaptive sample limit (include/adaptive/hc_trifocal_adaptive.h,
// hcAdaptiveGate): k_track_gated's configuration and body with ADAPT on, which adds
// three pieces: a path is also skipped at dequeue (and, with inflight_stop, stopped
// at a step boundary) once its sample's ordinal within its triplet has reached the
// triplet's limit KArgs::group_limit[t], and a scored path lowers that limit to the
// caller's table entry of its joint count (one agent-scope atomicMin).  Again a
// kernel of its own, named after all the others, so the existing instantiations
// keep their code and their names in kernel traces.
template <bool LUS>
__global__ void __launch_bounds__(WG_THREADS, HC_ABORT_MINW) k_track_adaptive(KArgs a) {
    constexpr bool ABORT = true, ARCH = false, GROUPED = true, GATED = true, P2C = false, ADAPT = true;
    constexpr int LULAT = HC_LU_LATB_COLS;
#include "hc_track_body.inc"
}

}  // namespace hc
