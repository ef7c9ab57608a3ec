// hc_kernels.hip -- MI355X (gfx950) GPU-HC tracker kernels + the C-ABI of
// include/hc_trifocal.h.
//
// Replaces magmaHC/gpu-kernels/kernel_GPUHC_trifocal_2op1p_30x30_PH_CodeOpt_TrunPaths[_TrunRANSAC][_Volta].cu
// (the four CUDA/MAGMA kernels + launchers, magmaHC-kernels.hpp:24-105).
//
// Design: a persistent grid of 256-thread workgroups.  Each
// wavefront tracks two homotopy paths at a time, one per 32-lane half (lane
// r < 30 of a half owns Jacobian row r, RHS r and x_r in VGPRs).  A half
// whose path ends dequeues the next path id b = sample*312 + track from a
// device work queue (one agent-scope atomicAdd per path), so no slot idles
// while work remains.  One loop iteration runs one predictor or corrector
// "stage" for both halves: p(t) (LDS) + dH/dt|H + dH/dx from the compacted
// index tables + the register LU.  Early abort (TrunRANSAC) scores converged
// paths on the device and raises an agent-scope flag.
//
// One translation unit: the device side is the headers below, one per concern,
// this file the host side.  The plain kernels are emitted in the order of these
// includes (k_prep_tables, k_cgesv, k_eval, k_ring_check), which is part of the
// library's build id: keep it.  (The P2C mode's plain kernels
// are templates for that reason: hc_p2c.hpp.)
#include "hc_layout.hpp"
#include "hc_prep.hpp"
#include "hc_components.hpp"
#include "hc_ring.hpp"
#include "hc_score.hpp"
#include "hc_track.hpp"
#include "hc_p2c.hpp"
#include "../../include/hc_trifocal_testing.h"
#include "../../include/p2c/hc_trifocal_p2c.h"
#include "../../include/lu/hc_lu_testing.h"
#include "../../include/lu/hc_lu_rowtable_testing.h"
#include "../../include/lu/hc_lu_compact_testing.h"
#include "../../include/eval/hc_eval_testing.h"
#include "../../include/adaptive/hc_trifocal_adaptive.h"

#include <atomic>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <utility>

namespace hc {

// ---------------------------------------------------------------- host side
thread_local hipError_t g_last_hip_error = hipSuccess;   // shared with hc_pose.hip (hc_last_error_string)
static inline hcStatus launch_status(hcStatus on_fail) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { g_last_hip_error = e; return on_fail; }
    return HC_SUCCESS;
}

static size_t ws_bytes_needed() { return (sizeof(Workspace) + 255) & ~(size_t)255; }
// + the time-slicing area of a launch of `paths` paths: the ring counters, the
// ring, then a suspend block per path.  The ring starts at a fixed offset, so
// a workspace reused for launches of other sizes keeps its entry i at one
// address (RQ_CLEARED counts entries from there); the suspend blocks follow
// this launch's ring (256-B aligned) and may overwrite cleared entries past
// it: k_prep_tables keeps that span as the dirty range (RQ_DLO, RQ_DHI) and
// re-zeroes it when a later launch's ring covers it.
struct SliceLayout {
    size_t rq, ring, susp;                // byte offsets from the workspace's base
    size_t total;                         // workspace bytes that hold all of it (hc_trifocal_workspace_size_for_steps)
    unsigned long long ring_cap;          // ring entries
    size_t susp_entry0, susp_entry1;      // the suspend blocks' span in ring-entry units (PrepArgs)
};
static SliceLayout slice_layout(long long paths, int max_steps) {
    if (paths < 0) paths = 0;
    if (max_steps < 0) max_steps = 0;
    SliceLayout a;
    a.ring_cap = ring_entries(paths, max_steps);
    const size_t ring_bytes = ((size_t)a.ring_cap * sizeof(unsigned long long) + 255) & ~(size_t)255;
    a.rq = ws_bytes_needed();
    a.ring = a.rq + RQ_WORDS * sizeof(unsigned);
    a.susp = a.ring + ring_bytes;
    a.total = a.susp + (size_t)paths * SUSP_WORDS * sizeof(unsigned long long);
    a.susp_entry0 = ring_bytes / 8;
    a.susp_entry1 = a.susp_entry0 + (size_t)paths * SUSP_WORDS;
    return a;
}
// Time slicing when the workspace has room for the area and the step counters
// fit the suspend block (slice_fits); KArgs::ring_cap and PrepArgs::susp_entry1
// are 32-bit words, so only where the ring and the suspend blocks' span fit them.
static bool sliced_launch(bool abort_mode, const hcTrackSettings &st, const SliceLayout &a, size_t wsb) {
    return !abort_mode && SLICE_Q > 0 && wsb >= a.total && a.ring_cap < 0xFFFFFF00ull &&
           a.susp_entry1 < (size_t)UINT_MAX && slice_fits(st.max_steps, st.max_corrections, st.delta_t_inc_steps);
}
// tests only (hc_trifocal_set_ring_test, include/hc_trifocal_testing.h): pusher
// delay of every 16th ring ticket; read by every launch of every thread
static std::atomic<int> g_ring_test{0};
// tests only (hc_trifocal_set_small_launch): -1 never the small-launch
// kernels, 0 by size, 1 always (tracking launches)
static std::atomic<int> g_small_launch{0};
// tests only (hc_trifocal_set_retry_reuse): 0 a sliced launch's retries
// recompute their first slope, as unsliced launches always do
static std::atomic<int> g_retry_reuse{1};

// Persistent grid: resident workgroups (occupancy API, cached per device and
// kernel) x CUs, capped by the work.  resident_wgs(k) = grid_for(INT_MAX, k).
static int grid_for(int waves_needed, const void *kernel) {
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, std::pair<int, int>> cache;   // -> (CUs, workgroups per CU)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    int cus = 0, per_cu = 0;
    {
        std::lock_guard<std::mutex> g(mu);
        auto it = cache.find({dev, kernel});
        if (it == cache.end()) {
            if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return -1;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, WG_THREADS, 0) != hipSuccess) per_cu = 1;
            if (per_cu < 1) per_cu = 1;
            it = cache.emplace(std::make_pair(dev, kernel), std::make_pair(cus, per_cu)).first;
        }
        cus = it->second.first;
        per_cu = it->second.second;
    }
    const int want = waves_needed / WAVES_PER_WG + (waves_needed % WAVES_PER_WG != 0);
    const int cap = cus * per_cu;
    return want < cap ? want : cap;
}
static int resident_wgs(const void *kernel) { return grid_for(INT_MAX, kernel); }

// The launches that exist, one per tracking entry point of hc_trifocal.h, and
// the one argument block each needs besides hcTrackArgs (the others stay null).
// Declared in the order of track_kernels' table (P2c: the pair named after it).
enum class TrackMode { GatedAbort, GroupedAbort, Abort, Ph, PhCodeopt, Track, P2c };
struct TrackLaunch {
    TrackMode mode;
    const hcAbortArgs *ab = nullptr;          // Abort
    const hcGroupedAbortArgs *gr = nullptr;   // GroupedAbort, GatedAbort (non-null: checked by the entry point)
    const hcJointGate *jg = nullptr;          // GatedAbort (validated by its entry point); with pad ==
                                              // HC_GATE_ADAPTIVE the head of an hcAdaptiveGate
    const hcP2cArgs *p2c = nullptr;           // P2c (non-null, its pointers too: checked by the entry point)
};

// (mode, small-launch decision) -> the kernel whose LU is specialised to this
// problem's dH/dx structure and its structure-agnostic twin.
// Term tables read from the workspace (L1/L2).  Tracking: 96 VGPRs, 31 KB
// LDS per workgroup -> 5 waves/SIMD.  Abort mode: HC_ABORT_MINW
// (hc_track.hpp).  The device compiler emits the instantiations in the order
// this function first names them, after the plain kernels: a
// new kernel is named after all of them, as the P2C pair below.
struct TrackKernels { const void *lus, *any; };
static TrackKernels track_kernels(TrackMode mode, bool small, bool adaptive = false) {
    static const void *const by_mode[2][6] = {
        {(const void *)k_track_gated<true>, (const void *)k_track_grouped<true>,
         (const void *)k_track<true, HC_ABORT_MINW, true>, (const void *)k_track<false, 5, true, true>,
         (const void *)k_track<false, 5, true, true>, (const void *)k_track<false, 5, true>},
        {(const void *)k_track_gated<false>, (const void *)k_track_grouped<false>,
         (const void *)k_track<true, HC_ABORT_MINW, true, false, false>,
         (const void *)k_track<false, 5, true, true, false>, (const void *)k_track<false, 5, true, true, false>,
         (const void *)k_track<false, 5, true, false, false>}};
    if (small) return {(const void *)k_track_small<true>, (const void *)k_track_small<false>};
    // (named last, after the small-launch pair: every older instantiation keeps its place)
    if (mode == TrackMode::P2c) return {(const void *)k_track_p2c<true>, (const void *)k_track_p2c<false>};
    // (and after those: the gated launch's adaptive mode, hcAdaptiveGate)
    if (mode == TrackMode::GatedAbort && adaptive)
        return {(const void *)k_track_adaptive<true>, (const void *)k_track_adaptive<false>};
    return {by_mode[0][(int)mode], by_mode[1][(int)mode]};
}

// A tracking launch goes to the latency-mode instantiations when at most half
// of the throughput kernel's path slots would be filled and every path is in a
// slot of the small kernel at once (or when the testing hook forces it)
static bool small_launch(TrackMode mode, long long paths) {
    const int small_mode = g_small_launch.load(std::memory_order_relaxed);
    if (mode != TrackMode::Track || small_mode < 0) return false;
    const long long slots = 2ll * WAVES_PER_WG * resident_wgs(track_kernels(mode, false).lus);   // two paths per wave
    const long long small_slots = 2ll * WAVES_PER_WG * resident_wgs(track_kernels(mode, true).lus);
    return small_mode > 0 || (slots > 0 && 2 * paths <= slots && paths <= small_slots);
}

static hcStatus enqueue_track(const void *kern, int grid, KArgs &k, hipStream_t s) {
    void *kargs[] = {&k};
    g_last_hip_error = hipLaunchKernel(kern, dim3(grid), dim3(WG_THREADS), kargs, 0, s);
    if (g_last_hip_error != hipSuccess) return HC_ERROR_LAUNCH;
    return launch_status(HC_ERROR_LAUNCH);
}

static hcStatus launch_track(const hcTrackArgs *t, const TrackLaunch &l, void *workspace, size_t wsb,
                             hcStream stream) {
    const bool gated = l.mode == TrackMode::GatedAbort;
    const bool grouped = gated || l.mode == TrackMode::GroupedAbort;
    const bool abort_mode = grouped || l.mode == TrackMode::Abort;
    const hcAbortArgs *ab = l.mode == TrackMode::Abort ? l.ab : nullptr;
    const hcGroupedAbortArgs *gr = grouped ? l.gr : nullptr;
    const hcP2cArgs *pc = l.mode == TrackMode::P2c ? l.p2c : nullptr;
    // the gated launch's adaptive mode: the gate is the head of an hcAdaptiveGate
    const hcAdaptiveGate *ag =
        gated && l.jg->pad == (int32_t)HC_GATE_ADAPTIVE ? reinterpret_cast<const hcAdaptiveGate *>(l.jg) : nullptr;
    if (!t || t->sub_ransac_iters < 0) return HC_ERROR_INVALID_VALUE;
    if (grouped && (gr->num_groups < 1 || !gr->groups || !gr->sample_group || !gr->group_found ||
                    !gr->trifocal_sols_batch_index))
        return HC_ERROR_INVALID_VALUE;
    if (ag && (!ag->need || !ag->need_offset || !ag->sample_ordinal || !ag->group_limit)) return HC_ERROR_INVALID_VALUE;
    if (!workspace || wsb < ws_bytes_needed()) return HC_ERROR_WORKSPACE;
    if (t->sub_ransac_iters == 0) return HC_SUCCESS;
    if ((!t->start_sols && !t->start_sols_array) || (!t->tracks && !t->track_array) || !t->converge || !t->infinity)
        return HC_ERROR_INVALID_VALUE;
    // (the P2C launch reads its own tables and coefficient blocks instead)
    if (!pc && (!t->start_params || !t->target_params || !t->diff_params || !t->unified_index))
        return HC_ERROR_INVALID_VALUE;
    if (t->settings.max_steps < 0 || t->settings.max_corrections < 0 || t->settings.delta_t_inc_steps < 0)
        return HC_ERROR_INVALID_VALUE;
    if (l.mode == TrackMode::Abort && (!ab || ab->num_triplet_edgels <= 0 || !ab->triplet_edge_locations ||
                                       !ab->intrinsic_matrix || !ab->found_trifocal_sols ||
                                       !ab->trifocal_sols_batch_index))
        return HC_ERROR_INVALID_VALUE;
    const long long paths = (long long)t->sub_ransac_iters * NTRK;
    if (paths > 0x7FFFFFFFll) return HC_ERROR_INVALID_VALUE;
    hipStream_t s = (hipStream_t)stream;
    Workspace *ws = (Workspace *)workspace;
    (void)hipGetLastError();  // errors of earlier, unrelated calls are not ours
    KArgs k{};
    k.num_paths = (int)paths;
    // abort mode dequeues sample-major, so whole hypotheses finish as early as possible
    k.ordered = abort_mode ? 0 : 1;
    // the archived ablations: PH_CodeOpt tracks without truncation, PH also with the explicit RK helpers
    // (the archived P2C kernel is ..._PH's in both)
    k.truncate = (l.mode == TrackMode::PhCodeopt || l.mode == TrackMode::Ph || pc) ? 0 : 1;
    k.explicit_rk = (l.mode == TrackMode::Ph || pc) ? 1 : 0;
    k.max_steps = t->settings.max_steps;
    k.max_corr = t->settings.max_corrections;
    k.inc_steps = t->settings.delta_t_inc_steps;
    k.start_sols = (const cf *)t->start_sols;
    k.start_sols_array = (const cf *const *)t->start_sols_array;
    k.tracks = (cf *)t->tracks;
    k.track_array = (cf *const *)t->track_array;
    k.start_params = (const cf *)t->start_params;
    // P2C: the samples' coefficient blocks take the places of target and diff (hc_track_body.inc)
    k.target_params = (const cf *)(pc ? pc->coeffs_hx : t->target_params);
    k.diff_params = (const cf *)(pc ? pc->coeffs_ht : t->diff_params);
    k.conv = t->converge;
    k.inf = t->infinity;
    k.stats = t->stats;
    k.ws = ws;
    // the mode's own argument block
    if (grouped) {
        k.inflight_stop = gr->inflight_stop ? 1 : 0;
        k.batch_index = gr->trifocal_sols_batch_index;
        k.groups = gr->groups;
        k.sample_group = gr->sample_group;
        k.group_found = gr->group_found;
        k.group_ticks = (unsigned long long *)gr->group_found_ticks;
        if (gated) {
            k.gate_ratio = l.jg->min_joint_ratio;
            k.joint_inliers = l.jg->joint_inliers;
        }
        if (ag) {
            k.need = ag->need;
            k.need_offset = (const long long *)ag->need_offset;
            k.sample_ordinal = ag->sample_ordinal;
            k.group_limit = ag->group_limit;
        }
    } else if (ab) {
        k.num_edgels = ab->num_triplet_edgels;
        k.inflight_stop = ab->inflight_stop ? 1 : 0;
        k.peer_found = ab->peer_found;
        k.edgels = ab->triplet_edge_locations;
        k.K = ab->intrinsic_matrix;
        k.found_flag = ab->found_trifocal_sols;
        k.batch_index = ab->trifocal_sols_batch_index;
    }
    const SliceLayout area = slice_layout(paths, t->settings.max_steps);
    const bool sliced = !pc && sliced_launch(abort_mode, t->settings, area, wsb);   // (no time slicing for P2C)
    if (sliced) {
        k.ring_cap = (unsigned)area.ring_cap;
        k.rq = (unsigned *)((char *)workspace + area.rq);
        k.ring = (unsigned long long *)((char *)workspace + area.ring);
        k.susp = (unsigned long long *)((char *)workspace + area.susp);
        k.slice_q = SLICE_Q;
        k.ring_test = g_ring_test.load(std::memory_order_relaxed);
        k.retry_reuse = g_retry_reuse.load(std::memory_order_relaxed);   // (the slope is kept in the suspend block)
    }
    // control block reset, compacted tables (skipped when cached), ring reset
    // (a grouped launch's flags are the caller's group_found words: Workspace::found stays 0, unused)
    PrepArgs pa{pc ? pc->hx_index : t->unified_index, ws, ab ? ab->found_trifocal_sols : nullptr, ab ? ab->peer_found : nullptr,
                k.rq, k.ring, k.ring_cap,
                sliced ? (unsigned)area.susp_entry0 : 0u,
                sliced ? (unsigned)area.susp_entry1 : 0u};
    if (pc) hipLaunchKernelGGL(k_prep_tables_p2c<true>, dim3(1), dim3(PREP_THREADS), 0, s, pa, pc->ht_index);
    else hipLaunchKernelGGL(k_prep_tables, dim3(1), dim3(PREP_THREADS), 0, s, pa);
    if (launch_status(HC_ERROR_LAUNCH) != HC_SUCCESS) return HC_ERROR_LAUNCH;
    // the twin is enqueued after the specialised kernel: exactly one of the two
    // tracks (EvalTables::lu_struct), the other returns at its first load
    const TrackKernels kern = track_kernels(l.mode, small_launch(l.mode, paths), ag != nullptr);
    const int grid = grid_for((int)((paths + 1) / 2), kern.lus);
    const int grid_any = grid_for((int)((paths + 1) / 2), kern.any);
    if (grid <= 0 || grid_any <= 0) return HC_ERROR_DEVICE;
    if (enqueue_track(kern.lus, grid, k, s) != HC_SUCCESS) return HC_ERROR_LAUNCH;
    if (enqueue_track(kern.any, grid_any, k, s) != HC_SUCCESS) return HC_ERROR_LAUNCH;
    if (k.rq) {   // a suspended path that was never resumed is reported, not left stale
        hipLaunchKernelGGL(k_ring_check, dim3(1), dim3(64), 0, s, ws, (const unsigned *)k.rq);
        return launch_status(HC_ERROR_LAUNCH);
    }
    return HC_SUCCESS;
}

static hcStatus read_control(const void *workspace, Workspace &h) {
    if (hipMemcpy(&h, workspace, 64, hipMemcpyDeviceToHost) != hipSuccess) return HC_ERROR_DEVICE;
    return HC_SUCCESS;
}

// rate of the s_memrealtime counter (hipDeviceAttributeWallClockRate, kHz)
static double wall_clock_hz() {
    int dev = 0, khz = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess ||
        khz <= 0)
        return 100.0e6;   // gfx9: constant 100 MHz
    return (double)khz * 1.0e3;
}

// A diagnostic build's device counters (hc_diag_*): copied out and, on request,
// put back to `init` (zeros if null)
template <typename T>
static int diag_read(const T &sym, unsigned long long *out, int reset, const T *init = nullptr) {
    void *p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(sym)) != hipSuccess ||
        hipMemcpy(out, p, sizeof(T), hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    if (!reset) return 0;
    return (init ? hipMemcpy(p, init, sizeof(T), hipMemcpyHostToDevice) : hipMemset(p, 0, sizeof(T))) == hipSuccess ? 0 : -1;
}

// tests only (include/lu/hc_lu_testing.h): one of the tracker's solves alone.
// The template parameters are what a tracking kernel that runs the variant
// knows (hc_track.hpp), and lu_mode (hc_lu.hpp) gives the solve from them, as
// in hc_track_body.inc.  Blocks where the variant has the problem's structure:
// the structure check's verdict is read back before the solve is launched.
template <bool ABORT, bool ARCH, int LULAT, bool LUS>
static hcStatus launch_cgesv_variant(int n, const hcComplex *A, const hcComplex *b, hcComplex *x, hipStream_t s) {
    constexpr LuMode M = lu_mode(ABORT, ARCH, LULAT, LUS);
    if (M.strct) {
        unsigned *bad = nullptr, h_bad = 0u;
        if ((g_last_hip_error = hipMalloc((void **)&bad, sizeof(unsigned))) != hipSuccess) return HC_ERROR_DEVICE;
        hipError_t e = hipMemsetAsync(bad, 0, sizeof(unsigned), s);
        if (e == hipSuccess) {
            const size_t rows = (size_t)n * NV;
            hipLaunchKernelGGL(k_cgesv_struct_check, dim3((unsigned)((rows + WG_THREADS - 1) / WG_THREADS)),
                               dim3(WG_THREADS), 0, s, n, (const cf *)A, bad);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&h_bad, bad, sizeof(unsigned), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        (void)hipFree(bad);
        if (e != hipSuccess) {
            g_last_hip_error = e;
            return HC_ERROR_LAUNCH;
        }
        if (h_bad != 0u) return HC_ERROR_INVALID_VALUE;
    }
    const int per = 2 * WAVES_PER_WG;
    hipLaunchKernelGGL((k_cgesv_variant<M.lat, M.strct, M.entchk, M.fuse>), dim3((n + per - 1) / per), dim3(WG_THREADS), 0, s,
                       n, (const cf *)A, (const cf *)b, (cf *)x);
    return launch_status(HC_ERROR_LAUNCH);
}

}  // namespace hc

extern "C" {
#ifdef HC_DIAG_PHASES
int hc_diag_phases(unsigned long long *out, int reset) { return hc::diag_read(hc::g_diag_phase, out, reset); }
#endif
#ifdef HC_DIAG_LUWORK
int hc_diag_luwork(unsigned long long *out, int reset) { return hc::diag_read(hc::g_diag_luwork, out, reset); }
#endif
#ifdef HC_DIAG_LIVE
int hc_diag_live(unsigned long long *out, int reset) { return hc::diag_read(hc::g_diag_live, out, reset); }
#endif
#ifdef HC_DIAG_TIMES
int hc_diag_span(unsigned long long *out, int reset) {
    static const unsigned long long init[4] = {~0ull, 0ull, 0ull, 0ull};
    return hc::diag_read(hc::g_diag_span, out, reset, &init);
}
#endif
#ifdef HC_DIAG_UTIL
int hc_diag_util(unsigned long long *out, int reset) { return hc::diag_read(hc::g_diag_util, out, reset); }
#endif

size_t hc_trifocal_workspace_size(void) { return hc::ws_bytes_needed(); }

size_t hc_trifocal_workspace_size_for(int sub_ransac_iters) {
    return hc_trifocal_workspace_size_for_steps(sub_ransac_iters, 80);
}

size_t hc_trifocal_workspace_size_for_steps(int sub_ransac_iters, int max_steps) {
    return hc::slice_layout(sub_ransac_iters > 0 ? (long long)sub_ransac_iters * hc::NTRK : 0, max_steps).total;
}

hcStatus hc_trifocal_2op1p_30x30_track(const hcTrackArgs *args, void *workspace, size_t workspace_bytes,
                                       hcStream stream) {
    return hc::launch_track(args, {hc::TrackMode::Track}, workspace, workspace_bytes, stream);
}

hcStatus hc_trifocal_2op1p_30x30_track_abort(const hcTrackArgs *args, const hcAbortArgs *abort_args,
                                             void *workspace, size_t workspace_bytes, hcStream stream) {
    return hc::launch_track(args, {hc::TrackMode::Abort, abort_args}, workspace, workspace_bytes, stream);
}

hcStatus hc_trifocal_2op1p_30x30_track_abort_grouped(const hcTrackArgs *args, const hcGroupedAbortArgs *g,
                                                     void *workspace, size_t workspace_bytes, hcStream stream) {
    if (!g) return HC_ERROR_INVALID_VALUE;
    return hc::launch_track(args, {hc::TrackMode::GroupedAbort, nullptr, g}, workspace, workspace_bytes, stream);
}

hcStatus hc_trifocal_2op1p_30x30_track_abort_gated(const hcTrackArgs *args, const hcGroupedAbortArgs *g,
                                                   const hcJointGate *gate, void *workspace,
                                                   size_t workspace_bytes, hcStream stream) {
    if (!g || !gate) return HC_ERROR_INVALID_VALUE;
    // > 0 and finite (the comparison is false for NaN)
    if (!(gate->min_joint_ratio > 0.0f) || gate->min_joint_ratio > 3.402823466e+38f) return HC_ERROR_INVALID_VALUE;
    return hc::launch_track(args, {hc::TrackMode::GatedAbort, nullptr, g, gate}, workspace, workspace_bytes, stream);
}

hcStatus hc_trifocal_2op1p_30x30_track_ph_codeopt(const hcTrackArgs *args, void *workspace, size_t workspace_bytes,
                                                  hcStream stream) {
    return hc::launch_track(args, {hc::TrackMode::PhCodeopt}, workspace, workspace_bytes, stream);
}

hcStatus hc_trifocal_2op1p_30x30_track_ph(const hcTrackArgs *args, void *workspace, size_t workspace_bytes,
                                          hcStream stream) {
    return hc::launch_track(args, {hc::TrackMode::Ph}, workspace, workspace_bytes, stream);
}

hcStatus hc_trifocal_2op1p_30x30_track_p2c(const hcTrackArgs *args, const hcP2cArgs *p2c, void *workspace,
                                           size_t workspace_bytes, hcStream stream) {
    if (!p2c || !p2c->hx_index || !p2c->ht_index || !p2c->coeffs_hx || !p2c->coeffs_ht) return HC_ERROR_INVALID_VALUE;
    hc::TrackLaunch l{hc::TrackMode::P2c};
    l.p2c = p2c;
    return hc::launch_track(args, l, workspace, workspace_bytes, stream);
}

hcStatus hc_trifocal_workspace_status(const void *workspace) {
    if (!workspace) return HC_ERROR_INVALID_VALUE;
    hc::Workspace h;
    const hcStatus st = hc::read_control(workspace, h);
    if (st != HC_SUCCESS) return st;
    if (h.status == 0u) return HC_SUCCESS;
    return h.status == (unsigned)HC_ERROR_TABLE ? HC_ERROR_TABLE : HC_ERROR_DEVICE;
}

hcStatus hc_trifocal_read_timings(const void *workspace, double *first_found_seconds) {
    if (!workspace || !first_found_seconds) return HC_ERROR_INVALID_VALUE;
    hc::Workspace h;
    const hcStatus st = hc::read_control(workspace, h);
    if (st != HC_SUCCESS) return st;
    *first_found_seconds = (h.t_found && h.t_start) ? (double)(long long)(h.t_found - h.t_start) / hc::wall_clock_hz() : -1.0;
    return HC_SUCCESS;
}

hcStatus hc_trifocal_read_timestamps(const void *workspace, uint64_t *start_ticks, uint64_t *found_ticks,
                                     double *tick_hz) {
    if (!workspace || !start_ticks || !found_ticks || !tick_hz) return HC_ERROR_INVALID_VALUE;
    hc::Workspace h;
    const hcStatus st = hc::read_control(workspace, h);
    if (st != HC_SUCCESS) return st;
    *start_ticks = h.t_start;
    *found_ticks = h.t_found;
    *tick_hz = hc::wall_clock_hz();
    return HC_SUCCESS;
}

hcStatus hc_cgesv_30x30_batched(int n, const hcComplex *A, const hcComplex *b, hcComplex *x, hcStream stream) {
    if (n < 0 || (n > 0 && (!A || !b || !x))) return HC_ERROR_INVALID_VALUE;
    if (n == 0) return HC_SUCCESS;
    (void)hipGetLastError();
    const int per = 2 * hc::WAVES_PER_WG;
    hipLaunchKernelGGL(hc::k_cgesv, dim3((n + per - 1) / per), dim3(hc::WG_THREADS), 0, (hipStream_t)stream, n,
                       (const hc::cf *)A, (const hc::cf *)b, (hc::cf *)x);
    return hc::launch_status(HC_ERROR_LAUNCH);
}

// tests only (include/lu/hc_lu_testing.h): launch_cgesv_variant above
hcStatus hc_cgesv_30x30_variant_batched(int variant, int n, const hcComplex *A, const hcComplex *b, hcComplex *x,
                                        hcStream stream) {
    if (variant < 0 || variant >= HC_LU_VARIANT_COUNT) return HC_ERROR_INVALID_VALUE;
    if (n < 0 || (n > 0 && (!A || !b || !x))) return HC_ERROR_INVALID_VALUE;
    if (n == 0) return HC_SUCCESS;
    hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
    switch (variant) {   // a kernel that runs it (hc_track.hpp):  <ABORT, ARCH, LULAT, LUS>
    case HC_LU_VARIANT_THROUGHPUT:      return hc::launch_cgesv_variant<false, false, 0, true>(n, A, b, x, s);
    case HC_LU_VARIANT_THROUGHPUT_TWIN: return hc::launch_cgesv_variant<false, false, 0, false>(n, A, b, x, s);
    case HC_LU_VARIANT_ABORT:           return hc::launch_cgesv_variant<true, false, HC_LU_LATB_COLS, true>(n, A, b, x, s);
    case HC_LU_VARIANT_ABORT_TWIN:      return hc::launch_cgesv_variant<true, false, HC_LU_LATB_COLS, false>(n, A, b, x, s);
    case HC_LU_VARIANT_SMALL:           return hc::launch_cgesv_variant<false, false, HC_SMALL_LAT, true>(n, A, b, x, s);
    case HC_LU_VARIANT_SMALL_TWIN:      return hc::launch_cgesv_variant<false, false, HC_SMALL_LAT, false>(n, A, b, x, s);
    case HC_LU_VARIANT_ARCHIVED:        return hc::launch_cgesv_variant<false, true, 0, true>(n, A, b, x, s);
    case HC_LU_VARIANT_ARCHIVED_TWIN:   return hc::launch_cgesv_variant<false, true, 0, false>(n, A, b, x, s);
    }
    return HC_ERROR_INVALID_VALUE;
}

hcStatus hc_cgesv_30x30_struct_batched(int n, const hcComplex *A, const hcComplex *b, hcComplex *x, hcStream stream) {
    return hc_cgesv_30x30_variant_batched(HC_LU_VARIANT_THROUGHPUT, n, A, b, x, stream);
}

hcStatus hc_trifocal_eval_batched(int n, const int32_t *unified_index, const hcComplex *x, const hcComplex *p,
                                  const hcComplex *d, hcComplex *Hx, hcComplex *Ht, hcComplex *H, void *workspace,
                                  size_t workspace_bytes, hcStream stream) {
    if (n < 0 || !unified_index || (n > 0 && (!x || !p || !d || !Hx || !Ht || !H))) return HC_ERROR_INVALID_VALUE;
    if (!workspace || workspace_bytes < hc::ws_bytes_needed()) return HC_ERROR_WORKSPACE;
    if (n == 0) return HC_SUCCESS;
    hipStream_t s = (hipStream_t)stream;
    hc::Workspace *ws = (hc::Workspace *)workspace;
    (void)hipGetLastError();
    hc::PrepArgs pa{unified_index, ws, nullptr, nullptr, nullptr, nullptr, 0u, 0u, 0u};
    hipLaunchKernelGGL(hc::k_prep_tables, dim3(1), dim3(hc::PREP_THREADS), 0, s, pa);
    if (hc::launch_status(HC_ERROR_LAUNCH) != HC_SUCCESS) return HC_ERROR_LAUNCH;
    const int per = 2 * hc::WAVES_PER_WG;
    hipLaunchKernelGGL(hc::k_eval, dim3((n + per - 1) / per), dim3(hc::WG_THREADS), 0, s, n, ws,
                       (const hc::cf *)x, (const hc::cf *)p, (const hc::cf *)d, (hc::cf *)Hx, (hc::cf *)Ht,
                       (hc::cf *)H);
    return hc::launch_status(HC_ERROR_LAUNCH);
}

// tests only (include/eval/hc_eval_testing.h, include/lu/hc_lu_compact_testing.h):
// k_eval_variant; compact_rows: its CROW form, Hx then n x 30 x LU_COMPACT_W.
// Blocks: the workspace's status is read back once the kernel has run.
static hcStatus eval_variant_run(int variant, bool compact_rows, unsigned flags, int n, const int32_t *unified_index,
                                 const hcComplex *x, const hcComplex *target, const hcComplex *diff,
                                 const hcComplex *start_params, const float *t, const uint8_t *kind, hcComplex *Hx,
                                 hcComplex *rhs, uint8_t *ent_ok, void *workspace, size_t workspace_bytes,
                                 hcStream stream) {
    if (variant < 0 || variant >= HC_EVAL_VARIANT_COUNT || (flags & ~HC_EVAL_REDO) != 0u) return HC_ERROR_INVALID_VALUE;
    const bool abs_tables = variant == HC_EVAL_VARIANT_ABS;
    if (n < 0 || (n > 0 && (!unified_index || !x || !target || !diff || !start_params || !t || !kind || !Hx || !rhs ||
                            (abs_tables && !ent_ok))))
        return HC_ERROR_INVALID_VALUE;
    if (!workspace || workspace_bytes < hc::ws_bytes_needed()) return HC_ERROR_WORKSPACE;
    if (n == 0) return HC_SUCCESS;
    hipStream_t s = (hipStream_t)stream;
    hc::Workspace *ws = (hc::Workspace *)workspace;
    (void)hipGetLastError();
    hc::PrepArgs pa{unified_index, ws, nullptr, nullptr, nullptr, nullptr, 0u, 0u, 0u};
    hipLaunchKernelGGL(hc::k_prep_tables, dim3(1), dim3(hc::PREP_THREADS), 0, s, pa);
    if (hc::launch_status(HC_ERROR_LAUNCH) != HC_SUCCESS) return HC_ERROR_LAUNCH;
    const int per = 2 * hc::WAVES_PER_WG;
    const dim3 grid((n + per - 1) / per), block(hc::WG_THREADS);
    const int redo = (flags & HC_EVAL_REDO) ? 1 : 0;
    if (compact_rows)
        hipLaunchKernelGGL((hc::k_eval_variant<true, true>), grid, block, 0, s, n, redo, ws, (const hc::cf *)x,
                           (const hc::cf *)target, (const hc::cf *)diff, (const hc::cf *)start_params, t, kind,
                           (hc::cf *)Hx, (hc::cf *)rhs, ent_ok);
    else if (abs_tables)
        hipLaunchKernelGGL(hc::k_eval_variant<true>, grid, block, 0, s, n, redo, ws, (const hc::cf *)x,
                           (const hc::cf *)target, (const hc::cf *)diff, (const hc::cf *)start_params, t, kind,
                           (hc::cf *)Hx, (hc::cf *)rhs, ent_ok);
    else
        hipLaunchKernelGGL(hc::k_eval_variant<false>, grid, block, 0, s, n, redo, ws, (const hc::cf *)x,
                           (const hc::cf *)target, (const hc::cf *)diff, (const hc::cf *)start_params, t, kind,
                           (hc::cf *)Hx, (hc::cf *)rhs, ent_ok);
    if (hc::launch_status(HC_ERROR_LAUNCH) != HC_SUCCESS) return HC_ERROR_LAUNCH;
    unsigned ctl[16];   // the control block (hc_layout.hpp: 64 bytes)
    hipError_t e = hipMemcpyAsync(ctl, workspace, sizeof(ctl), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        hc::g_last_hip_error = e;
        return HC_ERROR_DEVICE;
    }
    const unsigned status = ctl[offsetof(hc::Workspace, status) / sizeof(unsigned)];
    if (status == 0u) return HC_SUCCESS;
    return status == (unsigned)HC_ERROR_TABLE ? HC_ERROR_TABLE : HC_ERROR_DEVICE;
}

hcStatus hc_trifocal_eval_variant_batched(int variant, unsigned flags, int n, const int32_t *unified_index,
                                          const hcComplex *x, const hcComplex *target, const hcComplex *diff,
                                          const hcComplex *start_params, const float *t, const uint8_t *kind,
                                          hcComplex *Hx, hcComplex *rhs, uint8_t *ent_ok, void *workspace,
                                          size_t workspace_bytes, hcStream stream) {
    return eval_variant_run(variant, false, flags, n, unified_index, x, target, diff, start_params, t, kind, Hx, rhs,
                            ent_ok, workspace, workspace_bytes, stream);
}

hcStatus hc_trifocal_compact_rows_batched(int n, const int32_t *unified_index, const hcComplex *x,
                                          const hcComplex *target, const hcComplex *diff,
                                          const hcComplex *start_params, const float *t, const uint8_t *kind,
                                          hcComplex *rows, hcComplex *rhs, uint8_t *ent_ok, void *workspace,
                                          size_t workspace_bytes) {
    return eval_variant_run(HC_EVAL_VARIANT_ABS, true, 0u, n, unified_index, x, target, diff, start_params, t, kind,
                            rows, rhs, ent_ok, workspace, workspace_bytes, nullptr);
}

hcStatus hc_trifocal_p2c_eval_batched(int n, const int32_t *hx_index, const int32_t *ht_index, const hcComplex *x,
                                      const hcComplex *coeffs_hx, const hcComplex *coeffs_ht, const float *t,
                                      hcComplex *Hx, hcComplex *Ht, hcComplex *H, void *workspace,
                                      size_t workspace_bytes, hcStream stream) {
    if (n < 0 || !hx_index || !ht_index || (n > 0 && (!x || !coeffs_hx || !coeffs_ht || !t || !Hx || !Ht || !H)))
        return HC_ERROR_INVALID_VALUE;
    if (!workspace || workspace_bytes < hc::ws_bytes_needed()) return HC_ERROR_WORKSPACE;
    if (n == 0) return HC_SUCCESS;
    hipStream_t s = (hipStream_t)stream;
    hc::Workspace *ws = (hc::Workspace *)workspace;
    (void)hipGetLastError();
    hc::PrepArgs pa{hx_index, ws, nullptr, nullptr, nullptr, nullptr, 0u, 0u, 0u};
    hipLaunchKernelGGL(hc::k_prep_tables_p2c<true>, dim3(1), dim3(hc::PREP_THREADS), 0, s, pa, ht_index);
    if (hc::launch_status(HC_ERROR_LAUNCH) != HC_SUCCESS) return HC_ERROR_LAUNCH;
    const int per = 2 * hc::WAVES_PER_WG;
    hipLaunchKernelGGL(hc::k_eval_p2c<true>, dim3((n + per - 1) / per), dim3(hc::WG_THREADS), 0, s, n, ws,
                       (const hc::cf *)x, (const hc::cf *)coeffs_hx, (const hc::cf *)coeffs_ht, t, (hc::cf *)Hx,
                       (hc::cf *)Ht, (hc::cf *)H);
    return hc::launch_status(HC_ERROR_LAUNCH);
}

const char *hc_last_error_string(void) { return hipGetErrorString(hc::g_last_hip_error); }

static_assert(sizeof(hcIpcHandle) == sizeof(hipIpcMemHandle_t), "hcIpcHandle mirrors hipIpcMemHandle_t");

namespace hc {
// memory kind of each flag this process created (hc_shared_flag_memory_kind)
static std::mutex g_flag_mu;
static std::map<const void *, int> g_flag_kind;
}  // namespace hc

// The flag is polled by running kernels of other devices (system-scope loads
// and stores over xGMI), so it is allocated where HIP specifies cross-agent
// coherence while kernels run: uncached device memory first (every access
// goes to the owner's memory), fine-grained memory next, plain
// (coarse-grained, coherent only at synchronisation points) as the last
// resort -- each only if it can be exported with hipIpcGetMemHandle.
hcStatus hc_shared_flag_create(uint32_t **flag, hcIpcHandle *handle) {
    if (!flag || !handle) return HC_ERROR_INVALID_VALUE;
    static const unsigned kinds[3] = {hipDeviceMallocUncached, hipDeviceMallocFinegrained, hipDeviceMallocDefault};
    hipError_t last = hipSuccess;
    for (int k = 0; k < 3; k++) {
        void *p = nullptr;
        last = (kinds[k] == hipDeviceMallocDefault) ? hipMalloc(&p, 256) : hipExtMallocWithFlags(&p, 256, kinds[k]);
        if (last != hipSuccess) { (void)hipGetLastError(); continue; }
        hipIpcMemHandle_t h;
        if ((last = hipMemset(p, 0, 256)) != hipSuccess || (last = hipDeviceSynchronize()) != hipSuccess ||
            (last = hipIpcGetMemHandle(&h, p)) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(p);
            continue;
        }
        memcpy(handle, &h, sizeof(h));
        *flag = (uint32_t *)p;
        std::lock_guard<std::mutex> g(hc::g_flag_mu);
        hc::g_flag_kind[p] = 2 - k;
        return HC_SUCCESS;
    }
    hc::g_last_hip_error = last;
    return HC_ERROR_DEVICE;
}

int hc_shared_flag_memory_kind(const uint32_t *flag) {
    std::lock_guard<std::mutex> g(hc::g_flag_mu);
    const auto it = hc::g_flag_kind.find(flag);
    return it == hc::g_flag_kind.end() ? -1 : it->second;
}

hcStatus hc_shared_flag_open(const hcIpcHandle *handle, uint32_t **flag) {
    if (!flag || !handle) return HC_ERROR_INVALID_VALUE;
    hipIpcMemHandle_t h;
    memcpy(&h, handle, sizeof(h));
    void *p = nullptr;
    if ((hc::g_last_hip_error = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess)) != hipSuccess)
        return HC_ERROR_DEVICE;
    *flag = (uint32_t *)p;
    return HC_SUCCESS;
}

hcStatus hc_shared_flag_reset(uint32_t *flag, hcStream stream) {
    if (!flag) return HC_ERROR_INVALID_VALUE;
    if ((hc::g_last_hip_error = hipMemsetAsync(flag, 0, sizeof(uint32_t), (hipStream_t)stream)) != hipSuccess)
        return HC_ERROR_LAUNCH;
    return HC_SUCCESS;
}

hcStatus hc_shared_flag_close(uint32_t *flag, int opened) {
    if (!flag) return HC_ERROR_INVALID_VALUE;
    if (!opened) {
        std::lock_guard<std::mutex> g(hc::g_flag_mu);
        hc::g_flag_kind.erase(flag);
    }
    hc::g_last_hip_error = opened ? hipIpcCloseMemHandle(flag) : hipFree(flag);
    return hc::g_last_hip_error == hipSuccess ? HC_SUCCESS : HC_ERROR_DEVICE;
}

int hc_trifocal_abi_version(void) { return HC_TRIFOCAL_ABI_VERSION; }

// tests only (include/hc_trifocal_testing.h): the tracker LU's structural
// patterns and column-group classes (hc_lu_struct.hpp)
unsigned hc_lu_struct_pattern(int row) { return row >= 0 && row < hc::NV ? hc::LU_STRUCT_PAT[row] : 0u; }
unsigned hc_lu_candidates(int step) { return step >= 0 && step < hc::NV ? hc::LU_BOUND.cand[step] : 0u; }
int hc_lu_search_span(int step) { return step >= 0 && step < hc::NV ? hc::lu_search_span(step) : -1; }
int hc_lu_step_level(int step) { return step >= 0 && step < hc::NV ? hc::LU_LEVELS.level[step] : -1; }
int hc_lu_group_class(int step, int group) {
    if (step < 0 || step >= hc::NV - 1 || group < 0 || group >= hc::LuChunks::count(step)) return -1;
    return hc::lu_group_class(step, group);
}
// tests only (include/lu/hc_lu_compact_testing.h): the compact row's column map
static_assert(HC_LU_COMPACT_WIDTH == hc::LU_COMPACT_W, "the header's row width");
int hc_lu_compact_column(int row, int position) {
    if (row < 0 || row >= hc::NV || position < 0 || position >= hc::LU_COMPACT_W) return -2;
    return hc::lu_compact_col(row, position);
}
// tests only (include/lu/hc_lu_rowtable_testing.h): a field of the fused levels'
// row records, decoded from the table the kernels copy to LDS (LU_ROWTAB)
int hc_lu_row_field(int level, int row, int field) {
    if (level < 0 || level >= hc::LU_REC_LEVELS || row < 0 || row >= hc::LU_REC_ROWS) return -2;
    hc::LuRowRec rec{0u, hc::LU_ROWTAB.w[level * hc::LU_REC_ROWS + row]};
    rec.bound = hc::LU_ROWTAB.w[hc::LU_REC_BOUND0 + ((rec.word >> hc::LU_REC_MEMBER_AT) & 31u)];
    const int mem = (int)((rec.word >> hc::LU_REC_MEMBER_AT) & 31u), k = (int)((rec.word >> hc::LU_REC_CHAIN_AT) & 15u);
    switch (field) {
    case HC_LU_ROW_MEMBER: return mem == hc::LU_REC_NO_MEMBER ? -1 : mem;
    case HC_LU_ROW_BOUND: return (int)rec.bound;
    case HC_LU_ROW_WINDOW: return (int)(rec.word & ((1u << hc::LU_REC_WIN_BITS) - 1u)) / 8 + 2 * row;
    case HC_LU_ROW_PARTNER: return (int)((rec.word >> hc::LU_REC_PARTNER_AT) & 31u);
    case HC_LU_ROW_PLACE: return (rec.word & hc::LU_REC_FIRST) ? 0 : (rec.word & hc::LU_REC_UP) ? 1 : 2;
    case HC_LU_ROW_CHAIN: return k == hc::LU_REC_NO_CHAIN ? -1 : k;
    default: return -2;
    }
}

hcStatus hc_trifocal_ring_check_test(void *workspace, size_t workspace_bytes, unsigned head, unsigned tail,
                                     unsigned avail, hcStream stream) {
    const hc::SliceLayout area = hc::slice_layout(0, 0);   // the counters' place does not depend on the launch
    if (!workspace || workspace_bytes < area.ring) return HC_ERROR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    unsigned *rq = (unsigned *)((char *)workspace + area.rq);
    const unsigned v[3] = {head, tail, avail};
    const int at[3] = {hc::RQ_HEAD, hc::RQ_TAIL, hc::RQ_AVAIL};
    (void)hipGetLastError();
    for (int i = 0; i < 3; i++)
        if ((hc::g_last_hip_error = hipMemcpyAsync(rq + at[i], &v[i], sizeof(unsigned), hipMemcpyHostToDevice, s)) !=
            hipSuccess)
            return HC_ERROR_LAUNCH;
    if ((hc::g_last_hip_error = hipStreamSynchronize(s)) != hipSuccess) return HC_ERROR_DEVICE;
    hipLaunchKernelGGL(hc::k_ring_check, dim3(1), dim3(64), 0, s, (hc::Workspace *)workspace, (const unsigned *)rq);
    return hc::launch_status(HC_ERROR_LAUNCH);
}

void hc_trifocal_set_ring_test(int delay_ticks) {
    hc::g_ring_test.store(delay_ticks > 0 ? (delay_ticks < HC_RING_TEST_MIN_TICKS ? HC_RING_TEST_MIN_TICKS : delay_ticks)
                                          : 0,
                          std::memory_order_relaxed);
}

void hc_trifocal_set_small_launch(int mode) {
    hc::g_small_launch.store(mode < 0 ? -1 : mode > 0 ? 1 : 0, std::memory_order_relaxed);
}

void hc_trifocal_set_retry_reuse(int on) { hc::g_retry_reuse.store(on ? 1 : 0, std::memory_order_relaxed); }

const char *hc_trifocal_version(void) {
    return "hc_trifocal gfx950 v10.13 (2 paths/wave, structurally sparse LDS-broadcast LU with lean pivot steps fused by level, the levels' per-row constants and row labels read from LDS tables, "
           "the fused solve's row kept in 16 positions (its column of each level, then columns 18..29), "
           "one exec region per pivot step for the eligible rows with the column groups through scratch windows, "
           "column groups by structural class (never-fillable groups untested, always-live groups unconditional), "
           "pivot search narrowed to the candidate rows' DPP group "
           "(abort kernel and tracking launches filling at most half of the path slots -- the latter at 3 waves/SIMD, "
           "16 columns per batch: batched latency mode, one LDS round trip per pivot step, every live-able column "
           "group untested), "
           "structure-agnostic twin kernels for other dH/dx structures, readlane back substitution (the throughput "
           "kernel's fused positions level by level through LDS), pipelined evals over "
           "per-slot prefix tables, 5 waves/SIMD, time slicing at step boundaries with least-attained-service "
           "issue priority, a rejected step's retry reuses its first RK4 slope, the throughput kernel's operand "
           "addresses read complete from per-slot tables and its finiteness check made on the dH/dx entries)";
}

}  // extern "C"
