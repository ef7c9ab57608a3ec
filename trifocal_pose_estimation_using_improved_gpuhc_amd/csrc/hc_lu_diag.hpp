// hc_lu_diag.hpp -- the counters the diagnostic builds compile into the LU
// (scripts/build_variant.sh: -DHC_DIAG_LUWORK, -DHC_DIAG_PHASES,
// -DHC_DIAG_LIVE).  In the product build every macro here expands to nothing.
#pragma once

#include "hc_device.hpp"

namespace hc {

#ifdef HC_DIAG_LUWORK
// diagnostic build: rank-1 update elements the solves execute (sum over the
// executed column groups of columns x active lanes), and the solves
// [0] executed elements, [1] completed sparse solves, [2] dense solves (path
// solves); wave-level: [3] sparse wave-solves, [4] live column groups, [5] rare
// pivot steps; [6..8] stages whose right-hand side ran the mixed / dH/dt-only /
// H-only evaluation, [9] stages that rebuilt the prefix tables (k_track),
// [10] path-level stage 0s taken from the kept slope of a rejected step (retry reuse);
// [11 + I] rare pivot steps of the sparse wave-solves at step I (counted where they
// happen, also in solves that end in `redo`), [41] sparse wave-solves with a rare
// step among the fusable steps 0..17 (what a fused level hands to its fallback)
constexpr int DIAG_LUWORK_RARE_AT = 11, DIAG_LUWORK_RARE_FUSABLE = DIAG_LUWORK_RARE_AT + NV;
constexpr int DIAG_LUWORK_WORDS = DIAG_LUWORK_RARE_FUSABLE + 1;
__device__ unsigned long long g_diag_luwork[DIAG_LUWORK_WORDS];
struct LuWork { unsigned long long acc, mask, groups, rare, excl, rare_fusable; };   // mask: lanes whose work counts (active
                                                                      // path slots); excl: lanes that update by l = 0
#define HC_LU_WORK(ncols) (lu_work_acc.acc += (unsigned long long)(ncols) * \
    (unsigned long long)__builtin_popcountll(__builtin_amdgcn_read_exec() & lu_work_acc.mask & ~lu_work_acc.excl))
#define HC_LU_WORK_GROUP() (lu_work_acc.groups++)
#define HC_LU_WORK_ARG , LuWork &lu_work_acc
#define HC_LU_WORK_PASS , lu_work_acc
// lu_solve's count_mask argument at a call site: the lanes whose work counts
#define HC_LU_COUNT(mask) (mask)
#else
#define HC_LU_WORK(ncols) do { } while (0)
#define HC_LU_WORK_GROUP() do { } while (0)
#define HC_LU_WORK_ARG
#define HC_LU_WORK_PASS
#define HC_LU_COUNT(mask) (~0ull)
#endif

#ifdef HC_DIAG_PHASES
__device__ unsigned long long g_diag_lu_mid[65536];   // per (workgroup, wave): see lu_solve
#endif

#ifdef HC_DIAG_LIVE
// diagnostic build: how often each column group of each pivot step is live
// (wave-level test), sampled on every eighth workgroup: [I][K] live count,
// [I][LIVE_SOLVES] sparse wave-solves that reached step I
constexpr int LIVE_SOLVES = 16;
__device__ unsigned long long g_diag_live[NV][LIVE_SOLVES + 1];
#define HC_DIAG_LIVE_HIT(I, K) do { if (lane_fresh() == 0 && (blockIdx.x & 7u) == 0u) \
    atomicAdd(&g_diag_live[I][K], 1ull); } while (0)
#else
#define HC_DIAG_LIVE_HIT(I, K) do { } while (0)
#endif

}  // namespace hc
