// k_prep_tables: what runs before the kernels of every launch (below).
#pragma once

#include "hc_layout.hpp"

namespace hc {

// Compacts the reference's padded unified index (38880 ints: dH/dx at
// ((c*8+j)*5+part)*30 + r, dH/dt at 36000 + (j*6+part)*30 + r; Data_Reader.cpp
// :167-189, ..._LimUnroll_L2Cache.cuh:57-148) into EvalTables.  Lane r < 30
// of the first wave = equation row r.  Every index and coefficient is
// validated; a table that does not fit sets HC_ERROR_TABLE and the tracker
// leaves its outputs untouched.  The tables persist in the workspace: a launch
// whose index table hashes to the one they were built from (all 256 threads
// hash it, ~10 KB each) skips the compaction.  The same pass writes the
// throughput kernel's slot-absolute address tables (AbsTables) from the
// finished words, so the two are always of one table.
//
// Also the per-launch reset of the time-slicing counters (rq != nullptr): head,
// tail and avail zeroed, the ring epoch bumped; ring entries not cleared yet
// (a workspace's first sliced launch, or a larger ring than before) are zeroed
// once (hash tags never match a zero entry).
constexpr unsigned TAB_MAGIC = 0x48435442u;   // "HCTB"
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {   // splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
constexpr int PREP_THREADS = 256;
// The P2C layout (include/p2c/hc_trifocal_p2c.h; the archived dev-eval-indxing-..._P2C.cuh
// :74-117): dH/dx at ((r*30 + c)*8 + j)*4 + part, parts (c, k, x_u, x_v), dH/dt at
// (r*16 + j)*5 + part, parts (c, k, x_u, x_v, x_w), in two tables.  A term names
// one coefficient k < 38 where a PH term names two parameters; the compaction
// carries it as the pair (a, b) = (k & 31, k >> 5), so the prefix keys, their
// places and the term words are built by the same code, and the prefix build
// jobs (D) address coefficient k's staging place instead of p[a] and p[b]
// (hc_eval.hpp build_prefix_rounds_p2c).
constexpr int P2C_HX_PARTS = 4, P2C_HT_PARTS = 5;
constexpr int P2C_HX_SIZE = NV * NV * HX_TERMS * P2C_HX_PARTS;   // 28800
constexpr int P2C_HT_SIZE = NV * HT_TERMS * P2C_HT_PARTS;        // 2400
constexpr unsigned long long P2C_HASH_TAG = 0x5032435F74626C73ull;   // tells the formats' hashes apart
__global__ void __launch_bounds__(PREP_THREADS) k_prep_tables(PrepArgs pa) {
    constexpr bool P2C = false;
    const int32_t *const D_in = nullptr;   // (k_prep_tables_p2c: the dH/dt table)
#include "hc_prep_body.inc"
}

}  // namespace hc
