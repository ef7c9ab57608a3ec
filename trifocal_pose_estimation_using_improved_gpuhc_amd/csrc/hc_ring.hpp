// The time-slicing ring of the tracker kernels: the agent-scope load / store
// helpers of the hand-over data, the ring protocol and the epilogue kernel that
// checks a sliced launch drained its ring.
//
// Time slicing.  A path that has run slice_q steps while other
// work waits is suspended at its step boundary: x and its step-control scalars
// go to the path's 256-B suspend block (two full cache lines, one store per
// half), the path id to a FIFO ring.  While new paths remain, the suspending
// half takes one (an unpaired push); after that it swaps with the oldest
// suspended path (a paired push + pop, i.e. round robin).  A half whose path
// ends takes a new path, else the oldest suspended one.  Every path thus starts
// early and the end of a launch is made of short remainders instead of whole
// late-dequeued long paths.  Bit-exact: at a step boundary x == x_last == the
// RK accumulator, and this is the whole vector state.
//
// Ring protocol (no CAS loops): tickets from atomicAdd on head / tail; avail
// counts published entries not yet claimed by unpaired pops (a semaphore:
// decrement, undo if it was empty and retry while the undo leaves it
// positive, so concurrent failures cannot hide an entry).  A paired pop needs
// no claim: its own push precedes it.  A claimed entry may still be in the
// pusher's hands (ticket taken, entry not yet written), hence the short wait
// on its tag.  An entry's tag hashes the launch epoch with its ticket, so the
// ring needs no clearing between launches (only once, when a workspace is
// first used or its ring grows: k_prep_tables).
#pragma once

#include "hc_layout.hpp"

namespace hc {

// How long a consumer waits for a claimed entry whose pusher holds the ticket
// but has not written it yet before it abandons the ticket (s_memrealtime
// ticks, 100 MHz: 1 ms).  Abandoning loses nothing: the pusher sees the mark
// when it writes and pushes the path again on a new ticket (ring_push).
constexpr unsigned long long RING_ABANDON_TICKS = 100000ull;
// Every sliced launch's ring entry is written once by one atomic exchange,
// either by its pusher (the tagged path id) or by a consumer that gave up
// waiting (the abandon mark: the tag with bit 0 cleared, never a published tag)
__device__ __forceinline__ unsigned long long ring_abandon_mark(unsigned tag) {
    return ((unsigned long long)(tag & ~1u) << 32) | 0xFFFFFFFFull;
}
// (tests, KArgs::ring_test: consumers abandon after an eighth of the pushers' delay)
__device__ __forceinline__ unsigned long long ring_wait_ticks(int ring_test) {
    return ring_test > 0 ? (unsigned long long)(ring_test / 8) : RING_ABANDON_TICKS;
}
// tag of ticket t's entry in launch `epoch` (never 0, so a cleared entry never
// matches; distinct epochs give distinct tags for the same ticket)
__device__ __forceinline__ unsigned ring_tag(unsigned epoch, unsigned t) {
    return ((epoch * 0x9E3779B1u) ^ (t * 0x85EBCA6Bu)) | 1u;
}

__device__ __forceinline__ unsigned ld_rlx(const unsigned *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The hand-over data of a suspended path (suspend block, ring entries) is
// written and read with agent-scope relaxed atomics: global_store/load with
// sc1, which write through to, and read from, the device-coherent level, so a
// block needs no cache-wide release / acquire fence (a release fence at agent
// scope is an L2 writeback on this chip).  Ordering, DESIGN.md §3:
//  * writer: block stores, then drain_stores() -- s_waitcnt vmcnt(0), which
//    returns only once every earlier store is acknowledged, written as an asm
//    statement with a "memory" clobber so the compiler cannot move a memory
//    access across it -- then the ring entry store (and, unpaired, the avail
//    increment), so an entry becomes visible only after its block;
//  * reader: the entry is loaded and its tag checked before the block's
//    address (path id) is known, and its loads are issued after that wait.
__device__ __forceinline__ void st_u64_h(unsigned long long *p, unsigned long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long ld_u64_h(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long pack2(unsigned lo, unsigned hi) {
    return (unsigned long long)lo | ((unsigned long long)hi << 32);
}
__device__ __forceinline__ void st_cf_rlx(cf *p, cf v) {
    st_u64_h(reinterpret_cast<unsigned long long *>(p), pack2(__float_as_uint(v.x), __float_as_uint(v.y)));
}
__device__ __forceinline__ cf ld_cf_rlx(const cf *p) {
    const unsigned long long u = ld_u64_h(reinterpret_cast<const unsigned long long *>(p));
    return cmk(__uint_as_float((unsigned)u), __uint_as_float((unsigned)(u >> 32)));
}
__device__ __forceinline__ int ld_i_rlx(const int *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// (pointers and sizes by value: a KArgs reference would put the kernel
// arguments in scratch memory)
__device__ __forceinline__ unsigned long long xchg_u64(unsigned long long *p, unsigned long long v) {
    return __hip_atomic_exchange(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Publishes suspended path b (its block already written and drained).  A
// pusher that finds its ticket abandoned -- it was paused between taking the
// ticket and writing the entry for longer than the consumer waits -- pushes
// again on a new ticket, paired or unpaired as before.  Accounting: every
// live entry is matched by one pop, either a claim on avail (unpaired
// entries publish one) or the paired pop its pusher makes next; an abandoned
// ticket takes one pop with it, and its consumer restores the balance
// (ring_pop gives its claim back; ring_pop_paired publishes its own paired
// push as claimable).  test_delay (tests only): every 16th ticket waits that
// many ticks before its exchange, so that its consumer abandons it.
__device__ __forceinline__ void ring_push(unsigned *rq, unsigned long long *ring, unsigned cap, unsigned epoch, int b,
                                          bool unpaired, Workspace *ws, int test_delay) {
    for (;;) {
        const unsigned t = atomicAdd(&rq[RQ_TAIL], 1u);
        if (t >= cap) {   // more re-pushes than RING_SLACK (the path is lost: reported)
            atomicMax(&ws->status, (unsigned)HC_ERROR_DEVICE);
            return;
        }
        if (__builtin_expect(test_delay > 0, 0) && (t & 15u) == 7u) {
            const unsigned long long w0 = __builtin_amdgcn_s_memrealtime();
            while (__builtin_amdgcn_s_memrealtime() - w0 < (unsigned long long)test_delay) __builtin_amdgcn_s_sleep(8);
        }
        const unsigned tag = ring_tag(epoch, t);
        const unsigned long long old = xchg_u64(&ring[t], ((unsigned long long)tag << 32) | (unsigned)b);
        if (__builtin_expect(old != ring_abandon_mark(tag), 1)) break;
    }
    if (unpaired) atomicAdd(&rq[RQ_AVAIL], 1u);
}
// The entry of ticket h: its pusher took ticket h before (head never passes
// tail), so it is written or about to be.  A pusher paused mid-push is waited
// for up to wait_ticks; then the ticket is abandoned (-2): one exchange writes
// the abandon mark, and if the pusher's entry arrived just before it, the
// exchange returns it and the path is taken after all.  Otherwise the pusher
// will see the mark and push again (ring_push), so no path is lost.  A path
// id outside the launch cannot come from the protocol: reported, -1.
__device__ __forceinline__ int ring_take(unsigned long long *ring, unsigned cap, unsigned epoch, Workspace *ws,
                                         unsigned h, const unsigned *rq, int num_paths, unsigned long long wait_ticks) {
    if (h >= cap) {
        atomicMax(&ws->status, (unsigned)HC_ERROR_DEVICE);
        return -1;
    }
    const unsigned tag = ring_tag(epoch, h);
    unsigned long long e = ld_u64_h(&ring[h]);
    if ((unsigned)(e >> 32) != tag) {
        const unsigned long long w0 = __builtin_amdgcn_s_memrealtime();
        for (;;) {
            __builtin_amdgcn_s_sleep(8);
            e = ld_u64_h(&ring[h]);
            if ((unsigned)(e >> 32) == tag) break;
            if (__builtin_amdgcn_s_memrealtime() - w0 > wait_ticks) {
                e = xchg_u64(&ring[h], ring_abandon_mark(tag));
                if ((unsigned)(e >> 32) == tag) break;
                atomicAdd(&ws->abandoned, 1u);
                return -2;
            }
        }
    }
    if ((unsigned)e < (unsigned)num_paths) return (int)(unsigned)e;
    if (atomicMax(&ws->status, (unsigned)HC_ERROR_DEVICE) == 0u) {
        // diagnostics: ticket, entry seen, tail, head
        ws->ring_fail[0] = h;
        ws->ring_fail[1] = (unsigned)e;
        ws->ring_fail[2] = ld_rlx(&rq[RQ_TAIL]);
        ws->ring_fail[3] = ld_rlx(&rq[RQ_HEAD]);
    }
    return -1;
}
// oldest suspended path id, or -1 if there is none
__device__ __forceinline__ int ring_pop(unsigned *rq, unsigned long long *ring, unsigned cap, unsigned epoch,
                                        Workspace *ws, int num_paths, unsigned long long wait_ticks) {
    int *avail = reinterpret_cast<int *>(&rq[RQ_AVAIL]);
    // after 16 abandoned tickets this pop gives up (-1: the half
    // idles); nothing is lost, the abandoned paths' pushers push them again
    // and keep popping while entries remain
    for (int tries = 0; tries < 16;) {
        if (ld_i_rlx(avail) <= 0) return -1;
        if (atomicSub(avail, 1) > 0) {
            const int b = ring_take(ring, cap, epoch, ws, atomicAdd(&rq[RQ_HEAD], 1u), rq, num_paths, wait_ticks);
            if (b != -2) return b;
            atomicAdd(avail, 1);   // abandoned: the claim goes back (its entry is still to be popped)
            tries++;
            continue;
        }
        if (atomicAdd(avail, 1) + 1 <= 0) return -1;
    }
    return -1;
}
// the swap's pop, right after its own push (no claim).  If its ticket is
// abandoned, the swap's own push has lost the pop that matched it: it is
// published as claimable (avail), and the half looks for a path with an
// unpaired pop
__device__ __forceinline__ int ring_pop_paired(unsigned *rq, unsigned long long *ring, unsigned cap, unsigned epoch,
                                               Workspace *ws, int num_paths, unsigned long long wait_ticks) {
    const int b = ring_take(ring, cap, epoch, ws, atomicAdd(&rq[RQ_HEAD], 1u), rq, num_paths, wait_ticks);
    if (b != -2) return b;
    atomicAdd(&rq[RQ_AVAIL], 1u);
    return ring_pop(rq, ring, cap, epoch, ws, num_paths, wait_ticks);
}

// Epilogue of a sliced launch: once the tracker has drained, every
// pushed ring entry has been taken (head == tail) and every unpaired push
// claimed (avail == 0).  Otherwise a suspended path was never resumed and its
// outputs are stale: HC_ERROR_DEVICE (hc_trifocal_workspace_status), with
// (~0, avail, tail, head) in ring_fail.  One thread, stream-ordered after k_track.
__global__ void __launch_bounds__(64) k_ring_check(Workspace *ws, const unsigned *rq) {
    if (threadIdx.x != 0) return;
    const unsigned head = ld_rlx(&rq[RQ_HEAD]), tail = ld_rlx(&rq[RQ_TAIL]), avail = ld_rlx(&rq[RQ_AVAIL]);
    if ((head != tail || avail != 0u) && atomicMax(&ws->status, (unsigned)HC_ERROR_DEVICE) == 0u) {
        ws->ring_fail[0] = 0xFFFFFFFFu;
        ws->ring_fail[1] = avail;
        ws->ring_fail[2] = tail;
        ws->ring_fail[3] = head;
    }
}

}  // namespace hc
