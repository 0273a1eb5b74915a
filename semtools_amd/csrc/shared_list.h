// One sorted top-k list per block in LDS, shared by the block's waves (scan_wide_kernel; tools/micro/shared_list.hip runs the same
// routine alone).  A list is up to 32 keys (dist_bits << 32 | row, ascending, KEY_PAD where empty), a lock word and a THRESHOLD: the
// list's kp-th key as {distance, row} in one aligned 64-bit word (low half the distance's bits), {+inf, 0xFFFFFFFF} while the list
// holds fewer than kp keys.  Readers test candidates against the threshold without the lock: it is written and read as one 64-bit
// access (a torn one could be tighter than either value and drop a true member) and it only ever falls, so a stale one is merely
// loose.  Whatever the order in which the waves arrive, the list ends as the kp smallest keys that were offered: the content is
// deterministic although the schedule is not.
#pragma once
#include "device_flags.h"

namespace smt {

constexpr int SHARED_LIST_KEYS = 32;                               // keys a list holds (kp <= 32: a wave's lanes 0 .. kp - 1 hold it while it changes)
constexpr unsigned long long SHARED_LIST_OPEN = 0xFFFFFFFF7F800000ull;   // the threshold of a list that is not full: {+inf, 0xFFFFFFFF}

__device__ __forceinline__ unsigned long long shared_list_threshold(const unsigned long long *thr)
{
    return __hip_atomic_load(thr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The whole wave calls this with wave-uniform arguments: (d, r) goes into the list if it is among its kp smallest.  d >= +0 or NaN
// (dist_f32), so the order of the keys is the order of (distance, row) the candidate test uses.
//   1. the threshold again: most candidates of a stale threshold end here, without the lock
//   2. the lock: lane 0, an LDS compare-and-swap, s_sleep between tries.  Bounded like every wait of the scan: after ~2 s of the
//      100 MHz wall clock *err is raised (the context reports it at the next drain) and the key is dropped
//   3. lanes 0 .. kp - 1 read the list; the position is the number of keys below the new one
//   4. the tail moves up one place, the new key goes in, the threshold follows (lane kp - 1 holds the kp-th key)
//   5. release
// A wave's LDS operations execute in order and the holder waits for nothing but LDS.
__device__ __forceinline__ void shared_list_insert(key_t64 *list, unsigned int *lock, unsigned long long *thr, float d, uint32_t r, int kp,
                                                   int lane, unsigned long long *err)
{
    const unsigned long long t = uniform_u64(shared_list_threshold(thr));
    const float td = __uint_as_float((uint32_t)t);
    const uint32_t tr = (uint32_t)(t >> 32);
    if (!((d < td) || (d == td && r < tr))) return;
    // (the lane asked of an opaque copy: as invariants of the caller's row loop the lane masks below would be hoisted into a dozen
    // scalar registers, which that loop does not have)
    asm volatile("" : "+v"(lane));
    // (the retry loop is the wave's, not lane 0's: a scalar loop needs no lane masks)
    auto try_lock = [&]() -> bool {
        unsigned int got = 0;
        if (lane == 0) {
            unsigned int expect = 0;
            got = __hip_atomic_compare_exchange_strong(lock, &expect, 1u, __ATOMIC_ACQUIRE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        return __builtin_amdgcn_readfirstlane((int)got) != 0;
    };
    if (!try_lock()) {
        const unsigned long long t0 = wall_clock64();
        bool got;
        do {
            __builtin_amdgcn_s_sleep(1);
            got = try_lock();
        } while (!got && wall_clock64() - t0 < 200000000ull);
        if (!got) {
            if (lane == 0) flag_store(err, 1ull);
            return;
        }
    }
    const key_t64 key = make_key(d, r);
    const key_t64 mine = lane < kp ? list[lane] : KEY_PAD;
    const int pos = __popcll(__ballot(mine < key));
    if (pos < kp) {
        const key_t64 prev = (key_t64)dpp_u<DPP_WAVE_SHR1>((uint32_t)mine) | ((key_t64)dpp_u<DPP_WAVE_SHR1>((uint32_t)(mine >> 32)) << 32);
        const key_t64 now = lane == pos ? key : prev;
        if (lane >= pos && lane < kp) list[lane] = now;
        if (lane == kp - 1 && now != KEY_PAD) __hip_atomic_store(thr, (now << 32) | (now >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (lane == 0) __hip_atomic_store(lock, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

}  // namespace smt
