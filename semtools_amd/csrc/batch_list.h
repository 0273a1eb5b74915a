// batch_list.h -- what the batched streaming kernels share (batch_slab.hip: wide f32 rows on the bf16 MFMA pipe; batch_half.hip: half
// rows on the f16 pipe; batch_byte.hip: byte rows on the int8 pipe; batch_nibble.hip: nibble rows, unpacked, on the same pipe): the frame of a launch (512 threads, a wave owns 32-row tiles dealt round robin, at most SLAB_MAX_LISTS
// blocks), the per-(block, query) lists in the block_lists area under an LDS lock word per query, the epilogue that turns a tile's
// accumulators into candidates, and the host side's grid, scratch layout and list test hook.
//
// LISTS.  The list of k' keys of a (block, query) pair lives IN the block_lists area the finish reads (global memory, L2 resident),
// ascending, preset to KEY_PAD; LDS holds the QB thresholds (the k'-th key, KEY_PAD while the list is short, 0 for a padding query)
// and QB lock words.  A wave that found a candidate takes the query's lock (lane 0 spins on a compare-and-swap; a wave holds one lock
// at a time), reads the list into its lanes, inserts by ballot rank, stores it back and publishes the new threshold.  A stale threshold
// only admits more: every candidate is compared again under the lock.
#pragma once
#include "wide_rows.h"
#include "device_utils.h"
#include "mfma_tile.h"
#include "gemm.h"

namespace smt {

constexpr int BS_THREADS = 512, BS_WAVES = BS_THREADS / 64;

__device__ __forceinline__ key_t64 readlane_key(key_t64 v, int l)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((key_t64)hi << 32) | lo;
}

// Lanes of one wave hand data to each other through LDS: only half the lanes write a slice, so without this the compiler takes a
// lane that wrote nothing to read what it read before.  Wavefront scope: no instruction, an ordering for the compiler alone.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The candidates `cand` (a lane mask; lane l: key ck) into the list of one (block, query) pair, under the query's lock (header: LISTS)
__device__ __forceinline__ void batch_list_insert(key_t64 *list, int kp, unsigned long long cand, key_t64 ck, int lane, unsigned int *lock,
                                                  key_t64 *thr)
{
    if (lane == 0)
        while (atomicCAS(lock, 0u, 1u) != 0u) __builtin_amdgcn_s_sleep(1);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    key_t64 key = lane < kp ? __hip_atomic_load(list + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : KEY_PAD;
    while (cand) {
        const int l = __builtin_ctzll(cand);
        cand &= cand - 1;
        const key_t64 c = readlane_key(ck, l);
        if (c < readlane_key(key, kp - 1)) {   // (wave-uniform)
            const int pos = __popcll(__ballot(key < c));
            const uint32_t slo = dpp_u<DPP_WAVE_SHR1>((uint32_t)key), shi = dpp_u<DPP_WAVE_SHR1>((uint32_t)(key >> 32));
            if (lane > pos) key = ((key_t64)shi << 32) | slo;
            else if (lane == pos) key = c;
            if (lane >= kp) key = KEY_PAD;
        }
    }
    if (lane < kp) __hip_atomic_store(list + lane, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    const key_t64 last = readlane_key(key, kp - 1);
    if (lane == 0) __hip_atomic_store(thr, last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // (one 8-byte LDS write: never torn)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (lane == 0) __hip_atomic_store(lock, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The thresholds, locks, zero-query masks and empty lists of a pass; the caller's __syncthreads() follows
template <int QB>
__device__ __forceinline__ void batch_lists_init(key_t64 *s_thr, unsigned int *s_lock, unsigned int *s_qz, const uint32_t *qzero, uint32_t nq_active,
                                                 int kp, key_t64 *block_lists, int lane, int wave)
{
    if (threadIdx.x < QB) {
        s_thr[threadIdx.x] = threadIdx.x < nq_active ? KEY_PAD : 0ull;   // padding queries: nothing is under 0
        s_lock[threadIdx.x] = 0u;
    }
    if (wave < QB / 32) {
        const unsigned long long z = __ballot(lane < 32 && qzero[wave * 32 + (lane & 31)] != 0u);
        if (lane == 0) s_qz[wave] = (unsigned int)z;
    }
    for (uint32_t i = threadIdx.x; i < nq_active * (uint32_t)kp; i += BS_THREADS) {
        const uint32_t qq = i / (uint32_t)kp, sl = i - qq * (uint32_t)kp;
        block_lists[((size_t)qq * gridDim.x + blockIdx.x) * kp + sl] = KEY_PAD;
    }
}

// The epilogue of a tile.  Accumulator register r of lane (j, h) of acc[t] is <unit query 32 t + acc_row(r, h), row j> times 1 / rxj's
// scale: d = max(1 - acc * rxj, 0), 1 against a zero row (xz) or for a zero query, 0 for both.  Scores under their query's threshold
// go into its list, one (register, half) pair at a time.
template <int NT>
__device__ __forceinline__ void batch_tile_nominate(const f32x16 (&acc)[NT], int nt_active, float rxj, bool xz, uint32_t rowj, bool validj,
                                                    const unsigned int *s_qz, key_t64 *s_thr, unsigned int *s_lock, key_t64 *block_lists, int kp,
                                                    int lane)
{
    const int h = lane >> 5;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t >= nt_active) break;   // (wave-uniform)
        const unsigned int qzm = s_qz[t] >> (4 * h);   // bit acc_row(r, 0): query acc_row(r, h)
        // which of the lane's 16 scores lie under their query's threshold (bit r <-> accumulator register r)
        auto score = [&](float a, bool qz) __attribute__((always_inline)) { return qz ? (xz ? 0.0f : 1.0f) : fmaxf(1.0f - a * rxj, 0.0f); };
        unsigned pass = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            // queries 32 t + 8 u + 4 h + c, c = 0 .. 3: registers 4 u + c
            const key_t64 *tq = s_thr + 32 * t + 8 * u + 4 * h;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const key_t64 k = make_key(score(acc[t][4 * u + c], (qzm >> (8 * u + c)) & 1u), rowj);
                if (k < __hip_atomic_load(tq + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) pass |= 1u << (4 * u + c);
            }
        }
        if (!validj) pass = 0;
        if (!__ballot(pass != 0)) continue;   // the common case: nothing under any threshold
        // the rare case, one (register, half) pair at a time: bit 2 r + hh of todo <-> query acc_row(r, hh) has candidates
        unsigned todo = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned long long m = __ballot((pass >> r) & 1u);
            todo |= ((uint32_t)m ? 1u : 0u) << (2 * r) | ((uint32_t)(m >> 32) ? 2u : 0u) << (2 * r);
        }
        while (todo) {
            const int rh = __builtin_ctz(todo), r = rh >> 1, hh = rh & 1;
            todo &= todo - 1;
            const int qq = 32 * t + acc_row(r, hh);
            const bool mine = h == hh && ((pass >> r) & 1u);
            const key_t64 ck = make_key(score(acc_select(acc[t], r), (qzm >> acc_row(r, 0)) & 1u), rowj);
            batch_list_insert(block_lists + ((size_t)qq * gridDim.x + blockIdx.x) * kp, kp, __ballot(mine), ck, lane, s_lock + qq, s_thr + qq);
        }
    }
}

// the grid of a pass: at most SLAB_MAX_LISTS blocks, no block without a tile
inline int batch_blocks(const smt_ctx *ctx, uint64_t n_tiles)
{
    const int cus = ctx->tune.scan_blocks > 0 ? ctx->tune.scan_blocks : std::max(ctx->num_cus, 1);
    return (int)std::max<uint64_t>(1, std::min<uint64_t>(std::min(cus, SLAB_MAX_LISTS), (n_tiles + BS_WAVES - 1) / BS_WAVES));
}

inline void batch_shape(smt_ctx *ctx, const SlabSearch &a, uint32_t &kp, uint64_t &n_tiles, int &blocks)
{
    kp = std::min<uint32_t>(64, a.k_out + (uint32_t)ctx->tune.guard_band);
    n_tiles = a.chunk_table ? (a.n_chunks + 7) / 8 : (a.rows + 31) / 32;
    blocks = batch_blocks(ctx, n_tiles);
}

// scratch of a call: [split image nq_pad x 1 KiB per 256 dimensions | zero flags nq_pad | lists], each 256-byte aligned
struct BatchScratch {
    uint32_t *split, *qzero;
    key_t64 *lists;
};
inline int batch_scratch(smt_ctx *ctx, uint32_t dim, uint32_t nq_pad, size_t list_keys, BatchScratch &s)
{
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t b_split = al((size_t)nq_pad * dim * 4), b_zero = al((size_t)nq_pad * 4);
    int rc = ensure_scratch(ctx, b_split + b_zero + list_keys * sizeof(key_t64));
    if (rc) return rc;
    char *base = reinterpret_cast<char *>(ctx->d_scratch);
    s.split = reinterpret_cast<uint32_t *>(base);
    s.qzero = reinterpret_cast<uint32_t *>(base + b_split);
    s.lists = reinterpret_cast<key_t64 *>(base + b_split + b_zero);
    return SMT_OK;
}

// The test hooks' body: split(nq_pad, scratch) and then pass(scratch, q0, nq_pass, kp, n_tiles, blocks, lists) per QB queries of a.nq,
// no finish; the list area [nq + 1][blocks][k'] is preset to 0x5A, every pass writes its queries' sets, the last set is the guard
// nothing may touch.
template <class Split, class Pass>
int debug_batch_lists(smt_ctx *ctx, const SlabSearch &a, uint32_t QB, Split split, Pass pass, key_t64 *out_keys_host, uint64_t out_cap_keys,
                      uint32_t *out_blocks, uint32_t *out_kp)
{
    SMT_REQUIRE(a.nq >= 1 && a.nq <= 256, "debug batch lists: 1 .. 256 queries");
    uint32_t kp;
    uint64_t n_tiles;
    int blocks;
    batch_shape(ctx, a, kp, n_tiles, blocks);
    SMT_REQUIRE(n_tiles >= 1, "debug batch lists: no row to scan");
    *out_blocks = (uint32_t)blocks;
    *out_kp = kp;
    const size_t n_keys = (size_t)(a.nq + 1) * blocks * kp;
    SMT_REQUIRE(out_cap_keys >= n_keys, "debug batch lists: output capacity");
    BatchScratch s;
    const uint32_t nq_pad = (a.nq + QB - 1) / QB * QB;
    int rc = batch_scratch(ctx, a.dim, nq_pad, n_keys, s);
    if (rc) return rc;
    SMT_HIP_CHECK(hipMemsetAsync(s.lists, 0x5A, n_keys * sizeof(key_t64), ctx->stream));
    if ((rc = split(nq_pad, s))) return rc;
    for (uint32_t q0 = 0; q0 < a.nq; q0 += QB)
        if ((rc = pass(s, q0, std::min<uint32_t>(QB, a.nq - q0), kp, n_tiles, blocks, s.lists + (size_t)q0 * blocks * kp))) return rc;
    SMT_HIP_CHECK(hipMemcpyAsync(out_keys_host, s.lists, n_keys * sizeof(key_t64), hipMemcpyDeviceToHost, ctx->stream));
    SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return SMT_OK;
}

}  // namespace smt
