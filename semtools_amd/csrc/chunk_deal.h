// chunk_deal.h -- how the streaming kernels deal the chunks of a corpus to their waves: K2 (scan_topk_kernel and the grouped
// kernels: scan_topk.hip, scan_pair.hip, scan_wide.hip, scan_deep.hip), K4 (scan_threshold_kernel: threshold.hip) and the large-k collect (largek_collect_kernel: topk_large.hip).
// The loop skeletons -- how many stages, what a descriptor is made from -- stay in the kernels.
#pragma once
#include "device_utils.h"

namespace smt {

// The block owns the chunks (U rows each) c(t) = ((t / waves) * gridDim.x + blockIdx.x) * waves + t % waves,
// t = 0, 1, ... -- the same rows a static grid-stride deal would give it -- but its waves CLAIM them from
// an LDS counter.  The CU's arbiter favours the older wave of each SIMD: with a static deal waves 0-3
// finished 12 us before waves 4-7 (of 145) and the CU ran half empty at the end.  Which wave reduces a
// chunk cannot change the block's top-k' (same row set), so the output is still a function of the data.
__device__ __forceinline__ uint64_t deal_chunk(uint32_t t, int waves_per_block)
{
    const uint64_t c = ((uint64_t)(t / waves_per_block) * gridDim.x + blockIdx.x) * waves_per_block + t % waves_per_block;
    return uniform_u64(c);  // the division runs on the VALU: tell the compiler the result is wave-uniform (scalar loads)
}

// The wave's next ticket from the block's counter (which starts at waves_per_block: wave w begins on ticket w).
__device__ __forceinline__ uint32_t deal_claim(uint32_t *s_next, int lane)
{
    uint32_t t = 0;
    if (lane == 0) t = atomicAdd(s_next, 1u);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
}

// Requests the U rows of a chunk from its descriptor: first corpus row | valid rows << 32 (0 rows beyond the end).  p: the kernel's
// parameter struct (its `corpus`), by reference -- handed the pointer by value the compiler addresses the rows through a vector
// register pair instead of the scalar base.
template <int U, bool NT, class P>
__device__ __forceinline__ void deal_issue_loads(const P &p, uint64_t desc, int lane, f32x4 (&c)[U], uint32_t (&row)[U])
{
    const uint32_t row0 = (uint32_t)desc, cnt = (uint32_t)(desc >> 32);
#pragma unroll
    for (int j = 0; j < U; ++j) {
        row[j] = row0 + ((uint32_t)j < cnt ? (uint32_t)j : 0u);  // rows beyond cnt re-read row0 (result discarded)
        const f32x4 *src = reinterpret_cast<const f32x4 *>(p.corpus + (uint64_t)row[j] * 256) + lane;
        c[j] = NT ? __builtin_nontemporal_load(src) : *src;
    }
}

}  // namespace smt
