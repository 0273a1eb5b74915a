// lane_list.h -- the top-k' lists of the scan kernels that keep one list per query and wave (scan_slab.hip, scan_half.hip): a
// lane-distributed sorted list, and the merge of a block's lists into ONE block list per query.  Independent of how a row is stored.
#pragma once
#include "device_utils.h"

namespace smt {

// (d, r) into a lane-distributed list kept in (distance asc, row asc) order; the threshold is the entry of lane kp - 1
__device__ __forceinline__ void slab_list_insert(float &ld, uint32_t &lr, float &thr_d, uint32_t &thr_r, float d, uint32_t r, int lane, int kp)
{
    const bool less = (ld < d) || (ld == d && lr < r);
    const int pos = __popcll(__ballot(less));
    const float sd = dpp_f<DPP_WAVE_SHR1>(ld);
    const uint32_t sr = dpp_u<DPP_WAVE_SHR1>(lr);
    if (lane > pos) { ld = sd; lr = sr; }
    else if (lane == pos) { ld = d; lr = r; }
    thr_d = readlane_f(ld, kp - 1);
    thr_r = (uint32_t)__builtin_amdgcn_readlane((int)lr, kp - 1);
}

__device__ __forceinline__ bool slab_under(float d, uint32_t r, float thr_d, uint32_t thr_r)
{
    return d < thr_d || (d == thr_d && r < thr_r);
}

// Block merge: every wave's candidates ranked among all of the block's, one barrier for all queries, every slot of a block list
// written once (its key, or the padding from the first slot no key ranks into).  s_keys: [NQ][waves][64] keys followed by
// [NQ][waves] counts (slab_list_smem_bytes); block_lists: [NQ][gridDim.x][kp].  Every thread of the block calls it.
template <int NQ>
__device__ __forceinline__ void slab_block_merge(key_t64 *s_keys, const float (&ld)[NQ], const uint32_t (&lr)[NQ], uint32_t nq_active, int kp,
                                                 key_t64 *block_lists, int lane, int wave, int waves_per_block)
{
    unsigned int *s_valid = reinterpret_cast<unsigned int *>(s_keys + (size_t)NQ * waves_per_block * 64);   // [NQ][waves]
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        const bool have = lane < kp && lr[n] != 0xFFFFFFFFu;
        s_keys[((size_t)n * waves_per_block + wave) * 64 + lane] = have ? make_key(ld[n], lr[n]) : KEY_PAD;
        const unsigned int cnt = (unsigned int)__popcll(__ballot(have));
        if (lane == 0) s_valid[n * waves_per_block + wave] = cnt;
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        if ((uint32_t)n >= nq_active) break;   // (uniform over the block)
        const key_t64 *keys_n = s_keys + (size_t)n * waves_per_block * 64;
        key_t64 *out = block_lists + ((size_t)n * gridDim.x + blockIdx.x) * kp;
        const key_t64 mine = keys_n[wave * 64 + lane];
        if (mine != KEY_PAD) {
            int rank = 0;
            for (int w = 0; w < waves_per_block; ++w)
                for (int i = 0; i < kp; ++i) rank += (keys_n[w * 64 + i] < mine) ? 1 : 0;
            if (rank < kp) out[rank] = mine;
        }
        if (wave == 0 && lane < kp) {
            unsigned int total = 0;
            for (int w = 0; w < waves_per_block; ++w) total += s_valid[n * waves_per_block + w];
            if ((unsigned int)lane >= total) out[lane] = KEY_PAD;
        }
    }
}
inline size_t slab_list_smem_bytes(int slots, int waves) { return (size_t)slots * waves * 64 * sizeof(key_t64) + (size_t)slots * waves * sizeof(unsigned int); }

}  // namespace smt
