// scan_half.hip -- K2 for HALF rows: scan_half_kernel<NQ, FILTERED>, rows of 256 binary16 values (512 B) against 1 or up to 4
// queries.  Launched by launch_search_slab (scan_slab.hip) like the wide kernels; followed by finish_slab.hip's <1, half> form.
//
// LAYOUT.  A wave load instruction still reads 1 KiB contiguous, as scan_topk.hip found the memory system wants -- so ONE
// global_load_dwordx4 covers TWO adjacent rows: lanes 0 .. 31 hold the eight halves 8 l .. 8 l + 7 of row r, lanes 32 .. 63 the same
// of row r + 1.  The queries sit in registers in the matching layout, eight floats per query and lane, both halves of the wave
// holding the same components.  A lane widens its eight halves (v_cvt_f32_f16, or inside v_fma_mix_f32 where the compiler forms
// it; either is exact.  SUPPOSED: that both honour subnormal halves under the default denormal mode -- the subnormal row of
// tests/test_gpu_half_rows.py decides it) and runs one chain of eight multiply-adds per (row, query) and one for |c|^2.
//
// ROWS IN FLIGHT.  A step takes EIGHT rows -- four loads, 4 KiB -- and the next eight are requested before the step is reduced:
// the bytes in flight per wave of the 256 kernel (U = 4 rows of 1 KiB plus the prefetched four).
//
// THE TREE.  A row lives in a 32-lane half, so a sum has five levels and both rows of a load reduce at once: the halves never mix.
// half_sum4 is wave_sum4 (device_utils.h) without its last level: two selecting xor steps, two rotations, one v_permlane16_swap and
// add -- 13 instructions where wave_sum4 has 15 -- and the four values it transposes are the step's four LOADS: afterwards lane l
// holds the sum for load l % 4 over its own half, that is for row 2 (l % 4) + l / 32 of the step: eight rows out of one tree.
// COUNTED, not measured: one query takes two trees a step (<c, q> and <c, c>), 26 instructions for eight rows; four queries take
// five, 65.  Plain per-value trees over a half (four DPP adds, a copy, the swap and an add: 7) would take 4 loads x 2 values x 7
// = 56 resp. 4 x 5 x 7 = 140.
//
// Lists, block merge, padding and order are lane_list.h's, shared with scan_slab.hip: a lane-distributed sorted list per query,
// k' = min(64, top_k + guard band), one block list of key_t64 per query, strictly ascending, padded with KEY_PAD.  Steps are dealt
// to the waves round robin as there (the claimed deal of chunk_deal.h was not tried; its loader is written for f32 rows).
// Range-filtered scans walk the chunk table of range_tables.hip: FILTER_CHUNK = 4 rows per entry are two pair loads, a step takes
// two entries.  A range may begin at an odd row, so a pair is two rows that follow each other, aligned to 512 B only.  A lane
// whose row does not exist -- the second row of the last pair of an odd count, the rows past an entry's count, the entry past the
// table's end -- reads a row that does (the last one, resp. the entry's first) and its result is dropped: nothing is read past the
// corpus.
#include "half_rows.h"
#include "lane_list.h"

namespace smt {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float half_dot8(const float (&c)[8], const float (&q)[8])
{
    float acc = c[0] * q[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) acc = fmaf(c[i], q[i], acc);
    return acc;
}

// header: the tree.  Lane l: the sum over its 32-lane half of the input with index l % 4.
__device__ __forceinline__ float half_sum4(float a, float b, float c, float d, int lane)
{
    const bool odd = lane & 1, upper = lane & 2;
    const float ab = (odd ? b : a) + dpp_f<DPP_XOR1>(odd ? a : b);
    const float cd = (odd ? d : c) + dpp_f<DPP_XOR1>(odd ? c : d);
    float v = (upper ? cd : ab) + dpp_f<DPP_XOR2>(upper ? ab : cd);
    v += dpp_f<DPP_ROW_ROR4>(v);
    v += dpp_f<DPP_ROW_ROR8>(v);
    return add_lane_xor16(v);
}

template <int NQ, bool FILTERED>
__global__ void __launch_bounds__(512) scan_half_kernel(SlabScanParams p)
{
    static_assert(NQ == 1 || NQ == 4, "1 or 4 query slots");
    constexpr int LOADS = HALF_STEP_ROWS / 2;                 // pair loads of a step
    constexpr int ENTRIES = HALF_STEP_ROWS / FILTER_CHUNK;    // chunk-table entries of a step
    static_assert(LOADS == 4 && FILTER_CHUNK == 4, "the tree transposes four loads; an entry is two pair loads");
    extern __shared__ __align__(16) unsigned char half_smem[];
    key_t64 *s_keys = reinterpret_cast<key_t64 *>(half_smem);   // [NQ][waves][64] (+ counts: lane_list.h)

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves_per_block = blockDim.x >> 6;
    const int kp = (int)p.kp;
    const int slot = lane & 3;               // the load whose sums this lane holds behind a tree
    const uint32_t hi = (uint32_t)lane >> 5; // which row of a pair
    const int sub = lane & 31;               // which sixteen bytes of the row

    float q[NQ][8], rq[NQ];
    bool qz[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        const f32x4 *qp = reinterpret_cast<const f32x4 *>(p.queries + (size_t)((uint32_t)n < p.nq_active ? n : 0) * SMT_DIM) + 2 * sub;
        const f32x4 lo4 = qp[0], hi4 = qp[1];
        q[n][0] = lo4.x; q[n][1] = lo4.y; q[n][2] = lo4.z; q[n][3] = lo4.w;
        q[n][4] = hi4.x; q[n][5] = hi4.y; q[n][6] = hi4.z; q[n][7] = hi4.w;
        const float a2 = wave_sum(hi ? 0.0f : half_dot8(q[n], q[n]));   // (both halves hold the query: one of them counts)
        qz[n] = (a2 == 0.0f);
        rq[n] = qz[n] ? 0.0f : __frsqrt_rn(a2);
    }

    float ld[NQ], thr_d[NQ];
    uint32_t lr[NQ], thr_r[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        ld[n] = __builtin_inff();
        lr[n] = 0xFFFFFFFFu;
        thr_d[n] = __builtin_inff();
        thr_r[n] = 0xFFFFFFFFu;
    }

    const uint64_t wave_global = (uint64_t)blockIdx.x * waves_per_block + wave;
    const uint64_t n_waves = (uint64_t)gridDim.x * waves_per_block;
    const uint64_t n_steps = FILTERED ? (p.n_chunks + ENTRIES - 1) / ENTRIES : (p.n_rows + HALF_STEP_ROWS - 1) / HALF_STEP_ROWS;
    const const_u64_ptr const_table = (const_u64_ptr)(uintptr_t)p.chunk_table;   // written by an earlier kernel: scalar loads
    // The row THIS lane reads in each load of step k (header: always a row that exists) and, bit j, whether it counts.
    // Unfiltered: load j = rows 8 k + 2 j, + 1.  Filtered: load j = rows 2 (j % 2), + 1 of table entry 2 k + j / 2.
    auto locate = [&](uint64_t k, uint32_t (&row)[LOADS], uint32_t &ok) {
        ok = 0;
#pragma unroll
        for (int j = 0; j < LOADS; ++j) {
            if constexpr (FILTERED) {
                const uint64_t e = k * ENTRIES + j / 2;
                const uint64_t desc = e < p.n_chunks ? const_table[uniform_u64(e)] : 0ull;
                const uint32_t first = (uint32_t)desc, cnt = (uint32_t)(desc >> 32), at = (uint32_t)(j % 2) * 2 + hi;
                const bool have = at < cnt;
                row[j] = first + (have ? at : 0u);
                ok |= (have ? 1u : 0u) << j;
            } else {
                const uint64_t v = k * HALF_STEP_ROWS + 2 * j + hi;
                const bool have = v < p.n_rows;
                row[j] = (uint32_t)(have ? v : p.n_rows - 1);
                ok |= (have ? 1u : 0u) << j;
            }
        }
    };
    auto issue = [&](const uint32_t (&row)[LOADS], f32x4 (&c)[LOADS]) {
#pragma unroll
        for (int j = 0; j < LOADS; ++j)
            c[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(reinterpret_cast<const char *>(p.corpus) + (uint64_t)row[j] * 512) + sub);
    };

    // software pipeline: the rows of the wave's next step are requested before the current step is reduced
    f32x4 cn[LOADS];
    uint32_t rown[LOADS], okn = 0;
    uint64_t k = wave_global;
    if (k < n_steps) {
        locate(k, rown, okn);
        issue(rown, cn);
    }
    while (k < n_steps) {
        f32x4 c4[LOADS];
#pragma unroll
        for (int j = 0; j < LOADS; ++j) c4[j] = cn[j];
        const uint32_t r_mine = slot == 0 ? rown[0] : slot == 1 ? rown[1] : slot == 2 ? rown[2] : rown[3];
        const bool ok_mine = ((okn >> slot) & 1u) != 0 && sub < LOADS;   // lanes 0 .. 3 and 32 .. 35 speak for the eight rows
        const uint64_t kn = k + n_waves;
        if (kn < n_steps) {
            locate(kn, rown, okn);
            issue(rown, cn);
        }
        float pa[NQ][LOADS], pb[LOADS];
#pragma unroll
        for (int j = 0; j < LOADS; ++j) {
            const f16x8 h = __builtin_bit_cast(f16x8, c4[j]);
            float c[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) c[i] = (float)h[i];
            pb[j] = half_dot8(c, c);
#pragma unroll
            for (int n = 0; n < NQ; ++n) pa[n][j] = half_dot8(c, q[n]);
        }
        const float b2 = half_sum4(pb[0], pb[1], pb[2], pb[3], lane);
#pragma unroll
        for (int n = 0; n < NQ; ++n) {
            const float t = half_sum4(pa[n][0], pa[n][1], pa[n][2], pa[n][3], lane);
            const float d = dist_f32(t, b2, rq[n], qz[n]);
            const bool cand = ok_mine && (uint32_t)n < p.nq_active && slab_under(d, r_mine, thr_d[n], thr_r[n]);
            uint64_t pending = __ballot(cand);
            while (pending) {
                const int j = __builtin_ctzll(pending);
                pending &= pending - 1;
                const float dj = readlane_f(d, j);
                const uint32_t rj = (uint32_t)__builtin_amdgcn_readlane((int)r_mine, j);
                if (slab_under(dj, rj, thr_d[n], thr_r[n])) slab_list_insert(ld[n], lr[n], thr_d[n], thr_r[n], dj, rj, lane, kp);
            }
        }
        k = kn;
    }

    slab_block_merge<NQ>(s_keys, ld, lr, p.nq_active, kp, p.block_lists, lane, wave, waves_per_block);
}

slab_scan_kernel_t half_scan_kernel_of(int slots, bool filtered)
{
    if (slots == 1) return filtered ? scan_half_kernel<1, true> : scan_half_kernel<1, false>;
    return filtered ? scan_half_kernel<4, true> : scan_half_kernel<4, false>;
}

}  // namespace smt
