// scan_narrow.hip -- K2 for NARROW rows: scan_narrow_kernel<RPL, NQ, FILTERED>, rows of 64 floats (256 B) against 1 or up to 4
// queries.  Launched by launch_search_slab (scan_slab.hip) like the wide and typed kernels; followed by finish_slab.hip's
// <64, float> form.  Neither the 256 scan nor the slab scan can read such a row: both give a wave ONE row per load.
//
// LAYOUT.  A wave load instruction still reads 1 KiB contiguous, as scan_topk.hip found the memory system wants -- so ONE
// global_load_dwordx4 covers RPL = FOUR adjacent rows: lanes 16 g .. 16 g + 15 hold row r + g, lane l the components
// 4 (l % 16) .. + 3 of its row.  A row sits in exactly one DPP row of 16 lanes: scan_byte.hip's geometry, and the loaded dwords ARE
// the operands -- nothing is widened.  The queries sit in registers in the matching layout, ONE float4 per query and lane, all four
// lane groups holding the same components.  RPL is a template parameter (D = 256 / RPL, 64 / RPL lanes a row); only RPL = 4 is
// built and instantiated: at RPL = 2 a row would span two DPP rows, the tree would need a level across them and a chunk-table entry
// two loads -- none of that is written.
//
// ROWS IN FLIGHT.  A step takes SIXTEEN rows -- four loads, 4 KiB -- and the next sixteen are requested before the step is reduced:
// the bytes in flight per wave that scan_byte.hip, scan_half.hip and the 256 kernel keep.
//
// PRODUCTS.  Per (row, query) a lane runs ONE chain of a product and three fused multiply-adds for <c, q>, and one per row for
// |c|^2: the counting rule's four (f32_err_narrow, wide_rows.h).
//
// THE TREE.  A sum has four levels, all inside a DPP row.  narrow_sum4 is wave_sum4 (device_utils.h) without its last two levels:
// two selecting xor steps (quad permutes) and two row rotations, 11 instructions, and the four values it transposes are the
// step's four LOADS: afterwards lane l holds the sum for load l % 4 over its own 16-lane row, that is for row 4 (l % 4) + l / 16 of
// the step -- SIXTEEN rows out of ONE tree per value, never one tree per row.  wave_sum4's v_permlane16_swap / v_permlane32_swap
// levels ADD DPP rows to each other; here every DPP row is a different corpus row, so there is nothing for them to add and they
// are not used: the sixteen sums already lie one per (quad lane, DPP row), and the distances are computed where they lie.
//
// DISTANCES AND LISTS.  dist_f32_rs runs lane-parallel on all sixteen rows of the step (lanes 16 g .. 16 g + 3 speak for them), then
// the candidates under the list's threshold are filed one by one into the lane-distributed lists of lane_list.h; block merge,
// padding and order are that header's, shared with the family.  Steps are dealt to the waves round robin as there.
//
// INSTRUCTIONS per load of four rows and lane, one query (counted in the source; the byte scan's figure beside it):
//   narrow:  4 (<c, q>) + 4 (|c|^2) multiply-adds + 2 x 11 / 4 tree = 13.5 vector instructions for 1 KiB
//   byte:    16 conversions + 16 multiply-adds + 4 dot products + 2 x 11 / 4 tree = 41.5 for 1 KiB
// and per further query 4 + 11 / 4 = 6.75 against 18.75.
//
// QUERIES.  Four VGPRs per query slot; slots of 1 and 4 under __launch_bounds__(512).  launch_search_slab runs passes of FOUR
// queries.  From the build (gfx950): no scratch and no spills in any instantiation (DESIGN.md has the register counts).
//
// RANGE FILTER.  The chunk table of range_tables.hip has FILTER_CHUNK = 4 rows per entry, so one entry is ONE load and a step takes
// four entries.  A range may begin at any row, so a load is aligned to 256 B only; global_load_dwordx4 asks a lane for no more than
// its own 16-byte alignment, which every (row, l % 16) has, so the FILTERED instantiation keeps the same load.  A lane group whose
// row does not exist -- rows past the corpus' end in the last load, rows past an entry's count, entries past the table's end --
// reads a row that does (the last one, resp. the entry's first, resp. row 0) and its result is dropped: nothing is read past the
// corpus.
#include "wide_rows.h"
#include "lane_list.h"

namespace smt {

__device__ __forceinline__ float narrow_dot4(const f32x4 &a, const f32x4 &b)
{
    float acc = a.x * b.x;
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    return fmaf(a.w, b.w, acc);
}

// header: the tree.  Lane l: the sum over its 16-lane row of the input with index l % 4.
__device__ __forceinline__ float narrow_sum4(float a, float b, float c, float d, int lane)
{
    const bool odd = lane & 1, upper = lane & 2;
    const float ab = (odd ? b : a) + dpp_f<DPP_XOR1>(odd ? a : b);
    const float cd = (odd ? d : c) + dpp_f<DPP_XOR1>(odd ? c : d);
    float v = (upper ? cd : ab) + dpp_f<DPP_XOR2>(upper ? ab : cd);
    v += dpp_f<DPP_ROW_ROR4>(v);
    v += dpp_f<DPP_ROW_ROR8>(v);
    return v;
}

template <int RPL, int NQ, bool FILTERED>
__global__ void __launch_bounds__(512) scan_narrow_kernel(SlabScanParams p)
{
    static_assert(RPL == 4, "four rows per 1 KiB load (64 dimensions) is what is built: header");
    static_assert(NQ == 1 || NQ == 4, "1 or 4 query slots");
    constexpr int D = 256 / RPL;                    // floats of a row
    constexpr int LPR = 64 / RPL;                   // lanes of a row: one DPP row
    constexpr int LOADS = NARROW_STEP_ROWS / RPL;   // loads of a step; filtered: one chunk-table entry each
    static_assert(LOADS == 4 && FILTER_CHUNK == RPL, "the tree transposes four loads; an entry is one load");
    extern __shared__ __align__(16) unsigned char narrow_smem[];
    key_t64 *s_keys = reinterpret_cast<key_t64 *>(narrow_smem);   // [NQ][waves][64] (+ counts: lane_list.h)

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves_per_block = blockDim.x >> 6;
    const int kp = (int)p.kp;
    const int slot = lane & 3;                    // the load whose sums this lane holds behind a tree
    const uint32_t grp = (uint32_t)lane / LPR;    // which row of a load
    const int sub = lane % LPR;                   // which float4 of the row

    f32x4 q[NQ];
    float rq[NQ];
    bool qz[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        q[n] = reinterpret_cast<const f32x4 *>(p.queries + (size_t)((uint32_t)n < p.nq_active ? n : 0) * D)[sub];
        const float a2 = wave_sum(grp ? 0.0f : narrow_dot4(q[n], q[n]));   // (every lane group holds the query: one of them counts)
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
    const uint64_t n_steps = FILTERED ? (p.n_chunks + LOADS - 1) / LOADS : (p.n_rows + NARROW_STEP_ROWS - 1) / NARROW_STEP_ROWS;
    const const_u64_ptr const_table = (const_u64_ptr)(uintptr_t)p.chunk_table;   // written by an earlier kernel: scalar loads
    // The row THIS lane reads in each load of step k (header: always a row that exists) and, bit j, whether it counts.
    // Unfiltered: load j = rows 16 k + 4 j .. + 3.  Filtered: load j = the rows of table entry 4 k + j.
    auto locate = [&](uint64_t k, uint32_t (&row)[LOADS], uint32_t &ok) {
        ok = 0;
#pragma unroll
        for (int j = 0; j < LOADS; ++j) {
            if constexpr (FILTERED) {
                const uint64_t e = k * LOADS + j;
                const uint64_t desc = e < p.n_chunks ? const_table[uniform_u64(e)] : 0ull;
                const uint32_t first = (uint32_t)desc, cnt = (uint32_t)(desc >> 32);
                const bool have = grp < cnt;
                row[j] = first + (have ? grp : 0u);
                ok |= (have ? 1u : 0u) << j;
            } else {
                const uint64_t v = k * NARROW_STEP_ROWS + RPL * j + grp;
                const bool have = v < p.n_rows;
                row[j] = (uint32_t)(have ? v : p.n_rows - 1);
                ok |= (have ? 1u : 0u) << j;
            }
        }
    };
    auto issue = [&](const uint32_t (&row)[LOADS], f32x4 (&c)[LOADS]) {
#pragma unroll
        for (int j = 0; j < LOADS; ++j)
            c[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(p.corpus + (uint64_t)row[j] * D) + sub);
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
        f32x4 c[LOADS];
#pragma unroll
        for (int j = 0; j < LOADS; ++j) c[j] = cn[j];
        const uint32_t r_mine = slot == 0 ? rown[0] : slot == 1 ? rown[1] : slot == 2 ? rown[2] : rown[3];
        const bool ok_mine = ((okn >> slot) & 1u) != 0 && sub < LOADS;   // lanes 16 g .. 16 g + 3 speak for the sixteen rows
        const uint64_t kn = k + n_waves;
        if (kn < n_steps) {
            locate(kn, rown, okn);
            issue(rown, cn);
        }
        const float b2 = narrow_sum4(narrow_dot4(c[0], c[0]), narrow_dot4(c[1], c[1]), narrow_dot4(c[2], c[2]), narrow_dot4(c[3], c[3]), lane);
        const bool b2_zero = b2 == 0.0f;
        const float rs_b2 = __frsqrt_rn(b2);
#pragma unroll
        for (int n = 0; n < NQ; ++n) {
            const float t = narrow_sum4(narrow_dot4(c[0], q[n]), narrow_dot4(c[1], q[n]), narrow_dot4(c[2], q[n]), narrow_dot4(c[3], q[n]), lane);
            const float d = dist_f32_rs(t, rs_b2, b2_zero, rq[n], qz[n]);
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

slab_scan_kernel_t narrow_scan_kernel_of(int slots, bool filtered)
{
    if (slots == 1) return filtered ? scan_narrow_kernel<4, 1, true> : scan_narrow_kernel<4, 1, false>;
    return filtered ? scan_narrow_kernel<4, 4, true> : scan_narrow_kernel<4, 4, false>;
}

}  // namespace smt
