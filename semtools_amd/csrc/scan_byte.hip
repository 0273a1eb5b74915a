// scan_byte.hip -- K2 for BYTE rows: scan_byte_kernel<NQ, FILTERED>, rows of 256 signed bytes (256 B) against 1 or up to 4
// queries.  Launched by launch_search_slab (scan_slab.hip) like the wide and half kernels; followed by finish_slab.hip's <1, int8_t>
// form.
//
// LAYOUT.  A wave load instruction still reads 1 KiB contiguous, as scan_topk.hip found the memory system wants -- so ONE
// global_load_dwordx4 covers FOUR adjacent rows: lanes 16 g .. 16 g + 15 hold row r + g, sixteen bytes each (lane l: the bytes
// 16 (l % 16) .. + 15 of its row).  A row sits in exactly one DPP row of 16 lanes.  The queries sit in registers in the matching
// layout, sixteen floats per query and lane, all four lane groups holding the same components.
//
// ROWS IN FLIGHT.  A step takes SIXTEEN rows -- four loads, 4 KiB -- and the next sixteen are requested before the step is reduced:
// the bytes in flight per wave that scan_half.hip and the 256 kernel keep.
//
// |c|^2, EXACT.  v_dot4_i32_i8 on each of a lane's four packed dwords with itself, four instructions per lane and load, and an
// INTEGER tree.  The sum is at most 256 x 128^2 = 2^22 < 2^24: its conversion to f32 is exact, |c|^2 carries no rounding at all
// (f32_err_byte, byte_rows.h, says what that means for the bound).  -128, which the library's own rounding never stores but an
// adopted corpus may, is an int8 like any other here.
//
// <c, q>, the SIGNED form.  A lane widens its sixteen bytes to f32 by sign extension and integer conversion -- exact -- and runs ONE
// chain of a product and fifteen fused multiply-adds per (row, query), so that the terms stay sum |c_i q_i| <= |c||q| as the
// counting rule wants.  The widening is written as (float)(int8_t); on gfx950 the compiler makes ONE instruction of it,
// v_cvt_f32_i32_sdwa with sext() and a byte select, no v_bfe_i32.  The offset-binary form (xor 0x80808080, v_cvt_f32_ubyteN, subtract 128 sum q at the end)
// was NOT built: it cancels terms up to 32 times larger than |c||q| and the certificate would have to carry that.
//
// THE TREE.  A sum has four levels, all inside a DPP row: no permlane, no cross-row step.  row_sum4 is half_sum4 (scan_half.hip)
// without its last level -- two selecting xor steps and two rotations, 11 instructions -- and the four values it transposes are the
// step's four LOADS: afterwards lane l holds the sum for load l % 4 over its own 16-lane row, that is for row 4 (l % 4) + l / 16
// of the step: SIXTEEN rows out of one tree per value.  The same function runs the integer tree of |c|^2.
//
// QUERIES.  Sixteen VGPRs per query slot; slots of 1 and 4 under __launch_bounds__(512), as scan_half_kernel.  The launch gives a
// CU one block of eight waves, two per SIMD, so a wave may hold 256 VGPRs before anything is lost.  From the build (gfx950, ROCm
// 7.2; repeated in profiles/byte_rows.json): 79 / 82 VGPRs with one slot (plain / filtered), 193 / 191 with four, no scratch in
// any instantiation.  So the four-slot kernels keep their queries in REGISTERS and launch_search_slab runs passes of FOUR
// queries; slots of 2 and queries in LDS were not needed and not built.
//
// MEASURED on an MI355X (tools/byte_rows_rate.py, profiles/byte_rows.json): one query over 1 GiB streams 6.39 TB/s where the half
// and f32 scans reach 6.79 and 6.83 in the same process -- 25.0 G rows/s, x 1.88 the half scan's, but NOT the HBM rate: the 16
// conversions, 16 multiply-adds and 4 dot products per lane and load hold it (supposed from the counts).
//
// Lists, block merge, padding and order are lane_list.h's, shared with scan_slab.hip and scan_half.hip.  Steps are dealt to the
// waves round robin as there.
// RANGE FILTER.  The chunk table of range_tables.hip has FILTER_CHUNK = 4 rows per entry, so one entry is ONE load and a step takes
// four entries.  A range may begin at any row, so a load is aligned to 256 B only; global_load_dwordx4 asks a lane for no more than
// its own 16-byte alignment, which every (row, l % 16) has, so the FILTERED instantiation keeps the same load.  A lane group whose
// row does not exist -- rows past the corpus' end in the last load, rows past an entry's count, entries past the table's end --
// reads a row that does (the last one, resp. the entry's first, resp. row 0) and its result is dropped: nothing is read past the
// corpus.
#include "byte_rows.h"
#include "lane_list.h"

namespace smt {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float byte_dot16(const float (&c)[16], const float (&q)[16])
{
    float acc = c[0] * q[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) acc = fmaf(c[i], q[i], acc);
    return acc;
}

template <int CTRL, typename T>
__device__ __forceinline__ T dpp_any(T v)
{
    return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}

// header: the tree, for float or int.  Lane l: the sum over its 16-lane row of the input with index l % 4.
template <typename T>
__device__ __forceinline__ T row_sum4(T a, T b, T c, T d, int lane)
{
    const bool odd = lane & 1, upper = lane & 2;
    const T ab = (odd ? b : a) + dpp_any<DPP_XOR1>(odd ? a : b);
    const T cd = (odd ? d : c) + dpp_any<DPP_XOR1>(odd ? c : d);
    T v = (upper ? cd : ab) + dpp_any<DPP_XOR2>(upper ? ab : cd);
    v += dpp_any<DPP_ROW_ROR4>(v);
    v += dpp_any<DPP_ROW_ROR8>(v);
    return v;
}

template <int NQ, bool FILTERED>
__global__ void __launch_bounds__(512) scan_byte_kernel(SlabScanParams p)
{
    static_assert(NQ == 1 || NQ == BYTE_PASS_QUERIES, "1 or 4 query slots");
    constexpr int LOADS = BYTE_STEP_ROWS / 4;   // loads of a step, four rows each; filtered: one chunk-table entry each
    static_assert(LOADS == 4 && FILTER_CHUNK == 4, "the tree transposes four loads; an entry is one load");
    extern __shared__ __align__(16) unsigned char byte_smem[];
    key_t64 *s_keys = reinterpret_cast<key_t64 *>(byte_smem);   // [NQ][waves][64] (+ counts: lane_list.h)

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves_per_block = blockDim.x >> 6;
    const int kp = (int)p.kp;
    const int slot = lane & 3;                 // the load whose sums this lane holds behind a tree
    const uint32_t grp = (uint32_t)lane >> 4;  // which row of a load
    const int sub = lane & 15;                 // which sixteen bytes of the row

    float q[NQ][16], rq[NQ];
    bool qz[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        const f32x4 *qp = reinterpret_cast<const f32x4 *>(p.queries + (size_t)((uint32_t)n < p.nq_active ? n : 0) * SMT_DIM) + 4 * sub;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 v = qp[i];
            q[n][4 * i] = v.x; q[n][4 * i + 1] = v.y; q[n][4 * i + 2] = v.z; q[n][4 * i + 3] = v.w;
        }
        const float a2 = wave_sum(grp ? 0.0f : byte_dot16(q[n], q[n]));   // (every lane group holds the query: one of them counts)
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
    const uint64_t n_steps = FILTERED ? (p.n_chunks + LOADS - 1) / LOADS : (p.n_rows + BYTE_STEP_ROWS - 1) / BYTE_STEP_ROWS;
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
                const uint64_t v = k * BYTE_STEP_ROWS + 4 * j + grp;
                const bool have = v < p.n_rows;
                row[j] = (uint32_t)(have ? v : p.n_rows - 1);
                ok |= (have ? 1u : 0u) << j;
            }
        }
    };
    auto issue = [&](const uint32_t (&row)[LOADS], u32x4 (&c)[LOADS]) {
#pragma unroll
        for (int j = 0; j < LOADS; ++j)
            c[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(p.corpus) + (uint64_t)row[j] * 256) + sub);
    };

    // software pipeline: the rows of the wave's next step are requested before the current step is reduced
    u32x4 cn[LOADS];
    uint32_t rown[LOADS], okn = 0;
    uint64_t k = wave_global;
    if (k < n_steps) {
        locate(k, rown, okn);
        issue(rown, cn);
    }
    while (k < n_steps) {
        u32x4 c4[LOADS];
#pragma unroll
        for (int j = 0; j < LOADS; ++j) c4[j] = cn[j];
        const uint32_t r_mine = slot == 0 ? rown[0] : slot == 1 ? rown[1] : slot == 2 ? rown[2] : rown[3];
        const bool ok_mine = ((okn >> slot) & 1u) != 0 && sub < LOADS;   // lanes 16 g .. 16 g + 3 speak for the sixteen rows
        const uint64_t kn = k + n_waves;
        if (kn < n_steps) {
            locate(kn, rown, okn);
            issue(rown, cn);
        }
        float pa[NQ][LOADS];
        int pb[LOADS];
#pragma unroll
        for (int j = 0; j < LOADS; ++j) {
            const u32x4 w = c4[j];
            int s = __builtin_amdgcn_sdot4((int)w.x, (int)w.x, 0, false);
            s = __builtin_amdgcn_sdot4((int)w.y, (int)w.y, s, false);
            s = __builtin_amdgcn_sdot4((int)w.z, (int)w.z, s, false);
            pb[j] = __builtin_amdgcn_sdot4((int)w.w, (int)w.w, s, false);
            float c[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) c[i] = (float)(int8_t)(w[i / 4] >> (8 * (i % 4)));
#pragma unroll
            for (int n = 0; n < NQ; ++n) pa[n][j] = byte_dot16(c, q[n]);
        }
        const float b2 = (float)row_sum4<int>(pb[0], pb[1], pb[2], pb[3], lane);   // exact: an integer below 2^24
        const bool b2_zero = b2 == 0.0f;
        const float rs_b2 = __frsqrt_rn(b2);
#pragma unroll
        for (int n = 0; n < NQ; ++n) {
            const float t = row_sum4<float>(pa[n][0], pa[n][1], pa[n][2], pa[n][3], lane);
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

slab_scan_kernel_t byte_scan_kernel_of(int slots, bool filtered)
{
    if (slots == 1) return filtered ? scan_byte_kernel<1, true> : scan_byte_kernel<1, false>;
    return filtered ? scan_byte_kernel<BYTE_PASS_QUERIES, true> : scan_byte_kernel<BYTE_PASS_QUERIES, false>;
}

}  // namespace smt
