// scan_nibble.hip -- K2 for NIBBLE rows: scan_nibble_kernel<NQ, FILTERED>, rows of 256 signed 4-bit integers (128 B) against 1 or
// up to 4 queries.  Launched by launch_search_slab (scan_slab.hip) like the half and byte kernels; followed by finish_slab.hip's
// <1, nibble_t> form.
//
// WHY INTEGERS.  The byte scan widens every component to f32 and runs one multiply-add each; it is held by the VALU, not by HBM
// (profiles/byte_rows.json).  A nibble scan built that way would need a third instruction per component to unpack it and deliver
// FEWER rows per second.  Here the dot product never leaves i32: v_dot8_i32_i4 multiplies eight nibble pairs and adds them to an
// accumulator in one instruction, and the query is made integers once per wave.
//
// LAYOUT.  A wave load instruction still reads 1 KiB contiguous, as scan_topk.hip found the memory system wants -- so ONE
// global_load_dwordx4 covers EIGHT adjacent rows: lanes 8 g .. 8 g + 7 hold row r + g, sixteen bytes each (lane l: the elements
// 32 (l % 8) .. + 31 of its row, four dwords of eight consecutive elements in the order v_dot8 pairs them: nibble_rows.h).
//
// ROWS IN FLIGHT.  A step takes THIRTY-TWO rows -- four loads, 4 KiB -- and the next thirty-two are requested before the step is
// reduced: the bytes in flight per wave that the half and byte scans keep.
//
// THE QUERY, INTEGERS ONCE PER WAVE.  u = q x rsqrt(|q|^2), n_i = rint(2^22 u_i), |n_i| <= 2^22 (+ 2 from the roundings of u).
// n_i is written as six BALANCED base-16 digits d_p in [-8, 7], n_i = sum d_p 16^p: their range, -8 947 848 .. 7 829 367, covers
// +-2^22; the 2^23 a seventh bit of scale would need does not fit, hence 2^22.  The digits come without a loop: n_i + 0x888888 is
// positive and below 16^6, its ordinary hex digit p is d_p + 8, and that xor 8 is d_p as a two's complement nibble.  A lane keeps,
// per query slot, 6 planes x 4 dwords, each plane packed in the row's nibble order; all eight lane groups hold the same.  A zero
// query has u = 0, every plane zero, and keeps the qz rule of dist_f32.
//
// PER (ROW, QUERY) a lane runs 24 v_dot8 -- six planes over its four dwords, D_p = sum c_i d_p,i -- and five shift-adds in Horner
// form, ((((D_5 16 + D_4) 16 + D_3) 16 + D_2) 16 + D_1) 16 + D_0 = sum c_i n_i; four more v_dot8 of the dwords with themselves
// give |c|^2.  COUNTED: 33 vector instructions per load of EIGHT rows at one query, plus the trees; the byte scan runs at least 36
// (16 conversions, 16 multiply-adds, 4 dot products) per load of FOUR rows: about 2.2 x fewer per row.
//
// EVERYTHING IS EXACT IN i32.  Per lane |sum c_i n_i| <= 32 x 8 x (2^22 + 2) < 2^30 + 2^10.  Over the row, by Cauchy-Schwarz,
// |<c, n>| <= |c|_2 |n|_2 <= 128 x (2^22 + 8) < 2^30 (|c|_2 <= 16 x 8; |n|_2 <= 2^22 |u|_2 + 16 x 1/2, |u|_2 <= 1 + 2^-22).  A
// partial Horner value is the same sum over the digits from p up, sum c_i (n_i div 16^p, balanced), bounded by 32 x 8 x
// (2^(22 - 4p) + 9) and shifted by four only while that keeps it under the full bound; a partial tree sum is the dot product of
// sub-vectors of c and n, bounded the same way.  |c|^2 <= 256 x 64 = 2^14.  Nothing comes near 2^31, and integer adds are
// order-free: the tree may transpose as it likes.
//
// THE TREE.  A row lives in EIGHT lanes, so a sum has three levels.  oct_sum4 is row_sum4 (scan_byte.hip) without its last
// rotation: two selecting xor steps (2 + 1, 2 + 1, then 2 + 1 instructions) transpose the step's four LOADS inside each quad, and
// ONE row rotation by four adds the group's other quad -- 10 integer instructions.  The rotation hands lanes 0 .. 3 of a 16-lane
// row the quad of ANOTHER group; so afterwards the lanes l with l & 4 set hold the sum for load l % 4 over their own group, that is
// for row 8 (l % 4) + l / 8 of the step: thirty-two lanes speak for THIRTY-TWO rows out of one tree per value.  COUNTED: one query
// takes two trees a step (<c, n> and |c|^2), 20 instructions for 32 rows; four queries take five, 50.
//
// AFTER THE TREE: one v_cvt_f32_i32 of <c, n> -- its only rounding --, times 2^-22 (exact), times rsqrt((float)|c|^2) (the
// conversion of an integer <= 2^14 is exact), d = max(0, 1 - that), a zero row by dist_f32's rule.  f32_err_nibble (nibble_rows.h)
// is derived from exactly these operations and the query's representation.
//
// QUERIES IN REGISTERS.  24 VGPRs per query slot, 96 with four; slots of 1 and 4 under __launch_bounds__(512) as the other scans:
// a CU runs one block of eight waves, two per SIMD, so a wave may hold 256 VGPRs before anything is lost.  From the build (gfx950,
// ROCm 7.2): 82 / 80 VGPRs with one slot (plain / filtered), 174 / 172 with four, no scratch in any instantiation: COUNTED, the
// 96 query VGPRs cost no occupancy under this launch.
//
// MEASURED on an MI355X (tools/nibble_rows_rate.py, profiles/nibble_rows.json): one query over 1 GiB streams 6.11 TB/s where the
// byte and f32 scans reach 6.39 and 6.81 in the same process -- 47.8 G rows/s, x 1.91 the byte scan's and x 7.2 the f32 scan's, but
// NOT the HBM rate: the kernel does not end HBM-bound.  A pass of four queries takes 481 us over 2^23 rows, 2.7 x the one-query
// launch, so the four-slot kernel is held by its 112 dot instructions per load outright.  SUPPOSED, from the counts and these two
// figures alone (no counter run): that the VALU holds the one-query kernel as well.  The issue rate of v_dot8_i32_i4 by itself was
// not measured.
//
// Lists, block merge, padding and order are lane_list.h's, shared with the wide, half and byte scans.  Steps are dealt to the waves
// round robin as there.
// RANGE FILTER.  The chunk table of range_tables.hip has FILTER_CHUNK = 4 rows (512 B) per entry, HALF a load: a step takes eight
// entries, load j the entries 8 k + 2 j and + 1, lane groups 0 .. 3 the rows of the first, 4 .. 7 of the second.  A range may begin
// at any row, so an entry is aligned to 128 B only; global_load_dwordx4 asks a lane for no more than its own 16-byte alignment,
// which every (row, l % 8) has.  A lane group whose row does not exist -- rows past the corpus' end in the last load, rows past an
// entry's count, entries past the table's end -- reads a row that does (the last one, resp. the entry's first, resp. row 0) and
// its result is dropped: nothing is read past the corpus.
#include "nibble_rows.h"
#include "lane_list.h"

namespace smt {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int NIBBLE_PLANES = 6;             // balanced base-16 digits of n_i = rint(2^22 u_i)
constexpr int NIBBLE_DIGIT_BIAS = 0x888888;  // 8 in each of the six digits: n + bias has the hex digits d_p + 8
constexpr float NIBBLE_QUERY_SCALE = 4194304.0f, NIBBLE_QUERY_UNSCALE = 1.0f / 4194304.0f;   // 2^22, 2^-22

template <int CTRL>
__device__ __forceinline__ int dpp_i(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false);
}

// header: the tree.  Lane l with l & 4 set: the sum over its 8-lane group of the input with index l % 4.
__device__ __forceinline__ int oct_sum4(int a, int b, int c, int d, int lane)
{
    const bool odd = lane & 1, upper = lane & 2;
    const int ab = (odd ? b : a) + dpp_i<DPP_XOR1>(odd ? a : b);
    const int cd = (odd ? d : c) + dpp_i<DPP_XOR1>(odd ? c : d);
    const int v = (upper ? cd : ab) + dpp_i<DPP_XOR2>(upper ? ab : cd);
    return v + dpp_i<DPP_ROW_ROR4>(v);
}

// the four dwords of a lane against four dwords of one plane (or themselves): 32 products into one i32
__device__ __forceinline__ int nibble_dot32(const u32x4 w, const int (&p)[4])
{
    int s = __builtin_amdgcn_sdot8((int)w.x, p[0], 0, false);
    s = __builtin_amdgcn_sdot8((int)w.y, p[1], s, false);
    s = __builtin_amdgcn_sdot8((int)w.z, p[2], s, false);
    return __builtin_amdgcn_sdot8((int)w.w, p[3], s, false);
}

template <int NQ, bool FILTERED>
__global__ void __launch_bounds__(512) scan_nibble_kernel(SlabScanParams p)
{
    static_assert(NQ == 1 || NQ == NIBBLE_PASS_QUERIES, "1 or 4 query slots");
    constexpr int LOADS = NIBBLE_STEP_ROWS / 8;                // loads of a step, eight rows each
    constexpr int ENTRIES = NIBBLE_STEP_ROWS / FILTER_CHUNK;   // chunk-table entries of a step
    static_assert(LOADS == 4 && FILTER_CHUNK == 4 && ENTRIES == 2 * LOADS, "the tree transposes four loads; an entry is half a load");
    extern __shared__ __align__(16) unsigned char nibble_smem[];
    key_t64 *s_keys = reinterpret_cast<key_t64 *>(nibble_smem);   // [NQ][waves][64] (+ counts: lane_list.h)

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves_per_block = blockDim.x >> 6;
    const int kp = (int)p.kp;
    const int slot = lane & 3;                 // the load whose sums this lane holds behind a tree
    const uint32_t grp = (uint32_t)lane >> 3;  // which row of a load
    const int sub = lane & 7;                  // which sixteen bytes of the row

    int qd[NQ][NIBBLE_PLANES][4];   // the digit planes of the query, this lane's 32 elements
    float sc[NQ];                   // 2^-22, or 0 for a zero query
    bool qz[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        const f32x4 *qp = reinterpret_cast<const f32x4 *>(p.queries + (size_t)((uint32_t)n < p.nq_active ? n : 0) * SMT_DIM);
        const f32x4 own = qp[lane];   // |q|^2 over the wave: four components a lane, the chain and tree f32_err_nibble counts
        const float a2 = wave_sum(fmaf(own.w, own.w, fmaf(own.z, own.z, fmaf(own.y, own.y, own.x * own.x))));
        qz[n] = (a2 == 0.0f);
        const float rq = qz[n] ? 0.0f : __frsqrt_rn(a2);
        sc[n] = qz[n] ? 0.0f : NIBBLE_QUERY_UNSCALE;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const f32x4 lo = qp[8 * sub + 2 * w], hi = qp[8 * sub + 2 * w + 1];
            const float e[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            uint32_t m[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) m[i] = (uint32_t)((int)__builtin_rintf(__fmul_rn(__fmul_rn(e[i], rq), NIBBLE_QUERY_SCALE)) + NIBBLE_DIGIT_BIAS);
#pragma unroll
            for (int d = 0; d < NIBBLE_PLANES; ++d) {
                uint32_t word = 0;
#pragma unroll
                for (int i = 0; i < 8; ++i) word |= ((m[i] >> (4 * d)) & 15u) << (4 * i);
                qd[n][d][w] = (int)(word ^ 0x88888888u);
            }
        }
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
    const uint64_t n_steps = FILTERED ? (p.n_chunks + ENTRIES - 1) / ENTRIES : (p.n_rows + NIBBLE_STEP_ROWS - 1) / NIBBLE_STEP_ROWS;
    const const_u64_ptr const_table = (const_u64_ptr)(uintptr_t)p.chunk_table;   // written by an earlier kernel: scalar loads
    // The row THIS lane reads in each load of step k (header: always a row that exists) and, bit j, whether it counts.
    // Unfiltered: load j = rows 32 k + 8 j .. + 7.  Filtered: load j = the rows of table entries 8 k + 2 j (groups 0 .. 3) and + 1.
    auto locate = [&](uint64_t k, uint32_t (&row)[LOADS], uint32_t &ok) {
        ok = 0;
#pragma unroll
        for (int j = 0; j < LOADS; ++j) {
            if constexpr (FILTERED) {
                const uint64_t e0 = k * ENTRIES + 2 * j, e1 = e0 + 1;   // (the same in every lane: both entries come by scalar loads)
                const uint64_t desc0 = e0 < p.n_chunks ? const_table[uniform_u64(e0)] : 0ull;
                const uint64_t desc1 = e1 < p.n_chunks ? const_table[uniform_u64(e1)] : 0ull;
                const uint64_t desc = (grp & 4u) ? desc1 : desc0;
                const uint32_t first = (uint32_t)desc, cnt = (uint32_t)(desc >> 32), at = grp & 3u;
                const bool have = at < cnt;
                row[j] = first + (have ? at : 0u);
                ok |= (have ? 1u : 0u) << j;
            } else {
                const uint64_t v = k * NIBBLE_STEP_ROWS + 8 * j + grp;
                const bool have = v < p.n_rows;
                row[j] = (uint32_t)(have ? v : p.n_rows - 1);
                ok |= (have ? 1u : 0u) << j;
            }
        }
    };
    auto issue = [&](const uint32_t (&row)[LOADS], u32x4 (&c)[LOADS]) {
#pragma unroll
        for (int j = 0; j < LOADS; ++j)
            c[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(p.corpus) + (uint64_t)row[j] * NIBBLE_ROW_BYTES) + sub);
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
        const bool ok_mine = ((okn >> slot) & 1u) != 0 && (lane & 4) != 0;   // lanes 8 g + 4 .. 8 g + 7 speak for the thirty-two rows
        const uint64_t kn = k + n_waves;
        if (kn < n_steps) {
            locate(kn, rown, okn);
            issue(rown, cn);
        }
        int pa[NQ][LOADS], pb[LOADS];
#pragma unroll
        for (int j = 0; j < LOADS; ++j) {
            const u32x4 w = c4[j];
            const int self[4] = {(int)w.x, (int)w.y, (int)w.z, (int)w.w};
            pb[j] = nibble_dot32(w, self);
#pragma unroll
            for (int n = 0; n < NQ; ++n) {
                int acc = nibble_dot32(w, qd[n][NIBBLE_PLANES - 1]);
#pragma unroll
                for (int d = NIBBLE_PLANES - 2; d >= 0; --d) acc = (int)((uint32_t)acc << 4) + nibble_dot32(w, qd[n][d]);
                pa[n][j] = acc;
            }
        }
        const float b2 = (float)oct_sum4(pb[0], pb[1], pb[2], pb[3], lane);   // exact: an integer <= 2^14
        const bool b2_zero = b2 == 0.0f;
        const float rs_b2 = __frsqrt_rn(b2);
#pragma unroll
        for (int n = 0; n < NQ; ++n) {
            const float t = (float)oct_sum4(pa[n][0], pa[n][1], pa[n][2], pa[n][3], lane);   // the one rounding of <c, n>
            const float d = dist_f32_rs(t, rs_b2, b2_zero, sc[n], qz[n]);
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

slab_scan_kernel_t nibble_scan_kernel_of(int slots, bool filtered)
{
    if (slots == 1) return filtered ? scan_nibble_kernel<1, true> : scan_nibble_kernel<1, false>;
    return filtered ? scan_nibble_kernel<NIBBLE_PASS_QUERIES, true> : scan_nibble_kernel<NIBBLE_PASS_QUERIES, false>;
}

}  // namespace smt
