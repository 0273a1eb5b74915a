// scan_pair.hip -- K2, grouped: scan_pair_kernel, up to four calls per corpus pass (tuning key scan_pair), and its group reducer.
// The protocol and the frame around the reducer: scan_group.h.
#include "scan_group.h"

namespace smt {

// (8 waves per SIMD = 64 VGPRs: what the select needs beside it, 2 x 64 + 4 x 96 = 512.  The four-query row loop with its queries
// in registers takes 81; with all four read from one LDS image per block and the norms held as wave-uniform values it fits.)
template <bool NT>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8))) scan_pair_kernel(ScanParams p, PairParams pp)
{
    constexpr int U = 4;
    constexpr int NQ = GROUP_MAX;
    extern __shared__ unsigned char smem_raw[];   // (no alignment attribute: see scan_topk_kernel)
    key_t64 *s_keys = reinterpret_cast<key_t64 *>(smem_raw);  // [NQ][waves][64]: the launch is sized for a full group

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves_per_block = blockDim.x >> 6;
    unsigned int *s_valid = reinterpret_cast<unsigned int *>(s_keys + (size_t)NQ * waves_per_block * 64);   // [NQ][waves] (256 B)
    f32x4 *s_q = reinterpret_cast<f32x4 *>(s_valid + 64);                                // [NQ][64]: the queries, one image per block
    unsigned long long *s_pair = reinterpret_cast<unsigned long long *>(s_q + NQ * 64);   // [0] absorbed?, [1] calls served, [2] record state as read, [3..5] lists
    unsigned long long *s_qptr = s_pair + 6;                                             // [3] queries taken along
    uint32_t *s_next = reinterpret_cast<uint32_t *>(s_qptr + 3);                         // the block's next unclaimed chunk
    const int kp = (int)p.kp;
    PairRecord *rec = pp.recs + p.step % PAIR_RECS;
    const unsigned long long tag = p.step << PAIR_SHIFT;

    // (the norms are the same in every lane: held as wave-uniform values they cost no vector register)
    float rq[NQ];
    bool qz[NQ];
#define SMT_LOAD_QUERY(n, ptr)                                                                                    \
    do {                                                                                                          \
        const f32x4 qn = reinterpret_cast<const f32x4 *>(ptr)[lane];                                              \
        if (wave == 0) s_q[(n) * 64 + lane] = qn;                                                                 \
        const float a2 = wave_sum(qn.x * qn.x + qn.y * qn.y + qn.z * qn.z + qn.w * qn.w);                         \
        qz[n] = readlane_f(a2, 0) == 0.0f;                                                                        \
        rq[n] = qz[n] ? 0.0f : readlane_f(__frsqrt_rn(a2), 0);                                                    \
    } while (0)
#pragma unroll
    for (int n = 1; n < NQ; ++n) { rq[n] = 0.0f; qz[n] = true; }
    SMT_LOAD_QUERY(0, p.queries);

    if (threadIdx.x == 0) {
        *s_next = (uint32_t)waves_per_block;
        unsigned long long cur;
        const unsigned long long code = group_look<0ull, PAIR_RECS>(p, pp, rec, tag, cur);
        s_pair[0] = code;
        s_pair[2] = cur;
    }
    __syncthreads();
    if (uniform_u64(s_pair[0]) == PAIR_ABSORBED) {
        if (blockIdx.x == 0 && wave == 0 && lane == 0)
            (void)__hip_atomic_fetch_add(pp.ctl + 3, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }

    SMT_GROUP_ROWS_BEGIN   // (the first rows are on their way before the decision is known)

    if (threadIdx.x == 0) s_pair[1] = group_await<NQ>(pp, rec, tag, s_pair[2], s_qptr, s_pair + 3);
    __syncthreads();
    const int n_on = (int)(uint32_t)uniform_u64(s_pair[1]);   // calls this pass serves, 1 .. NQ (an LDS read: told to be wave-uniform)
    if (n_on > 1) {   // (uniform over the block)
#pragma unroll
        for (int n = 1; n < NQ; ++n)
            if (n < n_on) SMT_LOAD_QUERY(n, (uintptr_t)uniform_u64(s_qptr[n - 1]));
        __syncthreads();   // the images are wave 0's stores
    }
#undef SMT_LOAD_QUERY

    // the row loop and the block merge of scan_topk_kernel<4, 4, NT, false>, the share of the queries that are not there skipped.
    // (ONE loop: instantiations behind a branch share the first rows' registers, and the allocator then takes more than either
    // alone -- the select needs this kernel at 64 VGPRs or fewer beside it.)
    //
    // The group reducer.  SMT_REDUCE_CHUNK4 (scan_topk_kernel's, used here at first with the queries read from LDS) runs one basic block per query: an LDS read of the query image with its wait directly
    // behind it, one wave_sum4 tree alone (its DPP wait states padded with s_nop) and a candidate test of nested exec-mask regions,
    // four times per chunk although the four queries test the same four rows -- the grouped pass was bound by instruction issue, not
    // by HBM.  Here the images are read at the top of the chunk, the trees run interleaved (device_utils.h: the heads of wave_sum4_multi,
    // <c, c> with the first two queries, then the other two -- five full trees at once do not fit 64 VGPRs --, then the row steps of
    // all five and ONE tail for the four query trees, wave_sum4_group_tail, which leaves tree g's total in row g), and ONE distance, ONE compare and ONE
    // ballot serve the sixteen (row, query) pairs: lane 16 g + j takes query g and row j, against its query's threshold.  The
    // arithmetic is frozen: per-lane FMA expression, tree and dist_f32 are bit for bit those of scan_topk_kernel<1, 4>, because an
    // UNCERTAIN answer depends on which near-ties the f32 scan nominated.  That is why query g sits in ROW g of the wave (lanes
    // 16 g .. 16 g + 3) and not in quad g: the rotations by 4 and 8 of wave_sum4 add the four quads of a row in an order that
    // depends on the quad -- lanes 4 .. 7 hold (q1 + q0) + (q3 + q2) where lanes 0 .. 3, which the one-query loop reads, hold
    // (q0 + q3) + (q2 + q1), one rounding apart -- while the same position of another row holds the same bits.
    // (The per-lane expression and the opaque tree values: SMT_ROW_DOT and SMT_OPAQUE, scan_group.h.)
#define SMT_GROUP_INSERT(n)                                                                                       \
    do {                                                                                                          \
        uint32_t m = (((n) < 2 ? pending_lo : pending_hi) >> (16 * ((n) & 1))) & 0xFu;                            \
        while (m) {                                                                                               \
            const int j = __builtin_ctz(m);                                                                       \
            m &= m - 1;                                                                                           \
            const float d = readlane_f(d4, 16 * (n) + j);                                                         \
            const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)r_mine, j);                               \
            const bool less = (ld[n] < d) || (ld[n] == d && lr[n] < r);                                           \
            const int pos = __popcll(__ballot(less));                                                             \
            /* (an earlier insert may have moved the threshold, the entry of lane kp - 1: the list is sorted over all */ \
            /* its lanes and a row comes once, so "(d, r) before the threshold" is "fewer than kp entries before (d, r)" */ \
            /* -- the same test, without a copy of the threshold in registers)                                          */ \
            if (pos < kp) {                                                                                       \
                const float sd = dpp_f<DPP_WAVE_SHR1>(ld[n]);                                                     \
                const uint32_t sr = dpp_u<DPP_WAVE_SHR1>(lr[n]);                                                  \
                if (lane > pos) { ld[n] = sd; lr[n] = sr; }                                                       \
                else if (lane == pos) { ld[n] = d; lr[n] = r; }                                                   \
                const float td = readlane_f(ld[n], kp - 1);                                                       \
                const uint32_t tr = (uint32_t)__builtin_amdgcn_readlane((int)lr[n], kp - 1);                      \
                if (gq == (n)) { s_mine->z = td; s_mine->w = __uint_as_float(tr); }                               \
            }                                                                                                     \
        }                                                                                                         \
    } while (0)
#define SMT_REDUCE_GROUP4(cq, rq4, VALID)                                                                         \
    do {                                                                                                          \
        const f32x4 qv0 = s_q[lane];                                                                              \
        const bool valid_mine = (uint32_t)jj < (VALID);   /* (VALID: the chunk's real rows, a wave-uniform count) */ \
        const uint32_t r_mine = (rq4) + (uint32_t)jj;   /* (a real row of the chunk is its first row + j) */      \
        /* <c, c> and the first two queries (a launch that serves one call reduces an image it does not use: a separate  */ \
        /* two-tree path costs registers, and the three interleaved trees cost what the two lone ones did).  One image   */ \
        /* at a time is live, read one query ahead of its products.                                                      */ \
        float part[3][4];                                                                                         \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) part[0][j] = SMT_ROW_DOT((cq)[j], (cq)[j]);                 \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        const f32x4 qv1 = s_q[64 + lane];                                                                         \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) part[1][j] = SMT_ROW_DOT((cq)[j], qv0);                     \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) part[2][j] = SMT_ROW_DOT((cq)[j], qv1);                     \
        float v3[3];                                                                                              \
        wave_sum4_multi_head<3>(part, v3, lane);                                                                  \
        SMT_OPAQUE(v3[0]); SMT_OPAQUE(v3[1]); SMT_OPAQUE(v3[2]);                                                  \
        /* twelve partial sums have become three: now there is room for the other two images and this lane's record, */ \
        /* which land behind the rest of the trees (the barriers keep the scheduler from moving the reads up)         */ \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        const f32x4 qv2 = s_q[128 + lane], qv3 = s_q[192 + lane];                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        /* The heads of queries 2 and 3 if the pass serves them; with one or two calls those trees do not exist and the tail is */ \
        /* fed registers that are there anyway (rows 2 and 3 are off).                                                          */ \
        float v5[5] = {v3[0], v3[1], v3[2], v3[1], v3[2]};                                                        \
        if (n_on > 2) {                                                                                           \
            float part2[2][4], v2[2];                                                                             \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                       \
                part2[0][j] = SMT_ROW_DOT((cq)[j], qv2);                                                          \
                part2[1][j] = SMT_ROW_DOT((cq)[j], qv3);                                                          \
            }                                                                                                     \
            wave_sum4_multi_head<2>(part2, v2, lane);                                                             \
            SMT_OPAQUE(v2[0]); SMT_OPAQUE(v2[1]);                                                                 \
            v5[3] = v2[0]; v5[4] = v2[1];                                                                         \
        }                                                                                                         \
        /* five values are live: this lane's record lands behind the row steps, then ONE tail for the four query trees -- tree */ \
        /* g's total comes out in row g, where this lane reads it                                                             */ \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        const f32x4 mine = *s_mine;   /* this lane's query: 1 / |q|, is it zero, threshold distance and row */    \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        wave_sum4_rows<5>(v5);                                                                                    \
        wave_sum4_group_tail(v5[0], v5[1], v5[2], v5[3], v5[4]);                                                  \
        const float b2 = v5[0], ab_mine = v5[1];                                                                  \
        const float d4 = dist_f32(ab_mine, b2, mine.x, mine.y != 0.0f);                                           \
        /* plain compares joined bitwise: no exec-mask region */                                                  \
        const uint32_t thr_r_mine = __float_as_uint(mine.w);                                                      \
        const bool cand = (on_mine & valid_mine) & ((d4 < mine.z) | ((d4 == mine.z) & (r_mine < thr_r_mine)));    \
        const uint64_t ballot = __ballot(cand);   /* (in two halves: 64-bit scalar compares take the VALU and a register pair) */ \
        const uint32_t pending_lo = (uint32_t)ballot & 0x000F000Fu, pending_hi = (uint32_t)(ballot >> 32) & 0x000F000Fu; \
        if (pending_lo | pending_hi) {   /* bits 16 g .. 16 g + 3: list g; query-major, rows ascending, as the per-query loop inserted */ \
            SMT_GROUP_INSERT(0);                                                                                  \
            SMT_GROUP_INSERT(1);                                                                                  \
            SMT_GROUP_INSERT(2);                                                                                  \
            SMT_GROUP_INSERT(3);                                                                                  \
        }                                                                                                         \
    } while (0)
    const int jj = lane & 3, gq = lane >> 4;         // this lane's row of the chunk and its query of the group
    const bool on_mine = gq < n_on;                  // (an absent query has thr = +inf and must never insert)
    // What a lane needs of ITS query -- 1 / |q|, "q is zero", the threshold (distance, row) -- lies in LDS, not in four registers
    // the loop does not have: a 16-byte record per lane in the key regions, which nothing else touches before the block merge
    // (behind the barrier that follows the loop).  Read once per chunk behind the first trees, rewritten by the lanes of a list
    // when an insert moves its threshold; a lane reads only what it wrote itself.
    f32x4 *s_mine = reinterpret_cast<f32x4 *>(smem_raw) + wave * 64 + lane;
    {
        const float rq_mine = gq == 0 ? rq[0] : gq == 1 ? rq[1] : gq == 2 ? rq[2] : rq[3];
        const bool qz_mine = gq == 0 ? qz[0] : gq == 1 ? qz[1] : gq == 2 ? qz[2] : qz[3];
        f32x4 rec;
        rec.x = rq_mine;
        rec.y = qz_mine ? 1.0f : 0.0f;
        rec.z = __builtin_inff();
        rec.w = __uint_as_float(0xFFFFFFFFu);
        *s_mine = rec;
    }
    float ld[NQ];
    uint32_t lr[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        ld[n] = __builtin_inff();
        lr[n] = 0xFFFFFFFFu;
    }
    SMT_GROUP_ROW_LOOP(SMT_REDUCE_GROUP4)
#undef SMT_REDUCE_GROUP4
#undef SMT_GROUP_INSERT
    __syncthreads();
    // a leader's block counts for the blocks of the calls it serves: the host's running totals count every launch
    // (thread 0 by wave and lane: threadIdx.x itself would be one more register alive across the loop)
    if (wave == 0 && lane == 0) (void)__hip_atomic_fetch_add(p.gate, (unsigned long long)n_on, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        if (n >= n_on) break;
        const bool have = lane < kp && lr[n] != 0xFFFFFFFFu;
        s_keys[((size_t)n * waves_per_block + wave) * 64 + lane] = have ? make_key(ld[n], lr[n]) : KEY_PAD;
        const unsigned int cnt = (unsigned int)__popcll(__ballot(have));
        if (lane == 0) s_valid[n * waves_per_block + wave] = cnt;
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        if (n >= n_on) break;
        const key_t64 *keys_n = s_keys + (size_t)n * waves_per_block * 64;
        key_t64 *out = (n == 0 ? p.block_lists : reinterpret_cast<key_t64 *>((uintptr_t)uniform_u64(s_pair[2 + n]))) + (size_t)blockIdx.x * kp;
        const key_t64 mine = keys_n[wave * 64 + lane];
        if (mine != KEY_PAD) {
            int rank = 0;
            for (int w = 0; w < waves_per_block; ++w)
                for (int i = 0; i < kp; ++i) rank += (keys_n[w * 64 + i] < mine) ? 1 : 0;
            if (rank < kp) out[rank] = mine;
        }
        if (wave == 0 && lane < kp) {   // the padding: slots [valid keys of the block, kp)
            unsigned int total = 0;
            for (int w = 0; w < waves_per_block; ++w) total += s_valid[n * waves_per_block + w];
            if ((unsigned int)lane >= total) out[lane] = KEY_PAD;
        }
    }
}

void launch_scan_pair_kernel(bool nt, int blocks, int threads, hipStream_t st, const ScanParams &p, const PairParams &pp)
{
    hipLaunchKernelGGL(nt ? scan_pair_kernel<true> : scan_pair_kernel<false>, dim3(blocks), dim3(threads), pair_smem_bytes(threads), st, p, pp);
}

}  // namespace smt
