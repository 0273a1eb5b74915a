// scan_wide.hip -- K2, grouped: scan_wide_kernel, up to eight calls per corpus pass (tuning key scan_take), and its two-phase
// reducer over shared lists.  The protocol and the frame around the reducer: scan_group.h.
#include "scan_group.h"

namespace smt {

// ------------------------------------------------------------- K2, groups of eight (tuning key scan_take)
// scan_pair_kernel's protocol with a longer reach: a leader of step i reads the slots of steps i + 2 .. i + 14 and takes the longest
// prefix that passes, up to seven calls, so one corpus pass serves up to eight.  A launch of this kernel says so in its slot
// (WIDE_FAMILY in kp_blocks) and has a record of its own kind (WideRecord, an array of its own): a leader takes launches of its own
// kernel only, and scan_pair_kernel refuses these by the same compare.  Marks, the own-record test, the bounded waits, the error
// flag, the gate and the first rows requested before the decision is known are scan_pair_kernel's.
// A chunk is reduced in two PHASES over the same sixteen row registers.  Phase A is SMT_REDUCE_GROUP4: <c, c> and queries 0 .. 3,
// query g in row g of the wave.  Phase B, behind a wave-uniform n_on > 4, keeps <c, c> (one register) and runs queries 4 .. 7
// through the same heads, row steps and tail (wave_sum4_group_tail_queries: the query trees' additions without the <c, c>
// column), query g + 4 in row g -- so every query's nominations are bit for bit the one-query loop's (the row-not-quad rule).
// SHARED LISTS: the block keeps ONE sorted list per query, in LDS (shared_list.h: 32 keys, so this kernel serves kp <= 32), and
// one 16-byte record per query, {1 / |q|, q is zero, threshold}.  Lanes 16 g .. 16 g + 15 read the record of their query at the top
// of a phase (a broadcast), test their row against its threshold, and the wave offers what passed to the lists, query-major, rows
// ascending.  A wave sees 1 / waves of the block's rows: against the block's threshold instead of its own, one in five of the
// inserts remains, and the block's list -- the kp smallest keys of the block's rows, whichever wave met them -- is the answer the
// block writes: there is no merge behind the row loop.
template <bool NT>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(8, 8))) scan_wide_kernel(ScanParams p, WideParams pp)
{
    constexpr int U = 4;
    constexpr int NQ = WIDE_MAX;
    extern __shared__ unsigned char smem_raw[];   // (no alignment attribute: see scan_topk_kernel)
    key_t64 *s_list = reinterpret_cast<key_t64 *>(smem_raw);  // [NQ][32]: the block's lists (shared_list.h)

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves_per_block = blockDim.x >> 6;
    f32x4 *s_rec = reinterpret_cast<f32x4 *>(s_list + NQ * SHARED_LIST_KEYS);            // [NQ]: {1 / |q|, q is zero, threshold distance, threshold row}
    unsigned int *s_lock = reinterpret_cast<unsigned int *>(s_rec + NQ);                 // [NQ] (64 B)
    f32x4 *s_q = reinterpret_cast<f32x4 *>(s_lock + 16);                                 // [NQ][64]: the queries, one image per block
    unsigned long long *s_ctl = reinterpret_cast<unsigned long long *>(s_q + NQ * 64);    // [0] absorbed?, [1] calls served, [2] record state as read, [3..10] the list sets, own first
    unsigned long long *s_qptr = s_ctl + 3 + NQ;                                         // [7] queries taken along
    uint32_t *s_next = reinterpret_cast<uint32_t *>(s_qptr + (NQ - 1));                  // the block's next unclaimed chunk
    const int kp = (int)p.kp;
    WideRecord *rec = pp.recs + p.step % WIDE_RECS;
    const unsigned long long tag = p.step << PAIR_SHIFT;

    const int jj = lane & 3, gq = lane >> 4;         // this lane's row of the chunk and its query of each phase's four
    // What a lane needs of ITS query of a phase -- 1 / |q|, "q is zero", the threshold (distance, row) -- is the query's record;
    // the norms are not held in registers (sixteen scalar registers for eight norms are not there).  Wave 0 sets up the lists, the
    // locks, the records and the query images; the barriers below stand between its stores and the row loop.
    typedef float norm_f32x2 __attribute__((ext_vector_type(2)));
    const norm_f32x2 *s_norm_a = reinterpret_cast<const norm_f32x2 *>(s_rec + gq);                   // this lane's record of phase A: the norm half ...
    const unsigned long long *s_thr_a = reinterpret_cast<const unsigned long long *>(s_rec + gq) + 1;   // ... and the threshold (phase B: four records on)
    group_lists_setup<NQ>(s_list, s_rec, s_lock, wave, lane);
    if (wave == 0) {
        const f32x4 q0 = reinterpret_cast<const f32x4 *>(p.queries)[lane];
        group_query_norm(s_q, s_rec, 0, 0, q0, lane);
    }

    if (threadIdx.x == 0) {
        *s_next = (uint32_t)waves_per_block;
        unsigned long long cur;
        const unsigned long long code = group_look<WIDE_FAMILY, WIDE_RECS>(p, pp, rec, tag, cur);
        s_ctl[0] = code;
        s_ctl[2] = cur;
        s_ctl[3] = (unsigned long long)(uintptr_t)p.block_lists;
    }
    __syncthreads();
    if (uniform_u64(s_ctl[0]) == PAIR_ABSORBED) {
        if (blockIdx.x == 0 && wave == 0 && lane == 0)
            (void)__hip_atomic_fetch_add(pp.ctl + 3, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }

    SMT_GROUP_ROWS_BEGIN   // (the first rows are on their way before the decision is known)

    if (threadIdx.x == 0) s_ctl[1] = group_await<NQ>(pp, rec, tag, s_ctl[2], s_qptr, s_ctl + 4);
    __syncthreads();
    const int n_on = (int)(uint32_t)uniform_u64(s_ctl[1]);   // calls this pass serves, 1 .. NQ (an LDS read: told to be wave-uniform)
    if (n_on > 1) {   // (uniform over the block)
        // a phase's images are requested together, before its first norm is reduced: seven round trips one after the other would
        // stand in front of the row loop (a slot without a call reads the first taken query again: its lanes never insert, on_mine
        // below); a pass of four or fewer does not look at phase B's slots
        if (wave == 0) {
            f32x4 qn[NQ - 1];
#pragma unroll
            for (int n = 1; n < NQ; ++n)
                if (n < 4 || n_on > 4) qn[n - 1] = reinterpret_cast<const f32x4 *>((uintptr_t)uniform_u64(s_qptr[n < n_on ? n - 1 : 0]))[lane];
#pragma unroll
            for (int n = 1; n < NQ; ++n)
                if (n < 4 || n_on > 4) group_query_norm(s_q, s_rec, n, n, qn[n - 1], lane);
        }
        __syncthreads();   // the images and the records are wave 0's stores
    }

    // a lane's record of phase h as it stands now: the norm half never changes, the threshold is one 64-bit read (shared_list.h)
#define SMT_WIDE_RECORD(MINE, h)                                                                                  \
    f32x4 MINE;                                                                                                   \
    do {                                                                                                          \
        const norm_f32x2 nz = s_norm_a[8 * (h)];   /* (8-byte units: phase B's record is four records on) */      \
        const unsigned long long t = shared_list_threshold(s_thr_a + 8 * (h));                                    \
        MINE.x = nz.x;                                                                                            \
        MINE.y = nz.y;                                                                                            \
        MINE.z = __uint_as_float((uint32_t)t);                                                                    \
        MINE.w = __uint_as_float((uint32_t)(t >> 32));                                                            \
    } while (0)
    // D4: the phase's distances, lane 16 g + j holds row j against query g + 4 h.  What passed the (possibly stale) threshold is
    // offered to the lists in the order of the ballot's bits: query-major, rows ascending.
#define SMT_WIDE_TEST_INSERT(h, MINE, ON, AB, D4)                                                                 \
    do {                                                                                                          \
        const float D4 = dist_f32(AB, b2, (MINE).x, (MINE).y != 0.0f);                                            \
        const uint32_t thr_r_mine = __float_as_uint((MINE).w);                                                    \
        const bool cand = ((ON) & valid_mine) & ((D4 < (MINE).z) | ((D4 == (MINE).z) & (r_mine < thr_r_mine)));   \
        uint64_t pending = __ballot(cand) & 0x000F000F000F000Full;                                                \
        while (pending) {                                                                                         \
            const int b = __builtin_ctzll(pending);                                                               \
            pending &= pending - 1;                                                                               \
            const int n = (b >> 4) + 4 * (h);                                                                     \
            const float d = readlane_f(D4, b);                                                                    \
            const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)r_mine, b);                               \
            shared_list_insert(s_list + n * SHARED_LIST_KEYS, s_lock + n, reinterpret_cast<unsigned long long *>(s_rec + n) + 1, d, r, \
                               kp, lane, pp.ctl);                                                                 \
        }                                                                                                         \
    } while (0)
    // phase A: SMT_REDUCE_GROUP4 of scan_pair_kernel, instruction for instruction up to the distance; phase B behind it
#define SMT_REDUCE_WIDE(cq, rq4, VALID)                                                                           \
    do {                                                                                                          \
        const f32x4 qv0 = s_q[lane];                                                                              \
        const bool valid_mine = (uint32_t)jj < (VALID);                                                           \
        const uint32_t r_mine = (rq4) + (uint32_t)jj;                                                             \
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
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        const f32x4 qv2 = s_q[128 + lane], qv3 = s_q[192 + lane];                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
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
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        SMT_WIDE_RECORD(mine, 0);                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        wave_sum4_rows<5>(v5);                                                                                    \
        wave_sum4_group_tail(v5[0], v5[1], v5[2], v5[3], v5[4]);                                                  \
        const float b2 = v5[0];                                                                                   \
        SMT_WIDE_TEST_INSERT(0, mine, on_mine, v5[1], d4);                                                        \
        if (n_on > 4) {                                                                                           \
            __builtin_amdgcn_sched_barrier(0);                                                                    \
            const f32x4 qv4 = s_q[256 + lane], qv5 = s_q[320 + lane];                                             \
            float part4[2][4], w2[2];                                                                             \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                       \
                part4[0][j] = SMT_ROW_DOT((cq)[j], qv4);                                                          \
                part4[1][j] = SMT_ROW_DOT((cq)[j], qv5);                                                          \
            }                                                                                                     \
            wave_sum4_multi_head<2>(part4, w2, lane);                                                             \
            SMT_OPAQUE(w2[0]); SMT_OPAQUE(w2[1]);                                                                 \
            float v4[4] = {w2[0], w2[1], w2[0], w2[1]};                                                           \
            if (n_on > 6) {                                                                                       \
                __builtin_amdgcn_sched_barrier(0);                                                                \
                const f32x4 qv6 = s_q[384 + lane], qv7 = s_q[448 + lane];                                         \
                float part6[2][4], x2[2];                                                                         \
                _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                   \
                    part6[0][j] = SMT_ROW_DOT((cq)[j], qv6);                                                      \
                    part6[1][j] = SMT_ROW_DOT((cq)[j], qv7);                                                      \
                }                                                                                                 \
                wave_sum4_multi_head<2>(part6, x2, lane);                                                         \
                SMT_OPAQUE(x2[0]); SMT_OPAQUE(x2[1]);                                                             \
                v4[2] = x2[0]; v4[3] = x2[1];                                                                     \
            }                                                                                                     \
            __builtin_amdgcn_sched_barrier(0);                                                                    \
            SMT_WIDE_RECORD(mine_b, 1);                                                                           \
            __builtin_amdgcn_sched_barrier(0);                                                                    \
            wave_sum4_rows<4>(v4);                                                                                \
            wave_sum4_group_tail_queries(v4[0], v4[1], v4[2], v4[3]);                                             \
            SMT_WIDE_TEST_INSERT(1, mine_b, on_mine_b, v4[0], d4b);                                               \
        }                                                                                                         \
    } while (0)
    const bool on_mine = gq < n_on, on_mine_b = gq + 4 < n_on;   // (an absent query has thr = +inf and must never insert)
    SMT_GROUP_ROW_LOOP(SMT_REDUCE_WIDE)
#undef SMT_REDUCE_WIDE
#undef SMT_WIDE_TEST_INSERT
#undef SMT_WIDE_RECORD
    __syncthreads();
    if (wave == 0 && lane == 0) (void)__hip_atomic_fetch_add(p.gate, (unsigned long long)n_on, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    group_lists_out(s_list, s_ctl + 3, n_on, kp, wave, waves_per_block, lane);
}

void launch_scan_wide_kernel(bool nt, int blocks, int threads, hipStream_t st, const ScanParams &p, const WideParams &pp)
{
    hipLaunchKernelGGL(nt ? scan_wide_kernel<true> : scan_wide_kernel<false>, dim3(blocks), dim3(threads), wide_smem_bytes(threads), st, p, pp);
}

}  // namespace smt
