// scan_deep.hip -- K2, grouped: scan_deep_kernel, up to sixteen calls per corpus pass (tuning key scan_deep), its wave-wide
// decision and its four-phase folded reducer over shared lists.  The protocol and the frame around the reducer: scan_group.h.
#include "scan_group.h"

namespace smt {

// ------------------------------------------------------------- K2, groups of sixteen (tuning key scan_deep)
// scan_wide_kernel with twice the reach: a leader of step i reads the slots of steps i + 2 .. i + 30 and takes the longest prefix
// that passes, up to fifteen calls, so one corpus pass serves up to sixteen.  What a pass costs beyond its queries' trees -- the row
// loads and their waits, the <c, c> tree, the chunk claims, the loop -- is paid once per pass, whatever it serves.  A launch of
// this kernel says so in its slot (DEEP_FAMILY in kp_blocks) and has a record of its own kind (DeepRecord, an array of its own): a
// leader takes launches of its own kernel only, and the two older kernels refuse these by their compare.  Marks, the own-record
// test, the bounded waits, the error flag, the gate and the first rows requested before the decision is known are theirs.
// A chunk is reduced in FOUR phases over the same sixteen row registers, four queries each, phases 1 .. 3 written once
// (SMT_DEEP_PHASE) and instanced three times, each behind a wave-uniform n_on > 4 h.  The sixteen queries x four rows of a chunk are
// 64 (row, query) pairs, one per lane: rows AND queries are permuted by lane (device_utils.h, the folded lane map), so that the
// row steps fold a phase's four trees into one register and the four phases' registers go through ONE tail, and one distance, one
// compare and one ballot serve the chunk.  Every addition is one of wave_sum4's with its two operands, possibly exchanged -- every
// query's nominations are bit for bit the one-query loop's.
// The lists are scan_wide_kernel's shared lists (shared_list.h, kp <= 32), sixteen of them.
// THE DECISION is taken by a wave, not a thread: group_decide reads slot after slot from pinned host memory, three dependent round
// trips each, and fifteen slots in a row would stand in front of every block of the leader.  Here lane j reads the slot of step
// i + 2 (j + 1), fields and both step checks included, one ballot gives the prefix, the lanes below it write the marks and the
// record's entries, and one agent-scope release publishes the lot.

// The deciding WAVE (all 64 lanes): group_decide with the slots read side by side.  A lane's slot is PENDING until its step number
// is there, then passes or fails once and for all (the same tests in the same order as group_decide: step, fields, step again);
// what is taken is the run of passing lanes from lane 0.  Only the first lane behind that run is waited for, as long as
// scan_pair_wait_us allows, for all of them together: the slot group_decide would be waiting at.  Returns the calls taken
// (wave-uniform); the caller publishes.
__device__ __forceinline__ unsigned int deep_decide(const ScanParams &p, const DeepParams &pp, DeepRecord *rec, int lane)
{
    enum : int { SLOT_PENDING = 0, SLOT_PASS = 1, SLOT_FAIL = 2 };
    const unsigned long long t0 = wall_clock64();
    const unsigned long long want = p.step + 2ull * (unsigned long long)(lane + 1);
    const PairSlot *s = pp.ring + (want & pp.ring_mask);
    const unsigned long long expect = (unsigned long long)p.kp | pp.family | (unsigned long long)gridDim.x << 32;
    const SelSlot *ss = pp.sel_ring ? pp.sel_ring + (want & pp.ring_mask) : nullptr;   // (wave-uniform: all lanes or none)
    int status = (unsigned int)lane < pp.max_take ? SLOT_PENDING : SLOT_FAIL;   // (max_take <= 15: lanes 15 .. 63 never pass)
    unsigned long long query = 0, lists = 0;
    SelSlot sel = {0, 0, 0, 0};
    unsigned int taken = 0;
    for (;;) {
        if (status == SLOT_PENDING) {
            const unsigned long long s1 = __hip_atomic_load(&s->step, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
            if (s1 == want) {
                const unsigned long long corpus = sys_load(&s->corpus), n_virtual = sys_load(&s->n_virtual), kp_blocks = sys_load(&s->kp_blocks);
                const unsigned long long absorbable = sys_load(&s->absorbable);
                query = sys_load(&s->query);
                lists = sys_load(&s->lists);
                if (ss) {   // select_group: the call's select parameters, inside the same pair of step checks
                    sel.out_rows = sys_load(&ss->out_rows);
                    sel.out_dist = sys_load(&ss->out_dist);
                    sel.out_status = sys_load(&ss->out_status);
                    sel.row_base = sys_load(&ss->row_base);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
                const bool still = sys_load(&s->step) == want;   // (or the host was rewriting the slot, a ring's length ahead)
                const bool same = corpus == (unsigned long long)(uintptr_t)p.corpus && n_virtual == p.n_virtual && kp_blocks == expect;
                status = (still && absorbable && same) ? SLOT_PASS : SLOT_FAIL;
            } else if (s1 > want) {
                status = SLOT_FAIL;   // (a LATER step's number: the slot was reused)
            }
        }
        const unsigned long long pass = __ballot(status == SLOT_PASS);
        taken = (unsigned int)__builtin_ctzll(~pass);
        const bool waited_for = status == SLOT_PENDING && (unsigned int)lane == taken;
        if (__ballot(waited_for) == 0ull || pp.wait_ticks == 0ull || wall_clock64() - t0 >= pp.wait_ticks) break;
        __builtin_amdgcn_s_sleep(32);
    }
    if ((unsigned int)lane < taken) {
        flag_store(&rec->query[lane], query);
        flag_store(&rec->lists[lane], lists);
        if (ss) {   // (the caller's agent-scope release publishes these with the rest)
            SelSlot *m = &pp.sel_recs[p.step % DEEP_RECS].member[lane];
            flag_store(&m->out_rows, sel.out_rows);
            flag_store(&m->out_dist, sel.out_dist);
            flag_store(&m->out_status, sel.out_status);
            flag_store(&m->row_base, sel.row_base);
        }
        flag_store(&pp.recs[want % DEEP_RECS].state, (want << PAIR_SHIFT) | PAIR_ABSORBED);   // the mark
    }
    if (lane == 0) flag_store(&rec->taken, (unsigned long long)taken);
    return taken;
}

template <bool NT>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(8, 8))) scan_deep_kernel(ScanParams p, DeepParams pp)
{
    constexpr int U = 4;
    constexpr int NQ = DEEP_MAX;
    extern __shared__ unsigned char smem_raw[];   // (no alignment attribute: see scan_topk_kernel)
    key_t64 *s_list = reinterpret_cast<key_t64 *>(smem_raw);  // [NQ][32]: the block's lists (shared_list.h)

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves_per_block = blockDim.x >> 6;
    f32x4 *s_rec = reinterpret_cast<f32x4 *>(s_list + NQ * SHARED_LIST_KEYS);            // [NQ]: {1 / |q|, q is zero, threshold distance, threshold row}
    unsigned int *s_lock = reinterpret_cast<unsigned int *>(s_rec + NQ);                 // [NQ] (64 B)
    f32x4 *s_q = reinterpret_cast<f32x4 *>(s_lock + 16);                                 // [NQ][64]: the queries, one image per block
    unsigned long long *s_ctl = reinterpret_cast<unsigned long long *>(s_q + NQ * 64);    // [0] absorbed?, [1] calls served, [2] record state as read, [3..18] the list sets, own first
    unsigned long long *s_qptr = s_ctl + 3 + NQ;                                         // [15] queries taken along
    uint32_t *s_next = reinterpret_cast<uint32_t *>(s_qptr + (NQ - 1));                  // the block's next unclaimed chunk
    const int kp = (int)p.kp;
    DeepRecord *rec = pp.recs + p.step % DEEP_RECS;
    const unsigned long long tag = p.step << PAIR_SHIFT;

    // this lane's row of the chunk and its query of the sixteen (device_utils.h, the folded lane map: 64 lanes, 64 pairs)
    const int jj = wave_sum4_folded_row(lane), gq = wave_sum4_folded_query(lane);
    // (the records, the lists and the locks: see scan_wide_kernel.  Wave 0 sets them up and the leader's image; the images of the
    // calls taken along are set up phase by phase, wave h those of phase h)
    typedef float norm_f32x2 __attribute__((ext_vector_type(2)));
    const norm_f32x2 *s_norm_a = reinterpret_cast<const norm_f32x2 *>(s_rec + gq);                   // this lane's query's record: the norm half ...
    const unsigned long long *s_thr_a = reinterpret_cast<const unsigned long long *>(s_rec + gq) + 1;   // ... and the threshold
    group_lists_setup<NQ>(s_list, s_rec, s_lock, wave, lane);
    // (lane l keeps its 16 bytes of query n in the slot it reads them from: slot s of phase h holds query 4 h + (s ^ i'))
#define SMT_QUERY_NORM(n, qn) group_query_norm(s_q, s_rec, wave_sum4_folded_slot(n, lane), n, qn, lane)
    if (wave == 0) {
        const f32x4 q0 = reinterpret_cast<const f32x4 *>(p.queries)[lane];
        SMT_QUERY_NORM(0, q0);

        // lane 0 looks at the record and the gate as thread 0 of scan_wide_kernel does; the block that wins the record decides with
        // its whole wave (deep_decide), while the others wait at the gate
        unsigned long long g = 0, cur = 0;
        unsigned int absorbed = 0, won = 0;
        if (lane == 0) {
            *s_next = (uint32_t)waves_per_block;
            g = p.gate_open ? flag_load(p.gate) : 0ull;
            cur = flag_load(&rec->state);
            if (pp.absorbable && cur == (tag | PAIR_ABSORBED))
                absorbed = 1;   // (marked by the leader, an earlier launch of this stream)
            else if ((cur >> PAIR_SHIFT) != p.step &&
                     __hip_atomic_compare_exchange_strong(&rec->state, &cur, tag | PAIR_DECIDING, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                          __HIP_MEMORY_SCOPE_AGENT))
                won = 1;
        }
        if (__builtin_amdgcn_readfirstlane((int)won) != 0) {
            const unsigned int taken = deep_decide(p, pp, rec, lane);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // every lane's entries and marks before lane 0's state
            if (lane == 0) {
                cur = tag | (taken ? PAIR_PAIRED : PAIR_ALONE);
                __hip_atomic_store(&rec->state, cur, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                (void)__hip_atomic_fetch_add(pp.ctl + (taken ? 1 : 2), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                (void)__hip_atomic_fetch_add(pp.ctl + DEEP_CTL_BY_SIZE + taken, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (lane == 0) {
            if (!absorbed && g < p.gate_open) gate_wait(p);
            s_ctl[0] = absorbed ? PAIR_ABSORBED : 0ull;
            s_ctl[2] = cur;
            s_ctl[3] = (unsigned long long)(uintptr_t)p.block_lists;
        }
    }
    __syncthreads();
    if (uniform_u64(s_ctl[0]) == PAIR_ABSORBED) {
        if (blockIdx.x == 0 && wave == 0 && lane == 0)
            (void)__hip_atomic_fetch_add(pp.ctl + 3, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }

    SMT_GROUP_ROWS_BEGIN   // (the first rows are on their way before the decision is known)

    // (group_await of scan_group.h with the record's entries copied side by side, as deep_decide wrote them)
    if (wave == 0) {
        unsigned long long cur = 0;
        if (lane == 0) {
            cur = s_ctl[2];   // (this step's: the block has won the record and decided, or lost it)
            if (cur == (tag | PAIR_DECIDING)) {   // bounded like flag_wait: a decision that never comes ends in an error code
                const unsigned long long t0 = wall_clock64();
                while ((cur = flag_load(&rec->state)) == (tag | PAIR_DECIDING)) {
                    __builtin_amdgcn_s_sleep(8);
                    if (flag_load(pp.ctl) != 0ull) break;
                    if (wall_clock64() - t0 > 200000000ull) { flag_store(pp.ctl, 1ull); break; }
                }
            }
        }
        cur = uniform_u64(cur);   // (lane 0's)
        unsigned long long served = 1;
        if (cur == (tag | PAIR_PAIRED)) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            unsigned long long taken = uniform_u64(flag_load(&rec->taken));
            if (taken > (unsigned long long)(NQ - 1)) taken = NQ - 1;   // (never: the record is this step's)
            if ((unsigned long long)lane < taken) {   // the entries side by side, as they were written
                s_qptr[lane] = flag_load(&rec->query[lane]);
                s_ctl[4 + lane] = flag_load(&rec->lists[lane]);
            }
            served = 1 + taken;
        } else if (cur != (tag | PAIR_ALONE)) {
            if (lane == 0) flag_store(pp.ctl, 1ull);   // (a wait that ran out, or a record that is not this step's: alone, and the context reports it)
        }
        if (lane == 0) s_ctl[1] = served;
    }
    __syncthreads();
    const int n_on = (int)(uint32_t)uniform_u64(s_ctl[1]);   // calls this pass serves, 1 .. NQ (an LDS read: told to be wave-uniform)
    if (n_on > 1) {   // (uniform over the block)
        // Wave h sets up phase h (a block of fewer waves: h, h + waves, ...): four images requested together, then their norms --
        // four query rows in registers at a time, not fifteen.  A slot without a call reads the first taken query again (its lanes
        // never insert); a phase the pass does not reach is not looked at.
        for (int h = wave; 4 * h < n_on; h += waves_per_block) {
            f32x4 qn[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = 4 * h + g;
                if (n > 0) qn[g] = reinterpret_cast<const f32x4 *>((uintptr_t)uniform_u64(s_qptr[n < n_on ? n - 1 : 0]))[lane];
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = 4 * h + g;
                if (n > 0) SMT_QUERY_NORM(n, qn[g]);
            }
        }
        __syncthreads();   // the images and the records are other waves' stores
    }
#undef SMT_QUERY_NORM

    // a lane's record as it stands now: the norm half never changes, the threshold is one 64-bit read (shared_list.h)
#define SMT_DEEP_RECORD(MINE)                                                                                     \
    f32x4 MINE;                                                                                                   \
    do {                                                                                                          \
        const norm_f32x2 nz = s_norm_a[0];                                                                        \
        const unsigned long long t = shared_list_threshold(s_thr_a);                                              \
        MINE.x = nz.x;                                                                                            \
        MINE.y = nz.y;                                                                                            \
        MINE.z = __uint_as_float((uint32_t)t);                                                                    \
        MINE.w = __uint_as_float((uint32_t)(t >> 32));                                                            \
    } while (0)
    // D4: the chunk's 64 distances, lane l holds row jj against query gq.  ONE distance, one compare, one ballot per chunk.  What
    // passed the (possibly stale) threshold is offered to the lists in the order of the ballot's bits; the lists hold the k'
    // smallest keys whatever the order.  The query of bit b is wave_sum4_folded_query(b), on scalars.
#define SMT_DEEP_TEST_INSERT(MINE, AB, D4)                                                                        \
    do {                                                                                                          \
        const float D4 = dist_f32_rs(AB, rs_b2, b2_zero, (MINE).x, (MINE).y != 0.0f);                             \
        const uint32_t thr_r_mine = __float_as_uint((MINE).w);                                                    \
        const bool cand = (on_mine & valid_mine) & ((D4 < (MINE).z) | ((D4 == (MINE).z) & (r_mine < thr_r_mine))); \
        uint64_t pending = __ballot(cand);                                                                        \
        while (pending) {                                                                                         \
            const int b = __builtin_ctzll(pending);                                                               \
            pending &= pending - 1;                                                                               \
            const int n = 4 * (b >> 4) + ((4 - ((b >> 2) & 3)) & 3);                                              \
            const float d = readlane_f(D4, b);                                                                    \
            const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)r_mine, b);                               \
            shared_list_insert(s_list + n * SHARED_LIST_KEYS, s_lock + n, reinterpret_cast<unsigned long long *>(s_rec + n) + 1, d, r, \
                               kp, lane, pp.ctl);                                                                 \
        }                                                                                                         \
    } while (0)
    // Phase h = 1 .. 3, behind a wave-uniform n_on > 4 h: the heads of the lane's four slots, two at a time (slot s of phase h in this
    // lane is query 4 h + (s ^ i'), device_utils.h), each pair folded by the mirror step as soon as its heads are done, the two results
    // by the rotation by 8: ONE register X, in which quad i of every row holds the row sums of query 4 h + i'.  A phase that is on
    // computes all four slots; queries that are not there have images that are there anyway, and their lanes are off.
    // (n_h: the calls of this phase and behind it, asked of an opaque scalar copy chunk by chunk: as invariants of the row loop the
    // compares would be hoisted into scalar registers that loop does not have)
#define SMT_DEEP_PHASE(cq, h, X)                                                                                  \
    do {                                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        const f32x4 qva = s_q[256 * (h) + lane], qvb = s_q[256 * (h) + 64 + lane];                                \
        float parta[2][4], t2[2];                                                                                 \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                           \
            parta[0][j] = SMT_ROW_DOT((cq)[j], qva);                                                              \
            parta[1][j] = SMT_ROW_DOT((cq)[j], qvb);                                                              \
        }                                                                                                         \
        wave_sum4_swizzled_head<2>(parta, t2);                                                                    \
        float s0 = wave_sum4_fold_mirror(t2[0], t2[1]);                                                           \
        SMT_OPAQUE(s0);                                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        const f32x4 qvc = s_q[256 * (h) + 128 + lane], qvd = s_q[256 * (h) + 192 + lane];                         \
        float partc[2][4], u2[2];                                                                                 \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                           \
            partc[0][j] = SMT_ROW_DOT((cq)[j], qvc);                                                              \
            partc[1][j] = SMT_ROW_DOT((cq)[j], qvd);                                                              \
        }                                                                                                         \
        wave_sum4_swizzled_head<2>(partc, u2);                                                                    \
        X = wave_sum4_fold_ror8(s0, wave_sum4_fold_mirror(u2[0], u2[1]));                                         \
        SMT_OPAQUE(X);                                                                                            \
    } while (0)
#define SMT_DEEP_ON(h, N)                                                                                         \
    int N = n_on - 4 * (h);                                                                                       \
    asm volatile("" : "+s"(N));
    // The chunk: phase 0 with the <c, c> tree beside its first two slots (the head of three), then the phases that are on, their
    // registers folded through ONE tail as they come (x_0 with x_1 behind phase 1, x_2 with x_3 behind phase 3, then the two: the
    // additions of wave_sum4_group_tail_queries), <c, c> through the replicating tail beside it.  Then lane l holds
    // <row jj, query gq> and <c, c> of row jj: one record read, one distance, one compare, one ballot.  A register of a phase
    // that is off is whatever it is (its rows of the wave are off, the other rows never see it).
#define SMT_REDUCE_DEEP(cq, rq4, VALID)                                                                           \
    do {                                                                                                          \
        const f32x4 qv0 = s_q[lane];                                                                              \
        float part[3][4];                                                                                         \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) part[0][j] = SMT_ROW_DOT((cq)[j], (cq)[j]);                 \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        const f32x4 qv1 = s_q[64 + lane];                                                                         \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) part[1][j] = SMT_ROW_DOT((cq)[j], qv0);                     \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) part[2][j] = SMT_ROW_DOT((cq)[j], qv1);                     \
        float v3[3];                                                                                              \
        wave_sum4_swizzled_head<3>(part, v3);                                                                     \
        float cc = wave_sum4_fold_cc_rows(v3[0]);                                                                 \
        float w0 = wave_sum4_fold_mirror(v3[1], v3[2]);                                                           \
        SMT_OPAQUE(cc); SMT_OPAQUE(w0);                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        const f32x4 qv2 = s_q[128 + lane], qv3 = s_q[192 + lane];                                                 \
        float part2[2][4], v2[2];                                                                                 \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                           \
            part2[0][j] = SMT_ROW_DOT((cq)[j], qv2);                                                              \
            part2[1][j] = SMT_ROW_DOT((cq)[j], qv3);                                                              \
        }                                                                                                         \
        wave_sum4_swizzled_head<2>(part2, v2);                                                                    \
        float x0 = wave_sum4_fold_ror8(w0, wave_sum4_fold_mirror(v2[0], v2[1]));                                  \
        SMT_OPAQUE(x0);                                                                                           \
        float x1, x2, x3;                                                                                         \
        asm volatile("" : "=v"(x1), "=v"(x2));                                                                    \
        SMT_DEEP_ON(1, n_h1)                                                                                      \
        if (n_h1 > 0) SMT_DEEP_PHASE(cq, 1, x1);                                                                  \
        wave_sum4_fold_tail16_cc(cc, x0, x1);                                                                     \
        SMT_DEEP_ON(2, n_h2)                                                                                      \
        if (n_h2 > 0) {                                                                                           \
            SMT_DEEP_PHASE(cq, 2, x2);                                                                            \
            asm volatile("" : "=v"(x3));                                                                          \
            SMT_DEEP_ON(3, n_h3)                                                                                  \
            if (n_h3 > 0) SMT_DEEP_PHASE(cq, 3, x3);                                                              \
            wave_sum4_fold_tail16(x2, x3);                                                                        \
        }                                                                                                         \
        wave_sum4_fold_tail32_cc(cc, x0, x2);                                                                     \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        SMT_DEEP_RECORD(mine);                                                                                    \
        const bool valid_mine = (uint32_t)jj < (VALID);                                                           \
        const uint32_t r_mine = (rq4) + (uint32_t)jj;                                                             \
        const float rs_b2 = __frsqrt_rn(cc);                                                                      \
        const bool b2_zero = cc == 0.0f;                                                                          \
        SMT_DEEP_TEST_INSERT(mine, x0, d4);                                                                       \
    } while (0)
    const bool on_mine = gq < n_on;   // (an absent query has thr = +inf and must never insert)
    // THE ROWS ARE PERMUTED BY LANE once a chunk has landed (device_utils.h swizzle_rows4_folded: register k of lane l holds row
    // k ^ m(l), m the folded map's row), in place on the buffer that is reduced, and the seventeen trees' heads run without selects
    // (wave_sum4_swizzled_head): what a lane keeps and sends in a head depends on the lane alone, so the choice is made once on
    // the sixteen row registers and not seventeen times on the products.  Every product is the same chain on the same operands
    // in another register, every addition has the operands of wave_sum4's, possibly exchanged.
#define SMT_DEEP_CHUNK(cur, rq4, VALID)                                                                           \
    swizzle_rows4_folded((cur)[0], (cur)[1], (cur)[2], (cur)[3], lane);                                           \
    SMT_REDUCE_DEEP(cur, rq4, VALID);                                                                             \
    /* (the permuted rows end here: without this they count as live into the next turn and are copied about) */   \
    asm volatile("" : "=v"((cur)[0]), "=v"((cur)[1]), "=v"((cur)[2]), "=v"((cur)[3]))
    SMT_GROUP_ROW_LOOP(SMT_DEEP_CHUNK)
#undef SMT_DEEP_CHUNK
#undef SMT_REDUCE_DEEP
#undef SMT_DEEP_ON
#undef SMT_DEEP_PHASE
#undef SMT_DEEP_TEST_INSERT
#undef SMT_DEEP_RECORD
    __syncthreads();
    if (wave == 0 && lane == 0) (void)__hip_atomic_fetch_add(p.gate, (unsigned long long)n_on, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    group_lists_out(s_list, s_ctl + 3, n_on, kp, wave, waves_per_block, lane);
}

void launch_scan_deep_kernel(bool nt, int blocks, int threads, hipStream_t st, const ScanParams &p, const DeepParams &pp)
{
    hipLaunchKernelGGL(nt ? scan_deep_kernel<true> : scan_deep_kernel<false>, dim3(blocks), dim3(threads), deep_smem_bytes(threads), st, p, pp);
}

}  // namespace smt
