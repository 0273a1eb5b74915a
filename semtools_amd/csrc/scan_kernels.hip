// scan_kernels.hip -- K2 (single/few-query cosine scan + per-wave top-k'): scan_topk_kernel, the grouped
// scan_pair_kernel (up to four calls per pass), scan_wide_kernel (up to eight) and scan_deep_kernel (up to sixteen) with their host/device pairing
// protocol, and launch_scan_topk, which runs the passes of a call
// and hands the block lists to the select stage (select.hip; optionally overlapped with the next scan: async
// select).  The chunk table of range-filtered scans is built in range_tables.hip, the cross-shard top-k merge
// lives in merge.hip, K4 (threshold mode) in threshold.hip.
// gfx950 only (wave64, DPP, 16 B/lane row loads).
//
// Replaces the `for doc / for line: f32::cosine(q, e)` loop and the
// sort/take of search_documents (reference src/search/mod.rs:84-119) and the
// exact filtered scan behind Store::search_line_embeddings
// (src/workspace/store.rs:481-546).
//
// Data layout: corpus row-major f32 [rows x 256]; one row = 1024 B = one
// wave-wide 16 B/lane load (perfectly coalesced).  A wave owns U rows per
// iteration (U independent 1 KiB loads in flight), reduces ab = <q,c> and
// b2 = <c,c> with DPP butterflies, and keeps its best k' candidates in a
// lane-distributed sorted list (lane i = i-th best).  The f32 scan only
// NOMINATES candidates: the merge stage recomputes the distance of the final
// k' rows with f64 accumulation in index order (simsimd "accurate" formula),
// so returned distances/ordering do not depend on the reduction tree.
#include "common.h"
#include "device_utils.h"
#include "device_flags.h"
#include "chunk_deal.h"
#include "shared_list.h"

namespace smt {

struct ScanParams {
    const float *corpus;
    const float *queries;  // [NQ x 256] (device)
    uint64_t n_virtual;    // unfiltered: rows to scan
    const uint64_t *chunk_table;  // FILTERED: one descriptor per chunk (row0 | valid rows << 32), see build_chunk_table_kernel
    uint64_t n_chunks;     // chunks to scan (FILTERED: table entries; else ceil(n_virtual / U))
    uint32_t kp;           // candidates kept per wave / per block (<= 64)
    uint32_t nq_active;    // queries of this pass that exist (<= NQ): a pass of 3 runs the 4-query kernel, slot 3 repeats query 0 and writes no list
    key_t64 *block_lists;  // [NQ][gridDim.x][kp]
    unsigned long long *stamps;  // optional (tuning key scan_debug_ptr): wall_clock64 per wave [start, loop end], per block [end]
    unsigned long long *flags;   // async select (or nullptr): [0] scan_done step, [1] select_done step, [2] blocks done, [3] timeout
    unsigned long long step;     // this launch's step number (>= 1)
    unsigned int *steal_ctr;     // STEAL: this launch's group counter (zero at launch), see scan_topk_kernel
    uint32_t steal_lr;           // STEAL: log2 of the rounds per group
    uint32_t steal_static;       // STEAL: a block's first steal_static groups are dealt statically (group g of block b = g * blocks + b)
    // START GATE (tuning keys scan_overlap, scan_gate_pct; nullptr = none): consecutive one-query scans run on two streams and overlap.
    // Every block adds 1 to *gate once its waves have finished their rows (a block of scan_pair_kernel: the number of calls its pass
    // serves; an absorbed launch nothing: the counter counts calls served, in blocks), and thread 0 of every block waits, before any row load,
    // until *gate >= gate_open -- the predecessor scan has finished scan_gate_pct per cent of its blocks' rows -- or gate_ticks of the
    // 100 MHz wall clock have passed.  The counter only grows (the host keeps the running total), so a later launch reads as "open"
    // too.  Advisory: it orders no data (list buffers and selects meet in stream order), so it can cost time, never an answer.
    unsigned long long *gate;
    unsigned long long gate_open;   // 0: no wait
    unsigned long long gate_ticks;
};

__device__ __forceinline__ void gate_wait(const ScanParams &p)
{
    if (flag_load(p.gate) >= p.gate_open) return;
    const unsigned long long t0 = wall_clock64();
    while (flag_load(p.gate) < p.gate_open && wall_clock64() - t0 < p.gate_ticks) __builtin_amdgcn_s_sleep(8);
}

// ------------------------------------------------------------------------- K2
// STEAL (round 6; unfiltered, 8-wave blocks): WHICH rows a block scans is decided while the kernel runs.  With the static deal every
// block owns the same number of rows, and the launch ends when the slowest block does: wall_clock64 stamps of 1 M-row launches
// (tools/scan_balance_async.py) show the blocks of one or two XCDs -- different ones from run to run -- finishing 10-14 us behind
// the median block (block ends 128 / 134 / 148 us: min / median / max), i.e. the kernel waits ~7 % of its time for a quarter of its
// blocks.  So the rounds (8 chunks = 32 rows, one per wave) are dealt in GROUPS of 2^steal_lr rounds, and only MOST of them up
// front: a block's first steal_static groups are static (group g of block b = g * gridDim.x + b, as before: nothing new in the
// loop but a compare), the last few per cent of the corpus are claimed group by group from a device counter -- STEAL_DEPTH groups
// ahead, by the wave that takes the first chunk of a group, the atomic's latency hidden behind that wave's row loads -- and
// published in an 8-entry LDS ring (group | base slot) that the waves' chunk claims look their rows up in.  Fast blocks simply
// come back for more.  (Everything dynamic was tried first: device-scope atomics on one address are served at ~65 per us on this
// part -- memory-side -- and 15 000 of them made the kernel 230 us instead of 151; a few hundred at the end are free.)
// RESULT, and why this is OFF by default (tuning key scan_steal = 0): the deal does what it should -- last block minus median
// block 2.7 us instead of 5-14 (profiles/r06_scan_balance.txt) -- and the launch is not a microsecond shorter (151.5 -> 152.5 us,
// profiles/r06_ab_steal.json): the median block moves UP to the last one, the last one does not come down.  The launch is bound by
// the part's AGGREGATE read rate (1.024 GB in 146-148 us of block time = 7.0 TB/s, the 0.88-0.90 of peak a 100 M-row launch shows
// too); blocks that finish early under the static deal are the ones that got a larger share of it, and their rows cost the same
// time whoever reads them.  Kept as an A/B switch with its parity test: it is the measurement that says the 1 M-row kernel has
// no imbalance left to recover, only its ramp.  Which block reduces a row cannot change
// the answer: the union of the blocks' k' best contains the k' best rows whatever the deal, and the select's threshold (the k'-th
// key of the union) is the k'-th smallest key of all rows either way.
constexpr int STEAL_DEPTH = 2;
template <int NQ, int U, bool NT, bool FILTERED, bool STEAL = false>
__global__ void __launch_bounds__(1024) scan_topk_kernel(ScanParams p)
{
    static_assert(!FILTERED || U == FILTER_CHUNK, "filtered scans use the chunk table's chunk size");
    static_assert(!STEAL || !FILTERED, "dynamic groups are for the unfiltered scan");
    // (No alignment attribute on smem_raw here, in scan_pair_kernel and in select.hip: while they shared a unit with the merge kernels,
    // whose declaration has none, that one decided the symbol's alignment -- ds_read2_b64 where a 16-byte base gives ds_read_b128.
    // Kept as it has always been compiled: other instructions in 32 kernels are a tuning change, to be measured on its own.)
    extern __shared__ unsigned char smem_raw[];
    key_t64 *s_keys = reinterpret_cast<key_t64 *>(smem_raw);  // [waves][64]

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves_per_block = blockDim.x >> 6;
    uint32_t *s_next = reinterpret_cast<uint32_t *>(s_keys + waves_per_block * 64);  // the block's next unclaimed chunk
    const uint64_t wave_global = (uint64_t)blockIdx.x * waves_per_block + wave;
    const int kp = (int)p.kp;
    if (p.stamps && lane == 0) p.stamps[wave_global * 2] = wall_clock64();

    f32x4 q[NQ];
    float rq[NQ];
    bool qz[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        q[n] = reinterpret_cast<const f32x4 *>(p.queries + ((uint32_t)n < p.nq_active ? n : 0) * 256)[lane];
        const float a2 = wave_sum(q[n].x * q[n].x + q[n].y * q[n].y + q[n].z * q[n].z + q[n].w * q[n].w);
        qz[n] = (a2 == 0.0f);
        rq[n] = qz[n] ? 0.0f : __frsqrt_rn(a2);
    }

    // lane-distributed sorted candidate lists
    float ld[NQ];
    uint32_t lr[NQ];
    float thr_d[NQ];
    uint32_t thr_r[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        ld[n] = __builtin_inff();
        lr[n] = 0xFFFFFFFFu;
        thr_d[n] = __builtin_inff();
        thr_r[n] = 0xFFFFFFFFu;
    }

    // (which chunks the block owns and how its waves claim them: chunk_deal.h)
    const uint64_t n_chunks = p.n_chunks;
    // the table was written by an earlier kernel and is read-only here: constant address space => scalar loads
    // (a plain global load is a VECTOR load that returns in order with the row loads and drains the pipeline)
    const const_u64_ptr const_table = (const_u64_ptr)(uintptr_t)p.chunk_table;
    auto chunk_id = [&](uint32_t t) -> uint64_t { return deal_chunk(t, waves_per_block); };
    auto claim = [&]() -> uint32_t { return deal_claim(s_next, lane); };
    // descriptor of chunk c: first corpus row | valid rows << 32 (0 rows beyond the end)
    auto fetch_desc = [&](uint64_t c) -> uint64_t {
        return c < n_chunks ? const_table[c] : 0ull;  // wave-uniform address in the constant address space: s_load
    };
    auto issue_loads = [&](uint64_t desc, f32x4 (&c)[U], uint32_t (&row)[U]) { deal_issue_loads<U, NT>(p, desc, lane, c, row); };
    // STEAL: ring[g & 7] = (group g of this block | its base slot / 2^steal_lr); the first STEAL_DEPTH groups are static
    uint2 *s_ring = reinterpret_cast<uint2 *>(s_next + 2);
    if (threadIdx.x == 0) *s_next = (uint32_t)waves_per_block;  // chunks 0..waves-1 are dealt: wave w starts on chunk w
    if constexpr (!STEAL) {   // (the host never gates a STEAL launch: launch_scan_topk)
        if (p.gate && threadIdx.x == 0 && p.gate_open) gate_wait(p);   // (the barrier below holds the other waves)
    }
    if constexpr (STEAL) {
        if (threadIdx.x < 8) s_ring[threadIdx.x] = make_uint2(0xFFFFFFFFu, 0u);
    }
    __syncthreads();

    // insert (d, r) into list n keeping (distance asc, row asc) order; the threshold is the entry of lane kp - 1
#define SMT_LIST_INSERT(n, d, r)                                                                                  \
    do {                                                                                                          \
        const bool less = (ld[n] < (d)) || (ld[n] == (d) && lr[n] < (r));                                         \
        const int pos = __popcll(__ballot(less));                                                                 \
        const float sd = dpp_f<DPP_WAVE_SHR1>(ld[n]);                                                             \
        const uint32_t sr = dpp_u<DPP_WAVE_SHR1>(lr[n]);                                                          \
        if (lane > pos) { ld[n] = sd; lr[n] = sr; }                                                               \
        else if (lane == pos) { ld[n] = (d); lr[n] = (r); }                                                       \
        thr_d[n] = readlane_f(ld[n], kp - 1);                                                                     \
        thr_r[n] = (uint32_t)__builtin_amdgcn_readlane((int)lr[n], kp - 1);                                       \
    } while (0)
    // One row against the NQ queries.  `valid` is wave-uniform and gates only the (rare) insert, never the
    // arithmetic: the four rows' DPP chains must stay free to interleave.  How `valid` is WRITTEN matters: with
    // "j < rows_in_chunk" clang hoists a branch in front of every row's reduction (+2 us per 1 M-row launch,
    // A/B on one box); "(v0 + j) < n" below does not trigger that, so the unfiltered loop keeps that form.
#define SMT_REDUCE_ROW(cj, rj, valid_expr)                                                                        \
    do {                                                                                                          \
        const bool valid = (valid_expr);                                                                          \
        const float b2 = wave_sum((cj).x * (cj).x + (cj).y * (cj).y + (cj).z * (cj).z + (cj).w * (cj).w);         \
        _Pragma("unroll") for (int n = 0; n < NQ; ++n) {                                                          \
            const float ab = wave_sum((cj).x * q[n].x + (cj).y * q[n].y + (cj).z * q[n].z + (cj).w * q[n].w);     \
            const float d = dist_f32(ab, b2, rq[n], qz[n]);                                                       \
            const uint32_t r = (rj);                                                                              \
            if (valid && (d < thr_d[n] || (d == thr_d[n] && r < thr_r[n]))) {                                     \
                SMT_LIST_INSERT(n, d, r);                                                                         \
            }                                                                                                     \
        }                                                                                                         \
    } while (0)

    // Four rows per chunk (the default U): the four rows' partial products are reduced TOGETHER -- wave_sum4 leaves the sum
    // of row j in the lanes with lane % 4 == j -- once for <c, c> and once per query, the distance is computed lane-parallel (four
    // (row, query) pairs per instruction) and one ballot finds the pairs under the query's threshold; only those (rare once the
    // lists have filled) are read out and inserted.  Per chunk and query 15 + ~14 instructions instead of 4 x (11 + ~14): with the
    // row-at-a-time form the reductions made two queries cost 1.4 x and four 2.3 x one query's pass (instruction issue, not HBM).
    // VALID(j): wave-uniform, is row j of the chunk a real row.
#define SMT_REDUCE_CHUNK4(cq, rq4, VALID)                                                                         \
    do {                                                                                                          \
        const int jj = lane & 3;                                                                                  \
        const bool ok_0 = VALID(0), ok_1 = VALID(1), ok_2 = VALID(2), ok_3 = VALID(3);                            \
        const bool valid_mine = jj == 0 ? ok_0 : jj == 1 ? ok_1 : jj == 2 ? ok_2 : ok_3;                          \
        const uint32_t r_mine = jj == 0 ? (rq4)[0] : jj == 1 ? (rq4)[1] : jj == 2 ? (rq4)[2] : (rq4)[3];          \
        float pb[4];                                                                                              \
        _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                             \
            pb[j] = (cq)[j].x * (cq)[j].x + (cq)[j].y * (cq)[j].y + (cq)[j].z * (cq)[j].z + (cq)[j].w * (cq)[j].w; \
        const float b2 = wave_sum4(pb[0], pb[1], pb[2], pb[3], lane);                                             \
        _Pragma("unroll") for (int n = 0; n < NQ; ++n) {                                                          \
            float pa[4];                                                                                          \
            const f32x4 qv = q[n];                                                                                \
            _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                         \
                pa[j] = (cq)[j].x * qv.x + (cq)[j].y * qv.y + (cq)[j].z * qv.z + (cq)[j].w * qv.w;                \
            const float ab = wave_sum4(pa[0], pa[1], pa[2], pa[3], lane);                                         \
            const float d4 = dist_f32(ab, b2, rq[n], qz[n]);                                                      \
            const bool cand = valid_mine && (d4 < thr_d[n] || (d4 == thr_d[n] && r_mine < thr_r[n]));             \
            uint32_t pending = (uint32_t)__ballot(cand) & 0xFu;                                                   \
            while (pending) {                                                                                     \
                const int j = __builtin_ctz(pending);                                                             \
                pending &= pending - 1;                                                                           \
                const float d = readlane_f(d4, j);                                                                \
                const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)r_mine, j);                           \
                if (d < thr_d[n] || (d == thr_d[n] && r < thr_r[n])) {   /* (an earlier insert may have moved the threshold) */ \
                    SMT_LIST_INSERT(n, d, r);                                                                     \
                }                                                                                                 \
            }                                                                                                     \
        }                                                                                                         \
    } while (0)
    // (one query too: 2 x 15 instead of 8 x 11 reduction instructions per chunk -- A/B of two builds on one box, tools/ab_libs.sh:
    // 155.6 -> 152.8 us per 1 M-row launch, 0.822 -> 0.838 of HBM)
    constexpr bool CHUNK4 = U == 4;

    // Software pipeline: the rows of the next chunk are requested right after the current chunk's rows arrived
    // (the register copy below waits for them) and fly during the current reduction; the chunk after that is
    // claimed meanwhile.  Measured alternatives, all slower at 1 M rows: a ping-pong over two register buffers
    // (two chunks in flight per wave: 160 vs 149 us), 16 waves/CU, U = 8 -- more than ~32 KiB of requests in
    // flight per CU costs bandwidth.
    if constexpr (!FILTERED) {
        auto issue_rows = [&](uint64_t v0, f32x4 (&c)[U], uint32_t (&row)[U]) {
#pragma unroll
            for (int j = 0; j < U; ++j) {
                uint64_t v = v0 + j;
                if (v >= p.n_virtual) v = p.n_virtual - 1;  // clamp (result discarded)
                row[j] = (uint32_t)v;
                const f32x4 *src = reinterpret_cast<const f32x4 *>(p.corpus + (uint64_t)row[j] * 256) + lane;
                c[j] = NT ? __builtin_nontemporal_load(src) : *src;
            }
        };
        // STEAL: a group this wave has asked the device counter for (lane 0 holds the answer once the atomic has returned)
        uint32_t pend_group = 0xFFFFFFFFu, pend_val = 0;
        auto chunk_v0 = [&](uint32_t t) -> uint64_t {
            if constexpr (STEAL) {
                // (8-wave blocks) round r = t / 8 of this block lies in its group g = r >> lr; the group's base comes from the ring
                const uint32_t r = t >> 3, g = r >> p.steal_lr, rho = r & ((1u << p.steal_lr) - 1u);
                uint32_t base;
                if (g < p.steal_static) {
                    base = g * gridDim.x + blockIdx.x;   // the static part of the deal: no look-up, no atomic
                } else {
                    // (a wave never waits while it holds an answer others may be waiting for: twice in a row only in the prologue)
                    if (pend_group != 0xFFFFFFFFu) {
                        if (lane == 0) s_ring[pend_group & 7u] = make_uint2(pend_group, p.steal_static * gridDim.x + pend_val);
                        pend_group = 0xFFFFFFFFu;
                    }
                    uint32_t tag, spins = 0;
                    do {
                        // (one address for the wave: a broadcast 8-byte read, so that tag and base come from ONE publish)
                        const unsigned long long e = *reinterpret_cast<volatile unsigned long long *>(s_ring + (g & 7u));
                        tag = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)e);
                        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(e >> 32));
                        if (++spins == (1u << 26)) __builtin_trap();   // (seconds: a publish that never comes must end in an error, not in a hung GPU)
                    } while (tag != g);   // (published STEAL_DEPTH groups ahead: the wait is for a wave that is late with its publish)
                }
                const uint64_t slot = ((uint64_t)base << p.steal_lr) + rho;
                const uint64_t v = (slot * 8u + (t & 7u)) * U;
                // the wave that takes the FIRST chunk of group g fetches group g + STEAL_DEPTH if that one is dynamic (unless its own
                // group lies past the end: then so do all later ones, and the ring gets a base that says so without asking the counter)
                if ((t & ((8u << p.steal_lr) - 1u)) == 0u && g + STEAL_DEPTH >= p.steal_static) {
                    if (pend_group != 0xFFFFFFFFu) {
                        if (lane == 0) s_ring[pend_group & 7u] = make_uint2(pend_group, p.steal_static * gridDim.x + pend_val);
                        pend_group = 0xFFFFFFFFu;
                    }
                    if (v < p.n_virtual) {
                        if (lane == 0) pend_val = atomicAdd(p.steal_ctr, 1u);
                        pend_group = g + STEAL_DEPTH;
                    } else if (lane == 0) {
                        s_ring[(g + STEAL_DEPTH) & 7u] = make_uint2(g + STEAL_DEPTH, 0x0FFFFFFFu);
                    }
                }
                return uniform_u64(v);
            } else {
                return (((uint64_t)(t / waves_per_block) * gridDim.x + blockIdx.x) * waves_per_block + t % waves_per_block) * U;
            }
        };
        // ... and publishes it once the answer is there: called where the wave has just waited for its row loads, which the atomic
        // was issued in front of
        auto publish = [&]() {
            if constexpr (STEAL) {
                if (pend_group != 0xFFFFFFFFu) {
                    if (lane == 0) s_ring[pend_group & 7u] = make_uint2(pend_group, p.steal_static * gridDim.x + pend_val);
                    pend_group = 0xFFFFFFFFu;
                }
            }
        };
        f32x4 cn[U];
        uint32_t rown[U];
        uint64_t v0 = chunk_v0((uint32_t)wave);
        uint64_t v0n = 0;
        if (v0 < p.n_virtual) {
            issue_rows(v0, cn, rown);
            v0n = chunk_v0(claim());
        }
        while (v0 < p.n_virtual) {
            f32x4 c[U];
            uint32_t row[U];
#pragma unroll
            for (int j = 0; j < U; ++j) { c[j] = cn[j]; row[j] = rown[j]; }
            publish();
            if (v0n < p.n_virtual) issue_rows(v0n, cn, rown);
            const uint64_t v0nn = chunk_v0(claim());
            if constexpr (CHUNK4) {
#define SMT_VALID_UNF(j) ((v0 + (j)) < p.n_virtual)
                SMT_REDUCE_CHUNK4(c, row, SMT_VALID_UNF);
#undef SMT_VALID_UNF
            } else {
#pragma unroll
                for (int j = 0; j < U; ++j) SMT_REDUCE_ROW(c[j], row[j], (v0 + j) < p.n_virtual);
            }
            v0 = v0n;
            v0n = v0nn;
        }
    } else {
        // range-filtered: one more stage in front -- [claim chunk c+2, request its descriptor (scalar load)] ->
        // [request the rows of c+1] -> [reduce c]
        f32x4 cn[U];
        uint32_t rown[U];
        uint64_t cA = chunk_id((uint32_t)wave), cB = n_chunks, cC = n_chunks;
        uint64_t dA = fetch_desc(cA), dB = 0;
        if (cA < n_chunks) {
            issue_loads(dA, cn, rown);
            cB = chunk_id(claim());
            dB = fetch_desc(cB);
            cC = chunk_id(claim());
        }
        while (cA < n_chunks) {
            f32x4 c[U];
            uint32_t row[U];
#pragma unroll
            for (int j = 0; j < U; ++j) { c[j] = cn[j]; row[j] = rown[j]; }
            if (cB < n_chunks) issue_loads(dB, cn, rown);
            const uint64_t dC = fetch_desc(cC);
            const uint64_t cD = chunk_id(claim());
            const uint64_t end = (dA & 0xFFFFFFFFull) + (dA >> 32);  // first row past this chunk
            if constexpr (CHUNK4) {
#define SMT_VALID_FIL(j) ((dA & 0xFFFFFFFFull) + (j) < end)
                SMT_REDUCE_CHUNK4(c, row, SMT_VALID_FIL);
#undef SMT_VALID_FIL
            } else {
#pragma unroll
                for (int j = 0; j < U; ++j) SMT_REDUCE_ROW(c[j], row[j], (dA & 0xFFFFFFFFull) + j < end);
            }
            cA = cB; dA = dB;
            cB = cC; dB = dC;
            cC = cD;
        }
    }
#undef SMT_REDUCE_ROW
#undef SMT_REDUCE_CHUNK4
#undef SMT_LIST_INSERT

    if (p.stamps && lane == 0) p.stamps[wave_global * 2 + 1] = wall_clock64();

    // async select: this launch fills the list buffer that the select of step-2 read, and the aux stream must
    // not fall behind: wait for the select of step-1 (it started when this scan did and takes ~14 us -- by the
    // time a block gets here the flag is long up, the wait normally reads it once)
    if (p.flags && threadIdx.x == 0 && p.step >= 2) flag_wait(p.flags, 1, p.step - 1);

    // block merge: rank every wave's candidates among all of the block's.  ONE barrier for all the queries of the pass, and no global
    // store in front of it: every query has its own LDS region (the loop's chunk counter and ring are dead by now), and every slot of
    // a block list is written exactly once -- its key, or the padding from the first slot no key ranks into.  (Until round 6 each
    // query took two barriers with the padding stored between them; a __syncthreads() waits for the wave's outstanding global
    // stores, so every query -- the one-query headline launch included -- paid a store round trip or two in its tail: a one-row
    // search cost 4.4 / 9.4 / 15 / 18.5 us of scan kernel with 1 / 2 / 3 / 4 queries.)
    __syncthreads();
    if constexpr (!STEAL) {
        if (p.gate && threadIdx.x == 0) (void)__hip_atomic_fetch_add(p.gate, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    unsigned int *s_valid = reinterpret_cast<unsigned int *>(s_keys + (size_t)NQ * waves_per_block * 64);   // [NQ][waves] valid keys per wave list
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
        if ((uint32_t)n >= p.nq_active) break;   // (uniform over the block)
        const key_t64 *keys_n = s_keys + (size_t)n * waves_per_block * 64;
        key_t64 *out = p.block_lists + ((size_t)n * gridDim.x + blockIdx.x) * kp;
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
    if (p.flags) {
        // publish: the block's list stores are ordered before its barrier (workgroup scope); ONE thread then
        // does the agent-scope release (one L2 write-back per block -- a __threadfence() in every thread cost
        // 50 us per launch), and the LAST block raises scan_done
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned long long prev = __hip_atomic_fetch_add(p.flags + 2, 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            if (prev == (unsigned long long)gridDim.x - 1) {
                flag_store(p.flags + 2, 0ull);
                __hip_atomic_store(p.flags + 0, p.step, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (p.stamps && threadIdx.x == 0) p.stamps[(uint64_t)gridDim.x * waves_per_block * 2 + blockIdx.x] = wall_clock64();
}

// ------------------------------------------------------------- K2, grouped (tuning key scan_pair)
// Queued one-query scans of the scan_overlap pipeline share a corpus pass.  Every call still launches its scan and its select at
// once; the scan of step i decides ON THE DEVICE, when it starts, how many of the steps i + 2, i + 4, i + 6 -- the next calls on its
// own stream -- it takes along: then it runs the row loop over up to four queries and writes up to four list sets, its own and the
// others', and the scans of the steps it took find themselves ABSORBED and exit before their gate and before any row load.  The
// selects run where they always did, each on its own list set with its own query, outputs and status word: the scan only
// nominates, so no answer changes.
//   host -> device: a ring of PairSlot in pinned host memory, indexed by step; the host fills slot i before it launches scan i and
//     writes the step number last (release); the reader checks the number before and after the fields (a slot reused PAIR_RING
//     steps later fails that check).
//   block -> block: one PairRecord per step in device memory, state = step << 3 | code.  One block wins a CAS on it, decides, and
//     publishes the record -- the group size and the (query, lists) of the calls taken -- with one agent-scope release; the others
//     wait for it with a bounded wait (PairParams::ctl[0] is raised when one runs out, and drain_async turns that into an error
//     code).
//   leader -> absorbed: the deciding block MARKS the records of the steps it takes (state = that step << 3 | PAIR_ABSORBED) before
//     it publishes its own, and a launch learns its fate from its OWN record, the one it reads anyway: marked, it exits; anything
//     else, it leads.  The marks are complete by stream order: leader and absorbed launch are on one stream.  (The other way round,
//     an absorbed step looking for its leader, needs the records of steps i - 2, i - 4 and i - 6.)  Record reuse: the record of
//     step s is that of s - PAIR_RECS, a launch of the same stream that finished long ago, and is touched by the leader of s and
//     by s alone; a mark for a step whose slot check failed is never written, so a cut descriptor ring (scan_pair_ring = 64, the
//     host more than 64 calls ahead) only ends groups early.
// The group is a PREFIX: a refused step i + 2 ends it, so the calls of a group are consecutive on their stream.
// WHEN a launch looks is decided by the host: only a launch that queues up behind a predecessor on its internal stream
// (hipStreamQuery at the call) runs this kernel at all -- a call made while the GPU keeps up, a launch bracketed by profiling events
// and the one after it run scan_topk_kernel as before, so their latency and the profiled kernel time are the plain kernel's.  The
// deciding block reads the slots before it waits at its gate, the others learn the decision after they have requested their first
// rows (the same rows either way): no row load starts later than in scan_topk_kernel.  (Looking only when the block had to wait
// at its gate was measured too: 78.7 instead of 78.2 us per step, and under counter collection, which serialises kernels, nothing
// pairs at all -- profiles/scan_pairing.json.)
constexpr int PAIR_RING = 4096;   // slots: the host may run this many calls ahead of the GPU and still be found (256 KiB, pinned; tuning key scan_pair_ring uses fewer)
constexpr int PAIR_RECS = 64;     // records: record i is written by the leader of step i (a mark) and by step i, and read by step i
constexpr int GROUP_MAX = 4;      // calls one corpus pass serves: the leader's and up to three taken along
struct PairSlot {   // 64 bytes of pinned host memory
    unsigned long long step;        // written last
    unsigned long long corpus, n_virtual, query, lists;
    unsigned long long kp_blocks;   // kp | grid size << 32
    unsigned long long absorbable;
    unsigned long long pad;
};
struct PairRecord {   // 64 bytes
    unsigned long long state;       // step << 3 | PAIR_DECIDING / PAIR_ALONE / PAIR_PAIRED / PAIR_ABSORBED (any other step: undecided)
    unsigned long long taken;       // PAIR_PAIRED: calls taken along (1 .. GROUP_MAX - 1) ...
    unsigned long long query[GROUP_MAX - 1], lists[GROUP_MAX - 1];   // ... and theirs
};
struct PairParams {
    const PairSlot *ring;
    PairRecord *recs;
    unsigned long long *ctl;        // [0] a bounded wait ran out; launches that [1] took calls along, [2] ran alone, [3] were absorbed, [4..6] served 2, 3, 4 calls
    unsigned int absorbable;        // this launch's own slot says so: only then can a leader have marked its record
    unsigned int max_take;          // tuning key scan_pair: calls a launch may take along (1 .. GROUP_MAX - 1)
    unsigned long long wait_ticks;  // tuning key scan_pair_wait_us, in 10 ns ticks
    unsigned long long ring_mask;   // slots in use - 1 (tuning key scan_pair_ring)
};
enum : unsigned long long { PAIR_DECIDING = 1, PAIR_ALONE = 2, PAIR_PAIRED = 3, PAIR_ABSORBED = 4 };
constexpr int PAIR_SHIFT = 3;

__device__ __forceinline__ unsigned long long sys_load(const unsigned long long *f)
{
    return __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The deciding block: the slots of step + 2, + 4, + 6 -> how many of them this launch takes along (their queries and list sets
// go into the record), the longest prefix that passes.  scan_pair_wait_us bounds the waits for all of them together.
// (FAMILY: which group-capable kernel the leader runs, in spare bits of PairSlot::kp_blocks -- a leader takes launches of its own
// kernel only, their records are of its kind; RECS: the records of that kind)
template <unsigned long long FAMILY, int RECS, class PP, class REC>
__device__ __forceinline__ unsigned int group_decide(const ScanParams &p, const PP &pp, REC *rec)
{
    const unsigned long long t0 = wall_clock64();
    unsigned int taken = 0;
    while (taken < pp.max_take) {
        const unsigned long long want = p.step + 2ull * (taken + 1);
        const PairSlot *s = pp.ring + (want & pp.ring_mask);
        unsigned long long s1 = __hip_atomic_load(&s->step, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
        if (s1 < want && pp.wait_ticks) {   // (tests: corpora that scan faster than the host issues calls; a LATER step's number: the slot was reused)
            while (s1 < want && wall_clock64() - t0 < pp.wait_ticks) {
                __builtin_amdgcn_s_sleep(32);
                s1 = __hip_atomic_load(&s->step, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        if (s1 != want) break;
        const unsigned long long corpus = sys_load(&s->corpus), n_virtual = sys_load(&s->n_virtual), kp_blocks = sys_load(&s->kp_blocks);
        const unsigned long long absorbable = sys_load(&s->absorbable);
        const unsigned long long query = sys_load(&s->query), lists = sys_load(&s->lists);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        if (sys_load(&s->step) != want) break;   // the host was rewriting the slot (a ring's length ahead)
        const bool same = corpus == (unsigned long long)(uintptr_t)p.corpus && n_virtual == p.n_virtual &&
                          kp_blocks == ((unsigned long long)p.kp | FAMILY | (unsigned long long)gridDim.x << 32);
        if (!(absorbable && same)) break;
        flag_store(&rec->query[taken], query);
        flag_store(&rec->lists[taken], lists);
        flag_store(&pp.recs[want % RECS].state, (want << PAIR_SHIFT) | PAIR_ABSORBED);   // the mark
        ++taken;
    }
    flag_store(&rec->taken, (unsigned long long)taken);
    return taken;
}
__device__ __forceinline__ unsigned int pair_decide(const ScanParams &p, const PairParams &pp, PairRecord *rec)
{
    return group_decide<0ull, PAIR_RECS>(p, pp, rec);
}

// (8 waves per SIMD = 64 VGPRs: what the select needs beside it, 2 x 64 + 4 x 96 = 512.  The four-query row loop with its queries
// in registers takes 81; with all four read from one LDS image per block and the norms held as wave-uniform values it fits.)
template <bool NT>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8))) scan_pair_kernel(ScanParams p, PairParams pp)
{
    constexpr int U = 4;
    constexpr int NQ = GROUP_MAX;
    extern __shared__ unsigned char smem_raw[];
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
        // two independent reads, one round trip (scan_topk_kernel reads its gate here)
        const unsigned long long g = p.gate_open ? flag_load(p.gate) : 0ull;
        unsigned long long cur = flag_load(&rec->state);
        unsigned long long code = 0;
        if (pp.absorbable && cur == (tag | PAIR_ABSORBED)) {
            code = PAIR_ABSORBED;   // (marked by the leader, an earlier launch of this stream)
        } else {
            // the first block to get here looks for calls to take along while the others wait at the gate
            if ((cur >> PAIR_SHIFT) != p.step &&
                __hip_atomic_compare_exchange_strong(&rec->state, &cur, tag | PAIR_DECIDING, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT)) {
                const unsigned int taken = pair_decide(p, pp, rec);
                cur = tag | (taken ? PAIR_PAIRED : PAIR_ALONE);
                __hip_atomic_store(&rec->state, cur, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                (void)__hip_atomic_fetch_add(pp.ctl + (taken ? 1 : 2), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (taken) (void)__hip_atomic_fetch_add(pp.ctl + 3 + taken, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (g < p.gate_open) gate_wait(p);
        }
        s_pair[0] = code;
        s_pair[2] = cur;
    }
    __syncthreads();
    if (uniform_u64(s_pair[0]) == PAIR_ABSORBED) {
        if (blockIdx.x == 0 && wave == 0 && lane == 0)
            (void)__hip_atomic_fetch_add(pp.ctl + 3, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }

    auto chunk_v0 = [&](uint32_t t) -> uint64_t { return deal_chunk(t, waves_per_block) * U; };   // (chunk_deal.h)
    auto claim = [&]() -> uint32_t { return deal_claim(s_next, lane); };
    // (row numbers are far below 2^63: the sign of the difference is a scalar compare, where "<" on 64 bits takes the VALU and a
    // vector register pair for n_virtual -- this kernel has none to spare)
    // (... and the sign is asked of the high word behind an empty asm: the compiler folds "high word < 0" back into a 64-bit signed
    // compare, for which the scalar unit has no instruction -- a v_cmp_lt_i64 of two scalar values, three times per chunk)
    auto in_corpus = [&](uint64_t v) -> bool {
        uint32_t hi = (uint32_t)((v - p.n_virtual) >> 32);
        asm("" : "+s"(hi));
        return (int32_t)hi < 0;
    };
    // A chunk's rows are 1024 B apart and the load's immediate offset reaches 3072: a full chunk is ONE wave-uniform base address
    // in scalar registers, the lane's 16 B offset and four immediates -- no vector instruction.  Only the chunk that crosses
    // n_virtual clamps its rows one by one.  (The base passes through an empty asm: otherwise the compiler regroups the sum as
    // (corpus + 16 lane) + row offset, hoists the bracket into a vector register pair and adds the rest on the VALU, per row.  The
    // ragged chunk's rows pass through one too: loads of the same kind on both sides of a branch are joined behind it, and the
    // joined load is back at one address per row.)
    // (the global address space by name: a pointer made from an integer is a generic one, and its loads flat_load)
    typedef const f32x4 __attribute__((address_space(1))) *global_rows_ptr;
    auto row_ptr = [&](uint64_t v) -> global_rows_ptr {
        uint64_t base = (uint64_t)(uintptr_t)p.corpus + v * 1024u;
        asm volatile("" : "+s"(base));
        return (global_rows_ptr)(uintptr_t)base + lane;
    };
    auto issue_rows = [&](uint64_t v0, f32x4 (&c)[U]) {
        if (in_corpus(v0 + (U - 1))) {   // (uniform)
            const global_rows_ptr src = row_ptr(v0);
#pragma unroll
            for (int j = 0; j < U; ++j) c[j] = NT ? __builtin_nontemporal_load(src + 64 * j) : src[64 * j];
        } else {
#pragma unroll
            for (int j = 0; j < U; ++j) {
                uint64_t v = v0 + j;
                if (!in_corpus(v)) v = p.n_virtual - 1;  // clamp (result discarded)
                const global_rows_ptr src = row_ptr((uint64_t)(uint32_t)v);
                c[j] = NT ? __builtin_nontemporal_load(src) : *src;
                asm volatile("" : "+v"(c[j]));
            }
        }
    };
    // the first rows are on their way before the decision is known: they are the same rows either way
    f32x4 cn[U];
    uint64_t v0 = chunk_v0((uint32_t)wave);
    uint64_t v0n = 0;
    if (in_corpus(v0)) {
        issue_rows(v0, cn);
        v0n = chunk_v0(claim());
    }

    if (threadIdx.x == 0) {
        unsigned long long cur = s_pair[2];   // (this step's: the block has won the CAS and decided, or lost it)
        if (cur == (tag | PAIR_DECIDING)) {   // bounded like flag_wait: a decision that never comes ends in an error code
            const unsigned long long t0 = wall_clock64();
            while ((cur = flag_load(&rec->state)) == (tag | PAIR_DECIDING)) {
                __builtin_amdgcn_s_sleep(8);
                if (flag_load(pp.ctl) != 0ull) break;
                if (wall_clock64() - t0 > 200000000ull) { flag_store(pp.ctl, 1ull); break; }
            }
        }
        unsigned long long served = 1;
        if (cur == (tag | PAIR_PAIRED)) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            unsigned long long taken = flag_load(&rec->taken);
            if (taken > (unsigned long long)(NQ - 1)) taken = NQ - 1;   // (never: the record is this step's)
            for (unsigned long long j = 0; j < taken; ++j) {
                s_qptr[j] = flag_load(&rec->query[j]);
                s_pair[3 + j] = flag_load(&rec->lists[j]);
            }
            served = 1 + taken;
        } else if (cur != (tag | PAIR_ALONE)) {
            flag_store(pp.ctl, 1ull);   // (a wait that ran out, or a record that is not this step's: alone, and the context reports it)
        }
        s_pair[1] = served;
    }
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
    // (The per-lane expression spelled out as the compiler contracts "x qx + y qy + z qz + w qw" in the one-query loop -- y qy, then
    // fused adds of x, z, w -- so that no vectoriser's regrouping can move a rounding; SMT_OPAQUE keeps a tree's value a scalar: left
    // to itself the SLP vectoriser pairs the trees into v_pk_add_f32, which cannot carry a DPP operand.)
#define SMT_ROW_DOT(cj, qv) __builtin_fmaf((cj).w, (qv).w, __builtin_fmaf((cj).z, (qv).z, __builtin_fmaf((cj).x, (qv).x, (cj).y * (qv).y)))
#define SMT_OPAQUE(v) asm volatile("" : "+v"(v))
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
    // The software pipeline of scan_topk_kernel -- the next chunk's rows are requested once the current chunk's have arrived and fly
    // during its reduction -- without the register copy: the loop is unrolled by two and the two row buffers swap names.  The empty
    // wait on `cur` stands where the copy stood: it keeps the request timing (ONE chunk in flight per wave; two, the ping-pong,
    // measured slower), and the claims come in the same order, so every wave takes the chunks it took.
#define SMT_GROUP_STEP(cur, nxt)                                                                                  \
    do {                                                                                                          \
        asm volatile("s_waitcnt vmcnt(0)" : "+v"((cur)[0]), "+v"((cur)[1]), "+v"((cur)[2]), "+v"((cur)[3]) : : "memory"); \
        if (in_corpus(v0n)) issue_rows(v0n, nxt);                                                                 \
        const uint64_t v0nn = chunk_v0(claim());                                                                  \
        /* (the chunk's real rows, asked the scalar way) */                                                       \
        SMT_REDUCE_GROUP4(cur, (uint32_t)v0, in_corpus(v0 + (U - 1)) ? 4u : (uint32_t)(p.n_virtual - v0));        \
        v0 = v0n;                                                                                                 \
        v0n = v0nn;                                                                                               \
    } while (0)
    f32x4 cm[U];
    while (in_corpus(v0)) {
        SMT_GROUP_STEP(cn, cm);
        if (!in_corpus(v0)) break;
        SMT_GROUP_STEP(cm, cn);
    }
#undef SMT_GROUP_STEP
#undef SMT_REDUCE_GROUP4
#undef SMT_GROUP_INSERT
#undef SMT_OPAQUE
#undef SMT_ROW_DOT
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
// dynamic LDS of a scan_pair_kernel launch: the four key regions, the waves' key counts, the query images, the block's control words
static inline size_t pair_smem_bytes(int threads)
{
    return (size_t)GROUP_MAX * (threads / 64) * 64 * sizeof(key_t64) + 256 + (size_t)GROUP_MAX * 1024 + 9 * 8 + 16;
}

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
constexpr int WIDE_MAX = 8;       // calls one corpus pass of scan_wide_kernel serves: the leader's and up to seven taken along
constexpr int WIDE_RECS = 64;     // records (reuse distance 64 > 14, as PAIR_RECS)
constexpr unsigned long long WIDE_FAMILY = 1ull << 16;   // PairSlot::kp_blocks of a scan_wide_kernel launch (kp <= 64 below it, the grid above)
struct WideRecord {   // 128 bytes
    unsigned long long state;       // as PairRecord
    unsigned long long taken;       // PAIR_PAIRED: calls taken along (1 .. WIDE_MAX - 1) ...
    unsigned long long query[WIDE_MAX - 1], lists[WIDE_MAX - 1];   // ... and theirs
};
struct WideParams {
    const PairSlot *ring;
    WideRecord *recs;
    unsigned long long *ctl;        // PairParams::ctl, and behind it [7..10] launches that served 5, 6, 7, 8 calls
    unsigned int absorbable;
    unsigned int max_take;          // tuning key scan_take: calls a launch may take along (1 .. WIDE_MAX - 1)
    unsigned long long wait_ticks;
    unsigned long long ring_mask;
};

template <bool NT>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(8, 8))) scan_wide_kernel(ScanParams p, WideParams pp)
{
    constexpr int U = 4;
    constexpr int NQ = WIDE_MAX;
    extern __shared__ unsigned char smem_raw[];
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
    if (wave == 0) {
#pragma unroll
        for (int i = 0; i < NQ * SHARED_LIST_KEYS / 64; ++i) s_list[64 * i + lane] = KEY_PAD;
        if (lane < NQ) {
            f32x4 r;   // a query that is not there: zero, nothing under its threshold
            r.x = 0.0f;
            r.y = 1.0f;
            r.z = __builtin_inff();               // (SHARED_LIST_OPEN)
            r.w = __uint_as_float(0xFFFFFFFFu);
            s_rec[lane] = r;
            s_lock[lane] = 0u;
        }
    }
#define SMT_QUERY_NORM(n, qn)                                                                                     \
    do {                                                                                                          \
        s_q[(n) * 64 + lane] = (qn);                                                                              \
        const float a2 = wave_sum((qn).x * (qn).x + (qn).y * (qn).y + (qn).z * (qn).z + (qn).w * (qn).w);         \
        const bool qz = readlane_f(a2, 0) == 0.0f;                                                                \
        const float rq = qz ? 0.0f : readlane_f(__frsqrt_rn(a2), 0);                                              \
        if (lane == 0) { s_rec[n].x = rq; s_rec[n].y = qz ? 1.0f : 0.0f; }                                        \
    } while (0)
    if (wave == 0) {
        const f32x4 q0 = reinterpret_cast<const f32x4 *>(p.queries)[lane];
        SMT_QUERY_NORM(0, q0);
    }

    if (threadIdx.x == 0) {
        *s_next = (uint32_t)waves_per_block;
        const unsigned long long g = p.gate_open ? flag_load(p.gate) : 0ull;
        unsigned long long cur = flag_load(&rec->state);
        unsigned long long code = 0;
        if (pp.absorbable && cur == (tag | PAIR_ABSORBED)) {
            code = PAIR_ABSORBED;   // (marked by the leader, an earlier launch of this stream)
        } else {
            if ((cur >> PAIR_SHIFT) != p.step &&
                __hip_atomic_compare_exchange_strong(&rec->state, &cur, tag | PAIR_DECIDING, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT)) {
                const unsigned int taken = group_decide<WIDE_FAMILY, WIDE_RECS>(p, pp, rec);
                cur = tag | (taken ? PAIR_PAIRED : PAIR_ALONE);
                __hip_atomic_store(&rec->state, cur, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                (void)__hip_atomic_fetch_add(pp.ctl + (taken ? 1 : 2), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (taken) (void)__hip_atomic_fetch_add(pp.ctl + 3 + taken, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (g < p.gate_open) gate_wait(p);
        }
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

    // (the chunk deal, the scalar row test and the scalar row addresses: see scan_pair_kernel)
    auto chunk_v0 = [&](uint32_t t) -> uint64_t { return deal_chunk(t, waves_per_block) * U; };
    auto claim = [&]() -> uint32_t { return deal_claim(s_next, lane); };
    auto in_corpus = [&](uint64_t v) -> bool {
        uint32_t hi = (uint32_t)((v - p.n_virtual) >> 32);
        asm("" : "+s"(hi));
        return (int32_t)hi < 0;
    };
    typedef const f32x4 __attribute__((address_space(1))) *global_rows_ptr;
    auto row_ptr = [&](uint64_t v) -> global_rows_ptr {
        uint64_t base = (uint64_t)(uintptr_t)p.corpus + v * 1024u;
        asm volatile("" : "+s"(base));
        return (global_rows_ptr)(uintptr_t)base + lane;
    };
    auto issue_rows = [&](uint64_t v0, f32x4 (&c)[U]) {
        if (in_corpus(v0 + (U - 1))) {   // (uniform)
            const global_rows_ptr src = row_ptr(v0);
#pragma unroll
            for (int j = 0; j < U; ++j) c[j] = NT ? __builtin_nontemporal_load(src + 64 * j) : src[64 * j];
        } else {
#pragma unroll
            for (int j = 0; j < U; ++j) {
                uint64_t v = v0 + j;
                if (!in_corpus(v)) v = p.n_virtual - 1;  // clamp (result discarded)
                const global_rows_ptr src = row_ptr((uint64_t)(uint32_t)v);
                c[j] = NT ? __builtin_nontemporal_load(src) : *src;
                asm volatile("" : "+v"(c[j]));
            }
        }
    };
    // the first rows are on their way before the decision is known: they are the same rows either way
    f32x4 cn[U];
    uint64_t v0 = chunk_v0((uint32_t)wave);
    uint64_t v0n = 0;
    if (in_corpus(v0)) {
        issue_rows(v0, cn);
        v0n = chunk_v0(claim());
    }

    if (threadIdx.x == 0) {
        unsigned long long cur = s_ctl[2];   // (this step's: the block has won the CAS and decided, or lost it)
        if (cur == (tag | PAIR_DECIDING)) {   // bounded like flag_wait: a decision that never comes ends in an error code
            const unsigned long long t0 = wall_clock64();
            while ((cur = flag_load(&rec->state)) == (tag | PAIR_DECIDING)) {
                __builtin_amdgcn_s_sleep(8);
                if (flag_load(pp.ctl) != 0ull) break;
                if (wall_clock64() - t0 > 200000000ull) { flag_store(pp.ctl, 1ull); break; }
            }
        }
        unsigned long long served = 1;
        if (cur == (tag | PAIR_PAIRED)) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            unsigned long long taken = flag_load(&rec->taken);
            if (taken > (unsigned long long)(NQ - 1)) taken = NQ - 1;   // (never: the record is this step's)
            for (unsigned long long j = 0; j < taken; ++j) {
                s_qptr[j] = flag_load(&rec->query[j]);
                s_ctl[4 + j] = flag_load(&rec->lists[j]);
            }
            served = 1 + taken;
        } else if (cur != (tag | PAIR_ALONE)) {
            flag_store(pp.ctl, 1ull);   // (a wait that ran out, or a record that is not this step's: alone, and the context reports it)
        }
        s_ctl[1] = served;
    }
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
                if (n < 4 || n_on > 4) SMT_QUERY_NORM(n, qn[n - 1]);
        }
        __syncthreads();   // the images and the records are wave 0's stores
    }
#undef SMT_QUERY_NORM

#define SMT_ROW_DOT(cj, qv) __builtin_fmaf((cj).w, (qv).w, __builtin_fmaf((cj).z, (qv).z, __builtin_fmaf((cj).x, (qv).x, (cj).y * (qv).y)))
#define SMT_OPAQUE(v) asm volatile("" : "+v"(v))
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
    // (the two-buffer pipeline of scan_pair_kernel: one chunk in flight per wave, the claims in the same order)
#define SMT_WIDE_STEP(cur, nxt)                                                                                   \
    do {                                                                                                          \
        asm volatile("s_waitcnt vmcnt(0)" : "+v"((cur)[0]), "+v"((cur)[1]), "+v"((cur)[2]), "+v"((cur)[3]) : : "memory"); \
        if (in_corpus(v0n)) issue_rows(v0n, nxt);                                                                 \
        const uint64_t v0nn = chunk_v0(claim());                                                                  \
        SMT_REDUCE_WIDE(cur, (uint32_t)v0, in_corpus(v0 + (U - 1)) ? 4u : (uint32_t)(p.n_virtual - v0));          \
        v0 = v0n;                                                                                                 \
        v0n = v0nn;                                                                                               \
    } while (0)
    f32x4 cm[U];
    while (in_corpus(v0)) {
        SMT_WIDE_STEP(cn, cm);
        if (!in_corpus(v0)) break;
        SMT_WIDE_STEP(cm, cn);
    }
#undef SMT_WIDE_STEP
#undef SMT_REDUCE_WIDE
#undef SMT_WIDE_TEST_INSERT
#undef SMT_WIDE_RECORD
#undef SMT_OPAQUE
#undef SMT_ROW_DOT
    __syncthreads();
    if (wave == 0 && lane == 0) (void)__hip_atomic_fetch_add(p.gate, (unsigned long long)n_on, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the block's lists are its answer, sorted and padded: wave w writes those of queries w, w + waves, ...
    for (int n = wave; n < n_on; n += waves_per_block) {
        key_t64 *out = reinterpret_cast<key_t64 *>((uintptr_t)uniform_u64(s_ctl[3 + n])) + (size_t)blockIdx.x * kp;
        if (lane < kp) out[lane] = s_list[n * SHARED_LIST_KEYS + lane];
    }
}
// dynamic LDS of a scan_wide_kernel launch: the eight lists (32 keys each, whatever the block's size), the queries' records, the
// lock words, the query images, the block's control words
static inline size_t wide_smem_bytes(int threads)
{
    return (size_t)WIDE_MAX * 32 * sizeof(key_t64) + (size_t)WIDE_MAX * 16 + 64 + (size_t)WIDE_MAX * 1024 + 18 * 8 + 16;
}

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
constexpr int DEEP_MAX = 16;      // calls one corpus pass of scan_deep_kernel serves: the leader's and up to fifteen taken along
constexpr int DEEP_RECS = 64;     // records (reuse distance 64 > 30, as PAIR_RECS)
constexpr unsigned long long DEEP_FAMILY = 1ull << 17;   // PairSlot::kp_blocks of a scan_deep_kernel launch (next to WIDE_FAMILY)
struct DeepRecord {   // 256 bytes
    unsigned long long state;       // as PairRecord
    unsigned long long taken;       // PAIR_PAIRED: calls taken along (1 .. DEEP_MAX - 1) ...
    unsigned long long query[DEEP_MAX - 1], lists[DEEP_MAX - 1];   // ... and theirs
};
static_assert(sizeof(DeepRecord) == 256, "DeepRecord: state, taken and fifteen (query, lists) pairs");
// select_group (select.hip group_select_kernel): ONE select launch behind the leader serves every call of its pass, so the leader
// also needs each member's output buffers, status word and row base.  They travel as (query, lists) do: the host writes them into a
// second pinned ring beside the PairSlot ring (same index, same length, between the two stores of PairSlot::step, so the step checks
// around the fields cover them; PairSlot keeps its 64 bytes and the two older kernels never see the ring), the deciding wave copies
// them AT THE DECISION into a device record beside DeepRecord (same index, same reuse distance), and the select reads that copy --
// never the pinned slot, which the host may have lapped by then (scan_pair_ring = 64).  A launch that is followed by a group select
// says so in its slot (DEEP_SELGROUP, and its k_out above it: k' alone does not fix k_out when the guard band changes between
// calls), so a leader takes only calls whose select it will run, and calls that will run none of their own.
constexpr unsigned long long DEEP_SELGROUP = 1ull << 18;   // PairSlot::kp_blocks: the launch is followed by group_select_kernel ...
constexpr int DEEP_KOUT_SHIFT = 24;                        // ... and k_out (<= 56) in bits 24 .. 29
struct SelSlot {   // 32 bytes of pinned host memory, slot i beside PairSlot i
    unsigned long long out_rows, out_dist, out_status, row_base;
};
struct DeepSelRecord {   // 512 bytes
    SelSlot member[DEEP_MAX];   // [0 .. DEEP_MAX - 2]: the calls taken along, as DeepRecord::query
};
static_assert(DEEP_MAX == GROUP_SEL_MAX && offsetof(DeepRecord, state) == 8 * GROUP_REC_STATE && offsetof(DeepRecord, taken) == 8 * GROUP_REC_TAKEN &&
                  offsetof(DeepRecord, query) == 8 * GROUP_REC_QUERY && offsetof(DeepRecord, lists) == 8 * GROUP_REC_LISTS && sizeof(SelSlot) == 32,
              "group_select_kernel reads these records as 8-byte words (common.h GroupSelect)");
struct DeepParams {
    const PairSlot *ring;
    const SelSlot *sel_ring;        // select_group: the ring beside `ring`, or nullptr ...
    DeepSelRecord *sel_recs;        // ... and the records beside `recs`
    unsigned long long family;      // what a slot's kp_blocks holds beside k' and the grid: DEEP_FAMILY, and with select_group DEEP_SELGROUP | k_out << DEEP_KOUT_SHIFT
    DeepRecord *recs;
    unsigned long long *ctl;        // PairParams::ctl; [11..26] launches of this kernel that served 1 .. 16 calls
    unsigned int absorbable;
    unsigned int max_take;          // tuning key scan_deep: calls a launch may take along (1 .. DEEP_MAX - 1)
    unsigned long long wait_ticks;
    unsigned long long ring_mask;
};
constexpr int DEEP_CTL_BY_SIZE = 11;

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
    extern __shared__ unsigned char smem_raw[];
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
    if (wave == 0) {
#pragma unroll
        for (int i = 0; i < NQ * SHARED_LIST_KEYS / 64; ++i) s_list[64 * i + lane] = KEY_PAD;
        if (lane < NQ) {
            f32x4 r;   // a query that is not there: zero, nothing under its threshold
            r.x = 0.0f;
            r.y = 1.0f;
            r.z = __builtin_inff();               // (SHARED_LIST_OPEN)
            r.w = __uint_as_float(0xFFFFFFFFu);
            s_rec[lane] = r;
            s_lock[lane] = 0u;
        }
    }
#define SMT_QUERY_NORM(n, qn)                                                                                     \
    do {   /* (lane l keeps its 16 bytes of query n in the slot it reads them from: slot s of phase h holds query 4 h + (s ^ i')) */ \
        s_q[wave_sum4_folded_slot(n, lane) * 64 + lane] = (qn);                                                   \
        const float a2 = wave_sum((qn).x * (qn).x + (qn).y * (qn).y + (qn).z * (qn).z + (qn).w * (qn).w);         \
        const bool qz = readlane_f(a2, 0) == 0.0f;                                                                \
        const float rq = qz ? 0.0f : readlane_f(__frsqrt_rn(a2), 0);                                              \
        if (lane == 0) { s_rec[n].x = rq; s_rec[n].y = qz ? 1.0f : 0.0f; }                                        \
    } while (0)
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

    // (the chunk deal, the scalar row test and the scalar row addresses: see scan_pair_kernel)
    auto chunk_v0 = [&](uint32_t t) -> uint64_t { return deal_chunk(t, waves_per_block) * U; };
    auto claim = [&]() -> uint32_t { return deal_claim(s_next, lane); };
    auto in_corpus = [&](uint64_t v) -> bool {
        uint32_t hi = (uint32_t)((v - p.n_virtual) >> 32);
        asm("" : "+s"(hi));
        return (int32_t)hi < 0;
    };
    typedef const f32x4 __attribute__((address_space(1))) *global_rows_ptr;
    auto row_ptr = [&](uint64_t v) -> global_rows_ptr {
        uint64_t base = (uint64_t)(uintptr_t)p.corpus + v * 1024u;
        asm volatile("" : "+s"(base));
        return (global_rows_ptr)(uintptr_t)base + lane;
    };
    auto issue_rows = [&](uint64_t v0, f32x4 (&c)[U]) {
        if (in_corpus(v0 + (U - 1))) {   // (uniform)
            const global_rows_ptr src = row_ptr(v0);
#pragma unroll
            for (int j = 0; j < U; ++j) c[j] = NT ? __builtin_nontemporal_load(src + 64 * j) : src[64 * j];
        } else {
#pragma unroll
            for (int j = 0; j < U; ++j) {
                uint64_t v = v0 + j;
                if (!in_corpus(v)) v = p.n_virtual - 1;  // clamp (result discarded)
                const global_rows_ptr src = row_ptr((uint64_t)(uint32_t)v);
                c[j] = NT ? __builtin_nontemporal_load(src) : *src;
                asm volatile("" : "+v"(c[j]));
            }
        }
    };
    // the first rows are on their way before the decision is known: they are the same rows either way
    f32x4 cn[U];
    uint64_t v0 = chunk_v0((uint32_t)wave);
    uint64_t v0n = 0;
    if (in_corpus(v0)) {
        issue_rows(v0, cn);
        v0n = chunk_v0(claim());
    }

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

#define SMT_ROW_DOT(cj, qv) __builtin_fmaf((cj).w, (qv).w, __builtin_fmaf((cj).z, (qv).z, __builtin_fmaf((cj).x, (qv).x, (cj).y * (qv).y)))
#define SMT_OPAQUE(v) asm volatile("" : "+v"(v))
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
    // (the two-buffer pipeline of scan_pair_kernel: one chunk in flight per wave, the claims in the same order)
    // THE ROWS ARE PERMUTED BY LANE once a chunk has landed (device_utils.h swizzle_rows4_folded: register k of lane l holds row
    // k ^ m(l), m the folded map's row), in place on the buffer that is reduced, and the seventeen trees' heads run without selects
    // (wave_sum4_swizzled_head): what a lane keeps and sends in a head depends on the lane alone, so the choice is made once on
    // the sixteen row registers and not seventeen times on the products.  Every product is the same chain on the same operands
    // in another register, every addition has the operands of wave_sum4's, possibly exchanged.
#define SMT_DEEP_STEP(cur, nxt)                                                                                   \
    do {                                                                                                          \
        asm volatile("s_waitcnt vmcnt(0)" : "+v"((cur)[0]), "+v"((cur)[1]), "+v"((cur)[2]), "+v"((cur)[3]) : : "memory"); \
        if (in_corpus(v0n)) issue_rows(v0n, nxt);                                                                 \
        const uint64_t v0nn = chunk_v0(claim());                                                                  \
        swizzle_rows4_folded((cur)[0], (cur)[1], (cur)[2], (cur)[3], lane);                                       \
        SMT_REDUCE_DEEP(cur, (uint32_t)v0, in_corpus(v0 + (U - 1)) ? 4u : (uint32_t)(p.n_virtual - v0));          \
        /* (the permuted rows end here: without this they count as live into the next turn and are copied about) */ \
        asm volatile("" : "=v"((cur)[0]), "=v"((cur)[1]), "=v"((cur)[2]), "=v"((cur)[3]));                        \
        v0 = v0n;                                                                                                 \
        v0n = v0nn;                                                                                               \
    } while (0)
    f32x4 cm[U];
    while (in_corpus(v0)) {
        SMT_DEEP_STEP(cn, cm);
        if (!in_corpus(v0)) break;
        SMT_DEEP_STEP(cm, cn);
    }
#undef SMT_DEEP_STEP
#undef SMT_REDUCE_DEEP
#undef SMT_DEEP_ON
#undef SMT_DEEP_PHASE
#undef SMT_DEEP_TEST_INSERT
#undef SMT_DEEP_RECORD
#undef SMT_OPAQUE
#undef SMT_ROW_DOT
    __syncthreads();
    if (wave == 0 && lane == 0) (void)__hip_atomic_fetch_add(p.gate, (unsigned long long)n_on, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the block's lists are its answer, sorted and padded: wave w writes those of queries w, w + waves, ...
    for (int n = wave; n < n_on; n += waves_per_block) {
        key_t64 *out = reinterpret_cast<key_t64 *>((uintptr_t)uniform_u64(s_ctl[3 + n])) + (size_t)blockIdx.x * kp;
        if (lane < kp) out[lane] = s_list[n * SHARED_LIST_KEYS + lane];
    }
}
// dynamic LDS of a scan_deep_kernel launch: the sixteen lists (32 keys each, whatever the block's size), the queries' records, the
// lock words, the query images, the block's control words (3 + 16 list sets + 15 query addresses) and the chunk counter
static inline size_t deep_smem_bytes(int threads)
{
    return (size_t)DEEP_MAX * 32 * sizeof(key_t64) + (size_t)DEEP_MAX * 16 + 64 + (size_t)DEEP_MAX * 1024 + 34 * 8 + 16;
}

// ------------------------------------------------------------------ launchers
static inline uint32_t candidates_per_list(const smt_ctx *ctx, uint32_t k_out)
{
    // guard band: 8 extra f32 candidates so that f32-vs-f64 rank flips at the k-th boundary do not drop a true
    // top-k row; the select stage PROVES per query that the band was wide enough (SelectArgs::f32_err) and flags
    // the query otherwise.  k_out <= SCAN_MAX_K = 56, so the band never shrinks below 8; tuning key guard_band widens
    // it (lists hold at most 64 keys) for corpora with many near-duplicate lines -- every proof that succeeds saves
    // the exhaustive re-answer, at the price of a longer select (256 lists x k' keys).
    return std::min<uint32_t>(64, k_out + (uint32_t)ctx->tune.guard_band);
}

// host_timing (tuning key, off by default; tools/ab_select_group.py): clock_gettime around the runtime calls of a pipeline call,
// summed per kind in smt_ctx::host_ns
struct HostTimer {
    smt_ctx *ctx;
    bool on;
    timespec t;
    explicit HostTimer(smt_ctx *c) : ctx(c), on(c->tune.host_timing != 0)
    {
        if (on) clock_gettime(CLOCK_MONOTONIC, &t);
    }
    void lap(int kind)
    {
        if (!on) return;
        timespec n;
        clock_gettime(CLOCK_MONOTONIC, &n);
        ctx->host_ns[kind] += (uint64_t)((n.tv_sec - t.tv_sec) * 1000000000ll + (n.tv_nsec - t.tv_nsec));
        t = n;
    }
};

// What the launches of one call have in common: plan_scan decides before anything is enqueued, the next two steps fill in the rest.
struct ScanPlan {
    bool filtered, nt;
    int blocks, threads, U;   // grid, block, rows per chunk
    uint32_t kp;              // candidates kept per list
    uint64_t n_chunks;
    bool async, overlap;      // the pipeline: async select (one query per call), and of those the two-stream overlap
    bool pair;                // scan_pair: one-query launches may share a corpus pass
    // enter_pipeline
    uint64_t step = 0;        // of the pipeline (0: synchronous)
    key_t64 *lists = nullptr; // this step's list set, and behind the sets the chunk table of a filtered call
    uint64_t *table = nullptr;
    // overlap_prologue
    hipStream_t st = nullptr;
    unsigned long long gate_open = 0, gate_ticks = 0;
    bool may_pair = false;    // scan_pair: this launch runs scan_pair_kernel (it looks for a partner, and may find itself absorbed)
    bool wide = false;        // scan_take: ... or scan_wide_kernel, when the limit exceeds what scan_pair_kernel serves
    bool deep = false;        // scan_deep: ... or scan_deep_kernel, when it exceeds what scan_wide_kernel serves
    unsigned int absorbable = 0;
    bool sel_group = false;   // select_group: the launch is followed by group_select_kernel, not by a select of its own
    SelSlot sel = {0, 0, 0, 0};   // ... and what a leader's launch of it needs of this call
    uint32_t sel_k_out = 0;
};

static ScanPlan plan_scan(const smt_ctx *ctx, const ScanArgs &a)
{
    ScanPlan pl;
    pl.filtered = a.n_ranges > 0;
    pl.nt = ctx->tune.scan_nontemporal != 0;
    pl.kp = candidates_per_list(ctx, a.k_out);
    pl.blocks = ctx->tune.scan_blocks > 0 ? ctx->tune.scan_blocks : ctx->num_cus;
    if (pl.blocks > SEL_MAX_LISTS) pl.blocks = SEL_MAX_LISTS;
    pl.threads = ctx->tune.scan_threads;
    pl.U = pl.filtered ? FILTER_CHUNK : ctx->tune.scan_unroll;
    pl.n_chunks = pl.filtered ? a.n_chunks : (a.n_virtual + (uint64_t)pl.U - 1) / (uint64_t)pl.U;
    const uint64_t waves_per_block = (uint64_t)(pl.threads / 64);
    if ((uint64_t)pl.blocks * waves_per_block > pl.n_chunks) {  // tiny inputs: do not launch idle blocks
        const uint64_t need = (pl.n_chunks + waves_per_block - 1) / waves_per_block;
        pl.blocks = (int)(need > 0 ? need : 1);
    }
    // async select (one query per call): two list buffers alternate, the select of step i reads buffer i&1 on
    // the aux stream while the scan of step i+1 fills the other one
    pl.async = a.allow_async && ctx->tune.async_select && a.nq == 1;
    // scan_overlap: scan AND select of step i on scan stream i&1, behind an event on the main stream (the caller's inputs).  List
    // buffer b belongs to stream b, so stream order protects it and no flag is needed; the two streams let scan i+1 start while
    // scan i drains, paced by the start gate (ScanParams::gate).  (Not with STEAL: its counter ring is reset in stream order.)
    pl.overlap = pl.async && a.allow_overlap && ctx->tune.scan_overlap && !pl.filtered && ctx->tune.scan_steal == 0;
    // scan_pair: the launch may share its corpus pass with the call two steps later, or be absorbed by the one two steps earlier
    // (scan_pair_kernel).  Not with wave stamps (profiling of the plain kernel).
    pl.pair = pl.overlap && ctx->tune.scan_pair && pl.U == 4 && ctx->tune.scan_debug_ptr == 0;
    // more than three calls taken along: scan_wide_kernel, whose shared lists hold 32 keys and whose launch bound is 8 waves
    pl.wide = pl.pair && ctx->tune.scan_pair > GROUP_MAX - 1 && pl.kp <= 32 && pl.threads <= 512;
    // more than seven: scan_deep_kernel, under the same two conditions (a launch is of ONE family: deep, else wide, else the four-call kernel)
    pl.deep = pl.wide && ctx->tune.scan_pair > WIDE_MAX - 1;
    if (pl.deep) pl.wide = false;
    pl.st = ctx->stream;
    return pl;
}

// Leaves the other pipeline if the last call ran it, makes this one's, takes the step number and carves up the scratch buffer.
static int enter_pipeline(smt_ctx *ctx, const ScanArgs &a, ScanPlan &pl)
{
    int rc = SMT_OK;
    if (pl.async && ctx->async_overlap != pl.overlap && (rc = drain_async(ctx))) return rc;   // the two pipelines share the list buffers
    if (pl.async && (rc = pl.overlap ? ensure_overlap(ctx) : ensure_async(ctx))) return rc;
    if (!pl.async && (rc = drain_async(ctx))) return rc;
    pl.step = pl.overlap ? ++ctx->ov_step : pl.async ? ++ctx->async_step : 0;
    // (scan_overlap: scans of consecutive calls run at the same time, and their grids differ with the corpus -- the two buffers get a
    // fixed place, the largest one-query list set, or a small call's buffer 1 would lie inside a large call's buffer 0)
    const size_t list_bytes = pl.overlap ? (size_t)SEL_MAX_LISTS * 64 * sizeof(key_t64)
                                         : (((size_t)a.nq * pl.blocks * pl.kp * sizeof(key_t64)) + 255) & ~(size_t)255;
    const size_t table_bytes = pl.filtered ? (size_t)pl.n_chunks * sizeof(uint64_t) : 0;
    // (scan_overlap: a ring of thirty-two sets, step & 31, 8 MiB, whichever kernel runs.  A leading scan of step i fills the sets of
    // steps i, i + 2, ... at most i + 30, all on its own stream, and set s is shared by the steps s, s +- 32, s +- 64 ...: the last
    // readers of the sixteen sets it may write are the selects of steps i - 32, i - 30, ... i - 2, launched on the SAME stream before
    // scan i, so stream order alone has them finished.  The other stream's steps have the other parity and the other sixteen sets.
    // With fewer sets the scan of step i would write the set of step i + 30 into one that a select of the other stream, ordered
    // against nothing here, may be reading.  A leader with a shorter reach -- scan_wide_kernel's i + 14, scan_pair_kernel's i + 6 --
    // writes a subset of those sets: more sets than its reach needs only move a set's next writer further away.)
    const size_t n_sets = pl.overlap ? 2 * DEEP_MAX : 2;
    if ((rc = ensure_scratch(ctx, n_sets * list_bytes + table_bytes))) return rc;
    pl.lists = reinterpret_cast<key_t64 *>(reinterpret_cast<char *>(ctx->d_scratch) + (pl.step & (n_sets - 1)) * list_bytes);
    pl.table = reinterpret_cast<uint64_t *>(reinterpret_cast<char *>(ctx->d_scratch) + n_sets * list_bytes);
    return pl.pair ? ensure_pair(ctx) : SMT_OK;
}

// scan_overlap: the step's stream goes behind the caller's; timed-launch bracketing, may_pair / absorbable, the start gate.
static int overlap_prologue(smt_ctx *ctx, ScanPlan &pl)
{
    const uint64_t step = pl.step;
    hipStream_t st = pl.st = ctx->ov_stream[step & 1];
    // a predecessor that takes this call's query along reads it without waiting for ov_ready: only a query that no work queued on
    // the caller's stream can still be writing may be taken
    // ... and only a launch that queues up behind a predecessor on its stream can be absorbed by it, or has reason to look for a
    // partner itself (a call made while the GPU is idle must cost what it did: no look, no wait; scan_pair_wait_us: tests)
    // ov_skip_ready: the caller's stream is asked ONCE per call, and when it is empty there is nothing for the internal stream to be
    // ordered behind -- no event is recorded on the caller's stream and no barrier stands in front of the scan.  (Those markers were
    // also what the next call's query found on the caller's stream when the host ran far enough ahead of it.)  The answer serves as
    // `idle` too.  0: an event and a wait for every call, and the caller's stream asked only behind a predecessor, as before.
    const bool skip_ready = ctx->tune.ov_skip_ready != 0;
    HostTimer ht(ctx);
    bool caller_empty = false;
    if (skip_ready) caller_empty = hipStreamQuery(ctx->stream) == hipSuccess;
    if (pl.pair) {
        const bool behind = ctx->tune.scan_pair_wait_us > 0 || hipStreamQuery(st) != hipSuccess;
        const bool idle = behind && (skip_ready ? caller_empty : hipStreamQuery(ctx->stream) == hipSuccess);
        pl.absorbable = idle ? 1u : 0u;
        pl.may_pair = behind;
    }
    (void)hipGetLastError();   // (hipErrorNotReady is an answer here)
    ht.lap(0);
    if (!caller_empty) {
        SMT_HIP_CHECK(hipEventRecord(ctx->ov_ready[step & 1], ctx->stream));
        SMT_HIP_CHECK(hipStreamWaitEvent(st, ctx->ov_ready[step & 1], 0));
        ++ctx->ov_ready_records;
    }
    ht.lap(1);
    // a timed launch waits for its predecessor (and that one's select), and the launch after it waits for it: the events bracket a
    // kernel that has the part to itself, not a gate or an HBM shared with a neighbour
    const bool timed = prof_arms_next(ctx, "scan");
    if (timed || ctx->ov_after_timed) {
        SMT_HIP_CHECK(hipEventRecord(ctx->ov_done, ctx->ov_stream[(step & 1) ^ 1]));
        SMT_HIP_CHECK(hipStreamWaitEvent(st, ctx->ov_done, 0));
        // (a timed launch and its successor neither absorb nor get absorbed: the events keep bracketing a one-query pass)
        pl.may_pair = false;
        pl.absorbable = 0;
    }
    ctx->ov_after_timed = timed;
    // What the gate counts is CALLS served, in blocks: a plain launch's block adds 1 when its rows are done, a leader's block the
    // number of calls its pass serves, an absorbed launch nothing, and gate_total (launch_scan_topk, behind the passes) counts one grid per call.  So "gate_pct of
    // the predecessor" is: every call before the predecessor call is served, and gate_pct per cent of the predecessor call's
    // grid.  When that call is the m-th of n that one pass serves, the point lies at (m - 1 + gate_pct / 100) / n of the pass'
    // blocks: 75 % of a pair's pass and 87.5 % of a full group's at gate_pct = 50, while a leader still at its gate holds
    // successors back only until their bound.  The default by the sweeps: 50 for every mode.  (While the grouped
    // pass ran one tree per query, launches that take two or three calls along ran 4 us per step faster with no gate: two leaders
    // on a CU filled each other's stalls.  With the group reducer every gate from 5 to 100 measures 48.0 us per step and no gate
    // 50.1 with a spread of 3 us, profiles/scan_group_loop.json.)
    const int gate_pct = ctx->tune.scan_gate_pct >= 0 ? ctx->tune.scan_gate_pct : 50;
    if (gate_pct > 0 && ctx->gate_prev_blocks > 0) {
        pl.gate_open = ctx->gate_total - ctx->gate_prev_blocks + (ctx->gate_prev_blocks * (uint64_t)gate_pct + 99) / 100;
        // the bound: the predecessor's rows at 4 TB/s (half the part's HBM rate; 1 KiB rows, 10 ns ticks) + 20 us, at most 0.5 ms (a
        // grid that cannot be resident twice -- scan_blocks / scan_threads -- may hold back predecessor blocks while it waits)
        pl.gate_ticks = std::min<uint64_t>(ctx->gate_prev_rows / 39 + 2000, 50000);
    }
    return SMT_OK;
}

// The parameters of the pass over the queries q0 .. q0 + nq_active - 1 (STEAL: see steal_setup).
static ScanParams scan_params(const smt_ctx *ctx, const ScanArgs &a, const ScanPlan &pl, const uint64_t *chunk_table, uint32_t q0,
                              uint32_t nq_active)
{
    ScanParams p{};
    p.corpus = a.corpus;
    p.queries = a.queries + (size_t)q0 * 256;
    p.n_virtual = a.n_virtual;
    p.chunk_table = pl.filtered ? chunk_table : nullptr;
    p.n_chunks = pl.n_chunks;
    p.kp = pl.kp;
    p.nq_active = nq_active;
    p.block_lists = pl.lists + (size_t)q0 * pl.blocks * pl.kp;
    p.stamps = reinterpret_cast<unsigned long long *>(ctx->tune.scan_debug_ptr);
    p.flags = pl.async && !pl.overlap ? ctx->d_flags : nullptr;
    p.step = pl.step;
    p.gate = pl.overlap ? ctx->d_gate : nullptr;
    p.gate_open = pl.gate_open;
    p.gate_ticks = pl.gate_ticks;
    return p;
}

// Dynamic groups (scan_topk_kernel STEAL; tuning key scan_steal = rounds per group, 0 = the static deal): unfiltered scans of
// 8-wave blocks over enough rows that every block gets well past its static groups.  Each launch has its own counter: a ring
// of 64, zeroed together every 64th launch (one 256-byte memset in stream order).
static int steal_setup(smt_ctx *ctx, const ScanPlan &pl, ScanParams &p)
{
    if (pl.filtered || pl.U != 4 || pl.threads != 512 || ctx->tune.scan_steal <= 0 ||
        pl.n_chunks < (uint64_t)pl.blocks * 8u * (uint64_t)ctx->tune.scan_steal * 8u)
        return SMT_OK;
    if (!ctx->d_steal) SMT_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&ctx->d_steal), 64 * sizeof(unsigned int)));
    if (ctx->steal_seq % 64 == 0) SMT_HIP_CHECK(hipMemsetAsync(ctx->d_steal, 0, 64 * sizeof(unsigned int), ctx->stream));
    p.steal_ctr = ctx->d_steal + (ctx->steal_seq % 64);
    ++ctx->steal_seq;
    uint32_t lr = 0;
    while ((2 << lr) <= ctx->tune.scan_steal) ++lr;
    p.steal_lr = lr;
    // the dynamic share: scan_steal_pct per cent of the groups (at least STEAL_DEPTH + 1 per block stay static)
    const uint64_t n_groups = (pl.n_chunks + (8ull << lr) - 1) / (8ull << lr);
    const uint64_t per_block = n_groups / (uint64_t)pl.blocks;
    const uint64_t n_static = per_block * (uint64_t)(100 - ctx->tune.scan_steal_pct) / 100;
    p.steal_static = (uint32_t)std::max<uint64_t>(n_static, 3);
    return SMT_OK;
}

using scan_kernel_t = void (*)(ScanParams);
template <int NQ, int U>
static scan_kernel_t scan_kernel_of(bool nt, bool filtered, bool steal)
{
    if constexpr (U == FILTER_CHUNK) {   // (the chunk table's chunk, and the STEAL deal's, is four rows)
        if (filtered) return nt ? scan_topk_kernel<NQ, U, true, true> : scan_topk_kernel<NQ, U, false, true>;
        if (steal) return nt ? scan_topk_kernel<NQ, U, true, false, true> : scan_topk_kernel<NQ, U, false, false, true>;
    }
    return nt ? scan_topk_kernel<NQ, U, true, false> : scan_topk_kernel<NQ, U, false, false>;
}

// The instantiation for a pass of `slots` query slots (1, 2, 4) over chunks of U rows (a filtered scan: FILTER_CHUNK).
static scan_kernel_t scan_kernel_for(int slots, int U, bool nt, bool filtered, bool steal)
{
    if (slots > 1 && U == 2) U = 8;   // two and four queries are built for 4 and 8 rows per chunk: scan_unroll = 2 runs them at 8
    if (slots == 1) return U == 2 ? scan_kernel_of<1, 2>(nt, filtered, steal) : U == 4 ? scan_kernel_of<1, 4>(nt, filtered, steal)
                                                                                      : scan_kernel_of<1, 8>(nt, filtered, steal);
    if (slots == 2) return U == 4 ? scan_kernel_of<2, 4>(nt, filtered, steal) : scan_kernel_of<2, 8>(nt, filtered, steal);
    return U == 4 ? scan_kernel_of<4, 4>(nt, filtered, steal) : scan_kernel_of<4, 8>(nt, filtered, steal);
}

int ensure_pair(smt_ctx *ctx)
{
    if (ctx->h_pair_ring) return SMT_OK;
    SMT_HIP_CHECK(hipMalloc(&ctx->d_pair_recs, PAIR_RECS * sizeof(PairRecord)));
    SMT_HIP_CHECK(hipMemset(ctx->d_pair_recs, 0, PAIR_RECS * sizeof(PairRecord)));
    SMT_HIP_CHECK(hipMalloc(&ctx->d_wide_recs, WIDE_RECS * sizeof(WideRecord)));
    SMT_HIP_CHECK(hipMemset(ctx->d_wide_recs, 0, WIDE_RECS * sizeof(WideRecord)));
    SMT_HIP_CHECK(hipMalloc(&ctx->d_deep_recs, DEEP_RECS * sizeof(DeepRecord)));
    SMT_HIP_CHECK(hipMemset(ctx->d_deep_recs, 0, DEEP_RECS * sizeof(DeepRecord)));
    SMT_HIP_CHECK(hipMalloc(&ctx->d_deep_sel_recs, DEEP_RECS * sizeof(DeepSelRecord)));
    SMT_HIP_CHECK(hipMemset(ctx->d_deep_sel_recs, 0, DEEP_RECS * sizeof(DeepSelRecord)));
    SMT_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&ctx->d_sel_groups), (GROUP_SEL_MAX + 1) * sizeof(unsigned long long)));
    SMT_HIP_CHECK(hipMemset(ctx->d_sel_groups, 0, (GROUP_SEL_MAX + 1) * sizeof(unsigned long long)));
    SMT_HIP_CHECK(hipHostMalloc(&ctx->h_sel_ring, PAIR_RING * sizeof(SelSlot), hipHostMallocDefault));
    memset(ctx->h_sel_ring, 0, PAIR_RING * sizeof(SelSlot));
    SMT_HIP_CHECK(hipHostMalloc(&ctx->h_pair_ring, PAIR_RING * sizeof(PairSlot), hipHostMallocDefault));
    memset(ctx->h_pair_ring, 0, PAIR_RING * sizeof(PairSlot));
    return SMT_OK;
}

// Publishes this step's slot (what a predecessor needs to take the call along), then launches the group-capable one-query scan:
// scan_pair_kernel, scan_wide_kernel (pl.wide) or scan_deep_kernel (pl.deep).
template <class PP>
static void group_params(const smt_ctx *ctx, const ScanPlan &pl, PP &pp, int max_take)
{
    pp.absorbable = pl.absorbable;
    pp.ring_mask = (unsigned long long)std::min(ctx->tune.scan_pair_ring, PAIR_RING) - 1;
    pp.ring = reinterpret_cast<const PairSlot *>(ctx->h_pair_ring);
    pp.ctl = ctx->d_gate + 1;
    pp.wait_ticks = (unsigned long long)ctx->tune.scan_pair_wait_us * 100ull;
    pp.max_take = (unsigned int)std::min(std::max(ctx->tune.scan_pair, 1), max_take);
}
static int launch_scan_pair(smt_ctx *ctx, const ScanParams &p, const ScanPlan &pl)
{
    PairParams pp{};
    WideParams wp{};
    DeepParams dp{};
    group_params(ctx, pl, pp, GROUP_MAX - 1);
    group_params(ctx, pl, wp, WIDE_MAX - 1);
    group_params(ctx, pl, dp, DEEP_MAX - 1);
    PairSlot *slot = reinterpret_cast<PairSlot *>(ctx->h_pair_ring) + (p.step & pp.ring_mask);
    __atomic_store_n(&slot->step, 0ull, __ATOMIC_SEQ_CST);   // (a reader of the slot's previous use fails its second check)
    slot->corpus = (unsigned long long)(uintptr_t)p.corpus;
    slot->n_virtual = p.n_virtual;
    slot->query = (unsigned long long)(uintptr_t)p.queries;
    slot->lists = (unsigned long long)(uintptr_t)p.block_lists;
    dp.family = DEEP_FAMILY;
    if (pl.sel_group) {
        dp.family |= DEEP_SELGROUP | (unsigned long long)pl.sel_k_out << DEEP_KOUT_SHIFT;
        dp.sel_ring = reinterpret_cast<const SelSlot *>(ctx->h_sel_ring);
        dp.sel_recs = reinterpret_cast<DeepSelRecord *>(ctx->d_deep_sel_recs);
        reinterpret_cast<SelSlot *>(ctx->h_sel_ring)[p.step & pp.ring_mask] = pl.sel;   // (between the two stores of slot->step)
    }
    slot->kp_blocks = (unsigned long long)p.kp | (pl.wide ? WIDE_FAMILY : pl.deep ? dp.family : 0ull) | (unsigned long long)pl.blocks << 32;
    slot->absorbable = pp.absorbable;
    __atomic_store_n(&slot->step, p.step, __ATOMIC_RELEASE);
    pp.recs = reinterpret_cast<PairRecord *>(ctx->d_pair_recs);
    wp.recs = reinterpret_cast<WideRecord *>(ctx->d_wide_recs);
    dp.recs = reinterpret_cast<DeepRecord *>(ctx->d_deep_recs);
    if (pl.deep)
        hipLaunchKernelGGL(pl.nt ? scan_deep_kernel<true> : scan_deep_kernel<false>, dim3(pl.blocks), dim3(pl.threads),
                           deep_smem_bytes(pl.threads), pl.st, p, dp);
    else if (pl.wide)
        hipLaunchKernelGGL(pl.nt ? scan_wide_kernel<true> : scan_wide_kernel<false>, dim3(pl.blocks), dim3(pl.threads),
                           wide_smem_bytes(pl.threads), pl.st, p, wp);
    else
        hipLaunchKernelGGL(pl.nt ? scan_pair_kernel<true> : scan_pair_kernel<false>, dim3(pl.blocks), dim3(pl.threads),
                           pair_smem_bytes(pl.threads), pl.st, p, pp);
    SMT_HIP_CHECK(hipGetLastError());
    ctx->pair_live = true;
    return SMT_OK;
}

// One pass: `slots` query slots, of which p.nq_active hold a query.  THE launch site of scan_topk_kernel.
static int launch_scan_pass(smt_ctx *ctx, const ScanPlan &pl, const ScanParams &p, int slots)
{
    if (slots == 1 && pl.pair) {
        if (pl.may_pair) return launch_scan_pair(ctx, p, pl);
        ++ctx->pair_alone_host;
    }
    // per-query, per-wave key slots (the chunk counter and the STEAL ring live in the second query's until the merge) + the waves' key counts
    const size_t smem = (size_t)slots * (pl.threads / 64) * 64 * sizeof(key_t64) + 16 + 64 + 256;
    // (STEAL: groups of rounds dealt while the kernel runs -- 512-thread blocks, four rows per chunk: steal_setup)
    hipLaunchKernelGGL(scan_kernel_for(slots, pl.U, pl.nt, pl.filtered, p.steal_ctr != nullptr), dim3(pl.blocks), dim3(pl.threads), smem,
                       pl.st, p);
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

static SelectArgs select_args(const ScanArgs &a, const ScanPlan &pl)
{
    SelectArgs s;
    s.corpus = a.corpus;
    s.queries = a.queries;
    s.nq = a.nq;
    s.lists = pl.lists;
    s.n_lists = (uint32_t)pl.blocks;
    s.kp = pl.kp;
    s.list_stride = (uint64_t)pl.blocks * pl.kp;
    s.k_out = a.k_out;
    s.ws_threshold = a.ws_threshold;
    s.ws_thr_score = a.ws_thr_score;
    s.row_base = a.row_base;
    s.out_rows = a.out_rows;
    s.out_dist = a.out_dist;
    s.out_counts = a.out_counts;
    s.async_step = pl.overlap ? 0 : pl.step;
    s.stream = pl.st;
    s.out_stride = a.out_stride;
    s.f32_err = F32_ERR_SCAN;
    s.out_uncertain = a.out_uncertain;
    s.out_status = a.out_status;
    s.deliver = a.deliver;
    return s;
}

int launch_scan_topk(smt_ctx *ctx, const ScanArgs &a)
{
    SMT_REQUIRE(a.k_out >= 1 && a.k_out <= SCAN_MAX_K, "top_k for the scan path must be in [1, 56]");
    SMT_REQUIRE(a.rows < 0xFFFFFFFFull, "a shard holds fewer than 2^32-1 rows");
    ScanPlan pl = plan_scan(ctx, a);
    int rc = enter_pipeline(ctx, a, pl);
    if (rc != SMT_OK) return rc;
    HostTimer whole(ctx);
    if (pl.overlap && (rc = overlap_prologue(ctx, pl))) return rc;
    // select_group: a launch of scan_deep_kernel whose select is a plain one (rows, distances, status) is followed by ONE launch of
    // group_select_kernel for the calls its pass serves.  A call whose select carries more than the record holds keeps its own
    // select and is taken along by nobody.
    const SelectArgs sa = select_args(a, pl);
    if (pl.deep && pl.may_pair && ctx->tune.select_group) {
        pl.sel_group = group_select_serves(sa);
        if (pl.sel_group) {
            pl.sel = SelSlot{(unsigned long long)(uintptr_t)sa.out_rows, (unsigned long long)(uintptr_t)sa.out_dist,
                             (unsigned long long)(uintptr_t)sa.out_status, (unsigned long long)sa.row_base};
            pl.sel_k_out = sa.k_out;
        } else {
            pl.absorbable = 0;
        }
    }
    HostTimer ht(ctx);

    prof_begin_on(ctx, "scan", pl.st);
    const uint64_t *chunk_table = pl.table;
    if (pl.filtered && (rc = range_chunk_table(ctx, a, pl.table, &chunk_table))) return rc;
    for (uint32_t q0 = 0; q0 < a.nq;) {
        // (three queries ride in the four-query kernel: with the four rows of a chunk reduced together a pass costs 1.06 x / 1.4 x one
        // query's for two / four queries -- 172 / 230 us at 1 M rows -- against 335 us for a pass of two and a pass of one)
        const uint32_t left = a.nq - q0;
        const int slots = left >= 3 ? 4 : (int)left;
        ScanParams p = scan_params(ctx, a, pl, chunk_table, q0, std::min(left, 4u));
        if ((rc = steal_setup(ctx, pl, p)) || (rc = launch_scan_pass(ctx, pl, p, slots))) return rc;
        q0 += p.nq_active;
    }
    prof_end_on(ctx, "scan", pl.st);

    if (pl.overlap) {
        ctx->gate_total += (uint64_t)pl.blocks;
        ctx->gate_prev_blocks = (uint64_t)pl.blocks;
        ctx->gate_prev_rows = a.n_virtual;
        ctx->async_pending = true;
        ctx->async_overlap = true;
    } else if (pl.async) {
        ctx->async_overlap = false;
    }
    ht.lap(2);
    if (pl.sel_group) {
        GroupSelect gs;
        gs.rec = reinterpret_cast<const unsigned long long *>(reinterpret_cast<const DeepRecord *>(ctx->d_deep_recs) + pl.step % DEEP_RECS);
        gs.sel = reinterpret_cast<const unsigned long long *>(reinterpret_cast<const DeepSelRecord *>(ctx->d_deep_sel_recs) + pl.step % DEEP_RECS);
        gs.absorbed = (pl.step << PAIR_SHIFT) | PAIR_ABSORBED;
        gs.paired = (pl.step << PAIR_SHIFT) | PAIR_PAIRED;
        gs.hist = ctx->d_sel_groups;
        rc = launch_group_select(ctx, sa, gs);
    } else {
        rc = launch_select(ctx, sa);
    }
    ht.lap(3);
    // the aux stream's contract (smt_ctx_aux_stream): work a host chains there runs behind this call's select.  (select_group: the
    // select launch of an absorbed call does nothing, but it follows the leader's, which holds the call's answer, on this stream.)
    if (rc == SMT_OK && pl.overlap && ctx->aux_stream) {
        SMT_HIP_CHECK(hipEventRecord(ctx->ov_sel[pl.step & 1], pl.st));
        SMT_HIP_CHECK(hipStreamWaitEvent(ctx->aux_stream, ctx->ov_sel[pl.step & 1], 0));
    }
    ht.lap(4);
    if (pl.overlap) {
        whole.lap(5);
        if (whole.on) ++ctx->host_ns_calls;
    }
    return rc;
}

}  // namespace smt
