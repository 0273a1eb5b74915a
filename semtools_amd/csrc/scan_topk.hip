// scan_topk.hip -- K2: scan_topk_kernel, the plain scan of one pass (1, 2 or 4 query slots; unfiltered, range-filtered, STEAL), its
// instantiations and the launch of one pass.  (What K2 is and how its units divide: scan_params.h.)
#include "scan_params.h"

namespace smt {

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
    // (No alignment attribute on smem_raw here, in the grouped kernels and in select.hip: while they shared a unit with the merge kernels,
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

// THE launch site of scan_topk_kernel.
void launch_scan_topk_kernel(int slots, int U, bool nt, bool filtered, int blocks, int threads, hipStream_t st, const ScanParams &p)
{
    // per-query, per-wave key slots (the chunk counter and the STEAL ring live in the second query's until the merge) + the waves' key counts
    const size_t smem = (size_t)slots * (threads / 64) * 64 * sizeof(key_t64) + 16 + 64 + 256;
    // (STEAL: groups of rounds dealt while the kernel runs -- 512-thread blocks, four rows per chunk: steal_setup)
    hipLaunchKernelGGL(scan_kernel_for(slots, U, nt, filtered, p.steal_ctr != nullptr), dim3(blocks), dim3(threads), smem, st, p);
}

}  // namespace smt
