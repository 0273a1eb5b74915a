// scan_slab.hip -- K2 for WIDE rows: scan_slab_kernel<S, NQ, FILTERED>, rows of D = 256 S floats (S = 2, 3, 4 slabs of 1 KiB)
// against 1 or up to 4 queries, and the launch of a call's passes (scan + finish_slab.hip).  D = 256 never comes here; D = 64
// comes to the launch only (its kernel: scan_narrow.hip).
//
// LAYOUT.  A wave owns a row.  Lane l holds float4 number l of EVERY slab -- row[s * 64 + l], s = 0 .. S - 1 -- so each of the
// S load instructions of a row still reads 1 KiB contiguous, as the 256 kernel's one load does.  The queries sit in registers in
// the same layout (S float4 per query and lane).  A lane multiplies its 4 S components of the row with the query's as ONE chain of
// 4 S fused multiply-adds: the S slabs' partial products are added in registers, before any lane talks to another, and a (row, dot)
// pair goes through ONE reduction tree, not one per slab.
//
// ROWS IN FLIGHT.  scan_topk.hip found that more than about 32 KiB of requests in flight per CU costs bandwidth; its U = 4 rows of
// 1 KiB per wave (plus the prefetched four) are kept here as bytes: U = 2 rows at S = 2 (2 x 2 KiB + the prefetched 4 KiB per wave,
// what the 256 kernel has), U = 1 at S = 4 (4 + 4 KiB).  S = 3 gets U = 1: 3 + 3 KiB per wave, 48 KiB per CU with 8 waves -- U = 2
// would be 96 KiB, three times the figure the 256 kernel settled on.  SUPPOSED, not measured: that the 32 KiB rule carries over
// unchanged when the same bytes come as fewer, longer rows; tools/wide_rows_rate.py records the byte rates this choice reaches.
//
// THE TREE.  wave_sum4 (device_utils.h) reduces FOUR values over the wave for 15 instructions where wave_sum takes 11 for one, and
// leaves value j in the lanes with lane % 4 == j.  With fewer than four rows per step its four slots are filled with the step's
// (row, dot) pairs instead of four rows:
//   one query,   U = 2:  (<c0, q>, <c1, q>, <c0, c0>, <c1, c1>) -- one tree for both rows; slot j < 2 gets its |c_j|^2 from slot
//                        j + 2 with one quad permute
//   one query,   U = 1:  (<c, q>, <c, c>, <c, q>, <c, c>)       -- one tree; slot 0 gets |c|^2 from slot 1
//   four queries, per row: (<c, q0>, <c, q1>, <c, q2>, <c, q3>) in one tree, slot n = query n, and |c|^2 by wave_sum (every lane
//                        needs it)
// so the transposing tree still pays: 15 (+ 1) instructions where two to five wave_sum trees would take 22 to 55.  SUPPOSED from
// the instruction counts; the 256 kernel measured the same trade (2 x 15 against 8 x 11) at 155.6 -> 152.8 us.
// Either tree has six levels; f32_err_slab (wide_rows.h) counts them as the 256 bound does.
//
// Lists, block merge, padding and order are the 256 kernel's ideas, written again (lane_list.h, shared with scan_half.hip, whose
// kernel this file's launch_search_slab also launches, as it does scan_byte.hip's and scan_nibble.hip's): a lane-distributed sorted list per
// query, k' = min(64, top_k + guard band); every block merges its waves' lists by counting ranks into ONE block list of key_t64 per
// query, strictly ascending by (distance, row), padded with KEY_PAD.  Range-filtered scans walk the chunk table of
// range_tables.hip (first row | valid rows << 32, FILTER_CHUNK rows per entry), U rows of an entry per step.
#include "nibble_rows.h"
#include "lane_list.h"

namespace smt {

template <int S>
__device__ __forceinline__ float slab_dot(const f32x4 (&a)[S], const f32x4 (&b)[S])
{
    float acc = a[0].x * b[0].x;
    acc = fmaf(a[0].y, b[0].y, acc);
    acc = fmaf(a[0].z, b[0].z, acc);
    acc = fmaf(a[0].w, b[0].w, acc);
#pragma unroll
    for (int s = 1; s < S; ++s) {
        acc = fmaf(a[s].x, b[s].x, acc);
        acc = fmaf(a[s].y, b[s].y, acc);
        acc = fmaf(a[s].z, b[s].z, acc);
        acc = fmaf(a[s].w, b[s].w, acc);
    }
    return acc;
}

template <int S, int NQ, bool FILTERED>
__global__ void __launch_bounds__(512) scan_slab_kernel(SlabScanParams p)
{
    static_assert(S >= 2 && S <= 4 && (NQ == 1 || NQ == 4), "2..4 slabs, 1 or 4 query slots");
    constexpr int U = S == 2 ? 2 : 1;          // rows of a step (header: rows in flight)
    constexpr int D = 256 * S;
    constexpr int SUB = FILTER_CHUNK / U;      // steps per chunk-table entry
    extern __shared__ __align__(16) unsigned char slab_smem[];
    key_t64 *s_keys = reinterpret_cast<key_t64 *>(slab_smem);   // [NQ][waves][64]

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves_per_block = blockDim.x >> 6;
    const int kp = (int)p.kp;
    const int slot = lane & 3;

    f32x4 q[NQ][S];
    float rq[NQ];
    bool qz[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        const f32x4 *qp = reinterpret_cast<const f32x4 *>(p.queries + (size_t)((uint32_t)n < p.nq_active ? n : 0) * D);
#pragma unroll
        for (int s = 0; s < S; ++s) q[n][s] = qp[s * 64 + lane];
        const float a2 = wave_sum(slab_dot<S>(q[n], q[n]));
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

    // Steps are dealt to the waves of the launch round robin (step k to wave k mod all waves: neighbouring waves read neighbouring
    // rows).  Unfiltered: step k = rows [k U, k U + U).  Filtered: step k = rows [sub U, sub U + U) of table entry k / SUB.
    const uint64_t wave_global = (uint64_t)blockIdx.x * waves_per_block + wave;
    const uint64_t n_waves = (uint64_t)gridDim.x * waves_per_block;
    const uint64_t n_steps = FILTERED ? p.n_chunks * SUB : (p.n_rows + U - 1) / U;
    const const_u64_ptr const_table = (const_u64_ptr)(uintptr_t)p.chunk_table;   // written by an earlier kernel: scalar loads
    // the rows of step k (clamped to a real row where the step has fewer than U) and how many of them count
    auto locate = [&](uint64_t k, uint32_t (&row)[U], uint32_t &n_valid) {
        if constexpr (FILTERED) {
            const uint64_t desc = const_table[uniform_u64(k / SUB)];
            const uint32_t first = (uint32_t)desc, cnt = (uint32_t)(desc >> 32), at = (uint32_t)(k % SUB) * U;
            n_valid = cnt > at ? min(cnt - at, (uint32_t)U) : 0u;
#pragma unroll
            for (int j = 0; j < U; ++j) row[j] = first + (at + j < cnt ? at + j : 0u);
        } else {
            const uint64_t v0 = k * U;
            n_valid = (uint32_t)min(p.n_rows - v0, (uint64_t)U);
#pragma unroll
            for (int j = 0; j < U; ++j) row[j] = (uint32_t)(v0 + j < p.n_rows ? v0 + j : p.n_rows - 1);
        }
    };
    auto issue = [&](const uint32_t (&row)[U], f32x4 (&c)[U][S]) {
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const f32x4 *src = reinterpret_cast<const f32x4 *>(p.corpus + (uint64_t)row[j] * D) + lane;
#pragma unroll
            for (int s = 0; s < S; ++s) c[j][s] = __builtin_nontemporal_load(src + s * 64);
        }
    };

    // software pipeline: the rows of the wave's next step are requested before the current step is reduced
    f32x4 cn[U][S];
    uint32_t rown[U], nvn = 0;
    uint64_t k = wave_global;
    if (k < n_steps) {
        locate(k, rown, nvn);
        issue(rown, cn);
    }
    while (k < n_steps) {
        f32x4 c[U][S];
        uint32_t row[U];
        const uint32_t nv = nvn;
#pragma unroll
        for (int j = 0; j < U; ++j) {
            row[j] = rown[j];
#pragma unroll
            for (int s = 0; s < S; ++s) c[j][s] = cn[j][s];
        }
        const uint64_t kn = k + n_waves;
        if (kn < n_steps) {
            locate(kn, rown, nvn);
            issue(rown, cn);
        }
        if constexpr (NQ == 1) {
            // one tree for the step: slots (ab_0, ab_1, b2_0, b2_1) resp. (ab, b2, ab, b2) -- header
            float t, b2;
            if constexpr (U == 2) {
                t = wave_sum4(slab_dot<S>(c[0], q[0]), slab_dot<S>(c[1], q[0]), slab_dot<S>(c[0], c[0]), slab_dot<S>(c[1], c[1]), lane);
                b2 = dpp_f<DPP_XOR2>(t);
            } else {
                const float pa = slab_dot<S>(c[0], q[0]), pb = slab_dot<S>(c[0], c[0]);
                t = wave_sum4(pa, pb, pa, pb, lane);
                b2 = dpp_f<DPP_XOR1>(t);
            }
            const float d4 = dist_f32(t, b2, rq[0], qz[0]);   // lanes with slot < U: row `slot` of the step
            const uint32_t r_mine = row[slot < U ? slot : 0];
            const bool cand = (uint32_t)slot < nv && slab_under(d4, r_mine, thr_d[0], thr_r[0]);
            uint32_t pending = (uint32_t)__ballot(cand) & ((1u << U) - 1u);
            while (pending) {
                const int j = __builtin_ctz(pending);
                pending &= pending - 1;
                const float d = readlane_f(d4, j);
                const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)r_mine, j);
                if (slab_under(d, r, thr_d[0], thr_r[0])) slab_list_insert(ld[0], lr[0], thr_d[0], thr_r[0], d, r, lane, kp);
            }
        } else {
            const float rq_m = slot == 0 ? rq[0] : slot == 1 ? rq[1] : slot == 2 ? rq[2] : rq[3];
            const bool qz_m = slot == 0 ? qz[0] : slot == 1 ? qz[1] : slot == 2 ? qz[2] : qz[3];
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const float b2 = wave_sum(slab_dot<S>(c[j], c[j]));
                const float t = wave_sum4(slab_dot<S>(c[j], q[0]), slab_dot<S>(c[j], q[1]), slab_dot<S>(c[j], q[2]), slab_dot<S>(c[j], q[3]), lane);
                const float d4 = dist_f32(t, b2, rq_m, qz_m);   // slot n: this row against query n
                const float td = slot == 0 ? thr_d[0] : slot == 1 ? thr_d[1] : slot == 2 ? thr_d[2] : thr_d[3];
                const uint32_t tr = slot == 0 ? thr_r[0] : slot == 1 ? thr_r[1] : slot == 2 ? thr_r[2] : thr_r[3];
                const uint32_t r = row[j];
                const bool cand = (uint32_t)j < nv && (uint32_t)slot < p.nq_active && slab_under(d4, r, td, tr);
                const uint32_t pending = (uint32_t)__ballot(cand) & 0xFu;
#pragma unroll
                for (int n = 0; n < NQ; ++n) {
                    if (pending & (1u << n)) {   // (wave-uniform)
                        const float d = readlane_f(d4, n);
                        slab_list_insert(ld[n], lr[n], thr_d[n], thr_r[n], d, r, lane, kp);
                    }
                }
            }
        }
        k = kn;
    }

    slab_block_merge<NQ>(s_keys, ld, lr, p.nq_active, kp, p.block_lists, lane, wave, waves_per_block);
}

template <int S>
static slab_scan_kernel_t slab_scan_kernel_of(int slots, bool filtered)
{
    if (slots == 1) return filtered ? scan_slab_kernel<S, 1, true> : scan_slab_kernel<S, 1, false>;
    return filtered ? scan_slab_kernel<S, 4, true> : scan_slab_kernel<S, 4, false>;
}

constexpr int SLAB_THREADS = 512;   // 8 waves per block, as the 256 scan

// The passes of one call: up to four queries share a corpus pass (one query: the one-slot kernel), each pass followed by its finish.
int launch_search_slab(smt_ctx *ctx, const SlabSearch &a)
{
    const bool half = a.row_dtype == SMT_ROWS_F16;   // 512-byte rows of 256 halves: scan_half.hip, eight rows a step
    const bool byte = a.row_dtype == SMT_ROWS_I8;    // 256-byte rows of 256 int8: scan_byte.hip, sixteen rows a step
    const bool nibble = a.row_dtype == SMT_ROWS_I4;  // 128-byte rows of 256 int4: scan_nibble.hip, thirty-two rows a step
    const bool narrow = dim_is_narrow(a.dim);        // 256-byte rows of 64 floats: scan_narrow.hip, sixteen rows a step
    SMT_REQUIRE(half || byte || nibble ? a.dim == SMT_DIM : dim_in_family(a.dim), "wide scan: 64, 512, 768 or 1024 dimensions, or half, byte or nibble rows of 256");
    SMT_REQUIRE(a.k_out >= 1 && a.k_out <= SCAN_MAX_K, "wide scan: 1 <= top_k <= 56");
    SMT_REQUIRE(a.rows < 0xFFFFFFFFull, "wide scan: fewer than 2^32 - 1 rows per corpus");
    SMT_REQUIRE(a.nq >= 1 && a.queries && a.out_rows && a.out_dist, "wide scan: null argument");
    if ((a.chunk_table ? a.n_chunks : a.rows) > 0) {
        if (slab_batch_serves(ctx, a)) return launch_batch_slab(ctx, a);   // batch_slab.hip
        if (half_batch_serves(ctx, a)) return launch_batch_half(ctx, a);   // batch_half.hip
        if (byte_batch_serves(ctx, a)) return launch_batch_byte(ctx, a);   // batch_byte.hip
        if (nibble_batch_serves(ctx, a)) return launch_batch_nibble(ctx, a);   // batch_nibble.hip
    }
    const int S = (int)(a.dim / 256);
    const int U = nibble ? NIBBLE_STEP_ROWS : byte ? BYTE_STEP_ROWS : half ? HALF_STEP_ROWS : narrow ? NARROW_STEP_ROWS : S == 2 ? 2 : 1;
    const bool filtered = a.chunk_table != nullptr;
    const uint64_t n_steps = !filtered ? (a.rows + U - 1) / U
                             : nibble  ? (a.n_chunks + NIBBLE_STEP_ROWS / FILTER_CHUNK - 1) / (NIBBLE_STEP_ROWS / FILTER_CHUNK)
                             : byte    ? (a.n_chunks + BYTE_STEP_ROWS / FILTER_CHUNK - 1) / (BYTE_STEP_ROWS / FILTER_CHUNK)
                             : half    ? (a.n_chunks + HALF_STEP_ROWS / FILTER_CHUNK - 1) / (HALF_STEP_ROWS / FILTER_CHUNK)
                             : narrow  ? (a.n_chunks + NARROW_STEP_ROWS / FILTER_CHUNK - 1) / (NARROW_STEP_ROWS / FILTER_CHUNK)
                                       : a.n_chunks * (uint64_t)(FILTER_CHUNK / U);
    const uint32_t kp = std::min<uint32_t>(64, a.k_out + (uint32_t)ctx->tune.guard_band);
    const int waves = SLAB_THREADS / 64;
    const int cus = ctx->tune.scan_blocks > 0 ? ctx->tune.scan_blocks : std::max(ctx->num_cus, 1);
    const int blocks = (int)std::max<uint64_t>(1, std::min<uint64_t>(std::min(cus, SLAB_MAX_LISTS), (n_steps + waves - 1) / waves));
    if (n_steps == 0) return launch_finish_slab(ctx, a, nullptr, 0, kp, 0, a.nq);   // nothing to scan: padding, proved
    const size_t lists_bytes = (size_t)4 * blocks * kp * sizeof(key_t64);
    int rc = ensure_scratch(ctx, lists_bytes);
    if (rc) return rc;
    key_t64 *lists = reinterpret_cast<key_t64 *>(ctx->d_scratch);
    for (uint32_t q0 = 0; q0 < a.nq; q0 += 4) {
        const uint32_t nq_pass = std::min<uint32_t>(4, a.nq - q0);
        const int slots = nq_pass == 1 ? 1 : 4;
        SlabScanParams p;
        p.corpus = a.corpus;
        p.n_rows = a.rows;
        p.queries = a.queries + (size_t)q0 * a.dim;
        p.nq_active = nq_pass;
        p.kp = kp;
        p.chunk_table = a.chunk_table;
        p.n_chunks = a.n_chunks;
        p.block_lists = lists;
        const slab_scan_kernel_t kernel = nibble ? nibble_scan_kernel_of(slots, filtered)
                                        : byte   ? byte_scan_kernel_of(slots, filtered)
                                        : half   ? half_scan_kernel_of(slots, filtered)
                                        : narrow ? narrow_scan_kernel_of(slots, filtered)
                                        : S == 2 ? slab_scan_kernel_of<2>(slots, filtered)
                                        : S == 3 ? slab_scan_kernel_of<3>(slots, filtered) : slab_scan_kernel_of<4>(slots, filtered);
        const size_t smem = slab_list_smem_bytes(slots, waves);
        const char *prof_name = nibble ? "scan_nibble" : byte ? "scan_byte" : half ? "scan_half" : narrow ? "scan_narrow" : "scan_slab";
        prof_begin(ctx, prof_name);
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(SLAB_THREADS), smem, ctx->stream, p);
        prof_end(ctx, prof_name);
        SMT_HIP_CHECK(hipGetLastError());
        if ((rc = launch_finish_slab(ctx, a, lists, (uint32_t)blocks, kp, q0, nq_pass))) return rc;
    }
    return SMT_OK;
}

}  // namespace smt
