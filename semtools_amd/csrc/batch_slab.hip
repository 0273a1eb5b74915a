// batch_slab.hip -- WIDE rows, many queries per corpus pass on the bf16 MFMA pipe: batch_slab_split_kernel (the queries' operand image,
// once per call), batch_slab_kernel<S, FILTERED> (one streaming pass for up to QB = 64 / 32 / 32 queries at S = 2 / 3 / 4) and the launch
// of a call's passes, each followed by finish_slab_kernel.  No operand image of the corpus, no level plan, no candidate buffers: the
// kernel writes the block lists the finish stage already merges, re-scores in f64 and certifies under f32_err_batch_slab (wide_rows.h).
//
// WORK SPLIT.  A wave owns a TILE of 32 consecutive rows (filtered: 8 consecutive entries of the chunk table of range_tables.hip,
// FILTER_CHUNK rows each, rows an entry does not have masked); tiles are dealt to the waves of the launch round robin.  A block serves
// ONE pass: the operands of its QB queries lie in LDS for the whole launch, [slab][query] rows of 1040 bytes (QT_STRIDE_F4: the 32
// lanes of a ds_read_b128 start 65 float4 apart, conflict-free).
//
// ROWS.  A tile is read in UNITS of a quarter slab (64 dims): 8 instructions, each 128-byte runs of 8 rows -- gemm_rowreg.hip's row
// pattern (measured there at the HBM rate), not one row per instruction: a row per instruction leaves every 32-dim slice in 8 lanes
// of 32 registers, and the transpose buffer that could take whole rows (16.5 KiB per wave) does not fit beside 128 KiB of queries.
// A quarter slab is the unit because the NEXT unit is requested before the current one is multiplied: 32 VGPRs of rows in flight,
// 32 of operands and up to 32 of accumulators -- 188 to 219 VGPRs in all, no scratch; with half a slab per unit the build's resource
// report showed 16 to 51 registers spilled at every width.  |x|^2 is summed in f32 in the load layout (8 lanes per row, three xor
// steps per tile) and handed to lane (j, .) with four lane reads; the raw row is split into bf16 hi / lo (never rescaled) and goes
// through the wave's 2.5 KiB transpose buffer per 32-dim slice, hi then lo, exactly as gemm_rowreg.hip does.
//
// MEASURED (tools/wide_batch_rate.py, profiles/wide_batch.json, 1 GiB of rows): the kernel streams rows at 4.4 to 5.5 TB/s with up
// to 8 queries and at 3.0 TB/s (1.8 at 512 dimensions, 64 queries) with a full pass: converting and multiplying, not HBM, bounds a
// full pass.  1000 queries: 4.1 to 5.6 times the passes of four.
//
// PRODUCTS.  The QUERY quads are the MFMA's first operand, the rows the second: accumulator register r of lane (j, h) is
// <query acc_row(r, h) of the 32-query tile, row j of the row tile>, so 1/|x| is ONE value per lane and the 16 thresholds of a lane
// are four 32-byte LDS reads.  One f32x16 accumulator per 32-query tile, carried over the tile's 2 S units, mfma_bf16x3 per K-step.
// Epilogue: d = max(1 - acc / |x|, 0) (the query operand is the UNIT query), 1 against a zero row or for a zero query, 0 for both.
//
// LISTS (batch_list.h, shared with batch_half.hip).  Form built: the per-(block, query) list of k' keys lives IN the block_lists area the finish reads (global memory, L2
// resident: 64 x k' x 8 bytes per block), ascending, preset to KEY_PAD; LDS holds only the QB thresholds (the k'-th key, KEY_PAD while
// the list is short, 0 for a padding query) and QB lock words.  Why not LDS lists: 133,120 bytes of queries and 20,480 of transpose
// buffers leave 10 KiB at S = 2 and 4, the lists need 16 to 32.  Serialisation: an LDS LOCK WORD per query, taken by the wave that found
// a candidate (lane 0 spins on a compare-and-swap; a wave holds one lock at a time); under it the wave reads the list into its lanes,
// inserts by ballot rank as scan_slab_kernel does, stores it back and publishes the new threshold.  A stale threshold only admits
// more: every candidate is compared again under the lock.  An owner wave per query would need a queue in the LDS that is not there.
#include "batch_list.h"

namespace smt {

struct BatchSlabParams {
    const float *corpus;
    uint64_t n_rows;
    const uint32_t *split;         // the pass' first query: [QB][S][256] words (batch_slab_split_kernel)
    const uint32_t *qzero;         // the pass' first query: 1 = zero query or outside the domain
    uint32_t nq_active;            // 1 .. QB
    uint32_t kp;
    const uint64_t *chunk_table;   // FILTERED
    uint64_t n_chunks;
    uint64_t n_tiles;
    key_t64 *block_lists;          // [nq_active][gridDim.x][kp]
};

// One wave per query (padding queries included: zero operands).  The unit query q / |q| split into bf16 hi and lo, in the order the
// MFMA operand wants: quad (K-step m, half h) of slab s = words 8 (2 m + h) .. + 3 (hi), + 4 .. + 7 (lo) of the slab's 256.
__global__ void __launch_bounds__(256) batch_slab_split_kernel(const float *queries, uint32_t nq, uint32_t nq_pad, int S, uint32_t *split,
                                                               uint32_t *qzero)
{
    const int lane = threadIdx.x & 63;
    const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq_pad) return;
    f32x4 v[4];
    float a2 = 0.0f;
    uint32_t mx = 0;
    for (int s = 0; s < 4; ++s) {
        v[s] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (s < S && q < nq) v[s] = reinterpret_cast<const f32x4 *>(queries + (size_t)q * 256 * S)[s * 64 + lane];
        a2 = fmaf(v[s].x, v[s].x, a2); a2 = fmaf(v[s].y, v[s].y, a2); a2 = fmaf(v[s].z, v[s].z, a2); a2 = fmaf(v[s].w, v[s].w, a2);
        mx = max(max(mx, __float_as_uint(v[s].x) & 0x7fffffffu), max(__float_as_uint(v[s].y) & 0x7fffffffu, __float_as_uint(v[s].z) & 0x7fffffffu));
        mx = max(mx, __float_as_uint(v[s].w) & 0x7fffffffu);
    }
    a2 = wave_sum(a2);
    for (int o = 1; o < 64; o <<= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
    const bool zero = a2 == 0.0f || !magnitude_in_domain(mx) || q >= nq;   // counted as a zero query: the finish reports INVALID_QUERY
    const float rq = zero ? 0.0f : __frsqrt_rn(a2);
    for (int s = 0; s < S; ++s) {
        const f32x4 u = zero ? (f32x4){0.f, 0.f, 0.f, 0.f} : v[s] * rq;
        uint32_t h0, h1, l0, l1;
        bf16_split2(u.x, u.y, h0, l0);
        bf16_split2(u.z, u.w, h1, l1);
        uint32_t *dst = split + ((size_t)q * S + s) * 256 + (lane >> 1) * 8 + 2 * (lane & 1);
        dst[0] = h0; dst[1] = h1;
        dst[4] = l0; dst[5] = l1;
    }
    if (lane == 0) qzero[q] = zero ? 1u : 0u;
}

template <int S, bool FILTERED>
__global__ void __launch_bounds__(BS_THREADS, 2) batch_slab_kernel(BatchSlabParams p)
{
    static_assert(S >= 2 && S <= 4, "2..4 slabs");
    constexpr int QB = S == 2 ? 64 : 32;
    constexpr int NT = QB / 32;               // 32-query tiles of a pass
    constexpr int ROW_F4 = 64 * S;            // float4 per corpus row
    constexpr int USL = 2;                    // 32-dim slices of a unit: a quarter slab
    constexpr int UNITS = 8 / USL * S;        // units per row
    extern __shared__ __attribute__((aligned(16))) unsigned char bs_smem[];
    f32x4 *s_q = reinterpret_cast<f32x4 *>(bs_smem);                                   // [S][QB][65] float4
    unsigned char *s_t = bs_smem + (size_t)S * QB * QT_STRIDE_F4 * 16;                  // [waves][RR_TBUF]
    key_t64 *s_thr = reinterpret_cast<key_t64 *>(s_t + BS_WAVES * RR_TBUF);             // [QB]
    unsigned int *s_lock = reinterpret_cast<unsigned int *>(s_thr + QB);               // [QB]
    unsigned int *s_qz = s_lock + QB;                                                  // [NT] masks of zero queries

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, j = lane & 31;
    const int kp = (int)p.kp;
    const int nt_active = (int)((p.nq_active + 31) / 32);
    unsigned char *tbuf = s_t + wave * RR_TBUF;

    // ---- the pass' operands, thresholds, locks and empty lists
    for (int r = wave; r < S * QB; r += BS_WAVES) {   // LDS row r = (slab s, query qq)
        const int s = r / QB, qq = r - s * QB;
        s_q[r * QT_STRIDE_F4 + lane] = reinterpret_cast<const f32x4 *>(p.split + ((size_t)qq * S + s) * 256)[lane];
    }
    batch_lists_init<QB>(s_thr, s_lock, s_qz, p.qzero, p.nq_active, kp, p.block_lists, lane, wave);
    __syncthreads();

    const uint64_t n_waves = (uint64_t)gridDim.x * BS_WAVES;
    uint64_t tile = (uint64_t)blockIdx.x * BS_WAVES + wave;
    const f32x4 *corpus4 = reinterpret_cast<const f32x4 *>(p.corpus);
    // load view: this lane reads 16 bytes (float4 lane & 7 of a 32-dim slice) of tile rows 8 u + (lane >> 3), u = 0 .. 3
    auto locate = [&](uint64_t t, uint64_t (&rowv)[4]) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t tr = (uint32_t)(8 * u + (lane >> 3));
            if constexpr (FILTERED) {
                const uint64_t e = t * 8 + (tr >> 2);
                const uint64_t desc = e < p.n_chunks ? p.chunk_table[e] : 0ull;
                rowv[u] = (tr & 3u) < (uint32_t)(desc >> 32) ? (desc & 0xFFFFFFFFull) + (tr & 3u) : 0ull;   // rows there are not: row 0, masked
            } else {
                const uint64_t r = t * 32 + tr;
                rowv[u] = r < p.n_rows ? r : 0ull;
            }
        }
    };
    auto issue = [&](const uint64_t (&rowv)[4], int unit, f32x4 (&R)[4 * USL]) __attribute__((always_inline)) {
        const f32x4 *base = corpus4 + unit * (8 * USL) + (lane & 7);
#pragma unroll
        for (int i = 0; i < 4 * USL; ++i) R[i] = __builtin_nontemporal_load(base + rowv[i & 3] * ROW_F4 + 8 * (i >> 2));
    };
    const uint32_t t_wr = (uint32_t)((lane >> 3) * RR_TROW + (lane & 7) * 8);
    const uint32_t t_rd = (uint32_t)(j * RR_TROW + h * 16);
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

    f32x4 R[4 * USL];
    uint64_t rowv[4];
    if (tile < p.n_tiles) {
        locate(tile, rowv);
        issue(rowv, 0, R);
    }
    while (tile < p.n_tiles) {
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
        float x2[4] = {0.f, 0.f, 0.f, 0.f};
        const uint64_t tile_next = tile + n_waves;
#pragma unroll 1
        for (int unit = 0; unit < UNITS; ++unit) {
            // ---- this unit's rows: |x|^2 and the bf16 split in the load layout, then the transpose per 32-dim slice
            u32x4 Xh[2 * USL], Xl[2 * USL];
#pragma unroll
            for (int sl = 0; sl < USL; ++sl) {
                uint32_t hi[4][2], lo[4][2];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const f32x4 v = R[4 * sl + u];
                    x2[u] = fmaf(v.x, v.x, x2[u]); x2[u] = fmaf(v.y, v.y, x2[u]); x2[u] = fmaf(v.z, v.z, x2[u]); x2[u] = fmaf(v.w, v.w, x2[u]);
                    bf16_split2(v.x, v.y, hi[u][0], lo[u][0]);
                    bf16_split2(v.z, v.w, hi[u][1], lo[u][1]);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) *reinterpret_cast<u32x2 *>(tbuf + t_wr + u * 8 * RR_TROW) = (u32x2){hi[u][0], hi[u][1]};
                Xh[2 * sl] = *reinterpret_cast<const u32x4 *>(tbuf + t_rd);
                Xh[2 * sl + 1] = *reinterpret_cast<const u32x4 *>(tbuf + t_rd + 32);
#pragma unroll
                for (int u = 0; u < 4; ++u) *reinterpret_cast<u32x2 *>(tbuf + t_wr + u * 8 * RR_TROW) = (u32x2){lo[u][0], lo[u][1]};
                Xl[2 * sl] = *reinterpret_cast<const u32x4 *>(tbuf + t_rd);
                Xl[2 * sl + 1] = *reinterpret_cast<const u32x4 *>(tbuf + t_rd + 32);
            }
            // ---- the next unit (or the next tile's first) is requested before this one is multiplied
            if (unit + 1 < UNITS) issue(rowv, unit + 1, R);
            else if (tile_next < p.n_tiles) {
                locate(tile_next, rowv);
                issue(rowv, 0, R);
            }
            // ---- products: K-steps 4 (unit & 3) .. + 3 of slab unit / 4 against every query tile of the pass
            const u32x4 *bq = reinterpret_cast<const u32x4 *>(s_q + ((unit >> 2) * QB + j) * QT_STRIDE_F4) + 16 * (unit & 3) + 2 * h;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (t < nt_active) {   // (wave-uniform)
                    const u32x4 *bt = bq + t * 32 * QT_STRIDE_F4;
#pragma unroll
                    for (int m = 0; m < 2 * USL; ++m) {
                        acc[t] = mfma_bf16x3(bt[4 * m], bt[4 * m + 1], Xh[m], Xl[m], acc[t]);
                        __builtin_amdgcn_sched_barrier(0);   // (the B reads stay at their K-step: hoisted together they cost 64 VGPRs)
                    }
                }
            }
        }

        // ---- 1 / |x| of row j into lane (j, .): row 8 u + i was summed by lanes 8 i .. 8 i + 7 of x2[u]
        float rxj = 0.0f;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float part = x2[u];
            part += __shfl_xor(part, 1);
            part += __shfl_xor(part, 2);
            part += __shfl_xor(part, 4);
            const float rb = part == 0.0f ? 0.0f : __frsqrt_rn(part);
            const float got = __shfl(rb, 8 * (j & 7));
            rxj = (j >> 3) == u ? got : rxj;
        }
        // accumulator view: lane (j, .) scores tile row j
        uint32_t rowj;
        bool validj;
        if constexpr (FILTERED) {
            const uint64_t e = tile * 8 + (uint32_t)(j >> 2);
            const uint64_t desc = e < p.n_chunks ? p.chunk_table[e] : 0ull;
            validj = (uint32_t)(j & 3) < (uint32_t)(desc >> 32);
            rowj = (uint32_t)desc + (uint32_t)(j & 3);
        } else {
            validj = tile * 32 + j < p.n_rows;
            rowj = (uint32_t)(tile * 32 + j);
        }
        batch_tile_nominate<NT>(acc, nt_active, rxj, rxj == 0.0f, rowj, validj, s_qz, s_thr, s_lock, p.block_lists, kp, lane);
        tile = tile_next;
    }
}

constexpr int batch_slab_qb(int S) { return S == 2 ? 64 : 32; }
static size_t batch_slab_smem(int S)
{
    const int QB = batch_slab_qb(S);
    return (size_t)S * QB * QT_STRIDE_F4 * 16 + (size_t)BS_WAVES * RR_TBUF + (size_t)QB * 12 + 16;
}
uint32_t slab_batch_qb(uint32_t dim) { return (uint32_t)batch_slab_qb((int)(dim / 256)); }

using batch_slab_kernel_t = void (*)(BatchSlabParams);
static batch_slab_kernel_t batch_slab_kernel_of(int S, bool filtered)
{
    if (S == 2) return filtered ? batch_slab_kernel<2, true> : batch_slab_kernel<2, false>;
    if (S == 3) return filtered ? batch_slab_kernel<3, true> : batch_slab_kernel<3, false>;
    return filtered ? batch_slab_kernel<4, true> : batch_slab_kernel<4, false>;
}

// split image + one pass: the queries [q0, q0 + nq_pass) of `a` into lists [nq_pass][blocks][kp]
static int batch_slab_pass(smt_ctx *ctx, const SlabSearch &a, const uint32_t *split, const uint32_t *qzero, uint32_t q0, uint32_t nq_pass,
                           uint32_t kp, uint64_t n_tiles, int blocks, key_t64 *lists)
{
    const int S = (int)(a.dim / 256);
    const bool filtered = a.chunk_table != nullptr;
    const batch_slab_kernel_t kernel = batch_slab_kernel_of(S, filtered);
    if (!(ctx->attr_done & ATTR_BATCH_SLAB)) {
        for (int s = 2; s <= 4; ++s)
            for (int f = 0; f < 2; ++f)
                SMT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(batch_slab_kernel_of(s, f != 0)),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        ctx->attr_done |= ATTR_BATCH_SLAB;
    }
    BatchSlabParams p;
    p.corpus = a.corpus;
    p.n_rows = a.rows;
    p.split = split + (size_t)q0 * a.dim;
    p.qzero = qzero + q0;
    p.nq_active = nq_pass;
    p.kp = kp;
    p.chunk_table = a.chunk_table;
    p.n_chunks = a.n_chunks;
    p.n_tiles = n_tiles;
    p.block_lists = lists;
    prof_begin(ctx, "batch_slab");
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(BS_THREADS), batch_slab_smem(S), ctx->stream, p);
    prof_end(ctx, "batch_slab");
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

static int batch_slab_split(smt_ctx *ctx, const SlabSearch &a, uint32_t nq_pad, uint32_t *split, uint32_t *qzero)
{
    prof_begin(ctx, "batch_slab_split");
    hipLaunchKernelGGL(batch_slab_split_kernel, dim3((nq_pad + 3) / 4), dim3(256), 0, ctx->stream, a.queries, a.nq, nq_pad, (int)(a.dim / 256),
                       split, qzero);
    prof_end(ctx, "batch_slab_split");
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

// The passes of one call on the batched route: the query split once, then per pass of QB queries the kernel and its finish under
// f32_err_batch_slab.  The last pass may be ragged: its padding queries nominate nothing and no list of theirs is read.
int launch_batch_slab(smt_ctx *ctx, const SlabSearch &a)
{
    const int S = (int)(a.dim / 256);
    const uint32_t QB = (uint32_t)batch_slab_qb(S);
    uint32_t kp;
    uint64_t n_tiles;
    int blocks;
    batch_shape(ctx, a, kp, n_tiles, blocks);
    const uint32_t nq_pad = (a.nq + QB - 1) / QB * QB;
    BatchScratch s;
    int rc = batch_scratch(ctx, a.dim, nq_pad, (size_t)QB * blocks * kp, s);
    if (rc) return rc;
    if ((rc = batch_slab_split(ctx, a, nq_pad, s.split, s.qzero))) return rc;
    const double err = S == 2 ? f32_err_batch_slab(2) : S == 3 ? f32_err_batch_slab(3) : f32_err_batch_slab(4);
    for (uint32_t q0 = 0; q0 < a.nq; q0 += QB) {
        const uint32_t nq_pass = std::min<uint32_t>(QB, a.nq - q0);
        if ((rc = batch_slab_pass(ctx, a, s.split, s.qzero, q0, nq_pass, kp, n_tiles, blocks, s.lists))) return rc;
        if ((rc = launch_finish_slab(ctx, a, s.lists, (uint32_t)blocks, kp, q0, nq_pass, err))) return rc;
    }
    return SMT_OK;
}

// Test hook (smt_debug_batch_slab_lists): the production split and the passes of a.nq queries, no finish (batch_list.h)
int debug_batch_slab_lists(smt_ctx *ctx, const SlabSearch &a, key_t64 *out_keys_host, uint64_t out_cap_keys, uint32_t *out_blocks,
                           uint32_t *out_kp)
{
    return debug_batch_lists(
        ctx, a, slab_batch_qb(a.dim), [&](uint32_t nq_pad, const BatchScratch &s) { return batch_slab_split(ctx, a, nq_pad, s.split, s.qzero); },
        [&](const BatchScratch &s, uint32_t q0, uint32_t nq_pass, uint32_t kp, uint64_t n_tiles, int blocks, key_t64 *lists) {
            return batch_slab_pass(ctx, a, s.split, s.qzero, q0, nq_pass, kp, n_tiles, blocks, lists);
        },
        out_keys_host, out_cap_keys, out_blocks, out_kp);
}

}  // namespace smt
