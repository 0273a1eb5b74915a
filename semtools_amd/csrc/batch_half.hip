// batch_half.hip -- HALF rows (256 binary16 values, 512 B), many queries per corpus pass on the f16 MFMA pipe: batch_half_split_kernel
// (the queries' operand image, once per call), batch_half_kernel<FILTERED, DIRECT> (one streaming pass for up to QB = 128 queries) and
// the launch of a call's passes, each followed by finish_slab_kernel under f32_err_batch_half (half_rows.h).  The frame -- 512 threads,
// a wave owns a TILE of 32 consecutive rows (filtered: 8 entries of the chunk table), tiles dealt round robin, the lists, the epilogue
// -- is batch_list.h's, shared with batch_slab.hip.  What differs from the wide kernel: a stored row already IS an f16 MFMA operand,
// so nothing is converted, split or rounded on the row side; only the query is split, into f16 hi + lo, once per call; two
// v_mfma_f32_32x32x16_f16 per 16 dimensions instead of three bf16 ones; and the LDS a query takes halves, which doubles QB.
//
// THE QUERY'S SCALE.  The unit query u = q / |q| is multiplied by 2^14 before it is split (f16_split2, mfma_tile.h): |2^14 u_i| <=
// 16384 < 65504, and a lo half that is subnormal -- or that a flush would lose, in the conversion or in the MFMA -- is below 2^-14,
// that is 2^-28 on u_i; over a row sum |x_i| <= 16 |x|, so the lost term is at most 2^-24 |x|: negligible whether or not the
// instruction keeps subnormal inputs.  The accumulator holds 2^14 <u, x>; the epilogue multiplies by 2^-14 / |x| (a power of two folded
// into one f32 factor: exact).  RANGES.  The stored halves are NOT normalised: up to 65504, down to subnormals.  The largest product
// is 2^14 x 65504 < 2^30, 256 of them stay below 2^39: fine in f32.  |x|^2 in f32 is at most 256 x 65504^2 = 1.1e12; the square of
// a subnormal half is at least 2^-48: a normal f32.  1 / |x| x 2^-14 lies within [5.8e-11, 2^10 x 2^-14 ... 2^24 x 2^-14]: normal.
//
// QUERIES IN LDS.  One row per query, 1 KiB: quad (K-step m, half h) = words 8 (2 m + h) .. + 3 (hi), + 4 .. + 7 (lo), rows
// QT_STRIDE_F4 float4 apart (1040 B: the 32 lanes of a ds_read_b128 start 65 float4 apart, conflict-free).  QB = 128: 133,120 bytes
// of queries, 20,480 of transpose buffers, 1,552 of thresholds, locks and masks -- 155,152 of the 160 KiB -- four 32-query tiles, 64
// accumulator registers.  Query tiles a ragged pass does not have are skipped wave-uniformly.
//
// ROWS.  Two forms, one template flag, tuning key half_batch_direct chooses (A/B: profiles/half_batch.json has both):
//   transposed (0)  gemm_rowreg.hip's row pattern: a UNIT is 64 dimensions of the tile's 32 rows, four instructions in which 8 lanes
//       read a 128-byte run of a row and a wave 8 rows; the next unit (or the next tile's first) is requested before the current one is
//       multiplied.  Each 32-dimension slice then goes ONCE through the wave's 2.5 KiB transpose buffer into operand layout (the
//       lanes that hold the slice write 16 bytes each, every lane reads its two K-steps): one write and read round, no hi / lo.
//   direct (1)      the K order is free as long as both operands agree, and lane (j, h) of K-step m wants exactly bytes
//       32 m + 16 h .. + 15 of row j: it loads them -- no LDS, no VALU, but 32-byte runs per row and instruction.
// |x|^2 is summed in f32 with exact widening of the halves (v_fma_mix_f32 / v_cvt_f32_f16, as scan_half.hip) in the load layout and
// handed to lane (j, .): three xor steps and four lane reads (transposed, as the wide kernel), one xor step (direct).
//
// MEASURED (tools/half_batch_rate.py, profiles/half_batch.json, 1 GiB of half rows, device form, top_k 10, ms per call against the scan's
// passes of four): 4 queries 0.273 / 0.327, 8: 0.318 / 0.637, 32: 0.563 / 2.55, 128: 1.61 / 10.2, 1000: 12.6 / 80.0 (6.3 times).  The
// kernel streams rows at 4.3 TB/s with 4 queries and at 0.69 TB/s with a full pass: a full pass is bound by the query reads from LDS
// and the MFMAs behind them, not by HBM.  The direct form is slower up to 32 queries (0.366 ms at 4, 0.392 at 8: the 32-byte runs cost
// a quarter of the row rate) and level with the transposed one from 64 on, so the transposed form is the default.  QB = 128 builds
// without scratch: 194 / 182 VGPRs (unfiltered / filtered), 149 / 142 direct.
//
// PRODUCTS.  The query quads are the MFMA's FIRST operand, the rows the second (mfma_f16x2_first): accumulator register r of lane
// (j, h) is <query acc_row(r, h) of the 32-query tile, row j>, so 1 / |x| is one value per lane.  32 MFMAs per (row tile, query tile).
// Epilogue (batch_list.h): d = max(1 - acc x 2^-14 / |x|, 0), 1 against a zero row or for a zero query, 0 for both.
//
// SUBNORMAL STORED HALVES.  The contract is over the stored values, so a row of subnormal halves must be nominated within the bound.
// Whether v_mfma_f32_32x32x16_f16 keeps subnormal INPUTS is observed, not assumed: tests/test_gpu_half_batch.py holds a row stored
// as subnormal halves only and rows with a few subnormal components; profiles/half_batch.json ("mfma_subnormal_inputs") records
// what an MI355X did: it KEEPS them -- the all-subnormal row was nominated at 1.4688e-04 against an exact 1.467e-04 -- so there is
// no per-corpus flag and every half corpus takes this route.
#include "half_rows.h"
#include "batch_list.h"

namespace smt {

constexpr int BH_QB = 128;
constexpr float BH_QUERY_SCALE = 16384.0f, BH_INV_SCALE = 1.0f / 16384.0f;

struct BatchHalfParams {
    const void *corpus;            // [n_rows][256] binary16
    uint64_t n_rows;
    const uint32_t *split;         // the pass' first query: [QB][256] words (batch_half_split_kernel)
    const uint32_t *qzero;         // the pass' first query: 1 = zero query or outside the domain
    uint32_t nq_active;            // 1 .. QB
    uint32_t kp;
    const uint64_t *chunk_table;   // FILTERED
    uint64_t n_chunks;
    uint64_t n_tiles;
    key_t64 *block_lists;          // [nq_active][gridDim.x][kp]
};

// One wave per query (padding queries included: zero operands).  2^14 q / |q| split into f16 hi and lo, in the order the MFMA operand
// wants (header: queries in LDS).  Zero and domain handling and the qzero flags are batch_slab_split_kernel's.
__global__ void __launch_bounds__(256) batch_half_split_kernel(const float *queries, uint32_t nq, uint32_t nq_pad, uint32_t *split, uint32_t *qzero)
{
    const int lane = threadIdx.x & 63;
    const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq_pad) return;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (q < nq) v = reinterpret_cast<const f32x4 *>(queries + (size_t)q * SMT_DIM)[lane];
    float a2 = fmaf(v.x, v.x, 0.0f);
    a2 = fmaf(v.y, v.y, a2); a2 = fmaf(v.z, v.z, a2); a2 = fmaf(v.w, v.w, a2);
    uint32_t mx = max(max(__float_as_uint(v.x) & 0x7fffffffu, __float_as_uint(v.y) & 0x7fffffffu),
                      max(__float_as_uint(v.z) & 0x7fffffffu, __float_as_uint(v.w) & 0x7fffffffu));
    a2 = wave_sum(a2);
    for (int o = 1; o < 64; o <<= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
    const bool zero = a2 == 0.0f || !magnitude_in_domain(mx) || q >= nq;   // counted as a zero query: the finish reports INVALID_QUERY
    const float rq = zero ? 0.0f : __frsqrt_rn(a2) * BH_QUERY_SCALE;
    const f32x4 u = zero ? (f32x4){0.f, 0.f, 0.f, 0.f} : v * rq;
    uint32_t h0, h1, l0, l1;
    f16_split2(u.x, u.y, h0, l0);
    f16_split2(u.z, u.w, h1, l1);
    uint32_t *dst = split + (size_t)q * 256 + (lane >> 1) * 8 + 2 * (lane & 1);
    dst[0] = h0; dst[1] = h1;
    dst[4] = l0; dst[5] = l1;
    if (lane == 0) qzero[q] = zero ? 1u : 0u;
}

// sum of the squares of eight halves, widened exactly
__device__ __forceinline__ float half_sumsq8(const u32x4 &r, float acc)
{
    const f16x8 hv = __builtin_bit_cast(f16x8, r);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float f = (float)hv[i];
        acc = fmaf(f, f, acc);
    }
    return acc;
}

template <bool FILTERED, bool DIRECT>
__global__ void __launch_bounds__(BS_THREADS, 2) batch_half_kernel(BatchHalfParams p)
{
    constexpr int QB = BH_QB;
    constexpr int NT = QB / 32;      // 32-query tiles of a pass
    constexpr int ROW_Q = 32;        // 16-byte quads per corpus row
    constexpr int UNITS = 4;         // units per row: 64 dimensions, four K-steps each
    constexpr int NR = DIRECT ? 1 : 4;   // rows a lane reads of a tile
    extern __shared__ __attribute__((aligned(16))) unsigned char bh_smem[];
    f32x4 *s_q = reinterpret_cast<f32x4 *>(bh_smem);                                   // [QB][65] float4
    unsigned char *s_t = bh_smem + (size_t)QB * QT_STRIDE_F4 * 16;                      // [waves][RR_TBUF]
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
    for (int r = wave; r < QB; r += BS_WAVES) s_q[r * QT_STRIDE_F4 + lane] = reinterpret_cast<const f32x4 *>(p.split + (size_t)r * 256)[lane];
    batch_lists_init<QB>(s_thr, s_lock, s_qz, p.qzero, p.nq_active, kp, p.block_lists, lane, wave);
    __syncthreads();

    const uint64_t n_waves = (uint64_t)gridDim.x * BS_WAVES;
    uint64_t tile = (uint64_t)blockIdx.x * BS_WAVES + wave;
    const u32x4 *corpus4 = reinterpret_cast<const u32x4 *>(p.corpus);
    // the corpus row behind tile row tr of tile t; rows there are not: row 0, masked in the epilogue
    auto row_of = [&](uint64_t t, uint32_t tr) __attribute__((always_inline)) -> uint64_t {
        if constexpr (FILTERED) {
            const uint64_t e = t * 8 + (tr >> 2);
            const uint64_t desc = e < p.n_chunks ? p.chunk_table[e] : 0ull;
            return (tr & 3u) < (uint32_t)(desc >> 32) ? (desc & 0xFFFFFFFFull) + (tr & 3u) : 0ull;
        } else {
            const uint64_t r = t * 32 + tr;
            return r < p.n_rows ? r : 0ull;
        }
    };
    // load view.  transposed: 16 bytes (quad lane & 7 of a unit) of tile rows 8 u + (lane >> 3), u = 0 .. 3; direct: tile row j
    auto locate = [&](uint64_t t, uint64_t (&rowv)[NR]) __attribute__((always_inline)) {
        if constexpr (DIRECT) rowv[0] = row_of(t, (uint32_t)j);
        else {
#pragma unroll
            for (int u = 0; u < 4; ++u) rowv[u] = row_of(t, (uint32_t)(8 * u + (lane >> 3)));
        }
    };
    auto issue = [&](const uint64_t (&rowv)[NR], int unit, u32x4 (&R)[4]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (DIRECT) R[i] = __builtin_nontemporal_load(corpus4 + rowv[0] * ROW_Q + unit * 8 + 2 * i + h);   // K-step i
            else R[i] = __builtin_nontemporal_load(corpus4 + rowv[i] * ROW_Q + unit * 8 + (lane & 7));                      // rows 8 i ..
        }
    };
    const uint32_t t_wr = (uint32_t)((lane >> 3) * RR_TROW + (lane & 3) * 16);
    const uint32_t t_rd = (uint32_t)(j * RR_TROW + h * 16);

    u32x4 R[4];
    uint64_t rowv[NR];
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
        float x2[NR];
#pragma unroll
        for (int u = 0; u < NR; ++u) x2[u] = 0.0f;
        const uint64_t tile_next = tile + n_waves;
#pragma unroll 1
        for (int unit = 0; unit < UNITS; ++unit) {
            // ---- this unit's rows: |x|^2 in the load layout, then (transposed) each 32-dim slice through the transpose buffer
            u32x4 X[4];
            if constexpr (DIRECT) {
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    x2[0] = half_sumsq8(R[m], x2[0]);
                    X[m] = R[m];
                }
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) x2[u] = half_sumsq8(R[u], x2[u]);
#pragma unroll
                for (int sl = 0; sl < 2; ++sl) {
                    wave_lds_sync();   // (the reads of the slice before are done)
                    if (((lane >> 2) & 1) == sl) {
#pragma unroll
                        for (int u = 0; u < 4; ++u) *reinterpret_cast<u32x4 *>(tbuf + t_wr + u * 8 * RR_TROW) = R[u];
                    }
                    wave_lds_sync();   // (other lanes wrote what this one reads)
                    X[2 * sl] = *reinterpret_cast<const u32x4 *>(tbuf + t_rd);
                    X[2 * sl + 1] = *reinterpret_cast<const u32x4 *>(tbuf + t_rd + 32);
                }
            }
            // ---- the next unit (or the next tile's first) is requested before this one is multiplied
            if (unit + 1 < UNITS) issue(rowv, unit + 1, R);
            else if (tile_next < p.n_tiles) {
                locate(tile_next, rowv);
                issue(rowv, 0, R);
            }
            // ---- products: K-steps 4 unit .. + 3 against every query tile of the pass
            const u32x4 *bq = reinterpret_cast<const u32x4 *>(s_q + j * QT_STRIDE_F4) + 16 * unit + 2 * h;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (t < nt_active) {   // (wave-uniform)
                    const u32x4 *bt = bq + t * 32 * QT_STRIDE_F4;
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        acc[t] = mfma_f16x2_first(bt[4 * m], bt[4 * m + 1], X[m], acc[t]);
                        __builtin_amdgcn_sched_barrier(0);   // (the query reads stay at their K-step: hoisted together they cost registers)
                    }
                }
            }
        }

        // ---- 2^-14 / |x| of row j into lane (j, .)
        float rxj = 0.0f;
        if constexpr (DIRECT) {
            const float part = x2[0] + __shfl_xor(x2[0], 32);
            rxj = part == 0.0f ? 0.0f : __frsqrt_rn(part);
        } else {   // row 8 u + i was summed by lanes 8 i .. 8 i + 7 of x2[u]
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
        batch_tile_nominate<NT>(acc, nt_active, rxj * BH_INV_SCALE, rxj == 0.0f, rowj, validj, s_qz, s_thr, s_lock, p.block_lists, kp, lane);
        tile = tile_next;
    }
}

static size_t batch_half_smem() { return (size_t)BH_QB * QT_STRIDE_F4 * 16 + (size_t)BS_WAVES * RR_TBUF + (size_t)BH_QB * 12 + 16; }
uint32_t half_batch_qb() { return (uint32_t)BH_QB; }

using batch_half_kernel_t = void (*)(BatchHalfParams);
static batch_half_kernel_t batch_half_kernel_of(bool filtered, bool direct)
{
    if (direct) return filtered ? batch_half_kernel<true, true> : batch_half_kernel<false, true>;
    return filtered ? batch_half_kernel<true, false> : batch_half_kernel<false, false>;
}

// one pass: the queries [q0, q0 + nq_pass) of `a` into lists [nq_pass][blocks][kp]
static int batch_half_pass(smt_ctx *ctx, const SlabSearch &a, const uint32_t *split, const uint32_t *qzero, uint32_t q0, uint32_t nq_pass,
                           uint32_t kp, uint64_t n_tiles, int blocks, key_t64 *lists)
{
    if (!(ctx->attr_done & ATTR_BATCH_HALF)) {
        for (int f = 0; f < 4; ++f)
            SMT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(batch_half_kernel_of(f & 1, f & 2)),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        ctx->attr_done |= ATTR_BATCH_HALF;
    }
    BatchHalfParams p;
    p.corpus = a.corpus;
    p.n_rows = a.rows;
    p.split = split + (size_t)q0 * 256;
    p.qzero = qzero + q0;
    p.nq_active = nq_pass;
    p.kp = kp;
    p.chunk_table = a.chunk_table;
    p.n_chunks = a.n_chunks;
    p.n_tiles = n_tiles;
    p.block_lists = lists;
    prof_begin(ctx, "batch_half");
    hipLaunchKernelGGL(batch_half_kernel_of(a.chunk_table != nullptr, ctx->tune.half_batch_direct != 0), dim3(blocks), dim3(BS_THREADS),
                       batch_half_smem(), ctx->stream, p);
    prof_end(ctx, "batch_half");
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

static int batch_half_split(smt_ctx *ctx, const SlabSearch &a, uint32_t nq_pad, uint32_t *split, uint32_t *qzero)
{
    prof_begin(ctx, "batch_half_split");
    hipLaunchKernelGGL(batch_half_split_kernel, dim3((nq_pad + 3) / 4), dim3(256), 0, ctx->stream, a.queries, a.nq, nq_pad, split, qzero);
    prof_end(ctx, "batch_half_split");
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

// The passes of one call on the batched route: the query split once, then per pass of QB queries the kernel and its finish under
// f32_err_batch_half.  The last pass may be ragged: its padding queries nominate nothing and no list of theirs is read.
int launch_batch_half(smt_ctx *ctx, const SlabSearch &a)
{
    SMT_REQUIRE(a.row_dtype == SMT_ROWS_F16 && a.dim == SMT_DIM, "half batch: half rows of 256");
    uint32_t kp;
    uint64_t n_tiles;
    int blocks;
    batch_shape(ctx, a, kp, n_tiles, blocks);
    const uint32_t nq_pad = (a.nq + BH_QB - 1) / BH_QB * BH_QB;
    BatchScratch s;
    int rc = batch_scratch(ctx, a.dim, nq_pad, (size_t)BH_QB * blocks * kp, s);
    if (rc) return rc;
    if ((rc = batch_half_split(ctx, a, nq_pad, s.split, s.qzero))) return rc;
    for (uint32_t q0 = 0; q0 < a.nq; q0 += BH_QB) {
        const uint32_t nq_pass = std::min<uint32_t>(BH_QB, a.nq - q0);
        if ((rc = batch_half_pass(ctx, a, s.split, s.qzero, q0, nq_pass, kp, n_tiles, blocks, s.lists))) return rc;
        if ((rc = launch_finish_slab(ctx, a, s.lists, (uint32_t)blocks, kp, q0, nq_pass, f32_err_batch_half))) return rc;
    }
    return SMT_OK;
}

// Test hook (smt_debug_batch_half_lists): the production split and the passes of a.nq queries, no finish (batch_list.h)
int debug_batch_half_lists(smt_ctx *ctx, const SlabSearch &a, key_t64 *out_keys_host, uint64_t out_cap_keys, uint32_t *out_blocks,
                           uint32_t *out_kp)
{
    SMT_REQUIRE(a.row_dtype == SMT_ROWS_F16 && a.dim == SMT_DIM, "half batch: half rows of 256");
    return debug_batch_lists(
        ctx, a, BH_QB, [&](uint32_t nq_pad, const BatchScratch &s) { return batch_half_split(ctx, a, nq_pad, s.split, s.qzero); },
        [&](const BatchScratch &s, uint32_t q0, uint32_t nq_pass, uint32_t kp, uint64_t n_tiles, int blocks, key_t64 *lists) {
            return batch_half_pass(ctx, a, s.split, s.qzero, q0, nq_pass, kp, n_tiles, blocks, lists);
        },
        out_keys_host, out_cap_keys, out_blocks, out_kp);
}

}  // namespace smt
