// batch_byte.hip -- BYTE rows (256 signed bytes, 256 B, no scale), many queries per corpus pass on the int8 MFMA pipe:
// batch_byte_split_kernel (the queries' digit image, once per call), batch_byte_kernel<FILTERED> (one streaming pass for up to
// QB = 128 queries) and the launch of a call's passes, each followed by finish_slab_kernel under f32_err_batch_byte (byte_rows.h).
// The frame -- 512 threads, a wave owns a TILE of 32 consecutive rows (filtered: 8 entries of the chunk table), tiles dealt round
// robin, the lists, the epilogue -- is batch_list.h's, shared with batch_slab.hip and batch_half.hip.  What differs from the half
// kernel: the arithmetic is INTEGER and exact, the query is three int8 digit planes instead of two f16 halves, the whole row tile
// is resident in operand layout and the query tiles run past it one at a time, and a load instruction takes four whole rows.
//
// THE QUERY AS DIGITS.  A stored row already IS an int8 MFMA operand.  The unit query u = q / |q| (f32, as batch_half_split_kernel
// computes it) becomes the integer n_i = rint(u_i 2^22), |n_i| <= 2^22 (+ 1 where the f32 quotient lands an ulp over 1), and n_i
// three balanced base-256 digits: n = 65536 d0 + 256 d1 + d2 with d1, d2 in [-128, 127] and |d0| <= 64 (64 only for a one-hot
// query; a scale of 2^23 would take d0 to 128).  Each digit plane has an i32 accumulator of its own: |A_d| <= 256 x 128 x 128 =
// 2^22, so no MFMA result is rounded and each converts to f32 exactly.  score = (65536 A0 + 256 A1 + A2) x 2^-22 / |c|: two fused
// multiply-adds (combine), then batch_list.h's epilogue with rxj = 2^-22 / |c| -- |c|^2 an exact integer (v_dot4_i32_i8 on the
// operand registers, at most 2^22), one rsqrt, the power of two folded in exactly.  f32_err_batch_byte counts what is left.
//
// QUERIES IN LDS.  One row per query, 768 B: plane d = 16-byte units 16 d .. + 15, unit 2 m + h = the digits of dimensions
// 32 m + 16 h .. + 15, which is what lane (., h) feeds K-step m with.  Rows are BB_QSTRIDE = 49 units (784 B) apart: the 32 lanes of
// a ds_read_b128 start an odd number of units apart, as QT_STRIDE_F4 = 65 does for 1 KiB rows.  QB = 128: 100,352 bytes of queries,
// 36,864 of transpose buffers, 1,552 of thresholds, locks and masks -- 138,768 of the 160 KiB.  QB = 160 would need 164,240:
// 400 bytes too many beside these transpose buffers, and quarter slices would double the transpose's write rounds, so 128 stays.
//
// ROWS.  One global_load_dwordx4 of a wave reads 1 KiB: FOUR whole rows, lane l the bytes 16 (l % 16) .. + 15 of row l / 16 of the
// four (scan_byte.hip's load); eight of them are a tile, 32 VGPRs in LOAD layout.  The MFMA wants lane (j, h) to hold 16 bytes of
// row j per K-step -- OPERAND layout, 8 int4.  The K order is free as long as both operands agree; the natural one, K-step m of lane
// (j, h) = bytes 32 m + 16 h .. + 15, is also the cheapest: a 16-byte load unit IS an operand unit, so the transpose moves whole
// ds_write_b128 / ds_read_b128 and no byte is shuffled.  It runs through the wave's buffer of 32 rows x 144 B (128 used; 9 units: 16
// lanes of a read fall into 16 different units) in two SLICES of 128 bytes a row: the lanes that hold the slice (l % 16 / 8 == s)
// write their eight registers, every lane reads its four K-steps.  16 half-occupied writes and 8 reads a tile, against 24 query
// reads per query tile.  The next tile's eight loads are issued once the load registers are free: before anything is multiplied.
//
// THE LOOP.  Three digit accumulators are 48 registers a query tile; four tiles at once, as batch_half_kernel holds them, would be
// 192.  So the ROWS stay (32 VGPRs, operand layout) and the query tiles pass by one at a time: 24 ds_read_b128 of digits and
// 24 v_mfma_i32_32x32x32_i8 per (row tile, query tile), the digits combined, batch_tile_nominate<1> on that tile alone with its
// pointers advanced.  Query tiles a ragged pass does not have are skipped wave-uniformly.  The loop over the four tiles is unrolled
// (the accumulators of one tile are dead before the next begins, so the compiler may start a tile's digit reads under the epilogue
// of the one before): 14.5 against 15.1 ms at 1000 queries, 1.84 against 1.93 at 128, for 206 VGPRs instead of 160.
//
// PRODUCTS.  The digits are the MFMA's FIRST operand, the rows the second: accumulator register r of lane (j, h) is <query
// acc_row(r, h) of the 32-query tile, row j>, so 2^-22 / |c| is one value per lane.  Epilogue (batch_list.h): d = max(1 - score, 0),
// 1 against a zero row or for a zero query, 0 for both.  -128, which an adopted corpus may hold, is an int8 like any other.
//
// BUILD (gfx950, from the resource report; profiles/byte_batch.json repeats it): 206 / 202 VGPRs (unfiltered / filtered), no AGPRs,
// no scratch, 138,768 bytes of dynamic LDS a block; the split kernel 13 VGPRs.
//
// MEASURED (tools/byte_batch_rate.py, profiles/byte_batch.json, 1 GiB of byte rows = 4 Mi rows, device form, top_k 10, ms per call
// against the scan's passes of four): 4 queries 0.286 / 0.386, 8: 0.333 / 0.770, 32: 0.598 / 3.08, 128: 1.84 / 12.3, 1000: 14.5 /
// 96.3 (6.7 times); the answers are the same bytes in every cell.  The kernel streams rows at 4.0 TB/s (15.7 G rows/s) with 4 queries
// and at 0.60 TB/s (2.3 G rows/s) with a full pass.  A full pass takes 1.84 ms where the half route takes 1.61 ms over the same
// GiB -- but over TWICE the rows: per row and query it is 0.57 of the half route's time.  The largest |nominated - f64| the list
// tests saw is 2.7e-7 against the derived 3.49e-6.  NOT built: a direct-load form (32-byte runs cost the half kernel a quarter
// of its row rate), QB above 128.
#include "byte_rows.h"
#include "batch_list.h"

namespace smt {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int BB_QB = 128;
constexpr int BB_QWORDS = 192;        // words of a query's image: three planes of 256 digits
constexpr int BB_QSTRIDE = 49;        // 16-byte units between queries in LDS (48 used)
constexpr int BB_TROW = 144;          // bytes per row in the transpose buffer (128 used: a slice)
constexpr int BB_TBUF = 32 * BB_TROW; // per wave
constexpr float BB_QUERY_SCALE = 4194304.0f, BB_INV_SCALE = 1.0f / 4194304.0f;   // 2^22

struct BatchByteParams {
    const void *corpus;            // [n_rows][256] int8
    uint64_t n_rows;
    const uint32_t *split;         // the pass' first query: [QB][192] words (batch_byte_split_kernel)
    const uint32_t *qzero;         // the pass' first query: 1 = zero query or outside the domain
    uint32_t nq_active;            // 1 .. QB
    uint32_t kp;
    const uint64_t *chunk_table;   // FILTERED
    uint64_t n_chunks;
    uint64_t n_tiles;
    key_t64 *block_lists;          // [nq_active][gridDim.x][kp]
};

// One wave per query (padding queries included: zero operands).  rint(2^22 q / |q|) in three balanced base-256 digits, plane by
// plane in dimension order (header: queries in LDS).  Zero and domain handling and the qzero flags are batch_half_split_kernel's.
__global__ void __launch_bounds__(256) batch_byte_split_kernel(const float *queries, uint32_t nq, uint32_t nq_pad, uint32_t *split, uint32_t *qzero)
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
    const float rq = zero ? 0.0f : __frsqrt_rn(a2);
    uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float u = zero ? 0.0f : v[i] * rq;            // the unit query's component, one rounding
        const int n = (int)rintf(u * BB_QUERY_SCALE);       // (the power of two is exact)
        const int d2 = ((n + 128) & 255) - 128, n1 = (n - d2) >> 8;
        const int d1 = ((n1 + 128) & 255) - 128, d0 = (n1 - d1) >> 8;
        w[0] |= (uint32_t)(d0 & 255) << (8 * i);
        w[1] |= (uint32_t)(d1 & 255) << (8 * i);
        w[2] |= (uint32_t)(d2 & 255) << (8 * i);
    }
    uint32_t *dst = split + (size_t)q * BB_QWORDS + lane;
    dst[0] = w[0]; dst[64] = w[1]; dst[128] = w[2];
    if (lane == 0) qzero[q] = zero ? 1u : 0u;
}

// sum of the squares of sixteen int8, exact
__device__ __forceinline__ int byte_sumsq16(const u32x4 &r, int acc)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_sdot4((int)r[i], (int)r[i], acc, false);
    return acc;
}

template <bool FILTERED>
__global__ void __launch_bounds__(BS_THREADS, 2) batch_byte_kernel(BatchByteParams p)
{
    constexpr int QB = BB_QB;
    constexpr int ROW_Q = 16;        // 16-byte units per corpus row
    constexpr int LOADS = 8;         // load instructions of a tile, four rows each; filtered: one chunk-table entry each
    static_assert(FILTER_CHUNK == 4, "an entry of the chunk table is one load");
    extern __shared__ __attribute__((aligned(16))) unsigned char bb_smem[];
    u32x4 *s_q = reinterpret_cast<u32x4 *>(bb_smem);                                   // [QB][49] units
    unsigned char *s_t = bb_smem + (size_t)QB * BB_QSTRIDE * 16;                        // [waves][BB_TBUF]
    key_t64 *s_thr = reinterpret_cast<key_t64 *>(s_t + BS_WAVES * BB_TBUF);             // [QB]
    unsigned int *s_lock = reinterpret_cast<unsigned int *>(s_thr + QB);               // [QB]
    unsigned int *s_qz = s_lock + QB;                                                  // [QB / 32] masks of zero queries

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, j = lane & 31;
    const int kp = (int)p.kp;
    const int nt_active = (int)((p.nq_active + 31) / 32);
    unsigned char *tbuf = s_t + wave * BB_TBUF;

    // ---- the pass' operands, thresholds, locks and empty lists
    if (lane < 3 * 16)
        for (int r = wave; r < QB; r += BS_WAVES) s_q[r * BB_QSTRIDE + lane] = reinterpret_cast<const u32x4 *>(p.split + (size_t)r * BB_QWORDS)[lane];
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
    // load view: instruction i reads tile rows 4 i .. + 3, lane l unit l % 16 of row 4 i + l / 16
    auto issue = [&](uint64_t t, u32x4 (&R)[LOADS]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < LOADS; ++i)
            R[i] = __builtin_nontemporal_load(corpus4 + row_of(t, (uint32_t)(4 * i + (lane >> 4))) * ROW_Q + (lane & 15));
    };
    const uint32_t t_wr = (uint32_t)((lane >> 4) * BB_TROW + (lane & 7) * 16);
    const uint32_t t_rd = (uint32_t)(j * BB_TROW + h * 16);
    const u32x4 *aq = s_q + j * BB_QSTRIDE + h;   // this lane's digits of query j of a tile: unit 16 d + 2 m (+ h)

    u32x4 R[LOADS];
    if (tile < p.n_tiles) issue(tile, R);
    while (tile < p.n_tiles) {
        // ---- load layout -> operand layout, two slices of 128 bytes a row through the wave's buffer
        u32x4 X[8];
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
            wave_lds_sync();   // (the reads of the slice before are done)
            if (((lane >> 3) & 1) == sl) {
#pragma unroll
                for (int i = 0; i < LOADS; ++i) *reinterpret_cast<u32x4 *>(tbuf + t_wr + i * 4 * BB_TROW) = R[i];
            }
            wave_lds_sync();   // (other lanes wrote what this one reads)
#pragma unroll
            for (int m = 0; m < 4; ++m) X[4 * sl + m] = *reinterpret_cast<const u32x4 *>(tbuf + t_rd + 32 * m);
        }
        // ---- the next tile is requested before this one is multiplied
        const uint64_t tile_next = tile + n_waves;
        if (tile_next < p.n_tiles) issue(tile_next, R);

        // ---- 2^-22 / |c| of row j into lane (j, .): an exact integer sum, one rsqrt
        int c2 = 0;
#pragma unroll
        for (int m = 0; m < 8; ++m) c2 = byte_sumsq16(X[m], c2);
        c2 += __shfl_xor(c2, 32);
        const float rxj = c2 == 0 ? 0.0f : __frsqrt_rn((float)c2);
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

        // ---- the query tiles pass by the resident rows one at a time
#pragma unroll
        for (int t = 0; t < QB / 32; ++t) {
            if (t >= nt_active) break;   // (wave-uniform)
            const u32x4 *at = aq + t * 32 * BB_QSTRIDE;
            i32x16 A[3];
#pragma unroll
            for (int d = 0; d < 3; ++d)
#pragma unroll
                for (int r = 0; r < 16; ++r) A[d][r] = 0;
#pragma unroll
            for (int m = 0; m < 8; ++m)
#pragma unroll
                for (int d = 0; d < 3; ++d)
                    A[d] = __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(i32x4, at[16 * d + 2 * m]), __builtin_bit_cast(i32x4, X[m]), A[d], 0, 0, 0);
            f32x16 acc[1];
#pragma unroll
            for (int r = 0; r < 16; ++r)   // every conversion exact; the first step's rounding is 2^-27 of the cosine, the second's 2^-24
                acc[0][r] = fmaf((float)A[0][r], 65536.0f, fmaf((float)A[1][r], 256.0f, (float)A[2][r]));
            batch_tile_nominate<1>(acc, 1, rxj * BB_INV_SCALE, c2 == 0, rowj, validj, s_qz + t, s_thr + 32 * t, s_lock + 32 * t,
                                   p.block_lists + (size_t)32 * t * gridDim.x * kp, kp, lane);
        }
        tile = tile_next;
    }
}

static size_t batch_byte_smem() { return (size_t)BB_QB * BB_QSTRIDE * 16 + (size_t)BS_WAVES * BB_TBUF + (size_t)BB_QB * 12 + 16; }
uint32_t byte_batch_qb() { return (uint32_t)BB_QB; }

// one pass: the queries [q0, q0 + nq_pass) of `a` into lists [nq_pass][blocks][kp]
static int batch_byte_pass(smt_ctx *ctx, const SlabSearch &a, const uint32_t *split, const uint32_t *qzero, uint32_t q0, uint32_t nq_pass,
                           uint32_t kp, uint64_t n_tiles, int blocks, key_t64 *lists)
{
    const bool filtered = a.chunk_table != nullptr;
    if (!(ctx->attr_done & ATTR_BATCH_BYTE)) {
        SMT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(batch_byte_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        SMT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(batch_byte_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        ctx->attr_done |= ATTR_BATCH_BYTE;
    }
    BatchByteParams p;
    p.corpus = a.corpus;
    p.n_rows = a.rows;
    p.split = split + (size_t)q0 * BB_QWORDS;
    p.qzero = qzero + q0;
    p.nq_active = nq_pass;
    p.kp = kp;
    p.chunk_table = a.chunk_table;
    p.n_chunks = a.n_chunks;
    p.n_tiles = n_tiles;
    p.block_lists = lists;
    prof_begin(ctx, "batch_byte");
    hipLaunchKernelGGL(filtered ? batch_byte_kernel<true> : batch_byte_kernel<false>, dim3(blocks), dim3(BS_THREADS), batch_byte_smem(), ctx->stream, p);
    prof_end(ctx, "batch_byte");
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

static int batch_byte_split(smt_ctx *ctx, const SlabSearch &a, uint32_t nq_pad, uint32_t *split, uint32_t *qzero)
{
    prof_begin(ctx, "batch_byte_split");
    hipLaunchKernelGGL(batch_byte_split_kernel, dim3((nq_pad + 3) / 4), dim3(256), 0, ctx->stream, a.queries, a.nq, nq_pad, split, qzero);
    prof_end(ctx, "batch_byte_split");
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

// The passes of one call on the batched route: the digit image once, then per pass of QB queries the kernel and its finish under
// f32_err_batch_byte.  The last pass may be ragged: its padding queries nominate nothing and no list of theirs is read.
int launch_batch_byte(smt_ctx *ctx, const SlabSearch &a)
{
    SMT_REQUIRE(a.row_dtype == SMT_ROWS_I8 && a.dim == SMT_DIM, "byte batch: byte rows of 256");
    uint32_t kp;
    uint64_t n_tiles;
    int blocks;
    batch_shape(ctx, a, kp, n_tiles, blocks);
    const uint32_t nq_pad = (a.nq + BB_QB - 1) / BB_QB * BB_QB;
    BatchScratch s;
    int rc = batch_scratch(ctx, a.dim, nq_pad, (size_t)BB_QB * blocks * kp, s);   // (the image takes 768 of the 1 KiB a query has there)
    if (rc) return rc;
    if ((rc = batch_byte_split(ctx, a, nq_pad, s.split, s.qzero))) return rc;
    for (uint32_t q0 = 0; q0 < a.nq; q0 += BB_QB) {
        const uint32_t nq_pass = std::min<uint32_t>(BB_QB, a.nq - q0);
        if ((rc = batch_byte_pass(ctx, a, s.split, s.qzero, q0, nq_pass, kp, n_tiles, blocks, s.lists))) return rc;
        if ((rc = launch_finish_slab(ctx, a, s.lists, (uint32_t)blocks, kp, q0, nq_pass, f32_err_batch_byte))) return rc;
    }
    return SMT_OK;
}

// Test hook (smt_debug_batch_byte_lists): the production split and the passes of a.nq queries, no finish (batch_list.h)
int debug_batch_byte_lists(smt_ctx *ctx, const SlabSearch &a, key_t64 *out_keys_host, uint64_t out_cap_keys, uint32_t *out_blocks,
                           uint32_t *out_kp)
{
    SMT_REQUIRE(a.row_dtype == SMT_ROWS_I8 && a.dim == SMT_DIM, "byte batch: byte rows of 256");
    return debug_batch_lists(
        ctx, a, BB_QB, [&](uint32_t nq_pad, const BatchScratch &s) { return batch_byte_split(ctx, a, nq_pad, s.split, s.qzero); },
        [&](const BatchScratch &s, uint32_t q0, uint32_t nq_pass, uint32_t kp, uint64_t n_tiles, int blocks, key_t64 *lists) {
            return batch_byte_pass(ctx, a, s.split, s.qzero, q0, nq_pass, kp, n_tiles, blocks, lists);
        },
        out_keys_host, out_cap_keys, out_blocks, out_kp);
}

}  // namespace smt
