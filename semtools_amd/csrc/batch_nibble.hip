// batch_nibble.hip -- NIBBLE rows (256 signed 4-bit integers, 128 B, no scale), many queries per corpus pass on the int8 MFMA pipe:
// batch_nibble_split_kernel (the queries' digit image, once per call), batch_nibble_kernel<FILTERED> (one streaming pass for up to
// QB = 128 queries) and the launch of a call's passes, each followed by finish_slab_kernel under f32_err_batch_nibble
// (nibble_rows.h).  The frame -- 512 threads, a wave owns a TILE of 32 consecutive rows (filtered: 8 entries of the chunk table),
// tiles dealt round robin, the lists, the epilogue -- is batch_list.h's, shared with batch_slab.hip, batch_half.hip and
// batch_byte.hip.  gfx950 has no int4 MFMA, so the rows become int8 operands in registers; what differs from the byte kernel is
// everything in front of the MFMAs: the load takes EIGHT rows, the transpose moves PACKED rows in one slice, the unpack needs no
// sign extension, and the query image is written in the order the unpack leaves the rows in.
//
// THE OPERAND WITHOUT SIGN EXTENSION.  A stored byte b holds element e0 in its low and e1 in its high nibble (nibble_rows.h).
// (b << 4) & 0xF0, read as int8, is 16 e0: the nibble's sign bit lands on the byte's.  b & 0xF0 is 16 e1.  On a packed dword P of
// eight elements, (P << 4) & 0xF0F0F0F0 is the int8 operand dword of the four EVEN elements times 16 and P & 0xF0F0F0F0 that of the
// four ODD ones: a shift and two ands, THREE vector instructions for two operand dwords, no per-byte arithmetic shift.  -8, which an
// adopted corpus may hold, gives -128, an int8 like any other.  The 16 is a power of two and leaves through the scale exactly.
//
// THE QUERY AS DIGITS is batch_byte.hip's: n_i = rint(u_i 2^22), n = 65536 d0 + 256 d1 + d2 balanced base 256, |d0| <= 64, one
// int8 plane and one i32 accumulator per digit.  RECOUNTED for operands 16 c: |A_d| <= 256 dimensions x 128 (|digit|) x 128
// (16 x |-8|) = 2^22, the byte route's figure: no MFMA result is rounded and each converts to f32 exactly.  score = (65536 A0 +
// 256 A1 + A2) x 2^-26 / |c|: two fused multiply-adds, then batch_list.h's epilogue with rxj = 2^-26 / |c| (2^-22 for the query's
// scale, 2^-4 for the 16).  |c|^2 is an exact integer, at most 256 x 64 = 2^14, by v_dot8_i32_i4 on the PACKED registers
// (16 instructions a lane, as scan_nibble.hip squares its dwords), one rsqrt.  f32_err_batch_nibble counts what is left.
//
// THE QUERY IMAGE FOLLOWS THE ROWS.  The K order of an MFMA is free as long as both operands agree.  A 16-byte packed unit u of a
// row holds the 32 elements 32 u .. + 31 and unpacks into TWO operand units of 16: byte 4 w + i of the even one is element
// 32 u + 8 w + 2 i, of the odd one element 32 u + 8 w + 2 i + 1.  Lane (j, h) of the MFMA holds the packed units 2 g + h, g = 0 .. 3,
// of row j; K-step m = 2 g + p takes the even (p = 0) or odd (p = 1) operand of unit 2 g + h from lane (j, h).  So in a query's
// image, plane d = 16-byte units 16 d .. + 15 as in the byte kernel, unit 2 m + h of a plane holds in byte 4 w + i the digit of
// dimension 32 (2 g + h) + 8 w + 2 i + p.  batch_nibble_split_kernel writes that: a lane has four consecutive dimensions, its even
// two and its odd two are each HALF an image word, and one exchange with the neighbouring lane completes a word per lane and
// plane.  No byte is shuffled on the row side.  The byte split is not shared: it would have to change to take an order.
//
// QUERIES IN LDS: batch_byte.hip's layout, 768 B a query, rows BN_QSTRIDE = 49 units apart, QB = 128: 100,352 bytes of queries,
// 36,864 of transpose buffers, 1,552 of thresholds, locks and masks -- 138,768 of the 160 KiB.
//
// ROWS.  One global_load_dwordx4 of a wave reads 1 KiB: EIGHT whole rows, lane l the unit l % 8 of row l / 8 of the eight
// (scan_nibble.hip's load); FOUR of them are a tile, 16 VGPRs in LOAD layout where the byte kernel has 32.  They reach lane (j, h)
// through the wave's buffer of 32 rows x 144 B (128 used; 9 units: the 16 lanes of a read fall into 16 different units), still
// PACKED and in ONE slice, since a whole row is 128 B: four full-occupancy ds_write_b128 and four ds_read_b128 a tile -- half the
// bytes of the byte kernel's 16 half-occupied writes and 8 reads.  The next tile's four loads are issued once the load registers
// are free: before anything is unpacked or multiplied.  COUNTED: the unpack is 16 packed dwords x 3 = 48 vector instructions a
// tile into the 32 resident operand VGPRs, against 96 MFMAs of 16 passes each for a full pass.
//
// THE LOOP, PRODUCTS, EPILOGUE are batch_byte.hip's: rows resident, the four query tiles pass by one at a time, 24 ds_read_b128
// and 24 v_mfma_i32_32x32x32_i8 each, digits the first operand and rows the second, tiles a ragged pass does not have skipped
// wave-uniformly, batch_tile_nominate<1> per query tile with its pointers advanced.
//
// BUILD (gfx950, from the resource report; profiles/nibble_batch.json repeats it): 170 / 172 VGPRs (unfiltered / filtered) where the
// byte kernel has 206 / 202, no AGPRs, no scratch, 138,768 bytes of dynamic LDS a block; the split kernel 17 VGPRs, no scratch.
// In the unfiltered kernel's code: 96 v_mfma_i32_32x32x32_i8 and 96 + 4 ds_read_b128 (four query tiles, the transpose), 4 + 1
// ds_write_b128, 4 + 4 + 1 global_load_dwordx4 (first tile, next tile, the query image), 16 v_dot8_i32_i4.
//
// MEASURED (tools/nibble_batch_rate.py, profiles/nibble_batch.json, 1 GiB of nibble rows = 8 Mi rows, device form, top_k 10, medians
// of nine alternating rounds, ms per call against the scan's passes of four): 4 queries 0.377 / 0.504, 5: 0.389 / 0.699, 6: 0.403 /
// 0.953, 8: 0.431 / 1.005, 16: 0.537 / 2.01, 32: 0.752 / 4.02, 128: 2.45 / 16.1, 1000: 19.5 / 125.7 (6.5 times); every cell wins
// beyond both spreads and the answers are the same bytes in every cell, so nibble_batch_min ships at 4.  The kernel streams rows at
// 2.87 TB/s (22.4 G rows/s) with 4 queries and at 0.45 TB/s (3.5 G rows/s) with a full pass.  A full pass over 8 Mi rows takes
// 2.45 ms [2.44, 2.47] where the byte route takes 2.58 ms [2.56, 2.60] over the same number of rows in the same process: x 0.95,
// the MFMA work being equal.  SUPPOSED, no counter run: the unpack and the packed one-slice transpose cost less than the byte
// kernel's two-slice transpose and its second GiB of rows.  The largest |nominated - f64| the list tests saw is 2.95e-7 against the derived 3.49e-6.  NOT measured: what holds a
// full pass (no counter run); |c|^2 by v_dot4 on the operands instead of v_dot8 on the packed registers; the loop rolled.  NOT
// built: a direct-load form without the LDS transpose, QB above 128, the f8f6f4 MFMA formats.
#include "nibble_rows.h"
#include "batch_list.h"

namespace smt {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int BN_QB = 128;
constexpr int BN_QWORDS = 192;        // words of a query's image: three planes of 256 digits
constexpr int BN_QSTRIDE = 49;        // 16-byte units between queries in LDS (48 used)
constexpr int BN_TROW = 144;          // bytes per row in the transpose buffer (128 used: a whole packed row)
constexpr int BN_TBUF = 32 * BN_TROW; // per wave
constexpr float BN_QUERY_SCALE = 4194304.0f;            // 2^22
constexpr float BN_INV_SCALE = 1.0f / 67108864.0f;      // 2^-26: the query's 2^22 and the operands' 16
constexpr uint32_t BN_HIGH_NIBBLES = 0xF0F0F0F0u;

struct BatchNibbleParams {
    const void *corpus;            // [n_rows][128] bytes, two elements each
    uint64_t n_rows;
    const uint32_t *split;         // the pass' first query: [QB][192] words (batch_nibble_split_kernel)
    const uint32_t *qzero;         // the pass' first query: 1 = zero query or outside the domain
    uint32_t nq_active;            // 1 .. QB
    uint32_t kp;
    const uint64_t *chunk_table;   // FILTERED
    uint64_t n_chunks;
    uint64_t n_tiles;
    key_t64 *block_lists;          // [nq_active][gridDim.x][kp]
};

// One wave per query (padding queries included: zero operands).  rint(2^22 q / |q|) in three balanced base-256 digits, the
// arithmetic, the zero and domain handling and the qzero flags batch_byte_split_kernel's; the ORDER is the unpacked rows' (header:
// the query image follows the rows).  Lane L has dimensions 4 L .. + 3 = elements 4 (L & 1) .. + 3 of packed dword L / 2; image
// word (dword L / 2, parity L & 1) is written by lane L: its low half from the even lane of the pair, its high half from the odd.
__global__ void __launch_bounds__(256) batch_nibble_split_kernel(const float *queries, uint32_t nq, uint32_t nq_pad, uint32_t *split, uint32_t *qzero)
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
    uint32_t hw[3][2] = {{0u, 0u}, {0u, 0u}, {0u, 0u}};   // [plane][parity]: the lane's two even resp. odd dimensions, a byte each
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float u = zero ? 0.0f : v[i] * rq;            // the unit query's component, one rounding
        const int n = (int)rintf(u * BN_QUERY_SCALE);       // (the power of two is exact)
        const int d2 = ((n + 128) & 255) - 128, n1 = (n - d2) >> 8;
        const int d1 = ((n1 + 128) & 255) - 128, d0 = (n1 - d1) >> 8;
        const int sh = 8 * (i >> 1);
        hw[0][i & 1] |= (uint32_t)(d0 & 255) << sh;
        hw[1][i & 1] |= (uint32_t)(d1 & 255) << sh;
        hw[2][i & 1] |= (uint32_t)(d2 & 255) << sh;
    }
    const int p = lane & 1;                       // the parity this lane's word holds
    const int dw = lane >> 1;                     // packed dword of the row: unit dw / 4 = 2 g + h, dword dw % 4 of it
    const int unit = dw >> 2, g = unit >> 1, h = unit & 1;
    uint32_t *dst = split + (size_t)q * BN_QWORDS + 4 * (2 * (2 * g + p) + h) + (dw & 3);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const uint32_t got = (uint32_t)__shfl_xor((int)(p ? hw[d][0] : hw[d][1]), 1);   // each lane sends the half its neighbour's word lacks
        dst[64 * d] = p ? (got | hw[d][1] << 16) : (hw[d][0] | got << 16);
    }
    if (lane == 0) qzero[q] = zero ? 1u : 0u;
}

template <bool FILTERED>
__global__ void __launch_bounds__(BS_THREADS, 2) batch_nibble_kernel(BatchNibbleParams p)
{
    constexpr int QB = BN_QB;
    constexpr int ROW_Q = 8;         // 16-byte units per corpus row
    constexpr int LOADS = 4;         // load instructions of a tile, eight rows each; filtered: two chunk-table entries each
    static_assert(FILTER_CHUNK == 4, "an entry of the chunk table is half a load");
    extern __shared__ __attribute__((aligned(16))) unsigned char bn_smem[];
    u32x4 *s_q = reinterpret_cast<u32x4 *>(bn_smem);                                   // [QB][49] units
    unsigned char *s_t = bn_smem + (size_t)QB * BN_QSTRIDE * 16;                        // [waves][BN_TBUF]
    key_t64 *s_thr = reinterpret_cast<key_t64 *>(s_t + BS_WAVES * BN_TBUF);             // [QB]
    unsigned int *s_lock = reinterpret_cast<unsigned int *>(s_thr + QB);               // [QB]
    unsigned int *s_qz = s_lock + QB;                                                  // [QB / 32] masks of zero queries

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, j = lane & 31;
    const int kp = (int)p.kp;
    const int nt_active = (int)((p.nq_active + 31) / 32);
    unsigned char *tbuf = s_t + wave * BN_TBUF;

    // ---- the pass' operands, thresholds, locks and empty lists
    if (lane < 3 * 16)
        for (int r = wave; r < QB; r += BS_WAVES) s_q[r * BN_QSTRIDE + lane] = reinterpret_cast<const u32x4 *>(p.split + (size_t)r * BN_QWORDS)[lane];
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
    // load view: instruction i reads tile rows 8 i .. + 7, lane l unit l % 8 of row 8 i + l / 8
    auto issue = [&](uint64_t t, u32x4 (&R)[LOADS]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < LOADS; ++i)
            R[i] = __builtin_nontemporal_load(corpus4 + row_of(t, (uint32_t)(8 * i + (lane >> 3))) * ROW_Q + (lane & 7));
    };
    const uint32_t t_wr = (uint32_t)((lane >> 3) * BN_TROW + (lane & 7) * 16);
    const uint32_t t_rd = (uint32_t)(j * BN_TROW + h * 16);
    const u32x4 *aq = s_q + j * BN_QSTRIDE + h;   // this lane's digits of query j of a tile: unit 16 d + 2 m (+ h)

    u32x4 R[LOADS];
    if (tile < p.n_tiles) issue(tile, R);
    while (tile < p.n_tiles) {
        // ---- load layout -> lane (j, h), packed, the whole row in one slice through the wave's buffer
        u32x4 P[4];
        wave_lds_sync();   // (the reads of the tile before are done)
#pragma unroll
        for (int i = 0; i < LOADS; ++i) *reinterpret_cast<u32x4 *>(tbuf + t_wr + i * 8 * BN_TROW) = R[i];
        wave_lds_sync();   // (other lanes wrote what this one reads)
#pragma unroll
        for (int g = 0; g < 4; ++g) P[g] = *reinterpret_cast<const u32x4 *>(tbuf + t_rd + 32 * g);
        // ---- the next tile is requested before this one is unpacked
        const uint64_t tile_next = tile + n_waves;
        if (tile_next < p.n_tiles) issue(tile_next, R);

        // ---- 2^-26 / |c| of row j into lane (j, .): an exact integer sum over the packed dwords, one rsqrt
        int c2 = 0;
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int w = 0; w < 4; ++w) c2 = __builtin_amdgcn_sdot8((int)P[g][w], (int)P[g][w], c2, false);
        c2 += __shfl_xor(c2, 32);
        const float rxj = c2 == 0 ? 0.0f : __frsqrt_rn((float)c2);
        // ---- packed -> operands, 16 x the elements: K-step 2 g the even, 2 g + 1 the odd elements of unit 2 g + h
        u32x4 X[8];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            X[2 * g] = (P[g] << 4) & BN_HIGH_NIBBLES;
            X[2 * g + 1] = P[g] & BN_HIGH_NIBBLES;
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

        // ---- the query tiles pass by the resident rows one at a time
#pragma unroll
        for (int t = 0; t < QB / 32; ++t) {
            if (t >= nt_active) break;   // (wave-uniform)
            const u32x4 *at = aq + t * 32 * BN_QSTRIDE;
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
            batch_tile_nominate<1>(acc, 1, rxj * BN_INV_SCALE, c2 == 0, rowj, validj, s_qz + t, s_thr + 32 * t, s_lock + 32 * t,
                                   p.block_lists + (size_t)32 * t * gridDim.x * kp, kp, lane);
        }
        tile = tile_next;
    }
}

static size_t batch_nibble_smem() { return (size_t)BN_QB * BN_QSTRIDE * 16 + (size_t)BS_WAVES * BN_TBUF + (size_t)BN_QB * 12 + 16; }
uint32_t nibble_batch_qb() { return (uint32_t)BN_QB; }

// one pass: the queries [q0, q0 + nq_pass) of `a` into lists [nq_pass][blocks][kp]
static int batch_nibble_pass(smt_ctx *ctx, const SlabSearch &a, const uint32_t *split, const uint32_t *qzero, uint32_t q0, uint32_t nq_pass,
                             uint32_t kp, uint64_t n_tiles, int blocks, key_t64 *lists)
{
    const bool filtered = a.chunk_table != nullptr;
    if (!(ctx->attr_done & ATTR_BATCH_NIBBLE)) {
        SMT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(batch_nibble_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        SMT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(batch_nibble_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        ctx->attr_done |= ATTR_BATCH_NIBBLE;
    }
    BatchNibbleParams p;
    p.corpus = a.corpus;
    p.n_rows = a.rows;
    p.split = split + (size_t)q0 * BN_QWORDS;
    p.qzero = qzero + q0;
    p.nq_active = nq_pass;
    p.kp = kp;
    p.chunk_table = a.chunk_table;
    p.n_chunks = a.n_chunks;
    p.n_tiles = n_tiles;
    p.block_lists = lists;
    prof_begin(ctx, "batch_nibble");
    hipLaunchKernelGGL(filtered ? batch_nibble_kernel<true> : batch_nibble_kernel<false>, dim3(blocks), dim3(BS_THREADS), batch_nibble_smem(), ctx->stream, p);
    prof_end(ctx, "batch_nibble");
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

static int batch_nibble_split(smt_ctx *ctx, const SlabSearch &a, uint32_t nq_pad, uint32_t *split, uint32_t *qzero)
{
    prof_begin(ctx, "batch_nibble_split");
    hipLaunchKernelGGL(batch_nibble_split_kernel, dim3((nq_pad + 3) / 4), dim3(256), 0, ctx->stream, a.queries, a.nq, nq_pad, split, qzero);
    prof_end(ctx, "batch_nibble_split");
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

// The passes of one call on the batched route: the digit image once, then per pass of QB queries the kernel and its finish under
// f32_err_batch_nibble.  The last pass may be ragged: its padding queries nominate nothing and no list of theirs is read.
int launch_batch_nibble(smt_ctx *ctx, const SlabSearch &a)
{
    SMT_REQUIRE(a.row_dtype == SMT_ROWS_I4 && a.dim == SMT_DIM, "nibble batch: nibble rows of 256");
    uint32_t kp;
    uint64_t n_tiles;
    int blocks;
    batch_shape(ctx, a, kp, n_tiles, blocks);
    const uint32_t nq_pad = (a.nq + BN_QB - 1) / BN_QB * BN_QB;
    BatchScratch s;
    int rc = batch_scratch(ctx, a.dim, nq_pad, (size_t)BN_QB * blocks * kp, s);   // (the image takes 768 of the 1 KiB a query has there)
    if (rc) return rc;
    if ((rc = batch_nibble_split(ctx, a, nq_pad, s.split, s.qzero))) return rc;
    for (uint32_t q0 = 0; q0 < a.nq; q0 += BN_QB) {
        const uint32_t nq_pass = std::min<uint32_t>(BN_QB, a.nq - q0);
        if ((rc = batch_nibble_pass(ctx, a, s.split, s.qzero, q0, nq_pass, kp, n_tiles, blocks, s.lists))) return rc;
        if ((rc = launch_finish_slab(ctx, a, s.lists, (uint32_t)blocks, kp, q0, nq_pass, f32_err_batch_nibble))) return rc;
    }
    return SMT_OK;
}

// Test hook (smt_debug_batch_nibble_lists): the production split and the passes of a.nq queries, no finish (batch_list.h)
int debug_batch_nibble_lists(smt_ctx *ctx, const SlabSearch &a, key_t64 *out_keys_host, uint64_t out_cap_keys, uint32_t *out_blocks,
                             uint32_t *out_kp)
{
    SMT_REQUIRE(a.row_dtype == SMT_ROWS_I4 && a.dim == SMT_DIM, "nibble batch: nibble rows of 256");
    return debug_batch_lists(
        ctx, a, BN_QB, [&](uint32_t nq_pad, const BatchScratch &s) { return batch_nibble_split(ctx, a, nq_pad, s.split, s.qzero); },
        [&](const BatchScratch &s, uint32_t q0, uint32_t nq_pass, uint32_t kp, uint64_t n_tiles, int blocks, key_t64 *lists) {
            return batch_nibble_pass(ctx, a, s.split, s.qzero, q0, nq_pass, kp, n_tiles, blocks, lists);
        },
        out_keys_host, out_cap_keys, out_blocks, out_kp);
}

}  // namespace smt
