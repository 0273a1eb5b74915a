// finish_slab.hip -- the finish stage of a WIDE scan (scan_slab.hip) and the exhaustive re-answer's kernel.
//
// finish_slab_kernel<D, RowT>, one block per query: merges the query's block lists, recomputes every surviving candidate's distance in f64
// in index order over all D components (D = 256 S, or 64: narrow rows, scan_narrow.hip, certified under f32_err_narrow) (simsimd's accurate form, oracle cosine_accurate), orders by (f64 distance, row),
// writes rows (+ row_base), distances, the count and the status word.
//
// MERGE.  The lists are sorted and their keys distinct, so the k'-th smallest of the lists' HEADS bounds the union's k'-th smallest
// key from above once k' lists are non-empty (k' lists hold a key that small).  Exactly k' lists then start at or under it, each
// with at most k' keys: at most k'^2 <= 4096 survivors, fewer lists than k' hold fewer keys than that in all.  The survivors are
// sorted in LDS (bitonic) and the first k' kept.
// RESCORE.  Candidate rows are staged in LDS a tile at a time (min(16, 8192 / D) rows of D floats, one wave per row, coalesced); one thread
// per candidate and sum then runs the D dependent f64 adds from LDS: <q, c> in wave 0, <c, c> in wave 1, <q, q> once in wave 2.
// The product of two f32 values is exact in f64, so a fused multiply-add rounds like the oracle's multiply and add.
// CERTIFICATE.  As select.hip's: when k' keys were nominated, a row outside them has scan distance >= the k'-th key's, hence exact
// distance >= that - f32_err_slab(S) (wide_rows.h); the answer is PROVED when the k_out-th exact distance lies under that floor.
// Fewer than k' nominated keys are all the rows there are: proved.  A query outside the domain: SMT_STATUS_INVALID_QUERY.
// HALF rows (half_rows.h) come here as <256, _Float16>: the row read widens the stored halves -- exactly, in integer arithmetic -- on
// their way into LDS or the sums, everything behind it is the f32 code; the bound is f32_err_half.  BYTE rows (byte_rows.h) come
// as <256, int8_t>: sign extension and an integer conversion, exact as well; the bound is f32_err_byte.  NIBBLE rows (nibble_rows.h)
// come as <256, nibble_t>: four components are two bytes, a shift pair sign-extends each nibble, an integer conversion follows --
// exact again; the bound is f32_err_nibble.
#include <type_traits>

#include "nibble_rows.h"
#include "device_utils.h"

namespace smt {

struct SlabFinishParams {
    const float *corpus;
    const float *queries;      // the pass' first query
    const key_t64 *lists;      // [queries of the pass][n_lists][kp]
    uint32_t n_lists, kp, k_out;
    uint64_t row_base;
    uint64_t *out_rows;        // the pass' first query's list, [.][k_out]
    double *out_dist;
    uint64_t *out_counts;      // or nullptr
    uint32_t *out_status;      // or nullptr
    double f32_err;
    unsigned long long *sticky;   // the context's count of answers that are not PROVED
};

constexpr int FIN_THREADS = 1024;
constexpr int FIN_SURV_CAP = 4096;   // k'^2 at k' = 64

// four components of a stored row, widened: e counts float4 (f32 rows) resp. groups of four halves, four bytes or four nibbles
template <typename RowT>
__device__ __forceinline__ f32x4 row_quad(const float *rows, uint64_t row, uint32_t dim, uint32_t e)
{
    if constexpr (std::is_same_v<RowT, nibble_t>) {
        const uint32_t w = reinterpret_cast<const uint16_t *>(reinterpret_cast<const uint8_t *>(rows) + row * (dim / 2))[e];
        f32x4 v;
        v.x = (float)((int)(w << 28) >> 28);
        v.y = (float)((int)(w << 24) >> 28);
        v.z = (float)((int)(w << 20) >> 28);
        v.w = (float)((int)(w << 16) >> 28);
        return v;
    } else if constexpr (sizeof(RowT) == 4) {
        return reinterpret_cast<const f32x4 *>(rows + row * dim)[e];
    } else if constexpr (sizeof(RowT) == 1) {
        const uint32_t w = reinterpret_cast<const uint32_t *>(reinterpret_cast<const int8_t *>(rows) + row * dim)[e];
        f32x4 v;
        v.x = (float)(int8_t)w;
        v.y = (float)(int8_t)(w >> 8);
        v.z = (float)(int8_t)(w >> 16);
        v.w = (float)(int8_t)(w >> 24);
        return v;
    } else {
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        const u32x2 h = reinterpret_cast<const u32x2 *>(reinterpret_cast<const uint16_t *>(rows) + row * dim)[e];
        f32x4 v;
        v.x = f32_from_half_bits((uint16_t)h.x);
        v.y = f32_from_half_bits((uint16_t)(h.x >> 16));
        v.z = f32_from_half_bits((uint16_t)h.y);
        v.w = f32_from_half_bits((uint16_t)(h.y >> 16));
        return v;
    }
}

template <int D, typename RowT>
__global__ void __launch_bounds__(FIN_THREADS) finish_slab_kernel(SlabFinishParams p)
{
    static_assert(D == 64 || (D % 256 == 0 && D <= 1024), "64 floats (narrow rows) or 1 .. 4 slabs of 256");
    constexpr int TB = 8192 / D < FIN_THREADS / 64 ? 8192 / D : FIN_THREADS / 64;   // candidate rows staged per tile
    constexpr int RS = D / 4 + 1;         // LDS row stride in float4: neighbouring rows start 16 bytes apart in the banks
    static_assert(TB <= FIN_THREADS / 64 && (size_t)TB * RS * 16 <= (size_t)FIN_SURV_CAP * 8 + 1024, "a wave per staged row; tiles share the survivors' space");
    extern __shared__ __align__(16) unsigned char fin_smem[];
    key_t64 *s_head = reinterpret_cast<key_t64 *>(fin_smem);    // [SLAB_MAX_LISTS]
    key_t64 *s_best = s_head + SLAB_MAX_LISTS;                   // [64]
    double *s_ab = reinterpret_cast<double *>(s_best + 64);      // [64]
    double *s_b2 = s_ab + 64;                                    // [64]
    double *s_d = s_b2 + 64;                                     // [64]
    double *s_a2 = s_d + 64;                                     // [1] (+ pad)
    key_t64 *s_tau = reinterpret_cast<key_t64 *>(s_a2 + 2);      // [1] (+ pad)
    uint32_t *s_r = reinterpret_cast<uint32_t *>(s_tau + 2);     // [64]
    unsigned int *s_rank = s_r + 64;                             // [64]
    unsigned int *s_cnt = s_rank + 64;                           // [0] survivors [1] valid candidates [2] max |q_i| bits
    float *s_q = reinterpret_cast<float *>(s_cnt + 4);           // [D]
    unsigned char *s_big = reinterpret_cast<unsigned char *>(s_q + D);
    key_t64 *s_surv = reinterpret_cast<key_t64 *>(s_big);        // [FIN_SURV_CAP]
    f32x4 *s_rows = reinterpret_cast<f32x4 *>(s_big);            // [TB][RS], once the best k' are known

    const uint32_t qi = blockIdx.x;
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int kp = (int)p.kp, L = (int)p.n_lists;
    const key_t64 *lists = p.lists + (size_t)qi * L * kp;
    const float *query = p.queries + (size_t)qi * D;
    uint64_t *orow = p.out_rows + (size_t)qi * p.k_out;
    double *odist = p.out_dist + (size_t)qi * p.k_out;

    if (t == 0) { *s_tau = KEY_PAD; s_cnt[0] = 0; s_cnt[1] = 0; s_cnt[2] = 0; }
    if (t < 64) { s_best[t] = KEY_PAD; s_rank[t] = 0; }
    for (int i = t; i < L; i += FIN_THREADS) s_head[i] = lists[(size_t)i * kp];
    uint32_t qmax = 0;
    for (int i = t; i < D; i += FIN_THREADS) {
        const float f = query[i];
        s_q[i] = f;
        qmax = max(qmax, __float_as_uint(f) & 0x7fffffffu);
    }
    __syncthreads();
    atomicMax(&s_cnt[2], qmax);
    // tau = the k'-th smallest head
    for (int i = t; i < L; i += FIN_THREADS) {
        const key_t64 h = s_head[i];
        if (h != KEY_PAD) {
            int rank = 0;
            for (int j = 0; j < L; ++j) rank += s_head[j] < h ? 1 : 0;
            if (rank == kp - 1) *s_tau = h;
        }
    }
    __syncthreads();
    const key_t64 tau = *s_tau;
    const int M = L * kp;
    for (int e = t; e < M; e += FIN_THREADS) {
        const key_t64 key = lists[e];
        if (key != KEY_PAD && key <= tau) {
            const unsigned int at = atomicAdd(&s_cnt[0], 1u);
            if (at < (unsigned)FIN_SURV_CAP) s_surv[at] = key;
        }
    }
    __syncthreads();
    const uint32_t n_surv = min(s_cnt[0], (unsigned)FIN_SURV_CAP);
    uint32_t np = 64;
    while (np < n_surv) np <<= 1;
    for (uint32_t i = n_surv + t; i < np; i += FIN_THREADS) s_surv[i] = KEY_PAD;
    __syncthreads();
    bitonic_sort(np, [&](uint32_t a, uint32_t b, bool up) {
        const key_t64 x = s_surv[a], y = s_surv[b];
        if ((x > y) == up && x != y) { s_surv[a] = y; s_surv[b] = x; }
    });
    if (t < kp) s_best[t] = s_surv[t];
    __syncthreads();   // (the survivors are dead from here: the row tiles take their place)

    for (int tile0 = 0; tile0 < kp; tile0 += TB) {
        if (wave < TB && tile0 + wave < kp && s_best[tile0 + wave] != KEY_PAD) {
            const uint32_t row = (uint32_t)(s_best[tile0 + wave] & 0xFFFFFFFFull);
#pragma unroll
            for (int e = lane; e < D / 4; e += 64) s_rows[wave * RS + e] = row_quad<RowT>(p.corpus, row, D, e);   // (a narrow row: lanes 0 .. 15)
        }
        __syncthreads();
        const f32x4 *q4 = reinterpret_cast<const f32x4 *>(s_q);
        if (wave < 2 && lane < TB && tile0 + lane < kp && s_best[tile0 + lane] != KEY_PAD) {
            const f32x4 *r4 = s_rows + lane * RS;
            double acc = 0.0;
            if (wave == 0) {
#pragma unroll 8
                for (int i = 0; i < D / 4; ++i) {
                    const f32x4 a = q4[i], b = r4[i];
                    acc = acc + (double)a.x * (double)b.x;
                    acc = acc + (double)a.y * (double)b.y;
                    acc = acc + (double)a.z * (double)b.z;
                    acc = acc + (double)a.w * (double)b.w;
                }
                s_ab[tile0 + lane] = acc;
            } else {
#pragma unroll 8
                for (int i = 0; i < D / 4; ++i) {
                    const f32x4 b = r4[i];
                    acc = acc + (double)b.x * (double)b.x;
                    acc = acc + (double)b.y * (double)b.y;
                    acc = acc + (double)b.z * (double)b.z;
                    acc = acc + (double)b.w * (double)b.w;
                }
                s_b2[tile0 + lane] = acc;
            }
        } else if (t == 128 && tile0 == 0) {
            double acc = 0.0;
#pragma unroll 8
            for (int i = 0; i < D / 4; ++i) {
                const f32x4 a = q4[i];
                acc = acc + (double)a.x * (double)a.x;
                acc = acc + (double)a.y * (double)a.y;
                acc = acc + (double)a.z * (double)a.z;
                acc = acc + (double)a.w * (double)a.w;
            }
            *s_a2 = acc;
        }
        __syncthreads();
    }

    if (t < kp) {
        double d = __builtin_inf();
        uint32_t r = 0xFFFFFFFFu;
        if (s_best[t] != KEY_PAD) {
            r = (uint32_t)(s_best[t] & 0xFFFFFFFFull);
            d = cos_finish_exact(s_ab[t], *s_a2, s_b2[t]);
            atomicAdd(&s_cnt[1], 1u);
        }
        s_d[t] = d;
        s_r[t] = r;
    }
    if (t < (int)p.k_out) { orow[t] = 0xFFFFFFFFFFFFFFFFull; odist[t] = __builtin_inf(); }
    if (t == 0 && p.out_status) p.out_status[qi] = 0u;
    __syncthreads();
    for (int pr = t; pr < kp * kp; pr += FIN_THREADS) {
        const int i = pr / kp, j = pr - i * kp;
        const uint32_t ri = s_r[i], rj = s_r[j];
        if (ri != 0xFFFFFFFFu && rj != 0xFFFFFFFFu) {
            const double di = s_d[i], dj = s_d[j];
            if (dj < di || (dj == di && rj < ri)) atomicAdd(&s_rank[i], 1u);
        }
    }
    __syncthreads();
    const bool mine = t < kp && s_r[t] != 0xFFFFFFFFu;
    if (mine && s_rank[t] < p.k_out) { orow[s_rank[t]] = p.row_base + s_r[t]; odist[s_rank[t]] = s_d[t]; }
    unsigned int code = 0u;   // of the one thread that decides
    if (!magnitude_in_domain(s_cnt[2])) {
        if (t == 0) code = 3u;   // SMT_STATUS_INVALID_QUERY: the list means nothing
    } else if (p.f32_err > 0.0 && L > 0 && s_best[kp - 1] != KEY_PAD) {
        // k' keys nominated (so k' >= k_out valid candidates): the owner of the k_out-th result compares it with the floor of the rest
        const double floor_out = (double)__uint_as_float((unsigned)(s_best[kp - 1] >> 32)) - p.f32_err;
        if (mine && s_rank[t] == p.k_out - 1 && !(floor_out > s_d[t])) code = 1u;   // SMT_STATUS_UNCERTAIN
    }
    if (code) {
        if (p.out_status) p.out_status[qi] = code;
        if (p.sticky) atomicAdd(p.sticky, 1ull);
    }
    if (t == 0 && p.out_counts) p.out_counts[qi] = s_cnt[1] < p.k_out ? s_cnt[1] : p.k_out;
}

static size_t finish_smem_bytes(uint32_t dim)
{
    return (size_t)SLAB_MAX_LISTS * 8 + 64 * 8 * 4 + 16 + 16 + 64 * 4 * 2 + 16 + (size_t)dim * 4 + (size_t)FIN_SURV_CAP * 8 + 1024;
}

int launch_finish_slab(smt_ctx *ctx, const SlabSearch &a, const key_t64 *lists, uint32_t n_lists, uint32_t kp, uint32_t first_query,
                       uint32_t nq_pass, double f32_err)
{
    SMT_REQUIRE(n_lists <= (uint32_t)SLAB_MAX_LISTS && kp >= a.k_out && kp <= 64 && nq_pass >= 1, "wide finish: <= 256 lists, k_out <= k' <= 64");
    const bool half = a.row_dtype == SMT_ROWS_F16, byte = a.row_dtype == SMT_ROWS_I8, nibble = a.row_dtype == SMT_ROWS_I4;
    SlabFinishParams p;
    p.corpus = a.corpus;
    p.queries = a.queries + (size_t)first_query * a.dim;
    p.lists = lists;
    p.n_lists = n_lists;
    p.kp = kp;
    p.k_out = a.k_out;
    p.row_base = a.row_base;
    p.out_rows = a.out_rows + (size_t)first_query * a.k_out;
    p.out_dist = a.out_dist + (size_t)first_query * a.k_out;
    p.out_counts = a.out_counts ? a.out_counts + first_query : nullptr;
    p.out_status = a.out_status ? a.out_status + first_query : nullptr;
    const int S = (int)(a.dim / 256);
    const bool narrow = dim_is_narrow(a.dim);
    p.f32_err = f32_err > 0.0 ? f32_err : nibble ? f32_err_nibble : byte ? f32_err_byte : half ? f32_err_half : narrow ? f32_err_narrow : S == 2 ? f32_err_slab(2) : S == 3 ? f32_err_slab(3) : f32_err_slab(4);
    p.sticky = ctx->d_status;
    const size_t smem = finish_smem_bytes(a.dim);
    prof_begin(ctx, "finish_slab");
    if (nibble) hipLaunchKernelGGL((finish_slab_kernel<256, nibble_t>), dim3(nq_pass), dim3(FIN_THREADS), smem, ctx->stream, p);
    else if (byte) hipLaunchKernelGGL((finish_slab_kernel<256, int8_t>), dim3(nq_pass), dim3(FIN_THREADS), smem, ctx->stream, p);
    else if (half) hipLaunchKernelGGL((finish_slab_kernel<256, _Float16>), dim3(nq_pass), dim3(FIN_THREADS), smem, ctx->stream, p);
    else if (narrow) hipLaunchKernelGGL((finish_slab_kernel<64, float>), dim3(nq_pass), dim3(FIN_THREADS), smem, ctx->stream, p);
    else if (S == 2) hipLaunchKernelGGL((finish_slab_kernel<512, float>), dim3(nq_pass), dim3(FIN_THREADS), smem, ctx->stream, p);
    else if (S == 3) hipLaunchKernelGGL((finish_slab_kernel<768, float>), dim3(nq_pass), dim3(FIN_THREADS), smem, ctx->stream, p);
    else hipLaunchKernelGGL((finish_slab_kernel<1024, float>), dim3(nq_pass), dim3(FIN_THREADS), smem, ctx->stream, p);
    prof_end(ctx, "finish_slab");
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

// The exhaustive re-answer (search_slab.cpp): the exact f64 distance of EVERY allowed row, one thread per row walking its D components
// in index order; the host then selects by (distance, row).  Slow (a thread's loads are its own row's: nothing coalesces), rare --
// only a query whose certificate failed comes here -- and correct.
// NARROW rows: the same sums, but a thread that walked its own 256-byte row would make a wave touch 64 rows 16 B at a time.  Here a
// wave load reads 1 KiB -- RPL = four rows (resp. the rows of one chunk-table entry), lane l float4 number l % 16 of row l / 16, the
// scan's geometry -- into LDS, a block stages its 128 slots so, and thread t then walks slot t's 64 components from LDS in index
// order.  Slot i is what it is in exact_all_slab_kernel; rows that do not exist are read as a row that does and not written.
template <int RPL>
__global__ void __launch_bounds__(128) exact_all_narrow_kernel(const float *corpus, uint64_t n_rows, const float *query,
                                                               const uint64_t *chunk_table, uint64_t n_chunks, double *out)
{
    static_assert(RPL == 4 && FILTER_CHUNK == RPL, "four rows per 1 KiB load; a chunk-table entry is one load");
    constexpr int D = 256 / RPL, LPR = 64 / RPL, SLOTS = 128, RS = D / 4 + 1;   // (stride 17 float4: neighbouring slots 16 B apart in the banks)
    __shared__ f32x4 s_rows[SLOTS * RS];
    __shared__ f32x4 s_q[D / 4];
    __shared__ unsigned char s_ok[SLOTS];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, grp = lane / LPR, sub = lane % LPR;
    if (t < D / 4) s_q[t] = reinterpret_cast<const f32x4 *>(query)[t];
    const uint64_t slot0 = (uint64_t)blockIdx.x * SLOTS;
    for (int l = wave; l < SLOTS / RPL; l += 2) {   // load l of the block: slots 4 l .. 4 l + 3
        const uint64_t i = slot0 + (uint64_t)l * RPL + grp;
        uint64_t row = 0;
        bool ok;
        if (chunk_table) {
            const uint64_t c = i / FILTER_CHUNK;
            const uint64_t desc = c < n_chunks ? chunk_table[c] : 0ull;
            ok = (uint32_t)grp < (uint32_t)(desc >> 32);
            row = (desc & 0xFFFFFFFFull) + (ok ? grp : 0);
        } else {
            ok = i < n_rows;
            row = ok ? i : n_rows - 1;
        }
        s_rows[(l * RPL + grp) * RS + sub] = reinterpret_cast<const f32x4 *>(corpus + row * D)[sub];
        if (sub == 0) s_ok[l * RPL + grp] = ok ? 1 : 0;
    }
    __syncthreads();
    if (!s_ok[t]) return;
    const f32x4 *r4 = s_rows + t * RS;
    double ab = 0.0, a2 = 0.0, b2 = 0.0;
#pragma unroll 4
    for (int e = 0; e < D / 4; ++e) {
        const f32x4 a = s_q[e], b = r4[e];
        const double ax = a.x, ay = a.y, az = a.z, aw = a.w, bx = b.x, by = b.y, bz = b.z, bw = b.w;
        ab = ab + ax * bx; a2 = a2 + ax * ax; b2 = b2 + bx * bx;
        ab = ab + ay * by; a2 = a2 + ay * ay; b2 = b2 + by * by;
        ab = ab + az * bz; a2 = a2 + az * az; b2 = b2 + bz * bz;
        ab = ab + aw * bw; a2 = a2 + aw * aw; b2 = b2 + bw * bw;
    }
    out[slot0 + t] = cos_finish_exact(ab, a2, b2);
}

template <typename RowT>
__global__ void __launch_bounds__(256) exact_all_slab_kernel(const float *corpus, uint64_t n_rows, uint32_t dim, const float *query,
                                                             const uint64_t *chunk_table, uint64_t n_chunks, double *out)
{
    __shared__ __align__(16) float s_q[1024];
    for (uint32_t i = threadIdx.x; i < dim; i += blockDim.x) s_q[i] = query[i];
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t row;
    if (chunk_table) {
        const uint64_t c = i / FILTER_CHUNK;
        if (c >= n_chunks) return;
        const uint64_t desc = chunk_table[c];
        const uint32_t j = (uint32_t)(i % FILTER_CHUNK);
        if (j >= (uint32_t)(desc >> 32)) return;
        row = (desc & 0xFFFFFFFFull) + j;
    } else {
        if (i >= n_rows) return;
        row = i;
    }
    const f32x4 *q4 = reinterpret_cast<const f32x4 *>(s_q);
    double ab = 0.0, a2 = 0.0, b2 = 0.0;
#pragma unroll 4
    for (uint32_t e = 0; e < dim / 4; ++e) {
        const f32x4 a = q4[e], b = row_quad<RowT>(corpus, row, dim, e);
        const double ax = a.x, ay = a.y, az = a.z, aw = a.w, bx = b.x, by = b.y, bz = b.z, bw = b.w;
        ab = ab + ax * bx; a2 = a2 + ax * ax; b2 = b2 + bx * bx;
        ab = ab + ay * by; a2 = a2 + ay * ay; b2 = b2 + by * by;
        ab = ab + az * bz; a2 = a2 + az * az; b2 = b2 + bz * bz;
        ab = ab + aw * bw; a2 = a2 + aw * aw; b2 = b2 + bw * bw;
    }
    out[i] = cos_finish_exact(ab, a2, b2);
}

int launch_exact_all_slab(smt_ctx *ctx, const float *corpus, int row_dtype, uint64_t rows, uint32_t dim, const float *query,
                          const uint64_t *chunk_table, uint64_t n_chunks, double *out)
{
    const bool half = row_dtype == SMT_ROWS_F16, byte = row_dtype == SMT_ROWS_I8, nibble = row_dtype == SMT_ROWS_I4;
    SMT_REQUIRE(half || byte || nibble ? dim == SMT_DIM : dim_in_family(dim), "wide rows: 64, 512, 768 or 1024 dimensions, or half, byte or nibble rows of 256");
    const uint64_t n = chunk_table ? n_chunks * FILTER_CHUNK : rows;
    if (n == 0) return SMT_OK;
    if (dim_is_narrow(dim) && !(half || byte || nibble)) {
        const uint64_t nb = (n + 127) / 128;
        SMT_REQUIRE(nb < (1ull << 31), "too many rows for one exhaustive launch");
        prof_begin(ctx, "exact_narrow");
        hipLaunchKernelGGL(exact_all_narrow_kernel<4>, dim3((unsigned)nb), dim3(128), 0, ctx->stream, corpus, rows, query, chunk_table, n_chunks, out);
        prof_end(ctx, "exact_narrow");
        SMT_HIP_CHECK(hipGetLastError());
        return SMT_OK;
    }
    const uint64_t blocks = (n + 255) / 256;
    SMT_REQUIRE(blocks < (1ull << 31), "too many rows for one exhaustive launch");
    prof_begin(ctx, "exact_slab");
    if (nibble) hipLaunchKernelGGL(exact_all_slab_kernel<nibble_t>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, corpus, rows, dim, query, chunk_table, n_chunks, out);
    else if (byte) hipLaunchKernelGGL(exact_all_slab_kernel<int8_t>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, corpus, rows, dim, query, chunk_table, n_chunks, out);
    else if (half) hipLaunchKernelGGL(exact_all_slab_kernel<_Float16>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, corpus, rows, dim, query, chunk_table, n_chunks, out);
    else hipLaunchKernelGGL(exact_all_slab_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, corpus, rows, dim, query, chunk_table, n_chunks, out);
    prof_end(ctx, "exact_slab");
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

}  // namespace smt
