// topk_large.hip -- top-k for 57 <= k <= 1024 without a sort of every row.
//   1. largek_tau: an evenly spaced sample of the scanned rows is scored in f32 (largek_sample_kernel) and one block per
//      query picks a sampled order statistic by radix select (largek_tau_kernel): about LK_TARGET x (k + guard) rows are
//      expected at or below it.  It is widened by F32_ERR_SCAN, and clamped to the workspace threshold plus that band.
//      Shards of at most LK_CAP_MAX rows skip the sample: tau = +inf, every row is collected.
//   2. largek_collect: the K4 streaming loop (threshold.hip: one coalesced 1 KiB row per wave instruction, next chunk
//      prefetched, chunks claimed from the block's LDS counter), unfiltered or over the chunk table, one query per
//      blockIdx.y.  Rows with d32 <= tau go to the query's candidate buffer as keys (d32 bits << 32 | row), one global
//      atomic per wave flush.  The count goes on past the capacity: an overflow is seen, never silent.
//   3. largek_finish: one block per query sorts the keys in LDS, rescores the best k + guard exactly (f64, index order:
//      device_utils.h exact_distance, the code of the select and of rescore_rows_kernel), orders them by (f64 distance,
//      row), applies the workspace score filter, writes the padded list and the verdict of the select's certificate:
//      a row that was not rescored has d32 >= min(tau, first key not rescored), so exact distance >= that - F32_ERR_SCAN.
// tau only moves cost: a bad sample gives an UNCERTAIN / OVERFLOW verdict (the host form re-answers), never a wrong PROVED.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "device_utils.h"
#include "chunk_deal.h"

namespace smt {

namespace {

constexpr uint32_t LK_CAP_MAX = 16384;   // candidate keys per query: the finish sorts them in LDS (128 KiB)
constexpr uint32_t LK_TARGET = 3;        // rows expected under tau, in units of k + guard
constexpr uint32_t LK_MIN_RANK = 8;      // tau is at least the 8th sampled distance (a lower rank scatters the count too widely)
constexpr uint32_t LK_MAX_QUERIES = 256; // queries per round of the three launches (bounds the scratch)
constexpr int LK_HIT_BUF = 256;          // per-wave LDS buffer of the collect (keys)
constexpr int LK_SORT_MAX = 2048;        // rescored rows per query: k + guard <= 1024 + 64, padded to a power of two
constexpr int LK_THREADS = 1024;
constexpr uint32_t LK_K3_MIN_NQ = 5;     // unfiltered batches from this size take the K3 sweep instead of a pass per query

struct SampleParams {
    const float *corpus;
    const float *queries;
    uint64_t n_virtual;
    const smt_range *ranges;
    const uint64_t *prefix;
    uint32_t n_ranges;
    uint32_t S;
    float *samp;   // [nq][S]
};

__device__ __forceinline__ uint32_t lk_map_virtual(uint64_t v, const smt_range *ranges, const uint64_t *prefix, uint32_t n_ranges)
{
    uint32_t lo = 0, hi = n_ranges;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (prefix[mid] <= v) lo = mid; else hi = mid;
    }
    return (uint32_t)(ranges[lo].begin + (v - prefix[lo]));
}

// grid (blocks, nq) x 256: sample s of query blockIdx.y is virtual row s * n / S; four rows per wave step (wave_sum4)
__global__ void __launch_bounds__(256) largek_sample_kernel(SampleParams p)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t qi = blockIdx.y;
    const f32x4 q = reinterpret_cast<const f32x4 *>(p.queries + (size_t)qi * 256)[lane];
    const float a2 = wave_sum(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    const bool qz = (a2 == 0.0f);
    const float rq = qz ? 0.0f : __frsqrt_rn(a2);
    const uint32_t stride = gridDim.x * 4u * 4u;
    for (uint32_t s0 = (blockIdx.x * 4u + (uint32_t)wave) * 4u; s0 < p.S; s0 += stride) {
        f32x4 c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t s = s0 + j < p.S ? s0 + j : p.S - 1;
            const uint64_t v = (uint64_t)s * p.n_virtual / p.S;
            const uint32_t row = p.n_ranges ? lk_map_virtual(v, p.ranges, p.prefix, p.n_ranges) : (uint32_t)v;
            c[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(p.corpus + (uint64_t)row * 256) + lane);
        }
        float pb[4], pa[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pb[j] = c[j].x * c[j].x + c[j].y * c[j].y + c[j].z * c[j].z + c[j].w * c[j].w;
            pa[j] = c[j].x * q.x + c[j].y * q.y + c[j].z * q.z + c[j].w * q.w;
        }
        const float b2 = wave_sum4(pb[0], pb[1], pb[2], pb[3], lane);
        const float ab = wave_sum4(pa[0], pa[1], pa[2], pa[3], lane);
        float d = dist_f32(ab, b2, rq, qz);
        if (!(d == d)) d = __builtin_inff();
        if (lane < 4 && s0 + (uint32_t)lane < p.S) p.samp[(size_t)qi * p.S + s0 + lane] = d;
    }
}

struct TauParams {
    const float *samp;   // [nq][S]
    uint32_t S;
    uint32_t rank;       // 1-based: tau is the rank-th smallest sampled distance
    int skip;            // 1: tau = +inf (every row is collected)
    int ws_threshold;
    float ws_clamp;      // with ws_threshold: tau <= this (the threshold's distance plus the band)
    double err;          // widening of the sampled distance: the band of the distances the collect compares with tau
    float *tau;          // [nq]
    unsigned int *counts;  // [nq]: zeroed here for the collect
};

// one block per query: radix select (4 x 8 bits) of the rank-th smallest sampled f32 distance (non-negative: the bits order
// like the values)
__global__ void __launch_bounds__(LK_THREADS) largek_tau_kernel(TauParams p)
{
    __shared__ unsigned int s_hist[256];
    __shared__ unsigned int s_sel[2];   // prefix found so far, rank still wanted within it
    const uint32_t qi = blockIdx.x;
    if (threadIdx.x == 0) { p.counts[qi] = 0; s_sel[0] = 0; s_sel[1] = p.rank; }
    if (p.skip) {
        if (threadIdx.x == 0) p.tau[qi] = __builtin_inff();
        return;
    }
    const uint32_t *samp = reinterpret_cast<const uint32_t *>(p.samp) + (size_t)qi * p.S;
    uint32_t mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (threadIdx.x < 256) s_hist[threadIdx.x] = 0;
        __syncthreads();
        const uint32_t prefix = s_sel[0];
        for (uint32_t i = threadIdx.x; i < p.S; i += blockDim.x) {
            const uint32_t v = samp[i];
            if ((v & mask) == prefix) atomicAdd(&s_hist[(v >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t want = s_sel[1], d = 0;
            for (; d < 255; ++d) {
                if (s_hist[d] >= want) break;
                want -= s_hist[d];
            }
            s_sel[0] = prefix | (d << shift);
            s_sel[1] = want;
        }
        mask |= 255u << shift;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float t = __uint_as_float(s_sel[0]);
        if (t < __builtin_inff()) t = nextafterf((float)((double)t + p.err), __builtin_inff());
        if (p.ws_threshold) t = fminf(t, p.ws_clamp);
        p.tau[qi] = t;
    }
}

struct CollectParams {
    const float *corpus;
    const float *queries;
    uint64_t n_virtual;
    const uint64_t *chunk_table;   // FILTERED: row0 | valid rows << 32 per chunk (range_tables.hip)
    uint64_t n_chunks;
    const float *tau;              // [nq]
    key_t64 *cand;                 // [nq][cap]
    unsigned int *counts;          // [nq]: rows under tau, counted past cap
    uint32_t cap;
};

// grid (blocks, nq): the K4 loop of threshold.hip with the test d32 <= tau[q] and keys in place of rows
template <bool FILTERED>
__global__ void __launch_bounds__(1024) largek_collect_kernel(CollectParams p)
{
    constexpr int U = FILTER_CHUNK;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves_per_block = blockDim.x >> 6;
    const uint32_t qi = blockIdx.y;
    volatile key_t64 *s_hits = reinterpret_cast<key_t64 *>(smem_raw) + wave * LK_HIT_BUF;
    uint32_t *s_next = reinterpret_cast<uint32_t *>(reinterpret_cast<key_t64 *>(smem_raw) + waves_per_block * LK_HIT_BUF);

    const f32x4 q = reinterpret_cast<const f32x4 *>(p.queries + (size_t)qi * 256)[lane];
    const float a2 = wave_sum(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    const bool qz = (a2 == 0.0f);
    const float rq = qz ? 0.0f : __frsqrt_rn(a2);
    const float tau = p.tau[qi];
    key_t64 *cand = p.cand + (size_t)qi * p.cap;
    unsigned int *count = p.counts + qi;

    const uint64_t n_chunks = p.n_chunks;
    const const_u64_ptr const_table = (const_u64_ptr)(uintptr_t)p.chunk_table;
    // (the chunk deal of all streaming kernels: chunk_deal.h)
    auto fetch_desc = [&](uint64_t c) -> uint64_t {
        if (c >= n_chunks) return 0ull;
        if (FILTERED) return const_table[c];
        const uint64_t v0 = c * U;
        const uint64_t left = p.n_virtual - v0;
        return v0 | ((left < (uint64_t)U ? left : (uint64_t)U) << 32);
    };
    if (threadIdx.x == 0) *s_next = (uint32_t)waves_per_block;
    __syncthreads();

    uint32_t n_buf = 0;  // wave-uniform: keys waiting in s_hits
    auto flush = [&]() {
        if (n_buf == 0) return;
        unsigned int base = 0;
        if (lane == 0) base = atomicAdd(count, n_buf);
        base = (unsigned int)__builtin_amdgcn_readfirstlane((int)base);
        __builtin_amdgcn_wave_barrier();
        for (uint32_t i = lane; i < n_buf; i += 64) {
            const uint64_t slot = (uint64_t)base + i;
            if (slot < p.cap) cand[slot] = s_hits[i];   // beyond cap: counted, not stored (SMT_STATUS_OVERFLOW)
        }
        __builtin_amdgcn_wave_barrier();
        n_buf = 0;
    };

    f32x4 cn[U];
    uint32_t rown[U];
    uint64_t cA = deal_chunk((uint32_t)wave, waves_per_block), cB = n_chunks, cC = n_chunks;
    uint64_t dA = fetch_desc(cA), dB = 0;
    if (cA < n_chunks) {
        deal_issue_loads<U, true>(p, dA, lane, cn, rown);
        cB = deal_chunk(deal_claim(s_next, lane), waves_per_block);
        dB = fetch_desc(cB);
        if (FILTERED) cC = deal_chunk(deal_claim(s_next, lane), waves_per_block);
    }
    while (cA < n_chunks) {
        f32x4 c[U];
        uint32_t row[U];
#pragma unroll
        for (int j = 0; j < U; ++j) { c[j] = cn[j]; row[j] = rown[j]; }
        const uint64_t first = dA & 0xFFFFFFFFull, end = first + (dA >> 32);
        if (cB < n_chunks) deal_issue_loads<U, true>(p, dB, lane, cn, rown);
        uint64_t cN, dN;
        if (FILTERED) { cN = cC; dN = fetch_desc(cC); cC = deal_chunk(deal_claim(s_next, lane), waves_per_block); }
        else { cN = deal_chunk(deal_claim(s_next, lane), waves_per_block); dN = fetch_desc(cN); }

        float pb[4], pa[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pb[j] = c[j].x * c[j].x + c[j].y * c[j].y + c[j].z * c[j].z + c[j].w * c[j].w;
            pa[j] = c[j].x * q.x + c[j].y * q.y + c[j].z * q.z + c[j].w * q.w;
        }
        const float b2 = wave_sum4(pb[0], pb[1], pb[2], pb[3], lane);
        const float ab = wave_sum4(pa[0], pa[1], pa[2], pa[3], lane);
        float d = dist_f32(ab, b2, rq, qz);
        if (!(d == d)) d = __builtin_inff();
        const int jj = lane & 3;
        bool pass_mine = false;
        key_t64 my_key = 0;
        if (lane < 4) {
            pass_mine = (first + (uint64_t)jj < end) && (d <= tau);
            my_key = make_key(d, jj == 0 ? row[0] : jj == 1 ? row[1] : jj == 2 ? row[2] : row[3]);
        }
        const unsigned long long m = __ballot(pass_mine);
        if (m != 0ull) {
            const uint32_t cnt = (uint32_t)__popcll(m);
            if (n_buf + cnt > (uint32_t)LK_HIT_BUF) flush();
            if (pass_mine) s_hits[n_buf + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = my_key;
            n_buf += cnt;
        }
        cA = cB; dA = dB;
        cB = cN; dB = dN;
    }
    flush();
}

struct FinishParams {
    const float *corpus;
    const float *queries;
    const key_t64 *cand;          // [nq][cap]
    const unsigned int *counts;   // [nq]
    const float *tau;             // [nq]
    uint32_t cap;
    uint32_t k_list;              // slots per list
    uint32_t k_eff;               // min(k_list, rows scanned)
    uint32_t kg;                  // rows rescored: k_eff + guard
    int ws_threshold;
    float ws_thr_score;
    uint64_t row_base;
    uint64_t *out_rows;
    double *out_dist;
    uint64_t out_stride;
    uint32_t *out_status;         // [nq] or nullptr
    uint64_t *out_uncertain;      // [nq] or nullptr
    unsigned long long *status;   // the context's counter of non-zero verdicts
    double err;                   // |collected key's distance - exact distance| bound: F32_ERR_SCAN, or the K3 sweep's nominating band
};

__global__ void __launch_bounds__(LK_THREADS) largek_finish_kernel(FinishParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ uint64_t s_dbits[LK_SORT_MAX];   // f64 distance bits (non-negative or +inf: they order like the values)
    __shared__ uint32_t s_row[LK_SORT_MAX];
    __shared__ unsigned int s_misc[2];          // [0] max |query| bits, [1] valid rescored rows
    key_t64 *s_keys = reinterpret_cast<key_t64 *>(smem_raw);
    const uint32_t qi = blockIdx.x;
    const unsigned int count = p.counts[qi];
    const uint32_t n = count < p.cap ? count : p.cap;
    uint32_t np = 1;
    while (np < n) np <<= 1;
    if (threadIdx.x < 2) s_misc[threadIdx.x] = 0;
    for (uint32_t i = threadIdx.x; i < np; i += blockDim.x) s_keys[i] = i < n ? p.cand[(size_t)qi * p.cap + i] : KEY_PAD;
    __syncthreads();
    if (threadIdx.x < 256) atomicMax(&s_misc[0], __float_as_uint(p.queries[(size_t)qi * 256 + threadIdx.x]) & 0x7fffffffu);
    bitonic_sort(np, [&](uint32_t a, uint32_t b, bool up) {
        const key_t64 x = s_keys[a], y = s_keys[b];
        if ((x > y) == up && x != y) { s_keys[a] = y; s_keys[b] = x; }
    });
    const uint32_t m = n < p.kg ? n : p.kg;
    uint32_t mp = 1;
    while (mp < m) mp <<= 1;
    const f32x4 *q4 = reinterpret_cast<const f32x4 *>(p.queries + (size_t)qi * 256);
    for (uint32_t i = threadIdx.x; i < mp; i += blockDim.x) {
        uint64_t dbits = 0x7FF0000000000000ull;
        uint32_t r = 0xFFFFFFFFu;
        if (i < m) {
            const uint32_t row = (uint32_t)(s_keys[i] & 0xFFFFFFFFull);
            const double d = exact_distance(q4, reinterpret_cast<const f32x4 *>(p.corpus + (uint64_t)row * 256));
            const bool keep = (d == d) && (!p.ws_threshold || (1.0 - d) > (double)p.ws_thr_score);   // store.rs:502-503
            if (keep) { dbits = (uint64_t)__double_as_longlong(d); r = row; atomicAdd(&s_misc[1], 1u); }
        }
        s_dbits[i] = dbits;
        s_row[i] = r;
    }
    __syncthreads();
    bitonic_sort(mp, [&](uint32_t a, uint32_t b, bool up) {
        const uint64_t da = s_dbits[a], db = s_dbits[b];
        const uint32_t ra = s_row[a], rb = s_row[b];
        const bool gt = da > db || (da == db && ra > rb);
        const bool lt = da < db || (da == db && ra < rb);
        if (up ? gt : lt) { s_dbits[a] = db; s_dbits[b] = da; s_row[a] = rb; s_row[b] = ra; }
    });
    const uint32_t valid = s_misc[1];
    const uint32_t n_out = valid < p.k_eff ? valid : p.k_eff;
    uint64_t *orow = p.out_rows + (size_t)qi * p.out_stride;
    double *odist = p.out_dist + (size_t)qi * p.out_stride;
    for (uint32_t t = threadIdx.x; t < p.k_list; t += blockDim.x) {
        if (t < n_out) { orow[t] = p.row_base + s_row[t]; odist[t] = __longlong_as_double((long long)s_dbits[t]); }
        else { orow[t] = 0xFFFFFFFFFFFFFFFFull; odist[t] = __builtin_inf(); }
    }
    if (threadIdx.x == 0) {
        unsigned int code;
        if (!magnitude_in_domain(s_misc[0])) code = 3u;               // SMT_STATUS_INVALID_QUERY (domain.hip)
        else if (count > p.cap) code = 2u;                            // SMT_STATUS_OVERFLOW: rows under tau were dropped
        else {
            // the certificate of the select (SelectArgs::f32_err): rows outside the rescored ones have d32 > tau (not collected)
            // or d32 >= the first key not rescored, so exact distance >= floor_out
            const float next32 = n > m ? __uint_as_float((unsigned)(s_keys[m] >> 32)) : __builtin_inff();
            const double floor_out = (double)fminf(p.tau[qi], next32) - p.err;
            bool certain;
            if (valid >= p.k_eff) certain = floor_out > __longlong_as_double((long long)s_dbits[p.k_eff - 1]);
            else certain = p.ws_threshold ? !((1.0 - floor_out) > (double)p.ws_thr_score) : floor_out == __builtin_inf();
            code = certain ? 0u : 1u;                                 // SMT_STATUS_UNCERTAIN
        }
        if (p.out_status) p.out_status[qi] = code;
        if (p.out_uncertain) p.out_uncertain[qi] = code;
        if (code && p.status) atomicAdd(p.status, 1ull);
    }
}

size_t lk_align(size_t x) { return (x + 255) & ~(size_t)255; }

// the route's own buffer (the K3 sweep stages its queries in the scratch): grown like ensure_scratch, after the streams drain
int ensure_largek(smt_ctx *ctx, size_t bytes)
{
    if (bytes <= ctx->largek_bytes) return SMT_OK;
    SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (int rc_side = sync_side_streams(ctx)) return rc_side;
    if (ctx->d_largek) SMT_HIP_CHECK(hipFree(ctx->d_largek));
    ctx->d_largek = nullptr;
    ctx->largek_bytes = 0;
    const size_t want = std::max(bytes, (size_t)1 << 20);
    SMT_HIP_CHECK(hipMalloc(&ctx->d_largek, want));
    ctx->largek_bytes = want;
    return SMT_OK;
}

}  // namespace

// The whole route for a.nq queries, enqueued on the context's stream without a host synchronisation (unless the scratch
// grows).  Lists [nq][k_out] at out_rows / out_dist (out_stride apart), verdicts in out_status / out_uncertain.
int launch_topk_large(smt_ctx *ctx, const ScanArgs &a)
{
    SMT_REQUIRE(a.k_out >= 1 && a.k_out <= LARGEK_MAX_K, "large-k route: top_k must be in [1, 1024]");
    SMT_REQUIRE(a.rows < 0xFFFFFFFFull, "a shard holds fewer than 2^32 rows");
    if (a.nq == 0) return SMT_OK;
    const uint64_t n = a.n_virtual;
    const uint64_t out_stride = a.out_stride ? a.out_stride : a.k_out;
    const uint32_t k_eff = (uint32_t)std::min<uint64_t>(a.k_out, n);
    if (k_eff == 0) {   // nothing to scan: padding, and an empty answer is a proved one
        if (a.out_status) SMT_HIP_CHECK(hipMemsetAsync(a.out_status, 0, (size_t)a.nq * sizeof(uint32_t), ctx->stream));
        if (a.out_uncertain) SMT_HIP_CHECK(hipMemsetAsync(a.out_uncertain, 0, (size_t)a.nq * sizeof(uint64_t), ctx->stream));
        if (out_stride == (uint64_t)2 * a.k_out && reinterpret_cast<uint64_t *>(a.out_dist) == a.out_rows + a.k_out)
            return launch_merge_topk_packed_on(ctx, ctx->stream, a.out_rows, 0, a.nq, 1, a.k_out, a.out_rows);
        return launch_merge_topk(ctx, a.out_rows, a.out_dist, 0, a.nq, 1, a.k_out, a.out_rows, a.out_dist);
    }
    const uint32_t guard = std::max<uint32_t>(64, k_eff / 16);
    const uint32_t kg = k_eff + guard;
    // sample size, rank and capacity: S = max(8192, n / 256) sampled rows; tau = the rank-th smallest of them, with
    // rank >= LK_MIN_RANK and rank * n / S ~ LK_TARGET x (k + guard) rows expected under it; capacity 3 x that expectation
    const bool skip = n <= LK_CAP_MAX;
    uint32_t S = 0, rank = 1, cap = (uint32_t)n;
    if (!skip) {
        S = (uint32_t)std::min<uint64_t>(n, std::max<uint64_t>(8192, n / 256));
        const uint64_t want = (uint64_t)LK_TARGET * kg;
        rank = (uint32_t)std::min<uint64_t>(S, std::max<uint64_t>(LK_MIN_RANK, (want * S + n - 1) / n));
        const uint64_t expect = (uint64_t)rank * n / S;
        cap = (uint32_t)std::min<uint64_t>(LK_CAP_MAX, std::max<uint64_t>((uint64_t)8 * kg, 3 * expect));
        cap = (cap + 255) & ~255u;
        if (cap > LK_CAP_MAX) cap = LK_CAP_MAX;
    }
    uint32_t cap_p = 1;
    while (cap_p < cap) cap_p <<= 1;
    const uint32_t nq_round = std::min<uint32_t>(a.nq, LK_MAX_QUERIES);
    const bool filtered = a.n_ranges > 0;
    const size_t b_samp = lk_align((size_t)nq_round * S * sizeof(float));
    const size_t b_tau = lk_align((size_t)nq_round * sizeof(float));
    const size_t b_cnt = lk_align((size_t)nq_round * sizeof(unsigned int));
    const size_t b_cand = lk_align((size_t)nq_round * cap * sizeof(key_t64));
    const size_t b_table = filtered ? lk_align((size_t)a.n_chunks * sizeof(uint64_t)) : 0;
    int rc = ensure_largek(ctx, b_samp + b_tau + b_cnt + b_cand + b_table);
    if (rc) return rc;
    char *base = reinterpret_cast<char *>(ctx->d_largek);
    float *samp = reinterpret_cast<float *>(base);
    float *tau = reinterpret_cast<float *>(base + b_samp);
    unsigned int *counts = reinterpret_cast<unsigned int *>(base + b_samp + b_tau);
    key_t64 *cand = reinterpret_cast<key_t64 *>(base + b_samp + b_tau + b_cnt);
    const uint64_t *table = nullptr;
    if (filtered && (rc = range_chunk_table(ctx, a, reinterpret_cast<uint64_t *>(base + b_samp + b_tau + b_cnt + b_cand), &table))) return rc;

    const size_t finish_smem = (size_t)cap_p * sizeof(key_t64);
    static bool attrs_set[64] = {};
    if (ctx->device >= 0 && ctx->device < 64 && !attrs_set[ctx->device]) {
        SMT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(largek_finish_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)(LK_CAP_MAX * sizeof(key_t64))));
        attrs_set[ctx->device] = true;
    }
    const int blocks = ctx->tune.scan_blocks > 0 ? ctx->tune.scan_blocks : ctx->num_cus;
    const int threads = ctx->tune.scan_threads;
    const size_t collect_smem = (size_t)(threads / 64) * LK_HIT_BUF * sizeof(key_t64) + 16;
    // Unfiltered batches of LK_K3_MIN_NQ or more queries collect in ONE sweep of the batched kernel with preset thresholds
    // (launch_gemm_threshold) instead of a streaming pass per query; its keys carry the nominating distance, whose band (bf16 x 3 over
    // the f32 rows, f16 x 2 over the operand image) widens tau and the certificate alike
    const bool k3 = !filtered && !skip && a.nq >= LK_K3_MIN_NQ;
    const double err = !k3 ? F32_ERR_SCAN : a.image ? F32_ERR_F16X2 : F32_ERR_BF16X3;
    const float ws_clamp = nextafterf((float)(1.0 - (double)a.ws_thr_score + 2 * err), INFINITY);
    for (uint32_t q0 = 0; q0 < a.nq; q0 += nq_round) {
        const uint32_t nqr = std::min<uint32_t>(nq_round, a.nq - q0);
        const float *queries = a.queries + (size_t)q0 * 256;
        prof_begin(ctx, "largek_tau");
        if (!skip) {
            SampleParams sp;
            sp.corpus = a.corpus;
            sp.queries = queries;
            sp.n_virtual = n;
            sp.ranges = a.ranges;
            sp.prefix = a.range_prefix;
            sp.n_ranges = a.n_ranges;
            sp.S = S;
            sp.samp = samp;
            const unsigned sb = (unsigned)std::min<uint64_t>((uint64_t)std::max(1, blocks / 4), (S + 15) / 16);
            hipLaunchKernelGGL(largek_sample_kernel, dim3(sb, nqr), dim3(256), 0, ctx->stream, sp);
        }
        TauParams tp;
        tp.samp = samp;
        tp.S = S;
        tp.rank = rank;
        tp.skip = skip ? 1 : 0;
        tp.ws_threshold = a.ws_threshold;
        tp.ws_clamp = ws_clamp;
        tp.err = err;
        tp.tau = tau;
        tp.counts = counts;
        hipLaunchKernelGGL(largek_tau_kernel, dim3(nqr), dim3(LK_THREADS), 0, ctx->stream, tp);
        prof_end(ctx, "largek_tau");
        SMT_HIP_CHECK(hipGetLastError());

        if (k3) {
            const key_t64 *c_out = nullptr;
            const unsigned int *n_out = nullptr;
            uint32_t stride = 0;
            if ((rc = launch_gemm_threshold(ctx, a.corpus, a.rows, a.image, a.image_zero, queries, nqr, tau, &c_out, &n_out, &stride, cap,
                                            cand, counts)))
                return rc;
        } else {
        CollectParams cp;
        cp.corpus = a.corpus;
        cp.queries = queries;
        cp.n_virtual = n;
        cp.chunk_table = table;
        cp.n_chunks = filtered ? a.n_chunks : (n + FILTER_CHUNK - 1) / FILTER_CHUNK;
        cp.tau = tau;
        cp.cand = cand;
        cp.counts = counts;
        cp.cap = cap;
        prof_begin(ctx, "largek_collect");
        if (filtered) hipLaunchKernelGGL((largek_collect_kernel<true>), dim3(blocks, nqr), dim3(threads), collect_smem, ctx->stream, cp);
        else hipLaunchKernelGGL((largek_collect_kernel<false>), dim3(blocks, nqr), dim3(threads), collect_smem, ctx->stream, cp);
        prof_end(ctx, "largek_collect");
        SMT_HIP_CHECK(hipGetLastError());
        }

        FinishParams fp;
        fp.corpus = a.corpus;
        fp.queries = queries;
        fp.cand = cand;
        fp.counts = counts;
        fp.tau = tau;
        fp.cap = cap;
        fp.k_list = a.k_out;
        fp.k_eff = k_eff;
        fp.kg = kg;
        fp.ws_threshold = a.ws_threshold;
        fp.ws_thr_score = a.ws_thr_score;
        fp.row_base = a.row_base;
        fp.out_rows = a.out_rows + (size_t)q0 * out_stride;
        fp.out_dist = a.out_dist + (size_t)q0 * out_stride;
        fp.out_stride = out_stride;
        fp.out_status = a.out_status ? a.out_status + q0 : nullptr;
        fp.out_uncertain = a.out_uncertain ? a.out_uncertain + q0 : nullptr;
        fp.status = ctx->d_status;
        fp.err = err;
        prof_begin(ctx, "largek_finish");
        hipLaunchKernelGGL(largek_finish_kernel, dim3(nqr), dim3(LK_THREADS), finish_smem, ctx->stream, fp);
        prof_end(ctx, "largek_finish");
        SMT_HIP_CHECK(hipGetLastError());
    }
    return SMT_OK;
}

}  // namespace smt
