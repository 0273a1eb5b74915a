// ivfpq_search.hip -- querying the IVF index: probe (query x centroid scores on the MFMA pipe, nprobe smallest per query), LUT or
// per-list projection, the ADC scan with its in-kernel re-score of the shortlist, and the search entry points.  ivfpq.h, DESIGN.md 4.6.
#include <atomic>
#include <chrono>
#include <cstddef>
#include <type_traits>

#include "ivfpq.h"

namespace smt {

// ------------------------------------------------------------------ query: probe

struct ProbeParams {
    const float *queries;     // [nq][256]
    const float *centroids;   // [nlist][256]
    const float *cnorm_half;
    uint32_t nlist;           // <= 4096
    uint32_t nprobe;
    uint32_t *probe_list;     // [nq][nprobe]
    float *probe_dot;         // [nq][nprobe]  q . c
};

// Coarse probe, two kernels (the first version was one block per query: 4096 wave-level dot products against
// centroids re-read from L2 by every query, then a 78-stage bitonic sort of all 4096 keys -- 0.45 ms per 1000
// queries, as much as the ADC scan itself):
//   ivf_score_kernel   S[q][c] = 0.5|c|^2 - q.c for all (query, centroid) pairs on the MFMA pipe; one block per
//                      centroid tile (32 centroids staged in LDS once), its waves sweep the query tiles;
//   ivf_probe_select_kernel   one WAVE per query holds its nlist scores in registers (64 per lane), finds the
//                      nprobe-th smallest by bisection on the orderable bit pattern, and emits the nprobe lists
//                      (order is irrelevant downstream; ties go to the smaller list id).
__global__ void __launch_bounds__(GEMM_THREADS, 2) ivf_score_kernel(const float *queries, uint32_t nq, const float *centroids,
                                                                    const float *cnorm_half, uint32_t nlist, float *scores)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    f32x4 *s_c = reinterpret_cast<f32x4 *>(smem_raw);  // [32][65] float4: this block's centroid tile
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, j = lane & 31;
    const uint32_t ct = blockIdx.x;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int idx = threadIdx.x + u * GEMM_THREADS;
        s_c[(idx >> 6) * QT_STRIDE_F4 + (idx & 63)] =
            reinterpret_cast<const f32x4 *>(centroids + (size_t)(ct * QT_ROWS + (idx >> 6)) * 256)[idx & 63];
    }
    const uint32_t cid = ct * QT_ROWS + j;
    const float cn = cnorm_half[cid];
    __syncthreads();
    const uint32_t n_tiles = (nq + 31) / 32;
    for (uint32_t tile = wave; tile < n_tiles; tile += GEMM_WAVES) {
        const uint32_t qrow = tile * 32 + j;
        const f32x4 *src = reinterpret_cast<const f32x4 *>(queries + (size_t)(qrow < nq ? qrow : 0) * 256) + h;
        f32x4 A[32];
#pragma unroll
        for (int m = 0; m < 32; ++m) A[m] = src[2 * m];
        const f32x16 acc = mfma_tile_32x32x256(A, s_c + j * QT_STRIDE_F4 + h);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t row = tile * 32 + acc_row(r, h);
            if (row < nq) scores[(size_t)row * nlist + cid] = cn - acc[r];
        }
    }
}

constexpr int SEL_SLOTS = PROBE_MAX_LISTS / 64;  // scores per lane

__global__ void __launch_bounds__(256) ivf_probe_select_kernel(ProbeParams p, const float *scores, uint32_t nq)
{
    const int lane = threadIdx.x & 63;
    const uint32_t qi = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (qi >= nq) return;  // wave-uniform
    const float *sc = scores + (size_t)qi * p.nlist;
    uint32_t v[SEL_SLOTS];
#pragma unroll
    for (int u = 0; u < SEL_SLOTS; ++u) {
        const uint32_t c = (uint32_t)u * 64u + (uint32_t)lane;
        v[u] = c < p.nlist ? f32_orderable(sc[c]) : 0xFFFFFFFFu;
    }
    // smallest T with #(v <= T) >= nprobe
    uint32_t lo = 0u, hi = 0xFFFFFFFFu;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        uint32_t cnt = 0;
#pragma unroll
        for (int u = 0; u < SEL_SLOTS; ++u) cnt += v[u] <= mid ? 1u : 0u;
        cnt = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_sum_u32(cnt));
        if (cnt >= p.nprobe) hi = mid; else lo = mid + 1u;
    }
    const uint32_t T = lo;
    uint32_t n_lt = 0;
#pragma unroll
    for (int u = 0; u < SEL_SLOTS; ++u) n_lt += v[u] < T ? 1u : 0u;
    n_lt = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_sum_u32(n_lt));
    uint32_t pos_lt = 0, pos_eq = n_lt;  // wave-uniform write cursors: "< T" first, then ties in list-id order
    uint32_t *out_l = p.probe_list + (size_t)qi * p.nprobe;
    float *out_d = p.probe_dot + (size_t)qi * p.nprobe;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int u = 0; u < SEL_SLOTS; ++u) {
        const uint32_t c = (uint32_t)u * 64u + (uint32_t)lane;
        const bool lt = v[u] < T, eq = v[u] == T && c < p.nlist;
        const unsigned long long m_lt = __ballot(lt), m_eq = __ballot(eq);
        uint32_t slot = 0xFFFFFFFFu;
        if (lt) slot = pos_lt + (uint32_t)__popcll(m_lt & below);
        else if (eq) slot = pos_eq + (uint32_t)__popcll(m_eq & below);
        if (slot < p.nprobe) {
            out_l[slot] = c;
            out_d[slot] = p.cnorm_half[c] - sc[c];  // q . c
        }
        pos_lt += (uint32_t)__popcll(m_lt);
        pos_eq += (uint32_t)__popcll(m_eq);
    }
}

// LUT[q][code][s] = <q_s, codebook[s][code]>; grid (nq, 32), 256 threads.  CODE-major: sub-quantiser s owns LDS bank s of the scan
// kernel's copy (ivf_adc_kernel, KIND 0), whatever the codes are.
__global__ void ivf_lut_kernel(const float *queries, const float *codebooks, float *lut)
{
    // 8 codes x 32 sub-quantisers per block, s fastest: the stores are coalesced (with one sub-quantiser per block and code = thread
    // they lay 128 B apart and this kernel doubled the probe stage, 0.11 -> 0.21 ms per 1000 queries); the 32 B codebook reads scatter
    // over the 256 KiB of codebooks, which every query re-reads from L2
    const uint32_t qi = blockIdx.x, s = threadIdx.x & 31u, code = blockIdx.y * 8u + (threadIdx.x >> 5);
    const float *q = queries + (size_t)qi * 256 + s * PQ_DSUB;
    const float *cb = codebooks + ((size_t)s * PQ_K + code) * PQ_DSUB;
    float acc = 0.f;
#pragma unroll
    for (int d = 0; d < PQ_DSUB; ++d) acc += q[d] * cb[d];
    lut[((size_t)qi * PQ_K + code) * PQ_M + s] = acc;
}


// w[pair][k] = scale_l[k] * (Q_l[k] . q) for every (query, probed list) pair; one wave per pair
__global__ void __launch_bounds__(256) lpca_project_kernel(const float *queries, const uint32_t *probe_list, uint64_t n_pairs,
                                                            uint32_t nprobe, const float *basis, const float *lscale, float *w)
{
    const uint64_t pair = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (pair >= n_pairs) return;
    const int lane = threadIdx.x & 63;
    const uint32_t l = probe_list[pair];
    const f32x4 q = reinterpret_cast<const f32x4 *>(queries + (pair / nprobe) * 256)[lane];
    const f32x4 *B = reinterpret_cast<const f32x4 *>(basis + (size_t)l * LP_DIMS * 256);
    float mine = 0.0f;
#pragma unroll 4
    for (int k = 0; k < LP_DIMS; ++k) {
        const f32x4 b = B[k * 64 + lane];
        const float y = wave_sum(q.x * b.x + q.y * b.y + q.z * b.z + q.w * b.w);
        if (lane == k) mine = y * lscale[(size_t)l * LP_DIMS + k];
    }
    if (lane < LP_DIMS) w[pair * LP_DIMS + lane] = mine;
}

// The index ranks by inner products with UNIT rows: the probe score 0.5|c|^2 - q.c and the ADC sums mean "cosine" only for a unit
// query.  Queries of any in-domain length are therefore brought to unit length first (one wave per query; a zero query stays zero);
// the exact select stage at the end re-scores against the query AS GIVEN, like every other path.
__global__ void __launch_bounds__(256) ivf_unit_queries_kernel(const float *queries, uint32_t nq, float *out)
{
    const uint32_t qi = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (qi >= nq) return;
    const int lane = threadIdx.x & 63;
    const f32x4 v = reinterpret_cast<const f32x4 *>(queries + (size_t)qi * 256)[lane];
    const float a2 = wave_sum(v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w);
    const float r = a2 > 0.0f ? __frsqrt_rn(a2) : 0.0f;
    reinterpret_cast<f32x4 *>(out + (size_t)qi * 256)[lane] = f32x4{v.x * r, v.y * r, v.z * r, v.w * r};
}

// ------------------------------------------------------------------ query: ADC scan
struct AdcParams {
    const float *queries;
    const float *lut;          // [nq][256][32]  (kind 0: code-major, see ivf_lut_kernel)
    const float *lw;           // [nq][nprobe][32] per-pair weights of the per-list PCA codes (kind 1), or nullptr
    const uint32_t *probe_list;
    const float *probe_dot;
    uint32_t nprobe;
    uint32_t nq;
    const uint64_t *list_offsets;
    const uint8_t *codes;      // [N][32] in list order
    const uint32_t *ids;       // [N] corpus row of each code
    const float *corpus;       // full-precision rows for the in-kernel re-score
    uint32_t n_seg;            // blocks per (query, probed list): a list is cut into segments of seg_len codes, each
    uint32_t seg_len;          //   with its own shortlist -- the re-scored fraction of a LONG list stays what it is for a short one
    uint32_t shortlist;        // ADC candidates kept per WAVE (<= 64); 4 or 8 waves per (query, list segment)
    uint32_t kp;               // re-scored candidates emitted per (query, list)  (<= 64)
    key_t64 *lists;            // [nq][nprobe][kp]
    const uint64_t *mask;      // RANGED: one bit per list position, set = the row lies in the caller's ranges (ivf_range_mask_kernel)
};

static_assert(std::is_standard_layout_v<AdcParams> && std::is_trivially_copyable_v<AdcParams>,
              "the RANGED re-score stage reads AdcParams fields from the kernel-argument segment by offsetof");

// ------------------------------------------------------------------ query: row ranges -> a bitmap in LIST order
// A search inside row ranges (smt_ivfpq_search_ranges) scans the same lists and skips the positions whose row lies outside.  The
// bitmap is in LIST order because that is the order the ADC scan walks: a wave's 64 consecutive positions lie in at most two
// adjacent words, where a bitmap in row order would cost one random 4-byte read per code through ids[].
// One lane per position, one wave per 64-bit word: a coalesced load of ids[p], a binary search of the sorted, disjoint, non-empty
// ranges (staged in LDS when they fit, read from global memory otherwise), one ballot, one 8-byte store by lane 0.  A block takes
// MASK_WORDS_PER_WAVE words per wave, so the ranges are staged once per 4096 positions.  No atomics; nothing is read but ids[0, n_rows) and
// ranges[0, n_ranges); positions at or past n_rows in the last word come out 0.
constexpr int MASK_THREADS = 256;
constexpr int MASK_WORDS_PER_WAVE = 16;
constexpr uint32_t MASK_LDS_RANGES = 1024;   // 16 KiB

__global__ void __launch_bounds__(MASK_THREADS) ivf_range_mask_kernel(const uint32_t *ids, uint64_t n_rows, const smt_range *ranges,
                                                                       uint32_t n_ranges, uint64_t *mask)
{
    __shared__ smt_range s_ranges[MASK_LDS_RANGES];
    const bool staged = n_ranges <= MASK_LDS_RANGES;   // block-uniform
    if (staged) {
        for (uint32_t e = threadIdx.x; e < n_ranges; e += MASK_THREADS) s_ranges[e] = ranges[e];
        __syncthreads();
    }
    // the last range with begin <= row, if there is one, is the only one that can hold the row
    auto inside = [n_ranges](const smt_range *r, uint64_t row) -> bool {
        uint32_t lo = 0, hi = n_ranges;   // #(begin <= row) lies in [lo, hi]
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (r[mid].begin <= row) lo = mid + 1; else hi = mid;
        }
        return lo != 0 && row < r[lo - 1].end;
    };
    const int lane = threadIdx.x & 63;
    const uint64_t n_words = (n_rows + 63) >> 6;
    const uint64_t w0 = ((uint64_t)blockIdx.x * (MASK_THREADS / 64) + (threadIdx.x >> 6)) * MASK_WORDS_PER_WAVE;
    for (int u = 0; u < MASK_WORDS_PER_WAVE; ++u) {
        const uint64_t w = w0 + u;
        if (w >= n_words) return;   // wave-uniform
        const uint64_t p = w * 64 + lane;
        bool in = false;
        if (p < n_rows) {
            const uint64_t row = ids[p];
            in = staged ? inside(s_ranges, row) : inside(ranges, row);
        }
        const unsigned long long word = __ballot(in);
        if (lane == 0) mask[w] = word;
    }
}

// KIND 0: product quantisation, the query's 256 x 32 LUT staged in LDS (32 KiB: 4 blocks per CU); KIND 1: per-list PCA codes scored
// with 32 block-uniform weights -- no LUT, 2-4 KiB of LDS per block, so the register budget (50 VGPRs) decides the occupancy:
// 8 waves per SIMD instead of 4.
// KIND 0's gathers are CONFLICT-FREE (round 6).  A lane scores its own row: 32 lookups LUT[s][code_s].  With the table laid out
// [s][code] and every lane on the same s at the same time, 32 random codes fell on the 32 banks of ds_read_b32 like balls into bins
// -- 3.5 LDS cycles per lane group instead of 1, 55 % of the kernel's LDS cycles were conflicts and the LDS, not HBM, bounded it
// (0.57 of HBM; profiles/r05_ivf/r05_ivf_pmc_lds.json).  Now the table is [code][s] -- sub-quantiser s lives in bank s -- and lane l
// walks the sub-quantisers in ITS OWN order, s = (t + l) mod 32 at step t: the 32 lanes of a group are on 32 different sub-quantisers,
// hence 32 different banks, at every step, whatever the codes are.  The code bytes stay as the build wrote them (no layout change in
// the index, its files or its append path): each lane rotates its 32-byte record by l mod 32 bytes in registers -- three conditional
// dword stages and one v_alignbyte per dword, 32 VALU instructions per row beside the 96 of the lookups.  (Until round 5 both kinds were one kernel and the unused LUT array halved the resident waves of
// the shipped coding: the re-score stage is random 1 KiB row reads, i.e. latency hidden by waves in flight.)
// RANGED: the search is inside row ranges; a position whose bit in p.mask is 0 stays empty -- no code bytes are loaded for it and it
// never becomes a candidate -- and everything after the distances (shortlists, bisection, compaction, re-score, merge) is the same
// code, so what holds for "the rows of a list segment" without ranges holds for its IN-RANGE rows with them.
#define IVF_ADC_KERNEL ivf_adc_kernel
#define IVF_ADC_POOL 0
#include "ivfpq_adc_body.h"
#undef IVF_ADC_KERNEL
#undef IVF_ADC_POOL
#define IVF_ADC_KERNEL ivf_adc_pool_kernel
#define IVF_ADC_POOL 1
#include "ivfpq_adc_body.h"
#undef IVF_ADC_KERNEL
#undef IVF_ADC_POOL

// ------------------------------------------------------------------ wide searches: the pool's finish
// One block per query over its P = lists x slots pool keys (ivf_adc_pool_kernel).  With `valid` keys that are not KEY_PAD and
// kg = min(valid, top_k + guard) (guard = max(64, top_k / 16) as in topk_large.hip, so kg <= 1088):
//   valid <= PF_SORT   every valid key goes to LDS and is sorted there; the first kg are taken;
//   otherwise          the kg-th smallest 64-BIT key is found by radix select (eight 8-bit passes over an LDS histogram, the pattern
//                      of largek_tau_kernel) and the keys at or below it are compacted into LDS.  Keys are unique -- a row lies in
//                      exactly one list segment and is part of its key -- so exactly kg pass: ties of the f32 distance break by row,
//                      nothing overflows, nothing depends on the order the threads arrive in.
// Those rows are re-scored with exact_distance against the query AS GIVEN, sorted by (f64 bits, row), and the top_k best written
// with row_base added, padded with (UINT64_MAX, +inf), out_stride apart; counts where wanted.
// A KEY_PAD key must never reach exact_distance (its row field is 0xFFFFFFFF: the load would leave the corpus).  Three things see to
// it: KEY_PAD is never counted, histogrammed or compacted; the re-score tests the key again; and it tests row < n_rows.
constexpr int PF_THREADS = 1024;
constexpr uint32_t PF_SORT = 2048;                        // LDS entries: the direct path's limit, and >= kg (LK_SORT_MAX of topk_large.hip)
constexpr size_t IVF_POOL_BUDGET = (size_t)256 << 20;     // bytes of pool per round of queries

struct PoolFinishParams {
    const float *corpus;
    uint64_t n_rows;             // rows the index covers: no other row can be in a key
    const float *queries;        // as given
    const key_t64 *pool;         // [nq][P]
    uint32_t P;
    uint32_t top_k;
    uint32_t kg;                 // top_k + guard
    uint64_t row_base;
    uint64_t *out_rows;
    double *out_dist;
    uint64_t *out_counts;        // [nq] or nullptr
    uint64_t out_stride;
    unsigned long long *status;  // the context's counter of non-zero verdicts: a query outside the domain is counted there
};

__global__ void __launch_bounds__(PF_THREADS) ivf_pool_finish_kernel(PoolFinishParams p)
{
    __shared__ key_t64 s_keys[PF_SORT];
    __shared__ uint64_t s_dbits[PF_SORT];   // f64 distance bits (non-negative or +inf: they order like the values)
    __shared__ uint32_t s_row[PF_SORT];
    __shared__ unsigned int s_hist[256];
    __shared__ unsigned long long s_prefix; // radix select: the digits found so far
    __shared__ unsigned int s_misc[5];      // [0] valid keys, [1] compaction cursor, [2] max |query| bits, [3] rows kept, [4] rank still wanted
    const uint32_t qi = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const key_t64 *pool = p.pool + (size_t)qi * p.P;
    if (threadIdx.x < 5) s_misc[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_prefix = 0ull;
    __syncthreads();
    if (threadIdx.x < 256) atomicMax(&s_misc[2], __float_as_uint(p.queries[(size_t)qi * 256 + threadIdx.x]) & 0x7fffffffu);
    {
        uint32_t cnt = 0;   // wave-uniform
        for (uint32_t i0 = threadIdx.x - lane; i0 < p.P; i0 += PF_THREADS) {
            const uint32_t i = i0 + lane;
            cnt += (uint32_t)__popcll(__ballot(i < p.P && pool[i] != KEY_PAD));
        }
        if (lane == 0 && cnt) atomicAdd(&s_misc[0], cnt);
    }
    __syncthreads();
    const uint32_t valid = s_misc[0];
    const uint32_t kg = valid < p.kg ? valid : p.kg;
    // keys that pass `take` go to consecutive LDS slots (one LDS atomic per wave and step; the order among them is settled by the sorts)
    auto compact = [&](key_t64 limit) {
        for (uint32_t i0 = threadIdx.x - lane; i0 < p.P; i0 += PF_THREADS) {
            const uint32_t i = i0 + lane;
            const key_t64 key = i < p.P ? pool[i] : KEY_PAD;
            const bool take = key != KEY_PAD && key <= limit;
            const unsigned long long m = __ballot(take);
            if (m == 0ull) continue;
            unsigned int at = 0;
            if (lane == 0) at = atomicAdd(&s_misc[1], (unsigned int)__popcll(m));
            at = (unsigned int)__builtin_amdgcn_readfirstlane((int)at) + (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
            if (take && at < PF_SORT) s_keys[at] = key;
        }
    };
    uint32_t m;   // rows to re-score: s_keys[0, m)
    if (valid <= PF_SORT) {
        uint32_t np = 1;
        while (np < valid) np <<= 1;
        for (uint32_t i = threadIdx.x; i < np; i += PF_THREADS) s_keys[i] = KEY_PAD;
        __syncthreads();
        compact(KEY_PAD);
        __syncthreads();
        bitonic_sort(np, [&](uint32_t a, uint32_t b, bool up) {
            const key_t64 x = s_keys[a], y = s_keys[b];
            if ((x > y) == up && x != y) { s_keys[a] = y; s_keys[b] = x; }
        });
        m = kg;
    } else {
        if (threadIdx.x == 0) s_misc[4] = kg;   // (1-based rank; kg >= 1 here)
        key_t64 mask = 0ull;
        for (int shift = 56; shift >= 0; shift -= 8) {
            if (threadIdx.x < 256) s_hist[threadIdx.x] = 0;
            __syncthreads();
            const key_t64 prefix = s_prefix;
            for (uint32_t i = threadIdx.x; i < p.P; i += PF_THREADS) {
                const key_t64 v = pool[i];
                if (v != KEY_PAD && (v & mask) == prefix) atomicAdd(&s_hist[(uint32_t)(v >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                uint32_t want = s_misc[4], d = 0;
                for (; d < 255; ++d) {
                    if (s_hist[d] >= want) break;
                    want -= s_hist[d];
                }
                s_prefix = prefix | ((key_t64)d << shift);
                s_misc[4] = want;
            }
            mask |= (key_t64)255 << shift;
            __syncthreads();
        }
        compact(s_prefix);   // (the kg-th smallest key: a real one, below KEY_PAD)
        __syncthreads();
        const uint32_t got = s_misc[1];
        m = got < PF_SORT ? got : PF_SORT;   // == kg: keys are unique
    }
    uint32_t mp = 1;
    while (mp < m) mp <<= 1;
    const f32x4 *q4 = reinterpret_cast<const f32x4 *>(p.queries + (size_t)qi * 256);
    for (uint32_t i = threadIdx.x; i < mp; i += PF_THREADS) {
        uint64_t dbits = 0x7FF0000000000000ull;
        uint32_t r = 0xFFFFFFFFu;
        const key_t64 key = i < m ? s_keys[i] : KEY_PAD;
        const uint32_t row = (uint32_t)(key & 0xFFFFFFFFull);
        if (key != KEY_PAD && (uint64_t)row < p.n_rows) {
            const double d = exact_distance(q4, reinterpret_cast<const f32x4 *>(p.corpus + (uint64_t)row * 256));
            if (d == d) { dbits = (uint64_t)__double_as_longlong(d); r = row; atomicAdd(&s_misc[3], 1u); }
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
    const uint32_t kept = s_misc[3];
    const uint32_t n_out = kept < p.top_k ? kept : p.top_k;
    uint64_t *orow = p.out_rows + (size_t)qi * p.out_stride;
    double *odist = p.out_dist + (size_t)qi * p.out_stride;
    for (uint32_t t = threadIdx.x; t < p.top_k; t += PF_THREADS) {
        if (t < n_out) { orow[t] = p.row_base + s_row[t]; odist[t] = __longlong_as_double((long long)s_dbits[t]); }
        else { orow[t] = 0xFFFFFFFFFFFFFFFFull; odist[t] = __builtin_inf(); }
    }
    if (threadIdx.x == 0) {
        if (p.out_counts) p.out_counts[qi] = n_out;
        // (a query outside the domain, domain.hip: the host forms refuse it before the launch, a device form counts it like the select)
        if (!magnitude_in_domain(s_misc[2]) && p.status) atomicAdd(p.status, 1ull);
    }
}

static void launch_adc_pool(uint32_t kind, int adc_waves, bool filtered, dim3 grid, hipStream_t st, const AdcParams &ap)
{
    if (filtered) {
        if (kind == 1) {
            if (adc_waves == 8) hipLaunchKernelGGL((ivf_adc_pool_kernel<512, 1, true>), grid, dim3(512), 0, st, ap);
            else hipLaunchKernelGGL((ivf_adc_pool_kernel<256, 1, true>), grid, dim3(256), 0, st, ap);
        } else {
            if (adc_waves == 8) hipLaunchKernelGGL((ivf_adc_pool_kernel<512, 0, true>), grid, dim3(512), 0, st, ap);
            else hipLaunchKernelGGL((ivf_adc_pool_kernel<256, 0, true>), grid, dim3(256), 0, st, ap);
        }
    } else if (kind == 1) {
        if (adc_waves == 8) hipLaunchKernelGGL((ivf_adc_pool_kernel<512, 1, false>), grid, dim3(512), 0, st, ap);
        else hipLaunchKernelGGL((ivf_adc_pool_kernel<256, 1, false>), grid, dim3(256), 0, st, ap);
    } else {
        if (adc_waves == 8) hipLaunchKernelGGL((ivf_adc_pool_kernel<512, 0, false>), grid, dim3(512), 0, st, ap);
        else hipLaunchKernelGGL((ivf_adc_pool_kernel<256, 0, false>), grid, dim3(256), 0, st, ap);
    }
}

}  // namespace smt

using namespace smt;


// The pinned buffer a ranged call writes its ranges into (smt_ctx::h_ivf_ranges), at least `bytes` long and free to be overwritten:
// the previous ranged call's upload has left it.  Waiting for that upload's event is not waiting for the stream -- the searches
// enqueued since go on running -- and a buffer that is never reused while in flight is what lets the _device form return at once.
static int ranges_pinned(smt_ctx *ctx, size_t bytes, smt_range **pin)
{
    if (!ctx->ivf_ranges_up) IVF_HIP(hipEventCreateWithFlags(&ctx->ivf_ranges_up, hipEventDisableTiming));
    else IVF_HIP(hipEventSynchronize(ctx->ivf_ranges_up));
    if (bytes > ctx->ivf_ranges_bytes) {
        if (ctx->h_ivf_ranges) IVF_HIP(hipHostFree(ctx->h_ivf_ranges));
        ctx->h_ivf_ranges = nullptr;
        ctx->ivf_ranges_bytes = 0;
        const size_t want = std::max(bytes, (size_t)1 << 16);
        IVF_HIP(hipHostMalloc(&ctx->h_ivf_ranges, want, hipHostMallocDefault));
        ctx->ivf_ranges_bytes = want;
    }
    *pin = reinterpret_cast<smt_range *>(ctx->h_ivf_ranges);
    return SMT_OK;
}

extern "C" {

// How a search cuts the probed lists into blocks: segments per list, their length, waves per block and shortlist per wave.  The same
// for the narrow and the wide route (`rerank` as the caller gave it, 0 = 512, checked).
struct AdcPlan {
    uint32_t n_seg, seg_len, shortlist;
    int adc_waves;
};

static AdcPlan adc_plan(const smt_ivfpq *ix, uint32_t nprobe, uint32_t rerank)
{
    AdcPlan pl;
    // A list longer than ADC_SEGMENT codes is scanned by several blocks, each with its own shortlist of `rerank`
    // candidates (config 5's 100 M rows over 4096 lists: 24 k codes per list -- one shortlist of 512 would re-score
    // 2 % of them and recall@10 drops to 0.75); the select stage takes at most 512 lists per query.
    constexpr uint64_t ADC_SEGMENT = 8192;
    // sized by the TYPICAL list (1.5 x the mean), not the longest: a block that finds its segment empty still costs a
    // launch slot (+0.3 ms per 1000 queries when every list got a second, almost always empty, segment); the last
    // segment of an unusually long list simply takes the rest
    const uint64_t typical = (ix->n_rows / std::max<uint32_t>(ix->nlist, 1u)) * 3 / 2;
    uint32_t n_seg = (uint32_t)std::max<uint64_t>(1, (typical + ADC_SEGMENT - 1) / ADC_SEGMENT);
    // ... and when that limit takes segments away (nprobe 128 over 100 M rows: 4 instead of 5), the typical list is cut into EQUAL
    // longer segments -- with ADC_SEGMENT kept, the last one took a double share behind one shortlist and recall@10 FELL with
    // nprobe (0.9795 at 32, 0.9708 at 128)
    const uint32_t want_seg = n_seg;
    n_seg = std::min<uint32_t>(n_seg, std::max<uint32_t>(1u, 512u / nprobe));
    const uint32_t seg_len = n_seg < want_seg ? (uint32_t)(((typical + n_seg - 1) / n_seg + 255) & ~(uint64_t)255) : (uint32_t)ADC_SEGMENT;
    // (... each with a shortlist longer by the same factor: the re-scored fraction of a list does not depend on nprobe)
    if (n_seg < want_seg) rerank = std::min<uint32_t>(512u, (rerank * want_seg + n_seg - 1) / n_seg);

    // waves per (query, list segment) block.  (PQ, kind 0, with 8-wave blocks -- two blocks' worth of waves sharing one 32 KiB LUT --
    // measured +4 % queries/s for -0.5 point of recall@10 at rerank 128: sixteen candidates per wave are too few.  Not taken.)
    pl.adc_waves = rerank > 256 ? 8 : 4;
    pl.shortlist = (rerank + pl.adc_waves - 1) / pl.adc_waves;  // per wave
    pl.n_seg = n_seg;
    pl.seg_len = seg_len;
    return pl;
}

// `filtered`: the search is inside `ranges` (VALID corpus-local rows: the callers check them); without it the ranges are not looked
// at and every launch, every scratch offset and every byte of the answer is what it was before ranges existed.  A filter that
// leaves nothing (no range, or empty ones only) is still a filter: the mask is all zeros and the answer is empty.
static int ivfpq_search_core(smt_ivfpq *ix, const float *queries, bool queries_on_device, uint32_t nq, uint32_t top_k, uint32_t nprobe,
                             uint32_t rerank, const smt_range *ranges, uint32_t n_ranges, bool filtered, uint64_t row_base,
                             uint64_t *d_or_user, double *d_od_user, uint64_t *d_oc_user,
                             uint64_t **d_or_out, size_t *out_bytes_contig, uint64_t out_stride = 0, smt::Delivery *deliver = nullptr,
                             bool wide = false)
{
    smt_ctx *ctx = ix->corpus->ctx;
    IVF_REQUIRE_FRESH(ix);
    SMT_REQUIRE(ix->corpus->rows >= ix->n_rows, "the corpus shrank after the index was built: rebuild");
    SMT_REQUIRE(nprobe >= 1 && nprobe <= ix->nlist && nprobe <= 512, "nprobe must be in [1, min(nlist, 512)]");
    if (wide) SMT_REQUIRE(top_k > SCAN_MAX_K && top_k <= LARGEK_MAX_K, "top_k must be <= 1024 for the wide IVF-PQ path");
    else SMT_REQUIRE(top_k <= 56, "top_k must be <= 56 for the IVF-PQ path");
    if (rerank == 0) rerank = 512;
    SMT_REQUIRE(rerank >= 4 && rerank <= 512, "rerank (full-precision re-scored ADC candidates per probed list) must be in [4, 512]");
    const AdcPlan plan = adc_plan(ix, nprobe, rerank);
    const uint32_t n_seg = plan.n_seg, seg_len = plan.seg_len, shortlist = plan.shortlist;
    const int adc_waves = plan.adc_waves;
    const uint32_t kp = top_k + 8;                // re-scored candidates handed to the exact select stage (narrow route)
    // wide: every re-scored row of a query goes to its pool, [nprobe * n_seg][waves * 64] keys (at most 512 x 512 = 2 MiB); a batch
    // whose pool would pass IVF_POOL_BUDGET runs in rounds of queries, each round the whole route on its part of the caller's buffers
    const uint32_t pool_slots = (uint32_t)adc_waves * 64u;
    const size_t pool_per_query = (size_t)nprobe * n_seg * pool_slots * sizeof(key_t64);
    if (wide && (size_t)nq * pool_per_query > IVF_POOL_BUDGET) {
        SMT_REQUIRE(queries_on_device && d_or_user && d_od_user && !deliver, "a wide search in rounds writes to the caller's device buffers");
        const uint32_t nq_round = (uint32_t)std::max<size_t>(1, IVF_POOL_BUDGET / pool_per_query);
        const uint64_t stride = out_stride ? out_stride : top_k;
        for (uint32_t q0 = 0; q0 < nq; q0 += nq_round) {
            const int rc_round = ivfpq_search_core(ix, queries + (size_t)q0 * 256, true, std::min(nq_round, nq - q0), top_k, nprobe, rerank, ranges,
                                                   n_ranges, filtered, row_base, d_or_user + (size_t)q0 * stride, d_od_user + (size_t)q0 * stride,
                                                   d_oc_user ? d_oc_user + q0 : nullptr, nullptr, nullptr, out_stride, nullptr, true);
            if (rc_round) return rc_round;
        }
        return SMT_OK;
    }
    // every temporary lives in the context's scratch (no hipMalloc/hipFree per call), results come back through
    // the pinned staging buffer
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_q = 0, b_q = 2 * al((size_t)nq * 256 * 4);   // [the queries as given (host form) | their unit-length copies]
    const size_t o_pl = o_q + b_q, b_pl = al((size_t)nq * nprobe * 4);
    const size_t o_pd = o_pl + b_pl, b_pd = b_pl;
    const size_t o_lut = o_pd + b_pd, b_lut = al((size_t)nq * PQ_M * PQ_K * 4);
    const size_t o_lists = o_lut + b_lut, b_lists = wide ? 0 : al((size_t)nq * nprobe * n_seg * kp * 8);
    const size_t o_or = o_lists + b_lists, b_or = (size_t)nq * top_k * 8;   // rows | dist | counts contiguous: one D2H
    const size_t o_od = o_or + b_or, b_od = b_or;
    const size_t o_oc = o_od + b_od, b_oc = al((size_t)nq * 8);
    const size_t o_sc = o_oc + b_oc, b_sc = al((size_t)nq * ix->nlist * 4);
    const size_t o_lw = o_sc + b_sc, b_lw = ix->kind == 1 ? al((size_t)nq * nprobe * PQ_M * 4) : 0;
    // inside ranges: the non-empty ranges and the list-order bitmap built from them, behind everything else (0 bytes without a filter)
    uint32_t n_rr = 0;
    for (uint32_t i = 0; filtered && i < n_ranges; ++i) n_rr += ranges[i].end > ranges[i].begin ? 1u : 0u;
    const uint64_t mask_words = (ix->n_rows + 63) / 64;
    const size_t o_rg = o_lw + b_lw, b_rg = filtered ? al((size_t)n_rr * sizeof(smt_range)) : 0;
    const size_t o_mask = o_rg + b_rg, b_mask = filtered ? al((size_t)mask_words * 8) : 0;
    const size_t o_pool = o_mask + b_mask, b_pool = wide ? al((size_t)nq * pool_per_query) : 0;   // (behind everything of the narrow route)
    int rc = smt::ensure_scratch(ctx, o_pool + b_pool);
    if (rc) return rc;
    char *base = reinterpret_cast<char *>(ctx->d_scratch);
    if (filtered) {   // (rebuilt on every call: no mask outlives its search)
        const smt_range *d_rg = reinterpret_cast<const smt_range *>(base + o_rg);
        if (n_rr) {   // through the context's pinned range buffer: enqueued, not waited for
            smt_range *pin = nullptr;
            if ((rc = ranges_pinned(ctx, (size_t)n_rr * sizeof(smt_range), &pin))) return rc;
            uint32_t w = 0;
            for (uint32_t i = 0; i < n_ranges; ++i)
                if (ranges[i].end > ranges[i].begin) pin[w++] = ranges[i];
            IVF_HIP(hipMemcpyAsync(base + o_rg, pin, (size_t)n_rr * sizeof(smt_range), hipMemcpyHostToDevice, ctx->stream));
            IVF_HIP(hipEventRecord(ctx->ivf_ranges_up, ctx->stream));
        }
        const uint64_t words_per_block = (uint64_t)(MASK_THREADS / 64) * MASK_WORDS_PER_WAVE;
        prof_begin(ctx, "ivf_mask");
        if (mask_words)
            hipLaunchKernelGGL(ivf_range_mask_kernel, dim3((unsigned)((mask_words + words_per_block - 1) / words_per_block)), dim3(MASK_THREADS),
                               0, ctx->stream, ix->d_ids, ix->n_rows, d_rg, n_rr, reinterpret_cast<uint64_t *>(base + o_mask));
        prof_end(ctx, "ivf_mask");
    }
    const float *d_q = queries;
    if (!queries_on_device) {
        IVF_HIP(hipMemcpyAsync(base + o_q, queries, (size_t)nq * 256 * 4, hipMemcpyHostToDevice, ctx->stream));
        d_q = reinterpret_cast<const float *>(base + o_q);
    }
    const float *d_q_given = d_q;   // (the exact select re-scores against these)
    {
        float *d_unit = reinterpret_cast<float *>(base + o_q + b_q / 2);
        hipLaunchKernelGGL(ivf_unit_queries_kernel, dim3((nq + 3) / 4), dim3(256), 0, ctx->stream, d_q, nq, d_unit);
        d_q = d_unit;
    }

    if (!(ctx->attr_done & ATTR_IVF_SCORE)) {
        IVF_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(ivf_score_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        ctx->attr_done |= ATTR_IVF_SCORE;
    }
    ProbeParams pp;
    pp.queries = d_q;
    pp.centroids = ix->d_centroids;
    pp.cnorm_half = ix->d_cnorm_half;
    pp.nlist = ix->nlist;
    pp.nprobe = nprobe;
    pp.probe_list = reinterpret_cast<uint32_t *>(base + o_pl);
    pp.probe_dot = reinterpret_cast<float *>(base + o_pd);
    float *d_scores = reinterpret_cast<float *>(base + o_sc);
    prof_begin(ctx, "ivf_probe");
    hipLaunchKernelGGL(ivf_score_kernel, dim3(ix->nlist / QT_ROWS), dim3(GEMM_THREADS), (size_t)QT_F4 * 16 + 64, ctx->stream, d_q, nq,
                       ix->d_centroids, ix->d_cnorm_half, ix->nlist, d_scores);
    hipLaunchKernelGGL(ivf_probe_select_kernel, dim3((nq + 3) / 4), dim3(256), 0, ctx->stream, pp, d_scores, nq);
    if (ix->kind == 1) {
        const uint64_t n_pairs = (uint64_t)nq * nprobe;
        hipLaunchKernelGGL(lpca_project_kernel, dim3((unsigned)((n_pairs * 64 + 255) / 256)), dim3(256), 0, ctx->stream, d_q, pp.probe_list,
                           n_pairs, nprobe, ix->d_basis, ix->d_lscale, reinterpret_cast<float *>(base + o_lw));
    } else {
        hipLaunchKernelGGL(ivf_lut_kernel, dim3(nq, PQ_K / 8), dim3(256), 0, ctx->stream, d_q, ix->d_codebooks, reinterpret_cast<float *>(base + o_lut));
    }
    prof_end(ctx, "ivf_probe");
    AdcParams ap;
    ap.queries = d_q;
    ap.lut = reinterpret_cast<float *>(base + o_lut);
    ap.lw = ix->kind == 1 ? reinterpret_cast<const float *>(base + o_lw) : nullptr;
    ap.probe_list = pp.probe_list;
    ap.probe_dot = pp.probe_dot;
    ap.nprobe = nprobe;
    ap.nq = nq;
    ap.list_offsets = ix->d_offsets;
    ap.codes = ix->d_codes;
    ap.ids = ix->d_ids;
    ap.corpus = ix->corpus->d_rows;
    ap.n_seg = n_seg;
    ap.seg_len = seg_len ? seg_len : 512;
    ap.shortlist = shortlist;
    ap.kp = kp;
    ap.lists = reinterpret_cast<key_t64 *>(base + (wide ? o_pool : o_lists));
    ap.mask = filtered ? reinterpret_cast<const uint64_t *>(base + o_mask) : nullptr;
    prof_begin(ctx, "ivf_adc");
    const dim3 adc_grid(((nq + 7) / 8) * 8 * nprobe * n_seg);   // (one line: see the XCD-aware order in the kernel)
    if (wide) launch_adc_pool(ix->kind, adc_waves, filtered, adc_grid, ctx->stream, ap);
    else if (filtered) {
        if (ix->kind == 1) {
            if (adc_waves == 8) hipLaunchKernelGGL((ivf_adc_kernel<512, 1, true>), adc_grid, dim3(512), 0, ctx->stream, ap);
            else hipLaunchKernelGGL((ivf_adc_kernel<256, 1, true>), adc_grid, dim3(256), 0, ctx->stream, ap);
        } else {
            if (adc_waves == 8) hipLaunchKernelGGL((ivf_adc_kernel<512, 0, true>), adc_grid, dim3(512), 0, ctx->stream, ap);
            else hipLaunchKernelGGL((ivf_adc_kernel<256, 0, true>), adc_grid, dim3(256), 0, ctx->stream, ap);
        }
    } else if (ix->kind == 1) {
        if (adc_waves == 8) hipLaunchKernelGGL((ivf_adc_kernel<512, 1, false>), adc_grid, dim3(512), 0, ctx->stream, ap);
        else hipLaunchKernelGGL((ivf_adc_kernel<256, 1, false>), adc_grid, dim3(256), 0, ctx->stream, ap);
    } else {
        if (adc_waves == 8) hipLaunchKernelGGL((ivf_adc_kernel<512, 0, false>), adc_grid, dim3(512), 0, ctx->stream, ap);
        else hipLaunchKernelGGL((ivf_adc_kernel<256, 0, false>), adc_grid, dim3(256), 0, ctx->stream, ap);
    }
    prof_end(ctx, "ivf_adc");
    IVF_HIP(hipGetLastError());
    uint64_t *d_or = d_or_user ? d_or_user : reinterpret_cast<uint64_t *>(base + o_or);
    double *d_od = d_od_user ? d_od_user : reinterpret_cast<double *>(base + o_od);
    uint64_t *d_oc = d_or_user ? d_oc_user : reinterpret_cast<uint64_t *>(base + o_oc);
    if (wide) {   // the pool's finish in place of the select stage
        PoolFinishParams fp;
        fp.corpus = ix->corpus->d_rows;
        fp.n_rows = ix->n_rows;
        fp.queries = d_q_given;
        fp.pool = ap.lists;
        fp.P = nprobe * n_seg * pool_slots;
        fp.top_k = top_k;
        fp.kg = top_k + std::max<uint32_t>(64, top_k / 16);
        fp.row_base = row_base;
        fp.out_rows = d_or;
        fp.out_dist = d_od;
        fp.out_counts = d_oc;
        fp.out_stride = out_stride ? out_stride : top_k;
        fp.status = ctx->d_status;
        prof_begin(ctx, "ivf_finish");
        hipLaunchKernelGGL(ivf_pool_finish_kernel, dim3(nq), dim3(PF_THREADS), 0, ctx->stream, fp);
        prof_end(ctx, "ivf_finish");
        IVF_HIP(hipGetLastError());
        if (d_or_out) *d_or_out = d_or;
        if (out_bytes_contig) *out_bytes_contig = b_or + b_od + (size_t)nq * 8;
        return SMT_OK;
    }
    SelectArgs sel;  // no exactness certificate: the index is approximate by contract (f32_err = 0)
    sel.corpus = ix->corpus->d_rows;
    sel.queries = d_q_given;
    sel.nq = nq;
    sel.lists = ap.lists;
    sel.n_lists = nprobe * n_seg;
    sel.kp = kp;
    sel.list_stride = (uint64_t)nprobe * n_seg * kp;
    sel.k_out = top_k;
    sel.row_base = row_base;
    sel.out_rows = d_or;
    sel.out_dist = d_od;
    sel.out_counts = d_oc;
    sel.out_stride = out_stride;
    if (deliver) {   // (host form, small answer: the select kernel carries [rows | distances | counts] home -- common.h Delivery)
        deliver->dev_out = reinterpret_cast<const unsigned long long *>(d_or);
        deliver->n_words = (uint32_t)((b_or + b_od + (size_t)nq * 8) / 8);
        sel.deliver = deliver;
    }
    rc = launch_select(ctx, sel);
    if (rc) return rc;
    if (d_or_out) *d_or_out = d_or;
    if (out_bytes_contig) *out_bytes_contig = b_or + b_od + (size_t)nq * 8;
    return SMT_OK;
}

// The wide host form, 57 <= top_k <= LARGEK_MAX_K: rounds of queries under the pool's byte budget, each round's answer copied home
// and waited for (no delivery by a kernel: nothing here is latency-bound at these sizes).
static int ivfpq_search_host_wide(smt_ivfpq *ix, const float *queries, uint32_t nq, uint32_t top_k, uint32_t nprobe, uint32_t rerank,
                                  const smt_range *ranges, uint32_t n_ranges, bool filtered, uint64_t row_base, uint64_t *out_rows,
                                  double *out_dist, uint64_t *out_counts, uint64_t out_cap)
{
    if (int rcr = smt::validate_ranges(ranges, n_ranges, ix->corpus->rows)) return rcr;
    SMT_REQUIRE(nprobe >= 1 && nprobe <= ix->nlist && nprobe <= 512, "nprobe must be in [1, min(nlist, 512)]");
    SMT_REQUIRE(rerank == 0 || (rerank >= 4 && rerank <= 512), "rerank (full-precision re-scored ADC candidates per probed list) must be in [4, 512]");
    smt_ctx *ctx = ix->corpus->ctx;
    IVF_HIP(hipSetDevice(ctx->device));
    { int rc_drain = smt::drain_async(ctx); if (rc_drain) return rc_drain; }
    if (nq == 0) return SMT_OK;
    for (uint32_t q = 0; q < nq; ++q) out_counts[q] = 0;
    if (int rcq = smt::require_queries_domain_host(queries, nq, "smt_ivfpq_search_wide")) return rcq;   // (domain.hip)
    const AdcPlan plan = adc_plan(ix, nprobe, rerank ? rerank : 512);
    const size_t pool_per_query = (size_t)nprobe * plan.n_seg * plan.adc_waves * 64 * sizeof(key_t64);
    const uint32_t nq_round = (uint32_t)std::min<size_t>(nq, std::max<size_t>(1, IVF_POOL_BUDGET / pool_per_query));
    const size_t b_or = (size_t)nq_round * top_k * 8;
    int rc = smt::ensure_pinned(ctx, 2 * b_or + (size_t)nq_round * 8);
    if (rc) return rc;
    char *h_ans = reinterpret_cast<char *>(ctx->h_pinned);
    bool truncated = false;
    for (uint32_t q0 = 0; q0 < nq; q0 += nq_round) {
        const uint32_t nqr = std::min(nq_round, nq - q0);
        uint64_t *d_or = nullptr;
        size_t out_bytes = 0;
        rc = ivfpq_search_core(ix, queries + (size_t)q0 * 256, false, nqr, top_k, nprobe, rerank, ranges, n_ranges, filtered, row_base, nullptr,
                               nullptr, nullptr, &d_or, &out_bytes, 0, nullptr, true);
        if (rc) return rc;
        IVF_HIP(hipMemcpyAsync(h_ans, d_or, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
        IVF_HIP(hipStreamSynchronize(ctx->stream));
        const size_t b_r = (size_t)nqr * top_k * 8;   // [rows | distances | counts] of this round
        const uint64_t *h_rows = reinterpret_cast<const uint64_t *>(h_ans);
        const double *h_dist = reinterpret_cast<const double *>(h_ans + b_r);
        const uint64_t *h_cnt = reinterpret_cast<const uint64_t *>(h_ans + 2 * b_r);
        for (uint32_t q = 0; q < nqr; ++q) {
            out_counts[q0 + q] = h_cnt[q];
            const uint64_t w = std::min<uint64_t>(h_cnt[q], out_cap);
            if (h_cnt[q] > out_cap) truncated = true;
            for (uint64_t i = 0; i < w; ++i) {
                out_rows[(size_t)(q0 + q) * out_cap + i] = h_rows[(size_t)q * top_k + i];
                out_dist[(size_t)(q0 + q) * out_cap + i] = h_dist[(size_t)q * top_k + i];
            }
        }
    }
    if (truncated) { smt::set_error("out_cap smaller than the number of hits"); return SMT_E_TRUNCATED; }
    return SMT_OK;
}

// the host form of the search, with or without ranges (`filtered`); `wide`: top_k up to LARGEK_MAX_K (57 and above through the pool)
static int ivfpq_search_host(smt_ivfpq *ix, const float *queries, uint32_t nq, uint32_t top_k, uint32_t nprobe, uint32_t rerank,
                             const smt_range *ranges, uint32_t n_ranges, bool filtered, uint64_t row_base, uint64_t *out_rows,
                             double *out_dist, uint64_t *out_counts, uint64_t out_cap, bool wide = false)
{
    SMT_REQUIRE(ix != nullptr, "index");
    SMT_REQUIRE(nq == 0 || (queries && out_rows && out_dist && out_counts), "null argument");
    SMT_REQUIRE(!wide || top_k <= LARGEK_MAX_K, "top_k must be <= 1024 for the wide IVF-PQ path");
    SMT_REQUIRE(n_ranges == 0 || ranges != nullptr, "ranges");
    if (wide && top_k > SCAN_MAX_K)
        return ivfpq_search_host_wide(ix, queries, nq, top_k, nprobe, rerank, ranges, n_ranges, filtered, row_base, out_rows, out_dist,
                                      out_counts, out_cap);
    if (int rcr = smt::validate_ranges(ranges, n_ranges, ix->corpus->rows)) return rcr;
    smt_ctx *ctx = ix->corpus->ctx;
    IVF_HIP(hipSetDevice(ctx->device));
    { int rc_drain = smt::drain_async(ctx); if (rc_drain) return rc_drain; }
    if (nq == 0) return SMT_OK;
    for (uint32_t q = 0; q < nq; ++q) out_counts[q] = 0;
    if (int rcq = smt::require_queries_domain_host(queries, nq, "smt_ivfpq_search")) return rcq;   // (domain.hip)
    if (top_k == 0) return SMT_OK;
    uint64_t *d_or = nullptr;
    size_t out_bytes = 0;
    const size_t b_or = (size_t)nq * top_k * 8, b_od = b_or;
    // a small answer is delivered by the select kernel (as in smt_search: search.cpp), a large one copied and waited for
    const bool direct = ctx->tune.direct_delivery != 0 && nq <= 32 && b_or + b_od + (size_t)nq * 8 <= 8192;
    int rc = smt::ensure_pinned(ctx, 64 + b_or + b_od + (size_t)nq * 8);
    if (rc) return rc;
    char *h_ans = reinterpret_cast<char *>(ctx->h_pinned) + 64;
    volatile unsigned long long *flag = reinterpret_cast<volatile unsigned long long *>(ctx->h_pinned);
    smt::Delivery dl;
    if (direct) {
        dl.host_out = reinterpret_cast<unsigned long long *>(h_ans);
        dl.host_flag = const_cast<unsigned long long *>(flag);
        dl.seq = ++ctx->deliver_seq;
        dl.done = ctx->d_status + 4;
        *flag = 0;
    }
    rc = ivfpq_search_core(ix, queries, false, nq, top_k, nprobe, rerank, ranges, n_ranges, filtered, row_base, nullptr, nullptr,
                           nullptr, &d_or, &out_bytes, 0, direct ? &dl : nullptr);
    if (rc) return rc;
    if (direct) {
        const auto t0 = std::chrono::steady_clock::now();
        unsigned long long got = 0;
        for (unsigned spins = 1; (got = *flag) == 0; ++spins) {
            if ((spins & 63) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(200)) {
                IVF_HIP(hipStreamSynchronize(ctx->stream));
                got = *flag;
                break;
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        if (got != dl.seq) {
            (void)hipStreamSynchronize(ctx->stream);
            (void)hipMemsetAsync(ctx->d_status + 4, 0, sizeof(unsigned long long), ctx->stream);
            smt::set_error("the select kernel did not deliver its answer (completion word %llu, expected %llu)", got, dl.seq);
            return SMT_E_HIP;
        }
        ++ctx->deliveries;
    } else {
        IVF_HIP(hipMemcpyAsync(h_ans, d_or, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
        IVF_HIP(hipStreamSynchronize(ctx->stream));
    }
    const uint64_t *h_rows = reinterpret_cast<const uint64_t *>(h_ans);
    const double *h_dist = reinterpret_cast<const double *>(h_ans + b_or);
    const uint64_t *h_cnt = reinterpret_cast<const uint64_t *>(h_ans + b_or + b_od);
    bool truncated = false;
    for (uint32_t q = 0; q < nq; ++q) {
        out_counts[q] = h_cnt[q];
        const uint64_t w = std::min<uint64_t>(h_cnt[q], out_cap);
        if (h_cnt[q] > out_cap) truncated = true;
        for (uint64_t i = 0; i < w; ++i) {
            out_rows[(size_t)q * out_cap + i] = h_rows[(size_t)q * top_k + i];
            out_dist[(size_t)q * out_cap + i] = h_dist[(size_t)q * top_k + i];
        }
    }
    if (truncated) { smt::set_error("out_cap smaller than the number of hits"); return SMT_E_TRUNCATED; }
    return SMT_OK;
}

static int ivfpq_search_dev(smt_ivfpq *ix, const float *queries_dev, uint32_t nq, uint32_t top_k, uint32_t nprobe, uint32_t rerank,
                            const smt_range *ranges, uint32_t n_ranges, bool filtered, uint64_t row_base, uint64_t *out_rows_dev,
                            double *out_dist_dev, bool wide = false)
{
    SMT_REQUIRE(ix != nullptr, "index");
    SMT_REQUIRE(nq == 0 || (queries_dev && out_rows_dev && out_dist_dev), "null argument");
    SMT_REQUIRE(top_k >= 1, "top_k");
    SMT_REQUIRE(!wide || top_k <= LARGEK_MAX_K, "top_k must be <= 1024 for the wide IVF-PQ path");
    SMT_REQUIRE(n_ranges == 0 || ranges != nullptr, "ranges");
    if (int rcr = smt::validate_ranges(ranges, n_ranges, ix->corpus->rows)) return rcr;
    smt_ctx *ctx = ix->corpus->ctx;
    IVF_HIP(hipSetDevice(ctx->device));
    { int rc_drain = smt::drain_async(ctx); if (rc_drain) return rc_drain; }
    if (nq == 0) return SMT_OK;
    return ivfpq_search_core(ix, queries_dev, true, nq, top_k, nprobe, rerank, ranges, n_ranges, filtered, row_base, out_rows_dev,
                             out_dist_dev, nullptr, nullptr, nullptr, 0, nullptr, wide && top_k > SCAN_MAX_K);
}

int smt_ivfpq_search(smt_ivfpq *ix, const float *queries, uint32_t nq, uint32_t top_k, uint32_t nprobe, uint32_t rerank,
                     uint64_t row_base, uint64_t *out_rows, double *out_dist, uint64_t *out_counts, uint64_t out_cap)
try {
    return ivfpq_search_host(ix, queries, nq, top_k, nprobe, rerank, nullptr, 0, false, row_base, out_rows, out_dist, out_counts, out_cap);
} catch (...) { return smt::api_catch(); }

int smt_ivfpq_search_ranges(smt_ivfpq *ix, const float *queries, uint32_t nq, uint32_t top_k, uint32_t nprobe, uint32_t rerank,
                            const smt_range *ranges, uint32_t n_ranges, uint64_t row_base, uint64_t *out_rows, double *out_dist,
                            uint64_t *out_counts, uint64_t out_cap)
try {
    return ivfpq_search_host(ix, queries, nq, top_k, nprobe, rerank, ranges, n_ranges, n_ranges != 0, row_base, out_rows, out_dist, out_counts,
                             out_cap);
} catch (...) { return smt::api_catch(); }

int smt_ivfpq_search_device(smt_ivfpq *ix, const float *queries_dev, uint32_t nq, uint32_t top_k, uint32_t nprobe, uint32_t rerank,
                            uint64_t row_base, uint64_t *out_rows_dev, double *out_dist_dev)
try {
    return ivfpq_search_dev(ix, queries_dev, nq, top_k, nprobe, rerank, nullptr, 0, false, row_base, out_rows_dev, out_dist_dev);
} catch (...) { return smt::api_catch(); }

int smt_ivfpq_search_ranges_device(smt_ivfpq *ix, const float *queries_dev, uint32_t nq, uint32_t top_k, uint32_t nprobe, uint32_t rerank,
                                   const smt_range *ranges, uint32_t n_ranges, uint64_t row_base, uint64_t *out_rows_dev,
                                   double *out_dist_dev)
try {
    return ivfpq_search_dev(ix, queries_dev, nq, top_k, nprobe, rerank, ranges, n_ranges, n_ranges != 0, row_base, out_rows_dev, out_dist_dev);
} catch (...) { return smt::api_catch(); }

int smt_ivfpq_search_wide(smt_ivfpq *ix, const float *queries, uint32_t nq, uint32_t top_k, uint32_t nprobe, uint32_t rerank,
                          const smt_range *ranges, uint32_t n_ranges, uint64_t row_base, uint64_t *out_rows, double *out_dist,
                          uint64_t *out_counts, uint64_t out_cap)
try {
    return ivfpq_search_host(ix, queries, nq, top_k, nprobe, rerank, ranges, ranges ? n_ranges : 0, ranges != nullptr, row_base, out_rows,
                             out_dist, out_counts, out_cap, true);
} catch (...) { return smt::api_catch(); }

int smt_ivfpq_search_wide_device(smt_ivfpq *ix, const float *queries_dev, uint32_t nq, uint32_t top_k, uint32_t nprobe, uint32_t rerank,
                                 const smt_range *ranges, uint32_t n_ranges, uint64_t row_base, uint64_t *out_rows_dev, double *out_dist_dev)
try {
    return ivfpq_search_dev(ix, queries_dev, nq, top_k, nprobe, rerank, ranges, ranges ? n_ranges : 0, ranges != nullptr, row_base,
                            out_rows_dev, out_dist_dev, true);
} catch (...) { return smt::api_catch(); }

}  // extern "C"

// one shard's answer in the packed exchange layout of group_exchange.cpp: [nq][2][top_k] words (global rows | f64 bits)
// (`filtered` apart from the count, as in search_topk_packed_local: a shard that the caller's ranges leave nothing returns NOTHING;
// ranges_local come out of layout_localize from ranges the caller validated)
int smt::ivfpq_search_packed(smt_ivfpq *ix, const float *queries_dev, uint32_t nq, uint32_t top_k, uint32_t nprobe, uint32_t rerank,
                             const smt_range *ranges_local, uint32_t n_ranges, bool filtered, uint64_t row_base, uint64_t *packed_dev,
                             bool wide)
{
    SMT_REQUIRE(ix && queries_dev && packed_dev, "null argument");
    smt_ctx *ctx = ix->corpus->ctx;
    IVF_HIP(hipSetDevice(ctx->device));
    { int rc_drain = smt::drain_async(ctx); if (rc_drain) return rc_drain; }
    return ivfpq_search_core(ix, queries_dev, true, nq, top_k, nprobe, rerank, ranges_local, n_ranges, filtered, row_base, packed_dev,
                             reinterpret_cast<double *>(packed_dev + top_k), nullptr, nullptr, nullptr, (uint64_t)2 * top_k, nullptr,
                             wide && top_k > SCAN_MAX_K);
}