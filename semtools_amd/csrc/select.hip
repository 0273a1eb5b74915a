// select.hip -- the select stage: block lists (one sorted list of k' keys per scan block, or per level select of the
// batched kernel) -> the best k_out rows per query with exact f64 distances, the exactness certificate and the status
// words, in one launch per call (final_select_kernel, launch_select); optionally on the aux stream while the next scan
// runs (async select, device_flags.h).  Also the stand-alone exact rescoring and row gather kernels, which run under the
// same "select" profiling label.
// gfx950 only (wave64).
#include "common.h"
#include "device_utils.h"
#include "device_flags.h"

namespace smt {

// --------------------------------------------------- exact f64 distance (A5): device_utils.h exact_distance
__global__ void rescore_rows_kernel(const float *corpus, const float *query, const uint32_t *rows,
                                    uint64_t n, double *out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        out[i] = exact_distance(reinterpret_cast<const f32x4 *>(query),
                                reinterpret_cast<const f32x4 *>(corpus + (uint64_t)rows[i] * 256));
}

// the same for the rows of MANY queries in one launch: row i belongs to query qidx[i] of the [n_queries][256] block
__global__ void rescore_rows_multi_kernel(const float *corpus, const float *queries, const uint32_t *rows, const uint32_t *qidx,
                                          uint64_t n, double *out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        out[i] = exact_distance(reinterpret_cast<const f32x4 *>(queries + (uint64_t)qidx[i] * 256),
                                reinterpret_cast<const f32x4 *>(corpus + (uint64_t)rows[i] * 256));
}

// dst[i] = src[idx[i]] for rows of 256 f32: one wave per row
__global__ void gather_rows256_kernel(const float *src, const uint32_t *idx, uint32_t n, float *dst)
{
    const uint32_t i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i < n)
        reinterpret_cast<f32x4 *>(dst + (size_t)i * 256)[threadIdx.x & 63] =
            reinterpret_cast<const f32x4 *>(src + (size_t)idx[i] * 256)[threadIdx.x & 63];
}

// ------------------------------------------------ select: prune, rank, rescore
// Input: n_lists sorted lists (one per scan block) of kp keys each, ascending,
// padded with KEY_PAD; valid keys are distinct (distinct rows).  We need the kp
// smallest keys of the union WITHOUT sorting M = n_lists*kp keys.
//
// Pruning bound.  For a column j (1-based) let c_j = ceil(kp / j) and let
// tau_j be the c_j-th smallest of the lists' j-th entries.  At least c_j lists
// hold >= j keys <= tau_j, i.e. >= kp keys of the union are <= tau_j, so the
// union's kp-th smallest key is <= tau_j.  tau = min over a dyadic set of
// columns {1,2,4,..,kp}.  Keys > tau can be dropped.  Survivors are few: if
// m_b = #keys of list b that are <= tau then #{b : m_b >= j} <= c_j' for the
// largest used column j' <= j, hence S = sum_b m_b <= sum_j' (gap_j' * c_j')
// which is <= kp * (log2(kp) + 2) in the WORST case (<= 512 for kp <= 72), and
// about kp + 2 on uncorrelated data (column 1 alone is then nearly tight).
// Survivors are ranked by counting (S^2 / threads compares), no sort.
constexpr int SEL_THREADS = 1024;
constexpr int SEL_MAX_COLS = 8;
constexpr int SEL_SURV_CAP = 1024;
constexpr int SEL_FEW_KEYS = 512;    // up to this many keys over all lists the select ranks them all (no column bounds)
constexpr int ROW_STRIDE_F4 = 65;  // LDS row stride in float4 (1040 B): conflict-free b128 reads
constexpr int PROD_STRIDE = 258;   // LDS row stride of the f64 product tables (2064 B)
constexpr int SEL_FAST_KP = 34;    // product tables fit the 160 KiB LDS up to this k' (k <= 26)

// c-th smallest key of `col[0..L)` (PAD = missing), published with atomicMin into *tau.
// Executed by ONE wave; slots beyond L hold PAD which never satisfies the predicates below.
template <int NS>
__device__ __forceinline__ void column_tau(const key_t64 *col, int L, int c, key_t64 *tau)
{
    const int lane = threadIdx.x & 63;
    uint32_t vh[NS], vl[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u) {
        const int b = lane + u * 64;
        const key_t64 x = b < L ? col[b] : KEY_PAD;
        vh[u] = (uint32_t)(x >> 32);
        vl[u] = (uint32_t)x;
    }
    uint32_t lo = 0, hi = 0xFFFFFFFFu;
    while (lo < hi) {  // smallest distance t with #{vh <= t} >= c   (mid <= 0xFFFFFFFE: PAD never counts)
        const uint32_t mid = lo + ((hi - lo) >> 1);
        int cnt = 0;
#pragma unroll
        for (int u = 0; u < NS; ++u) cnt += __popcll(__ballot(vh[u] <= mid));
        if (cnt >= c) hi = mid; else lo = mid + 1;
    }
    if (lo == 0xFFFFFFFFu) return;  // fewer than c entries: no bound from this column
    const uint32_t dstar = lo;
    int below = 0, ties = 0;
#pragma unroll
    for (int u = 0; u < NS; ++u) {
        below += __popcll(__ballot(vh[u] < dstar));
        ties += __popcll(__ballot(vh[u] == dstar));
    }
    const int need = c - below;  // need-th smallest row among the entries at distance dstar (>= 1)
    uint32_t rlo = 0xFFFFFFFFu;  // every tie needed: tau = (dstar, max row)
    if (ties != need) {
        rlo = 0;
        uint32_t rhi = 0xFFFFFFFFu;
        while (rlo < rhi) {
            const uint32_t mid = rlo + ((rhi - rlo) >> 1);
            int cnt = 0;
#pragma unroll
            for (int u = 0; u < NS; ++u) cnt += __popcll(__ballot(vh[u] == dstar && vl[u] <= mid));
            if (cnt >= need) rhi = mid; else rlo = mid + 1;
        }
    }
    if (lane == 0) atomicMin(tau, ((key_t64)dstar << 32) | (key_t64)rlo);
}

struct FinalParams {
    const float *corpus;
    const float *queries;
    const key_t64 *lists;  // query qi's lists start at lists + qi*list_stride: [n_lists][kp]
    uint64_t list_stride;  // in keys
    uint32_t n_lists;      // <= SEL_MAX_LISTS
    uint32_t kp;
    uint32_t k_out;
    int ws_threshold;
    float ws_thr_score;
    uint64_t row_base;
    uint64_t *out_rows;   // [nq][k_out]
    double *out_dist;     // [nq][k_out]
    uint64_t *out_counts; // [nq] or nullptr
    uint64_t out_stride;  // words between consecutive queries' output lists (>= k_out)
    double f32_err;       // > 0: exactness certificate (SelectArgs::f32_err)
    uint64_t *out_uncertain;       // [nq] or nullptr
    unsigned int *out_status;      // [nq] or nullptr (SelectArgs::out_status)
    unsigned long long *status;    // the context's sticky "uncertain selects" counter
    unsigned long long *dbg;  // optional: s_memtime stamps of query 0's phases (tuning key select_debug_ptr)
    unsigned long long *flags;  // async select (or nullptr), see ScanParams
    unsigned long long step;
    const unsigned int *overflow;  // SelectArgs::overflow
    // delivery by the last block to finish (common.h Delivery; host_flag == nullptr: none)
    const unsigned long long *dev_out;
    unsigned long long *host_out;
    unsigned long long *host_flag;
    unsigned long long *done;
    unsigned long long seq;
    uint32_t out_words;
};

#define SEL_STAMP(i) do { if (p.dbg && blockIdx.x == 0 && threadIdx.x == 0) p.dbg[i] = __builtin_readcyclecounter(); } while (0)

// One block per query.
// KREG = keys a thread holds in registers: 8 covers n_lists * k' <= 8192 (every k <= 24 at 256 lists) in 70
// VGPRs, so that the 16-wave block fits on a CU NEXT TO a scan block (async select); 36 covers the maximum
// (512 lists x 72) and takes the whole register file.
// OVF: the batched path's instantiation, which also reads the candidate-buffer overflow flag (SelectArgs::overflow).  A template
// parameter and not a null test: with the flag code in it final_select_kernel<8> allocated 106 VGPRs instead of 90 and no longer
// fitted on a CU NEXT TO a scan block (4 waves/SIMD x 96 + the scan's 2 x 56 <= 512) -- the async select of the one-query pipeline
// then waited for scan blocks to leave and a 1 M-row step went from 153 to 204 us (found by the round-5 closing bench run).
template <int KREG, bool OVF>
__device__ __forceinline__ void final_select_body(const FinalParams &p, const uint32_t qi, unsigned char *smem_raw)
{
    const int kp = (int)p.kp;
    const int L = (int)p.n_lists;
    // LDS carve (all offsets multiples of 16; no static LDS in this kernel): small arrays first, then one big
    // region used twice -- [candidate-row tiles | survivors | column entries] until the best k' are known,
    // then (fast path) the exact-product tables of the rescoring stage.
    unsigned int *s_srank = reinterpret_cast<unsigned int *>(smem_raw);        // [96]
    unsigned int *s_rank = s_srank + 96;                                        // [kp+pad] final ranks
    double *s_qd = reinterpret_cast<double *>(s_rank + 80);                     // [256] query as f64 (slow path)
    key_t64 *s_best = reinterpret_cast<key_t64 *>(s_qd + 256);                  // [kp] (+pad to even)
    double *s_d = reinterpret_cast<double *>(s_best + ((kp + 1) & ~1));        // [kp]
    double *s_b2 = s_d + ((kp + 1) & ~1);                                       // [kp] row norms^2 (fast path)
    uint32_t *s_r = reinterpret_cast<uint32_t *>(s_b2 + ((kp + 1) & ~1));      // [kp]
    key_t64 *s_tau = reinterpret_cast<key_t64 *>(s_r + ((kp + 3) & ~3));       // [1]
    double *s_a2 = reinterpret_cast<double *>(s_tau + 1);                       // [1] query norm^2
    unsigned int *s_cnt = reinterpret_cast<unsigned int *>(s_a2 + 1);          // [0]=survivors [1]=valid [2]=max |q_i| bits [3]=this block delivers
    unsigned char *s_big = reinterpret_cast<unsigned char *>(s_cnt + 4);
    f32x4 *s_rows = reinterpret_cast<f32x4 *>(s_big);                           // [kp+1][65] float4
    key_t64 *s_surv = reinterpret_cast<key_t64 *>(s_rows + (size_t)(kp + 1) * ROW_STRIDE_F4);  // [SEL_SURV_CAP]
    key_t64 *s_col = s_surv + SEL_SURV_CAP;                                      // [ncols][L] column entries
    double *s_P = reinterpret_cast<double *>(s_big);                            // [kp][PROD_STRIDE] q_i * c_i (exact in f64)
    double *s_B = s_P + (size_t)kp * PROD_STRIDE;                               // [kp][PROD_STRIDE] c_i * c_i
    double *s_Q = s_B + (size_t)kp * PROD_STRIDE;                               // [256]            q_i * q_i
    const bool fast_rescore = kp <= SEL_FAST_KP;

    const key_t64 *lists = p.lists + (size_t)qi * p.list_stride;
    if (p.flags) {
        // launched on the aux stream while the scan of this step may still be running on the main stream
        if (threadIdx.x == 0) {
            flag_wait(p.flags, 0, p.step);
            // acquire at agent scope by ONE thread (invalidates this CU's vector L1 and the XCD's non-coherent
            // L2 lines: the lists were written through other XCDs' L2s); the barrier hands it to the block
            (void)__hip_atomic_load(p.flags + 0, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
    }
    SEL_STAMP(0);

    static_assert(KREG == 8 || KREG == (SEL_MAX_LISTS * 72 + SEL_THREADS - 1) / SEL_THREADS, "8 or 36");
    if (L == 1) {
        // ONE list per query (the batched kernel's level select left the k' best of every query sorted at the head of its buffer;
        // an index search with one probed segment): it IS the answer's candidate set -- no column bounds, no compaction, no ranks.
        // (Round 5: those three phases were ~7 us of dependent latencies in front of every batched call's rescoring, 10 % of a
        // small batch over a small corpus.)
        if (threadIdx.x == 0) { *s_tau = KEY_PAD; s_cnt[0] = 0; s_cnt[1] = 0; s_cnt[2] = 0; }
        for (int t = threadIdx.x; t < kp; t += blockDim.x) { s_best[t] = lists[t]; s_rank[t] = 0; }
        __syncthreads();
    } else {
    // ---- ONE global-latency phase: every key of the L lists goes to registers (<= 36 per thread)
    const int M = L * kp;
    const int n_round = (M + SEL_THREADS - 1) / SEL_THREADS;  // block-uniform
    key_t64 kreg[KREG];
    if (KREG == 8 || n_round <= 8) {  // common case (k <= 24): 8 back-to-back loads, one wait
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int e = (int)threadIdx.x + i * SEL_THREADS;
            const key_t64 x = lists[e < M ? e : M - 1];  // clamped: no branch between the loads
            kreg[i] = e < M ? x : KEY_PAD;
        }
#pragma unroll
        for (int i = 8; i < KREG; ++i) kreg[i] = KEY_PAD;
    } else {
#pragma unroll
        for (int i = 0; i < KREG; ++i) {
            const int e = (int)threadIdx.x + i * SEL_THREADS;
            const key_t64 x = lists[e < M ? e : M - 1];
            kreg[i] = e < M ? x : KEY_PAD;
        }
    }

    // dyadic columns 1,2,4,.. < kp, plus kp: column jj holds entry (1 << jj) except the last = kp
    int ncols = 1;
    for (int j = 1; j < kp && ncols < SEL_MAX_COLS; j <<= 1) ++ncols;
    auto col_of = [&](int jj) { return jj < ncols - 1 ? (1 << jj) : kp; };
    // the column entries are fetched in the same latency window as the keys (<= 4 per thread)
    // FEW keys in all (a small corpus: 16 blocks x 11 keys for 1000 rows): no pruning bound -- every key is a survivor and the ranks
    // below order them directly.  (The column bounds are ~3 us of dependent bisection steps, a quarter of this stage, to prune a set
    // that is already small.)
    const bool few = M <= SEL_FEW_KEYS;   // block-uniform
    key_t64 cval[(SEL_MAX_COLS * SEL_MAX_LISTS) / SEL_THREADS];
    const int n_col_entries = few ? 0 : ncols * L;
    if (!few) {
#pragma unroll
        for (int u = 0; u < (SEL_MAX_COLS * SEL_MAX_LISTS) / SEL_THREADS; ++u) {
            int t = (int)threadIdx.x + u * SEL_THREADS;
            const bool ok = t < n_col_entries;
            t = ok ? t : 0;
            const int jj = t / L, bb = t - jj * L;
            const key_t64 x = lists[(size_t)bb * kp + (col_of(jj) - 1)];
            cval[u] = ok ? x : KEY_PAD;
        }
    }
    if (threadIdx.x == 0) { *s_tau = KEY_PAD; s_cnt[0] = 0; s_cnt[1] = 0; s_cnt[2] = 0; }
    for (int t = threadIdx.x; t < kp; t += blockDim.x) { s_best[t] = KEY_PAD; s_rank[t] = 0; }
    if (!few) {
#pragma unroll
        for (int u = 0; u < (SEL_MAX_COLS * SEL_MAX_LISTS) / SEL_THREADS; ++u) {
            const int t = (int)threadIdx.x + u * SEL_THREADS;
            if (t < n_col_entries) s_col[t] = cval[u];
        }
    }
    __syncthreads();
    SEL_STAMP(1);

    // tau_j = c_j-th smallest key of column j.  One wave per column: the column sits in registers
    // (4 or 8 keys per lane); bisection on the 32 distance bits with ballot counts, then -- only if
    // several entries share that distance -- on the row bits.  No sort, no O(L^2) ranks.
    if (!few) {
        const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        if (wave < ncols) {
            const int colv = col_of(wave);
            const int c = (kp + colv - 1) / colv;
            if (L <= 256) column_tau<4>(s_col + (size_t)wave * L, L, c, s_tau);
            else column_tau<8>(s_col + (size_t)wave * L, L, c, s_tau);
        }
        __syncthreads();
    }
    SEL_STAMP(2);
    const key_t64 tau = *s_tau;   // (few: still KEY_PAD -- every real key passes)

    // compact the survivors (keys <= tau) straight from the registers
#pragma unroll
    for (int i = 0; i < KREG; ++i) {
        if (i < n_round) {
            const key_t64 key = kreg[i];
            if (key != KEY_PAD && key <= tau) {
                const unsigned int slot = atomicAdd(&s_cnt[0], 1u);
                if (slot < (unsigned)SEL_SURV_CAP) s_surv[slot] = key;
            }
        }
    }
    __syncthreads();
    SEL_STAMP(3);
    const int S = min((int)s_cnt[0], SEL_SURV_CAP);  // bound above guarantees S <= cap for kp <= 72
    if (S <= 96) {
        // pair-parallel ranks: thread <-> (i, j), rank[i] += key[j] < key[i]
        for (int t = threadIdx.x; t < S; t += blockDim.x) s_srank[t] = 0;
        __syncthreads();
        for (int pr = threadIdx.x; pr < S * S; pr += blockDim.x) {
            const int i = pr / S, j = pr - i * S;
            if (s_surv[j] < s_surv[i]) atomicAdd(&s_srank[i], 1u);
        }
        __syncthreads();
        for (int t = threadIdx.x; t < S; t += blockDim.x)
            if ((int)s_srank[t] < kp) s_best[s_srank[t]] = s_surv[t];
    } else {
        // T = 1024 / S' threads share a survivor (S' = the power of two >= S): each ranks it against a T-th of the set and adds its
        // share to the survivor's counter.  (One thread per survivor walked all S keys alone while the other 1024 - S threads
        // idled: 176 survivors -- 16 lists x 11 keys, no column bounds -- took 2.9 us, 349 took 6.3.)  The counters reuse the column
        // entries' space, which nobody reads any more.
        unsigned int *s_rk = reinterpret_cast<unsigned int *>(s_col);
        for (int t = threadIdx.x; t < S; t += blockDim.x) s_rk[t] = 0;
        __syncthreads();
        int Sp = 128;
        while (Sp < S) Sp <<= 1;                      // <= SEL_SURV_CAP = SEL_THREADS
        // 8, 4, 2 or 1 threads per survivor.  (T = 1 needs S > 512: behind a pruning bound S <= 481 at k' = 72, the worst case, and
        // without one -- the few-keys shortcut -- S <= SEL_FEW_KEYS = 512, so no call reaches it today.  It stays for the day either
        // limit moves: tests/select_ref.py models S, tests/test_gpu_select.py reads it back.)
        const int T = SEL_THREADS / Sp;
        const int e = (int)threadIdx.x / T, part = (int)threadIdx.x - e * T;
        if (e < S) {
            const key_t64 key = s_surv[e];
            const int per = (S + T - 1) / T, lo = part * per, hi = min(S, lo + per);
            unsigned int rank = 0;
            int i = lo;
#pragma unroll 1
            for (; i + 4 <= hi; i += 4) {
                key_t64 x[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) x[u] = s_surv[i + u];
#pragma unroll
                for (int u = 0; u < 4; ++u) rank += (x[u] < key) ? 1u : 0u;
            }
            for (; i < hi; ++i) rank += (s_surv[i] < key) ? 1u : 0u;
            if (rank) atomicAdd(&s_rk[e], rank);
        }
        __syncthreads();
        for (int t = threadIdx.x; t < S; t += blockDim.x)
            if ((int)s_rk[t] < kp) s_best[s_rk[t]] = s_surv[t];
    }
    __syncthreads();
    if (p.dbg && blockIdx.x == 0 && threadIdx.x == 0) p.dbg[8] = (unsigned long long)S;
    }   // (L > 1)
    SEL_STAMP(4);

    // ---- exact rescoring (bit-identical to the oracle's index-order f64 sums, see exact_sums()).
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    double my_ab = 0.0, my_b2 = 0.0;
    const key_t64 my_key = (int)threadIdx.x < kp ? s_best[threadIdx.x] : KEY_PAD;
    if (fast_rescore) {
        // The product of two f32 values is EXACT in f64, so "acc = acc + (double)a * (double)b" only rounds in
        // the add.  All 1024 threads compute the products q_i*c_i, c_i*c_i, q_i*q_i into LDS in parallel (one
        // wave per candidate row, coalesced 16 B per lane); what stays sequential is one chain of 256 dependent
        // f64 ADDS per sum, run by 2*k'+1 threads in three different waves.  (Before: each of the k' threads
        // converted and multiplied inside its chain -- 9.2k cycles for this stage, now the adds alone.)
        const f32x4 qv = reinterpret_cast<const f32x4 *>(p.queries + (size_t)qi * 256)[lane];
        // a wave owns candidates wave, wave+16, (wave+32): request all its rows first (ONE global latency)
        constexpr int ROWS_PER_WAVE = (SEL_FAST_KP + SEL_THREADS / 64 - 1) / (SEL_THREADS / 64);  // 3
        f32x4 bv[ROWS_PER_WAVE];
        bool have[ROWS_PER_WAVE];
#pragma unroll
        for (int u = 0; u < ROWS_PER_WAVE; ++u) {
            const int c = wave + u * n_waves;
            have[u] = c < kp && s_best[c] != KEY_PAD;
            const uint32_t row = have[u] ? (uint32_t)(s_best[c] & 0xFFFFFFFFull) : 0u;
            bv[u] = reinterpret_cast<const f32x4 *>(p.corpus + (uint64_t)row * 256)[lane];
        }
        // (conversions only now: the query and all row loads above are in flight together)
        const double q0 = qv.x, q1 = qv.y, q2 = qv.z, q3 = qv.w;
        if (wave == n_waves - 1) {
            double *dst = s_Q + 4 * lane;
            dst[0] = q0 * q0; dst[1] = q1 * q1; dst[2] = q2 * q2; dst[3] = q3 * q3;
            // the query's largest magnitude, for the domain verdict below (domain.hip)
            atomicMax(&s_cnt[2], max(max(__float_as_uint(qv.x) & 0x7fffffffu, __float_as_uint(qv.y) & 0x7fffffffu),
                                     max(__float_as_uint(qv.z) & 0x7fffffffu, __float_as_uint(qv.w) & 0x7fffffffu)));
        }
#pragma unroll
        for (int u = 0; u < ROWS_PER_WAVE; ++u) {
            if (have[u]) {
                const int c = wave + u * n_waves;
                const double b0 = bv[u].x, b1 = bv[u].y, b2 = bv[u].z, b3 = bv[u].w;
                double *dp = s_P + (size_t)c * PROD_STRIDE + 4 * lane;
                double *db = s_B + (size_t)c * PROD_STRIDE + 4 * lane;
                dp[0] = q0 * b0; dp[1] = q1 * b1; dp[2] = q2 * b2; dp[3] = q3 * b3;
                db[0] = b0 * b0; db[1] = b1 * b1; db[2] = b2 * b2; db[3] = b3 * b3;
            }
        }
        __syncthreads();
        SEL_STAMP(5);
        // chains: threads [0,kp) sum P, threads [64,64+kp) sum B, thread 128 sums Q
        const int role = (int)threadIdx.x >> 6, idx = (int)threadIdx.x & 63;
        const double *src = nullptr;
        if (role == 0 && idx < kp && s_best[idx] != KEY_PAD) src = s_P + (size_t)idx * PROD_STRIDE;
        else if (role == 1 && idx < kp && s_best[idx] != KEY_PAD) src = s_B + (size_t)idx * PROD_STRIDE;
        else if (threadIdx.x == 128) src = s_Q;
        if (src) {
            double acc = 0.0;
#pragma unroll 16
            for (int i = 0; i < 256; ++i) acc = acc + src[i];
            if (role == 0) my_ab = acc;
            else if (role == 1) s_b2[idx] = acc;
            else *s_a2 = acc;
        }
        __syncthreads();
        if ((int)threadIdx.x < kp) my_b2 = s_b2[threadIdx.x];
    } else {
        // large k': stage the candidate rows (one wave per row, 16 B per lane) and the query converted to f64
        if (threadIdx.x < 256) {
            const float qf = p.queries[(size_t)qi * 256 + threadIdx.x];
            s_qd[threadIdx.x] = (double)qf;
            atomicMax(&s_cnt[2], __float_as_uint(qf) & 0x7fffffffu);
        }
        for (int c = wave; c < kp; c += n_waves) {
            if (s_best[c] != KEY_PAD) {
                const float *g = p.corpus + (uint64_t)(uint32_t)(s_best[c] & 0xFFFFFFFFull) * 256;
                s_rows[(size_t)c * ROW_STRIDE_F4 + lane] = reinterpret_cast<const f32x4 *>(g)[lane];
            }
        }
        __syncthreads();
        SEL_STAMP(5);
        // thread t < kp walks candidate t's row; thread 128 (another wave) walks the query
        if (my_key != KEY_PAD) {
            const f32x4 *r4 = s_rows + (size_t)threadIdx.x * ROW_STRIDE_F4;
#pragma unroll 8
            for (int i = 0; i < 64; ++i) {
                const f32x4 b = r4[i];
                const double a0 = s_qd[4 * i], a1 = s_qd[4 * i + 1], a2 = s_qd[4 * i + 2], a3 = s_qd[4 * i + 3];
                const double bx = b.x, by = b.y, bz = b.z, bw = b.w;
                my_ab = my_ab + a0 * bx; my_b2 = my_b2 + bx * bx;
                my_ab = my_ab + a1 * by; my_b2 = my_b2 + by * by;
                my_ab = my_ab + a2 * bz; my_b2 = my_b2 + bz * bz;
                my_ab = my_ab + a3 * bw; my_b2 = my_b2 + bw * bw;
            }
        }
        if (threadIdx.x == 128) {
            double a2 = 0.0;
#pragma unroll 8
            for (int i = 0; i < 256; ++i) a2 = a2 + s_qd[i] * s_qd[i];
            *s_a2 = a2;
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < kp) {
        double d = __builtin_inf();
        uint32_t r = 0xFFFFFFFFu;
        if (my_key != KEY_PAD) {
            r = (uint32_t)(my_key & 0xFFFFFFFFull);
            d = cos_finish_exact(my_ab, *s_a2, my_b2);
            if (p.ws_threshold) {
                // qdrant score_threshold keeps score > threshold (similarity metrics)
                if (!((1.0 - d) > (double)p.ws_thr_score)) { d = __builtin_inf(); r = 0xFFFFFFFFu; }
            }
        }
        s_d[threadIdx.x] = d;
        s_r[threadIdx.x] = r;
        if (r != 0xFFFFFFFFu) atomicAdd(&s_cnt[1], 1u);
    }
    uint64_t *orow = p.out_rows + (size_t)qi * p.out_stride;
    double *odist = p.out_dist + (size_t)qi * p.out_stride;
    if (threadIdx.x < p.k_out) { orow[threadIdx.x] = 0xFFFFFFFFFFFFFFFFull; odist[threadIdx.x] = __builtin_inf(); }
    if (threadIdx.x == 0 && p.out_uncertain) p.out_uncertain[qi] = 0;
    if (threadIdx.x == 0 && p.out_status) p.out_status[qi] = 0;
    __syncthreads();
    SEL_STAMP(6);
    for (int pr = threadIdx.x; pr < kp * kp; pr += blockDim.x) {
        const int i = pr / kp, j = pr - i * kp;
        const uint32_t ri = s_r[i], rj = s_r[j];
        if (ri != 0xFFFFFFFFu && rj != 0xFFFFFFFFu) {
            const double di = s_d[i], dj = s_d[j];
            if (dj < di || (dj == di && rj < ri)) atomicAdd(&s_rank[i], 1u);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < kp && s_r[threadIdx.x] != 0xFFFFFFFFu) {
        const unsigned rank = s_rank[threadIdx.x];
        if (rank < p.k_out) { orow[rank] = p.row_base + s_r[threadIdx.x]; odist[rank] = s_d[threadIdx.x]; }
    }
    if (!magnitude_in_domain(s_cnt[2])) {
        // The query is outside the library's domain (a non-finite component, or a magnitude the f32 nominating kernels do not answer
        // for: domain.hip).  The host entry points refuse such queries before anything is launched; a device entry point says so
        // here -- SMT_STATUS_INVALID_QUERY: the list means nothing.
        if (threadIdx.x == 0) {
            if (p.out_uncertain) p.out_uncertain[qi] = 3;
            if (p.out_status) p.out_status[qi] = 3u;
            if (p.status) atomicAdd(p.status, 1ull);
        }
    } else if (p.f32_err > 0.0 && s_best[kp - 1] != KEY_PAD) {
        // Exactness certificate (SelectArgs::f32_err).  kp rows were nominated, so rows outside the lists may
        // exist; each of them has f32 distance >= tau32, hence exact distance >= tau32 - f32_err.  Exactly one
        // thread decides: the owner of the k_out-th result, or thread 0 when fewer than k_out rows qualified
        // (only possible with the workspace score threshold, which then bounds what an outside row would need).
        const double floor_out = (double)__uint_as_float((unsigned)(s_best[kp - 1] >> 32)) - p.f32_err;
        bool decide = false, uncertain = false;
        if ((int)threadIdx.x < kp && s_r[threadIdx.x] != 0xFFFFFFFFu && s_rank[threadIdx.x] == p.k_out - 1) {
            decide = true;
            uncertain = !(floor_out > s_d[threadIdx.x]);
        } else if (threadIdx.x == 0 && s_cnt[1] < p.k_out) {
            decide = true;
            uncertain = p.ws_threshold ? ((1.0 - floor_out) > (double)p.ws_thr_score) : true;
        }
        unsigned int code = uncertain ? 1u : 0u;   // SMT_STATUS_UNCERTAIN
        if constexpr (OVF) {
            if (decide && p.overflow[qi]) { uncertain = true; code = 2u; }   // rows were dropped on the way (SelectArgs::overflow): SMT_STATUS_OVERFLOW
        }
        if (decide && uncertain) {
            if (p.out_uncertain) p.out_uncertain[qi] = code;
            if (p.out_status) p.out_status[qi] = code;
            if (p.status) atomicAdd(p.status, 1ull);
        }
    } else if constexpr (OVF) {
        if (threadIdx.x == 0 && p.overflow[qi]) {
            if (p.out_uncertain) p.out_uncertain[qi] = 2;
            if (p.out_status) p.out_status[qi] = 2u;
            if (p.status) atomicAdd(p.status, 1ull);
        }
    }
    if (threadIdx.x == 0 && p.out_counts)
        p.out_counts[qi] = s_cnt[1] < p.k_out ? s_cnt[1] : p.k_out;
    if (p.flags) {
        __syncthreads();
        if (threadIdx.x == 0 && blockIdx.x == 0)  // async mode: one query per launch
            __hip_atomic_store(p.flags + 1, p.step, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (p.host_flag) {
        // Delivery (common.h): count this block as finished -- thread 0's agent-scope release covers the block's output stores, ordered
        // before it by the barrier, the same hand-over the scan kernel uses for its lists -- and let the LAST block carry every query's
        // answer home: ONE wave copies the device block to pinned host memory and raises the completion word behind it (its own
        // stores, one system-scope release; a fence in each of the 16 waves would be 16 write-backs of the L2).
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned long long prev = __hip_atomic_fetch_add(p.done, 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            s_cnt[3] = prev == (unsigned long long)gridDim.x - 1ull ? 1u : 0u;
        }
        __syncthreads();
        if (s_cnt[3] && threadIdx.x < 64) {
            for (uint32_t i = threadIdx.x; i < p.out_words; i += 64)
                p.host_out[i] = __hip_atomic_load(p.dev_out + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(p.done, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // system scope: the copy is out before the flag
            if (threadIdx.x == 0) __hip_atomic_store(p.host_flag, p.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    SEL_STAMP(7);
}

template <int KREG, bool OVF = false>
__global__ void __launch_bounds__(SEL_THREADS) final_select_kernel(FinalParams p)
{
    extern __shared__ unsigned char smem_raw[];   // (no alignment attribute: see scan_topk_kernel, scan_topk.hip)
    final_select_body<KREG, OVF>(p, blockIdx.x, smem_raw);
}

// One select launch for a pass of scan_deep_kernel (tuning key select_group): DEEP_MAX blocks behind a group-capable scan of the
// same stream.  Block g reads the scan's record of this step.  Marked absorbed: the leader's launch of this kernel, earlier on this
// stream, has the call's answer, and every block returns.  Otherwise the pass served n = 1 + taken calls: block 0 runs the call's own
// select with the parameters it was launched with, block g in 1 .. n - 1 that of member g - 1 -- the shared fields (corpus, n_lists,
// k', k_out, f32_err, the sticky counter: a leader takes calls that agree with it in all of them) and the member's own queries, list
// set, output buffers, status word and row base, as the deciding wave copied them into the record (scan_deep.hip deep_decide).
// The body is final_select_body<KREG, false> with query index 0, unchanged: every answer, verdict and count is what the member's
// own launch of final_select_kernel produced.
// ORDER: a member's outputs are written at the leader's place in stream order, earlier than at its own.  That is safe for the reason
// its query may be READ that early: a call is published as absorbable only when the caller's stream was empty at the call, so no
// work of the caller's can still be reading or writing those buffers, and what the caller enqueues later is ordered behind the
// call's own (empty) launch of this kernel, as before.
template <int KREG>
__global__ void __launch_bounds__(SEL_THREADS) group_select_kernel(FinalParams p, GroupSelect gs)
{
    extern __shared__ unsigned char smem_raw[];
    const uint32_t g = blockIdx.x;
    const unsigned long long state = uniform_u64(flag_load(gs.rec + GROUP_REC_STATE));
    uint32_t n = 0;   // calls this launch serves
    if (state != gs.absorbed) {
        n = 1;
        if (state == gs.paired) {
            const uint32_t taken = (uint32_t)uniform_u64(flag_load(gs.rec + GROUP_REC_TAKEN));
            n += taken < (uint32_t)GROUP_SEL_MAX ? taken : (uint32_t)GROUP_SEL_MAX - 1u;
        }
    }
    if (g == 0 && threadIdx.x == 0) (void)__hip_atomic_fetch_add(gs.hist + n, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (g >= n) return;
    FinalParams m = p;
    if (g > 0) {
        const unsigned long long *sel = gs.sel + 4 * (g - 1);
        m.queries = reinterpret_cast<const float *>((uintptr_t)uniform_u64(flag_load(gs.rec + GROUP_REC_QUERY + (g - 1))));
        m.lists = reinterpret_cast<const key_t64 *>((uintptr_t)uniform_u64(flag_load(gs.rec + GROUP_REC_LISTS + (g - 1))));
        m.out_rows = reinterpret_cast<uint64_t *>((uintptr_t)uniform_u64(flag_load(sel + 0)));
        m.out_dist = reinterpret_cast<double *>((uintptr_t)uniform_u64(flag_load(sel + 1)));
        m.out_status = reinterpret_cast<unsigned int *>((uintptr_t)uniform_u64(flag_load(sel + 2)));
        m.row_base = uniform_u64(flag_load(sel + 3));
        m.dbg = nullptr;
    }
    final_select_body<KREG, false>(m, 0, smem_raw);
}

static size_t final_smem_bytes(uint32_t kp)
{
    const size_t kp2 = (kp + 1) & ~1u;
    const size_t small = (size_t)(96 + 80) * 4 + 256 * 8 + kp2 * 8 * 3 + (size_t)((kp + 3) & ~3u) * 4 + 8 + 8 + 16;
    const size_t big_select = (size_t)(kp + 1) * ROW_STRIDE_F4 * 16 + (size_t)SEL_SURV_CAP * 8 + (size_t)SEL_MAX_COLS * SEL_MAX_LISTS * 8;
    const size_t big_rescore = kp <= (uint32_t)SEL_FAST_KP ? ((size_t)2 * kp * PROD_STRIDE + 256) * 8 : 0;
    return small + std::max(big_select, big_rescore) + 64;
}

// The four instantiations: [reads the overflow flag (the batched path)][more than 8 keys per thread]
using select_kernel_t = void (*)(FinalParams);
static const select_kernel_t SELECT_KERNELS[2][2] = {{final_select_kernel<8>, final_select_kernel<36>},
                                                     {final_select_kernel<8, true>, final_select_kernel<36, true>}};

static int select_attrs(smt_ctx *ctx)
{
    if (ctx->attr_done & ATTR_SELECT) return SMT_OK;   // per context == per device (a group runs several GPUs in one process)
    for (const auto &row : SELECT_KERNELS)
        for (const select_kernel_t kernel : row)
            SMT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                              160 * 1024));
    SMT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(group_select_kernel<8>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      160 * 1024));
    ctx->attr_done |= ATTR_SELECT;
    return SMT_OK;
}

static FinalParams final_params(const smt_ctx *ctx, const SelectArgs &a)
{
    FinalParams f;
    f.corpus = a.corpus;
    f.queries = a.queries;
    f.lists = a.lists;
    f.list_stride = a.list_stride;
    f.n_lists = a.n_lists;
    f.kp = a.kp;
    f.k_out = a.k_out;
    f.ws_threshold = a.ws_threshold;
    f.ws_thr_score = a.ws_thr_score;
    f.row_base = a.row_base;
    f.out_rows = a.out_rows;
    f.out_dist = a.out_dist;
    f.out_counts = a.out_counts;
    f.out_stride = a.out_stride ? a.out_stride : a.k_out;
    f.f32_err = a.f32_err;
    f.out_uncertain = a.out_uncertain;
    f.out_status = a.out_status;
    f.status = ctx->d_status;
    f.dbg = reinterpret_cast<unsigned long long *>(ctx->tune.select_debug_ptr);
    f.flags = a.async_step ? ctx->d_flags : nullptr;
    f.step = a.async_step;
    f.overflow = a.overflow;
    const Delivery *dl = a.async_step ? nullptr : a.deliver;
    f.dev_out = dl ? dl->dev_out : nullptr;
    f.host_out = dl ? dl->host_out : nullptr;
    f.host_flag = dl ? dl->host_flag : nullptr;
    f.done = dl ? dl->done : nullptr;
    f.seq = dl ? dl->seq : 0;
    f.out_words = dl ? dl->n_words : 0;
    return f;
}

// Block lists -> final answer in ONE launch (per query: prune + rank + rescore).
int launch_select(smt_ctx *ctx, const SelectArgs &a)
{
    SMT_REQUIRE(a.n_lists >= 1 && a.n_lists <= (uint32_t)SEL_MAX_LISTS, "select stage accepts 1..512 block lists");
    // the kernel's LDS carve (s_rank has 80 slots, the staged rows (kp + 1) x 1040 B) and its rank loops assume this
    SMT_REQUIRE(a.k_out >= 1 && a.k_out <= a.kp && a.kp <= 72, "select stage accepts 1 <= k_out <= k' <= 72");
    SMT_REQUIRE(a.async_step == 0 || (a.nq == 1 && ctx->aux_stream && ctx->d_flags), "async select handles one query per launch");
    int rc = select_attrs(ctx);
    if (rc) return rc;
    const FinalParams f = final_params(ctx, a);
    const bool small = (uint64_t)a.n_lists * a.kp <= (uint64_t)8 * SEL_THREADS;
    // async select: on the aux stream, outside the "select" profiling label, and never the batched path's instantiation
    const bool on_aux = a.async_step != 0;
    hipStream_t st = on_aux ? ctx->aux_stream : a.stream ? a.stream : ctx->stream;
    const bool timed = !on_aux && ctx->tune.prof_select;
    if (timed) prof_begin_on(ctx, "select", st);
    hipLaunchKernelGGL(SELECT_KERNELS[!on_aux && a.overflow ? 1 : 0][small ? 0 : 1], dim3(a.nq), dim3(SEL_THREADS),
                       final_smem_bytes(a.kp), st, f);
    if (timed) prof_end_on(ctx, "select", st);
    if (on_aux) ctx->async_pending = true;
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

// The select of a scan_deep_kernel pass (group_select_kernel, above): one query, a list set of at most 8 keys per thread, no
// overflow flag, no delivery and nothing on the aux stream -- launch_scan_topk asks for it only then.
bool group_select_serves(const SelectArgs &a)
{
    return a.nq == 1 && (uint64_t)a.n_lists * a.kp <= (uint64_t)8 * SEL_THREADS && a.async_step == 0 && !a.overflow && !a.deliver &&
           !a.out_counts && !a.out_uncertain && !a.ws_threshold && (a.out_stride == 0 || a.out_stride == a.k_out);
}
int launch_group_select(smt_ctx *ctx, const SelectArgs &a, const GroupSelect &gs)
{
    SMT_REQUIRE(a.n_lists >= 1 && a.n_lists <= (uint32_t)SEL_MAX_LISTS, "select stage accepts 1..512 block lists");
    SMT_REQUIRE(group_select_serves(a) && gs.rec && gs.sel && gs.hist, "group select: a plain one-query select of a grouped scan");
    int rc = select_attrs(ctx);
    if (rc) return rc;
    const FinalParams f = final_params(ctx, a);
    hipStream_t st = a.stream ? a.stream : ctx->stream;
    const bool timed = ctx->tune.prof_select;
    if (timed) prof_begin_on(ctx, "select", st);
    hipLaunchKernelGGL(group_select_kernel<8>, dim3(GROUP_SEL_MAX), dim3(SEL_THREADS), final_smem_bytes(a.kp), st, f, gs);
    if (timed) prof_end_on(ctx, "select", st);
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

int launch_rescore_rows(smt_ctx *ctx, const float *corpus, const float *query, const uint32_t *rows,
                        uint64_t n, double *out_dist)
{
    if (n == 0) return SMT_OK;
    const int threads = 64;
    const uint64_t blocks = (n + threads - 1) / threads;
    prof_begin(ctx, "select");
    hipLaunchKernelGGL(rescore_rows_kernel, dim3((unsigned)blocks), dim3(threads), 0, ctx->stream, corpus,
                       query, rows, n, out_dist);
    prof_end(ctx, "select");
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

int launch_gather_rows256(smt_ctx *ctx, const float *src, const uint32_t *idx_dev, uint32_t n, float *dst)
{
    if (n == 0) return SMT_OK;
    hipLaunchKernelGGL(gather_rows256_kernel, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, src, idx_dev, n, dst);
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

int launch_rescore_rows_multi(smt_ctx *ctx, const float *corpus, const float *queries, const uint32_t *rows, const uint32_t *qidx,
                              uint64_t n, double *out_dist)
{
    if (n == 0) return SMT_OK;
    const int threads = 64;
    prof_begin(ctx, "select");
    hipLaunchKernelGGL(rescore_rows_multi_kernel, dim3((unsigned)((n + threads - 1) / threads)), dim3(threads), 0, ctx->stream, corpus,
                       queries, rows, qidx, n, out_dist);
    prof_end(ctx, "select");
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

}  // namespace smt
