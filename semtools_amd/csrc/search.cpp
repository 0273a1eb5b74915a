// search.cpp -- the search entry points of libsemtools_hip.so (include/semtools_hip.h: smt_search, smt_search_topk_device, the merge
// calls) and the host logic behind them: which kernel answers a call (topk_dispatch), the exactness fall-backs, threshold mode,
// delivery.  No CPU fallback: every path ends in a HIP kernel.
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "common.h"

using namespace smt;

namespace smt {

// The three exclusive prefixes a range-filtered search stages beside its ranges: rows before range i (large-k path), FILTER_CHUNK-row
// chunks before it (K2 / K4 / the LDS-row kernel) and aligned 32-row tiles before it (gemm_rowreg_kernel: a tile counts for the
// FIRST range that touches it).  host = [prefix | chunk_prefix | tile_prefix], each nr + 1 words.
static void range_prefixes(const std::vector<smt_range> &rr, std::vector<uint64_t> &host)
{
    const size_t nr = rr.size();
    host.assign(3 * (nr + 1), 0);
    uint64_t *prefix = host.data(), *chunk_prefix = prefix + nr + 1, *tile_prefix = chunk_prefix + nr + 1;
    uint64_t last_tile = UINT64_MAX;
    for (size_t i = 0; i < nr; ++i) {
        const uint64_t len = rr[i].end - rr[i].begin;
        prefix[i + 1] = prefix[i] + len;
        chunk_prefix[i + 1] = chunk_prefix[i] + (len + FILTER_CHUNK - 1) / FILTER_CHUNK;
        const uint64_t ft = rr[i].begin >> 5, lt = (rr[i].end - 1) >> 5;
        tile_prefix[i + 1] = tile_prefix[i] + (lt - ft + 1) - (ft == last_tile ? 1 : 0);
        last_tile = lt;
    }
}

// ---------------------------------------------------------------- kept range sets (common.h RangeSet)
static inline uint64_t mix64(uint64_t x)
{
    x ^= x >> 32; x *= 0xD6E8FEB86659FD93ull; x ^= x >> 32; x *= 0xD6E8FEB86659FD93ull; x ^= x >> 32;
    return x;
}

static void range_set_free(RangeSet *rs)
{
    if (!rs) return;
    if (rs->dev) (void)hipFree(rs->dev);
    delete rs;
}

void corpus_range_sets_drop(smt_corpus *c)
{
    for (RangeSet *rs : c->range_sets) range_set_free(rs);
    c->range_sets.clear();
}

// The range filter of ONE search call, resolved in one place for the host form and the device exchange form alike: the set kept for
// the list if the corpus has one (only the queries go up), else the non-empty ranges and their three prefixes, which the caller
// stages with its own upload.  Two steps, because a call may end between them (nothing to scan, top_k = 0) and a list that ends a
// call early is never built: range_plan_find validates and identifies the list, range_plan_finish prefixes it (and builds the kept
// set on second sight).  Then bind() fixes the device pointers -- null without ranges -- and apply() hands them to a launch.
struct RangePlan {
    const smt_range *ranges_in = nullptr;   // the list as passed (empty ranges included: part of the identity)
    uint32_t n_in = 0;
    RangeSet *rset = nullptr;               // the kept set that answers for the list, or nullptr
    bool build = false;                     // seen before and not kept: range_plan_finish builds the set
    uint64_t h1 = 0, h2 = 0;
    std::vector<smt_range> rr;              // without a kept set: the non-empty ranges ...
    std::vector<uint64_t> prefixes;         // ... and [prefix | chunk_prefix | tile_prefix] (range_prefixes)
    uint32_t nr = 0;                        // ranges on the device
    uint64_t n_virtual = 0, n_chunks = 0, n_vtiles = 0;   // rows to scan (the caller starts it at the corpus' rows); chunks; tiles
    const smt_range *d_r = nullptr;
    const uint64_t *d_p = nullptr, *d_cp = nullptr, *d_tp = nullptr;

    size_t r_bytes() const { return (size_t)nr * sizeof(smt_range); }
    // bytes of [ranges | prefix | chunk_prefix | tile_prefix], and what of them the caller uploads (0: no ranges, or a kept set has them)
    size_t table_bytes() const { return r_bytes() + 3 * (size_t)(nr + 1) * sizeof(uint64_t); }
    size_t upload_bytes() const { return nr && !rset ? table_bytes() : 0; }
    void write(char *host) const
    {
        if (!upload_bytes()) return;
        memcpy(host, rr.data(), r_bytes());
        memcpy(host + r_bytes(), prefixes.data(), prefixes.size() * sizeof(uint64_t));
    }
    // dev: where the caller's upload of upload_bytes() lies (not read when there is none)
    void bind(char *dev)
    {
        if (rset) { d_r = rset->d_r; d_p = rset->d_p; d_cp = rset->d_cp; d_tp = rset->d_tp; }
        else if (nr) {
            d_r = reinterpret_cast<const smt_range *>(dev);
            d_p = reinterpret_cast<const uint64_t *>(dev + r_bytes());
            d_cp = d_p + (nr + 1);
            d_tp = d_cp + (nr + 1);
        }
    }
    void apply(ScanArgs &a) const
    {
        a.ranges = d_r; a.range_prefix = d_p; a.range_chunk_prefix = d_cp; a.range_tile_prefix = d_tp;
        a.n_ranges = nr; a.n_virtual = n_virtual; a.n_chunks = n_chunks; a.n_vtiles = n_vtiles;
        a.range_set = rset;
    }
};

// Ranges validated (as validate_ranges) and identified in one pass: p.n_virtual, and the set kept for this list if there is one --
// else its non-empty ranges (with p.build = true when the list has been seen before and deserves a set now).
static int range_plan_find(smt_corpus *corpus, const smt_range *ranges, uint32_t n, RangePlan &p)
{
    uint64_t prev_end = 0, t = 0, h1 = 0x9E3779B97F4A7C15ull ^ n, h2 = 0xC2B2AE3D27D4EB4Full + n;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t b = ranges[i].begin, e = ranges[i].end;
        SMT_REQUIRE(b <= e, "range begin > end");
        SMT_REQUIRE(e <= corpus->rows, "range extends past the corpus");
        SMT_REQUIRE(i == 0 || b >= prev_end, "ranges must be sorted and disjoint");
        prev_end = e;
        t += e - b;
        h1 = (h1 ^ b) * 0x100000001B3ull; h1 = (h1 ^ e) * 0x100000001B3ull; h1 ^= h1 >> 29;
        h2 = (h2 + b) * 0x9FB21C651E98DF25ull; h2 = ((h2 << 31) | (h2 >> 33)) + e;
    }
    h1 = mix64(h1); h2 = mix64(h2 ^ t);
    p.ranges_in = ranges; p.n_in = n;
    p.n_virtual = t;
    p.h1 = h1; p.h2 = h2;
    for (RangeSet *rs : corpus->range_sets)
        if (rs->h1 == h1 && rs->h2 == h2 && rs->n_in == n && rs->n_virtual == t && rs->host_ranges.size() == n &&
            (n == 0 || memcmp(rs->host_ranges.data(), ranges, (size_t)n * sizeof(smt_range)) == 0)) {   // (a collision must not answer for another subset)
            rs->last_use = ++corpus->range_clock;
            ++corpus->range_set_hits;
            p.rset = rs;
            return SMT_OK;
        }
    for (uint32_t i = 0; i < n; ++i) if (ranges[i].end > ranges[i].begin) p.rr.push_back(ranges[i]);
    for (auto &seen : corpus->range_seen)
        if (seen[0] == h1 && seen[1] == h2) { p.build = true; return SMT_OK; }
    corpus->range_seen[corpus->range_seen_next % 16][0] = h1;
    corpus->range_seen[corpus->range_seen_next % 16][1] = h2;
    ++corpus->range_seen_next;
    return SMT_OK;
}

// A new kept set for the plan's list (p.rr, p.prefixes): one device block, uploaded on the context's stream from pinned memory.
static int range_set_build(smt_corpus *corpus, RangePlan &p)
{
    smt_ctx *ctx = corpus->ctx;
    const uint32_t nr = p.nr;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t r_bytes = al((size_t)nr * sizeof(smt_range)), p_bytes = (size_t)(nr + 1) * sizeof(uint64_t);
    const size_t head = r_bytes + al(3 * p_bytes);
    const bool keep_tables = (p.n_vtiles + p.n_chunks) * 8 <= RANGE_SET_TABLE_BYTES_MAX;
    const size_t b_tile = keep_tables ? al((size_t)p.n_vtiles * 8) : 0, b_chunk = keep_tables ? al((size_t)p.n_chunks * 8) : 0;
    if (corpus->range_sets.size() >= (size_t)RANGE_SETS_MAX) {
        // the least recently used set goes; kernels of earlier calls may still read it
        size_t lru = 0;
        for (size_t i = 1; i < corpus->range_sets.size(); ++i)
            if (corpus->range_sets[i]->last_use < corpus->range_sets[lru]->last_use) lru = i;
        SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (int rc = sync_side_streams(ctx)) return rc;
        range_set_free(corpus->range_sets[lru]);
        corpus->range_sets.erase(corpus->range_sets.begin() + (long)lru);
    }
    RangeSet *rs = new RangeSet();
    if (hipMalloc(reinterpret_cast<void **>(&rs->dev), head + b_tile + b_chunk + 64) != hipSuccess) {
        (void)hipGetLastError();   // no room for a kept set: the call goes on without one
        delete rs;
        return SMT_OK;
    }
    rs->h1 = p.h1; rs->h2 = p.h2; rs->n_in = p.n_in; rs->nr = nr;
    rs->host_ranges.assign(p.ranges_in, p.ranges_in + p.n_in);
    rs->n_virtual = p.n_virtual; rs->n_chunks = p.n_chunks; rs->n_vtiles = p.n_vtiles;
    rs->d_r = reinterpret_cast<smt_range *>(rs->dev);
    rs->d_p = reinterpret_cast<uint64_t *>(rs->dev + r_bytes);
    rs->d_cp = rs->d_p + (nr + 1);
    rs->d_tp = rs->d_cp + (nr + 1);
    rs->d_tile_table = keep_tables ? reinterpret_cast<uint64_t *>(rs->dev + head) : nullptr;
    rs->d_chunk_table = keep_tables ? reinterpret_cast<uint64_t *>(rs->dev + head + b_tile) : nullptr;
    int rc = ensure_pinned_in(ctx, head);
    if (!rc) {
        // (h_pinned_in is reused by the caller for the queries: the upload must have left it before this returns -- once per set)
        char *pin = reinterpret_cast<char *>(ctx->h_pinned_in);
        memcpy(pin, p.rr.data(), (size_t)nr * sizeof(smt_range));
        memcpy(pin + r_bytes, p.prefixes.data(), 3 * p_bytes);
        hipError_t e = hipMemcpyAsync(rs->dev, pin, head, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { set_error("range set upload: %s", hipGetErrorString(e)); rc = SMT_E_HIP; }
    }
    if (rc) { range_set_free(rs); return rc; }
    rs->last_use = ++corpus->range_clock;
    ++corpus->range_set_builds;
    corpus->range_sets.push_back(rs);
    p.rset = rs;
    return SMT_OK;
}

// The second step: nr / n_chunks / n_vtiles from the kept set, or from the prefixes made here -- and the set itself when p.build.
static int range_plan_finish(smt_corpus *corpus, RangePlan &p)
{
    if (p.rset) { p.nr = p.rset->nr; p.n_chunks = p.rset->n_chunks; p.n_vtiles = p.rset->n_vtiles; return SMT_OK; }
    p.nr = (uint32_t)p.rr.size();
    if (!p.nr) return SMT_OK;
    range_prefixes(p.rr, p.prefixes);
    p.n_chunks = p.prefixes[2 * (p.nr + 1) - 1];
    p.n_vtiles = p.prefixes[3 * (p.nr + 1) - 1];
    return p.build ? range_set_build(corpus, p) : SMT_OK;
}

int range_tile_table(smt_ctx *ctx, const ScanArgs &a, uint64_t *scratch_table, const uint64_t **table)
{
    RangeSet *rs = a.range_set;
    if (rs && rs->d_tile_table) {
        if (!rs->have_tile_table) {
            int rc = launch_build_tile_table(ctx, a.ranges, a.range_tile_prefix, a.n_ranges, a.n_vtiles, rs->d_tile_table);
            if (rc) return rc;
            rs->have_tile_table = true;
        }
        *table = rs->d_tile_table;
        return SMT_OK;
    }
    *table = scratch_table;
    return launch_build_tile_table(ctx, a.ranges, a.range_tile_prefix, a.n_ranges, a.n_vtiles, scratch_table);
}

int range_chunk_table(smt_ctx *ctx, const ScanArgs &a, uint64_t *scratch_table, const uint64_t **table)
{
    RangeSet *rs = a.range_set;
    if (rs && rs->d_chunk_table) {
        if (!rs->have_chunk_table) {
            int rc = launch_build_chunk_table(ctx, a.ranges, a.range_chunk_prefix, a.n_ranges, a.n_chunks, rs->d_chunk_table);
            if (rc) return rc;
            rs->have_chunk_table = true;
        }
        *table = rs->d_chunk_table;
        return SMT_OK;
    }
    *table = scratch_table;
    return launch_build_chunk_table(ctx, a.ranges, a.range_chunk_prefix, a.n_ranges, a.n_chunks, scratch_table);
}

// ---------------------------------------------------------------- launch arguments, the order of an answer
// What every search call fills the same way; the caller adds what is its own (ranges: RangePlan::apply; outputs, stride, the
// workspace threshold, async flags, delivery).
static ScanArgs scan_args(const smt_corpus *corpus, const float *queries_dev, uint32_t nq, uint32_t k_out, uint64_t row_base)
{
    ScanArgs a;
    a.corpus = corpus->d_rows;
    a.rows = corpus->rows;
    a.queries = queries_dev;
    a.nq = nq;
    a.k_out = k_out;
    a.n_virtual = corpus->rows;
    a.row_base = row_base;
    return a;
}

// K4's arguments for ONE query of a call: every row of the plan with distance < max_distance
static ThresholdQuery threshold_query(const smt_corpus *corpus, const float *query_dev, const RangePlan &plan, double max_distance)
{
    ThresholdQuery t;
    t.corpus = corpus->d_rows;
    t.rows = corpus->rows;
    t.query = query_dev;
    t.ranges = plan.d_r; t.range_chunk_prefix = plan.d_cp;
    t.n_ranges = plan.nr; t.n_virtual = plan.n_virtual; t.n_chunks = plan.n_chunks;
    t.max_distance = max_distance;
    return t;
}

// The workspace score rule (store.rs:502-503): a hit needs score > threshold, the score in f64, the threshold an f32.
static inline bool ws_score_passes(double dist, float thr_score) { return (1.0 - dist) > (double)thr_score; }

// Which of a query's candidates make its answer, besides the caller's distance bound: at most k, past the workspace threshold.
struct HitRule {
    uint64_t k = 0;
    bool ws_thr = false;
    float thr_score = 0.f;
    uint64_t row_base = 0;
};

// The answer from n candidates with EXACT distances: those with distance <= bound (`strict`: < bound; either way NaN never passes;
// +inf = no bound) that pass the rule's threshold, in (distance asc, row asc) order, the first k of them, as global rows.
// `sorted`: the candidates come in that order already (K4).
static void order_hits(const uint32_t *rows, const double *dist, uint64_t n, double bound, bool strict, bool sorted, const HitRule &rule,
                       LocalHits &out)
{
    std::vector<uint64_t> order;
    for (uint64_t i = 0; i < n && !(sorted && order.size() >= rule.k); ++i) {
        if (strict ? !(dist[i] < bound) : !(dist[i] <= bound)) continue;
        if (rule.ws_thr && !ws_score_passes(dist[i], rule.thr_score)) continue;
        order.push_back(i);
    }
    if (!sorted)
        std::sort(order.begin(), order.end(), [&](uint64_t x, uint64_t y) {
            if (dist[x] != dist[y]) return dist[x] < dist[y];
            return rows[x] < rows[y];
        });
    const uint64_t m = std::min<uint64_t>(order.size(), rule.k);
    out.rows.resize(m);
    out.dist.resize(m);
    for (uint64_t i = 0; i < m; ++i) {
        out.rows[i] = rule.row_base + rows[order[i]];
        out.dist[i] = dist[order[i]];
    }
}

// Sweeps that may read the corpus' fp16 operand image instead of its f32 rows (the batched re-answer, the large-k route)
static inline bool image_sweep_allowed(const smt_ctx *ctx, const smt_corpus *corpus)
{
    return ctx->tune.gemm_image != 0 && corpus->rows <= (1ull << 28);
}

// Exhaustive answer for ONE query whose f32 nomination failed its exactness certificate: K4 collects every row
// whose exact distance is <= bound (its own f32 prefilter carries an 8e-6 guard band; rescoring is exact f64), in
// (distance asc, row asc) order; the answer is the first k of them (after the workspace score filter).
// `bound` is the k-th exact distance found so far -- an upper bound of the true k-th -- or, when fewer than k rows
// passed the workspace threshold, the largest distance that threshold admits.  O(rows <= bound): a cluster of
// near-duplicates costs its own size, exactly what the reference pays for every query (it sorts all N).
static int exact_fallback(smt_ctx *ctx, smt_corpus *corpus, const float *query_dev, const RangePlan &plan, double bound, const HitRule &rule,
                          LocalHits &out)
{
    const double inf = std::numeric_limits<double>::infinity();
    const ThresholdQuery t = threshold_query(corpus, query_dev, plan, std::nextafter(bound, inf));  // K4 keeps d < max_distance: include == bound
    const uint32_t *h_rows = nullptr;
    const double *h_dist = nullptr;
    uint64_t n_ok = 0;
    int rc = run_threshold_query(ctx, t, &h_rows, &h_dist, &n_ok);
    if (rc) return rc;
    order_hits(h_rows, h_dist, n_ok, inf, false, /*sorted=*/true, rule, out);
    return SMT_OK;
}

// The same re-answer for MANY queries of one call at once.  One sweep of the batched kernel collects, per query, every
// row whose nominating distance is <= bound + F32_ERR_BF16X3 (a superset of the rows with exact distance <= bound);
// they are re-scored exactly, ordered (distance, row) and cut at k -- what exact_fallback does with one K4 scan per
// query.  Queries whose band holds more rows than a candidate buffer (2048) come back in `left` for the K4 route.
// The same sweep answers threshold searches of several queries at once (`strict`: distance < bound, every hit: rule.k = all).
static int batched_fallback(smt_ctx *ctx, smt_corpus *corpus, const float *queries_dev, const std::vector<uint32_t> &redo,
                            const std::vector<double> &bounds, const HitRule &rule, std::vector<LocalHits> &out,
                            std::vector<uint32_t> &left, bool strict = false)
{
    const uint32_t n = (uint32_t)redo.size();
    float *d_qc = nullptr;   // compact copies of the uncertain queries + their f32 thresholds (rare path: plain hipMalloc)
    SMT_HIP_CHECK(hipMalloc(&d_qc, (size_t)n * (SMT_DIM + 2) * sizeof(float)));
    struct Free { float *p; ~Free() { (void)hipFree(p); } } guard{d_qc};
    float *d_tau = d_qc + (size_t)n * SMT_DIM;
    uint32_t *d_redo = reinterpret_cast<uint32_t *>(d_tau + n);
    std::vector<float> tau(n);
    // the sweep runs over the corpus' fp16 operand image when it has one (f16 x 2, half the bytes), else over the f32 rows (bf16 x 3)
    const void *image = nullptr;
    const uint32_t *image_zero = nullptr;
    if (image_sweep_allowed(ctx, corpus)) {
        if (int rc_img = corpus_image_sync(corpus, n, &image, &image_zero)) return rc_img;
    }
    const double band = image ? F32_ERR_F16X2 : F32_ERR_BF16X3;
    for (uint32_t i = 0; i < n; ++i) tau[i] = std::nextafter((float)(bounds[i] + band), std::numeric_limits<float>::infinity());
    SMT_HIP_CHECK(hipMemcpyAsync(d_redo, redo.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    int rc_g = launch_gather_rows256(ctx, queries_dev, d_redo, n, d_qc);   // (a copy per query cost 5 us apiece)
    if (rc_g) return rc_g;
    SMT_HIP_CHECK(hipMemcpyAsync(d_tau, tau.data(), n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    const key_t64 *d_cand = nullptr;
    const unsigned int *d_cnt = nullptr;
    uint32_t stride = 0;
    int rc = launch_gemm_threshold(ctx, corpus->d_rows, corpus->rows, image, image_zero, d_qc, n, d_tau, &d_cand, &d_cnt, &stride);
    if (rc) return rc;
    std::vector<unsigned int> cnt(n);
    std::vector<key_t64> keys((size_t)n * stride);
    SMT_HIP_CHECK(hipMemcpyAsync(cnt.data(), d_cnt, n * sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
    SMT_HIP_CHECK(hipMemcpyAsync(keys.data(), d_cand, keys.size() * sizeof(key_t64), hipMemcpyDeviceToHost, ctx->stream));
    SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    // exact distances of every collected row (the scratch that held the candidates is free again)
    std::vector<uint32_t> rows, qidx;
    std::vector<uint64_t> first(n + 1, 0);
    for (uint32_t i = 0; i < n; ++i) {
        first[i] = rows.size();
        if (cnt[i] > stride) continue;   // overflow: K4
        for (uint32_t c = 0; c < cnt[i]; ++c) {
            rows.push_back((uint32_t)(keys[(size_t)i * stride + c] & 0xFFFFFFFFull));
            qidx.push_back(i);
        }
    }
    first[n] = rows.size();
    std::vector<double> dist(rows.size());
    if (!rows.empty()) {   // ONE launch for the rows of all queries (a launch per query cost 11 us apiece: 11.5 of 17.5 ms at 1024 queries)
        const size_t b_rows = (rows.size() * sizeof(uint32_t) + 255) & ~(size_t)255;
        if ((rc = ensure_scratch(ctx, 2 * b_rows + rows.size() * sizeof(double)))) return rc;
        uint32_t *d_rows = reinterpret_cast<uint32_t *>(ctx->d_scratch);
        uint32_t *d_qidx = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(ctx->d_scratch) + b_rows);
        double *d_dist = reinterpret_cast<double *>(reinterpret_cast<char *>(ctx->d_scratch) + 2 * b_rows);
        SMT_HIP_CHECK(hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        SMT_HIP_CHECK(hipMemcpyAsync(d_qidx, qidx.data(), qidx.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        if ((rc = launch_rescore_rows_multi(ctx, corpus->d_rows, d_qc, d_rows, d_qidx, rows.size(), d_dist))) return rc;
        SMT_HIP_CHECK(hipMemcpyAsync(dist.data(), d_dist, rows.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    for (uint32_t i = 0; i < n; ++i) {
        if (cnt[i] > stride) { left.push_back(redo[i]); continue; }
        order_hits(rows.data() + first[i], dist.data() + first[i], first[i + 1] - first[i], bounds[i], strict, /*sorted=*/false, rule,
                   out[redo[i]]);
    }
    return SMT_OK;
}

// ---------------------------------------------------------------- K2 or K3
// Which kernel answers a top-k call of nq queries over `scanned` rows: the scan kernel (K2, <= 4 queries per corpus pass) or the
// batched kernel (K3, one pass for the whole batch; about 1.15 single-query passes whatever its size, while a K2 pass slows down
// with every query it carries).  A pure function of the tuning and the call; the rule as it stands (us per host call, K2 | K3; the
// measurements that moved each border over rounds 2-5 are in profiles/HISTORY.md, "topk_dispatch"):
//  * 8+ queries: K3, always.
//  * `rowreg` -- gemm_bf16x3 and gemm_rowreg on, and a range-filtered call fills its 32-row tiles (tiles_dense, common.h; it counts
//    with the rows it SCANS) -- is required by every rule below.
//  * gemm_min_nq (5) .. 7 queries: K3 at every size when unfiltered (five queries 1000 rows 89 | 76, 2 M 709 | 472); document subsets
//    once rows x queries >= 1.2 x gemm_min_rows_small (1 M), their tile table being one more launch (profiles/r04_k2_k3_small.json).
//  * up to two queries below gemm_min_nq (three, four), unfiltered: K3 between gemm_min_rows_small / 50 and 4/5 of it, 20 k .. 800 k
//    rows (three queries 50 k 88 | 79, 700 k 213 | 208, 1 M 259 | 266; two: K2 everywhere; profiles/r05_sweep_crossover.json).
//  * the fp16 operand image (gemm_image, a call over the whole corpus, not async; image_scan_min_rows > 0): K3 over 512-B rows
//    - from image_scan_min_rows (1.5 M) rows for one or two queries, 2/3 of that for three and more, filtered calls included (one
//      query 1.5 M 245 | 214, 4 M 612 | 461; profiles/r04_image_scan_sweep.json).  Calls of < 8 queries this large COUNT towards
//      building the image of an owned corpus that has none (topk_dispatch);
//    - an image that EXISTS answers unfiltered calls from image_use_min_rows (400 k) rows for one query, 1/5 of that for two, 1/60
//      for three and more (one query 300 k 83 | 86, 500 k 111 | 105; two 50 k 68 | 68, 100 k 77 | 71; profiles/r05_sweep_crossover.json).
struct Route {
    bool batched;            // K3 answers
    bool rowreg;             // ... with gemm_rowreg_kernel, which reads the image of a whole corpus
    bool counts_for_image;
};
// a: what the call asks (nq, n_virtual = the rows it scans, n_ranges, n_vtiles, allow_async); whole: it covers the corpus' own rows, all
// of them; has_image: the corpus has an operand image and may use it
static Route topk_route(const Tuning &tune, const ScanArgs &a, bool whole, bool has_image)
{
    const uint64_t scanned = a.n_virtual;
    const bool rowreg = tune.gemm_bf16x3 && tune.gemm_rowreg && (a.n_ranges == 0 || tiles_dense(scanned, a.n_vtiles));
    const uint64_t small = (uint64_t)tune.gemm_min_rows_small;
    const bool image_ok = rowreg && tune.gemm_image && !a.allow_async && whole && tune.image_scan_min_rows > 0;
    const uint64_t image_min = (uint64_t)tune.image_scan_min_rows * (a.nq >= 3 ? 2 : 3) / 3;
    const bool scan_sized = image_ok && scanned >= image_min;
    const uint64_t use_min = (uint64_t)tune.image_use_min_rows * (a.nq >= 3 ? 1 : a.nq == 2 ? 12 : 60) / 60;
    const bool use_sized = image_ok && a.n_ranges == 0 && tune.image_use_min_rows > 0 && scanned >= use_min;
    const bool mid_band = a.n_ranges == 0 && a.nq >= 3 && a.nq + 2 >= (uint32_t)tune.gemm_min_nq && small > 0 &&
                          scanned >= small / 50 && scanned <= small / 5 * 4;
    const bool batched = a.nq >= 8 ||
                         (rowreg && a.nq >= (uint32_t)tune.gemm_min_nq && (a.n_ranges == 0 || scanned * a.nq >= small + small / 5)) ||
                         (rowreg && mid_band) || ((scan_sized || use_sized) && has_image);
    return Route{batched, rowreg, scan_sized && a.nq < 8};
}

// One top-k launch by the rule above; a batched launch that answers SMT_E_UNSUPPORTED falls back to the scan kernel.
// A resident host asking one query at a time -- `semtools serve` -- never sends the batch of 8 that builds the image of an owned
// corpus: the fourth counted search builds it here, and the route is asked again because this same call then uses it.
static int topk_dispatch(smt_ctx *ctx, smt_corpus *corpus, ScanArgs &a)
{
    const bool whole = corpus->d_rows == a.corpus && corpus->rows == a.rows;
    Route r = topk_route(ctx->tune, a, whole, corpus->image && corpus->image_mode >= 0);
    if (r.counts_for_image && !corpus->image && corpus->owned && corpus->image_mode == 0 && ctx->tune.corpus_image != 0 &&
        ++corpus->small_searches >= 4) {
        const void *img;
        const uint32_t *zero;
        corpus->image_mode = 1;
        if (int rc_img = corpus_image_sync(corpus, a.nq, &img, &zero)) return rc_img;
        if (corpus->image_mode == 1) corpus->image_mode = 0;   // (-1 when there was no room)
        r = topk_route(ctx->tune, a, whole, corpus->image && corpus->image_mode >= 0);
    }
    if (r.batched && r.rowreg && whole) {
        if (int rc_img = corpus_image_sync(corpus, a.nq, &a.image, &a.image_zero)) return rc_img;
    }
    int rc = r.batched ? launch_gemm_topk(ctx, a) : launch_scan_topk(ctx, a);
    if (rc == SMT_E_UNSUPPORTED && r.batched) rc = launch_scan_topk(ctx, a);
    return rc;
}

// The large-k route (topk_large.hip) for a staged call: unfiltered batches of five or more queries sweep the corpus' fp16 operand image
// when it has one (f16 x 2, half the bytes), like the batched re-answer; everything else reads the f32 rows.
static int largek_route(smt_ctx *ctx, smt_corpus *corpus, ScanArgs &a)
{
    if (a.n_ranges == 0 && a.nq >= 5 && image_sweep_allowed(ctx, corpus)) {
        if (int rc_img = corpus_image_sync(corpus, a.nq, &a.image, &a.image_zero)) return rc_img;
    }
    return launch_topk_large(ctx, a);
}

bool query_is_zero(const float *q)
{
    for (uint32_t d = 0; d < SMT_DIM; ++d)
        if (q[d] != 0.0f) return false;
    return true;
}

void workspace_zero_query_hits(const smt_range *ranges, uint32_t n_ranges, uint64_t n_rows, uint32_t top_k, bool has_thr, double max_distance,
                               uint64_t row_base, LocalHits &out)
{
    out.rows.clear();
    out.dist.clear();
    if (has_thr && !(0.0f > 1.0f - (float)max_distance)) return;
    auto take = [&](uint64_t b, uint64_t e) {
        for (uint64_t r = b; r < e && out.rows.size() < top_k; ++r) { out.rows.push_back(row_base + r); out.dist.push_back(1.0); }
    };
    if (n_ranges == 0) take(0, n_rows);
    for (uint32_t i = 0; i < n_ranges && out.rows.size() < top_k; ++i) take(ranges[i].begin, ranges[i].end);
}

// A host-form call after its prologue (search_local_host_impl): queries and ranges on the device, the outputs' place behind them.
struct StagedCall {
    smt_ctx *ctx;
    smt_corpus *corpus;
    const float *d_q;        // [nq x 256]
    uint32_t nq;
    const RangePlan &plan;
    char *d_out;             // the stage behind the inputs: the result lists of a top-k call
    HitRule rule;            // k = min(top_k, rows to scan); the workspace threshold; row_base
    double max_distance;
};

static ScanArgs staged_scan_args(const StagedCall &c)
{
    ScanArgs a = scan_args(c.corpus, c.d_q, c.nq, (uint32_t)c.rule.k, c.rule.row_base);
    c.plan.apply(a);
    a.ws_threshold = c.rule.ws_thr ? 1 : 0;
    a.ws_thr_score = c.rule.thr_score;  // store.rs:502-503
    return a;
}

// The answer of a delivering launch (common.h Delivery): spin on the completion word (a small search is over in tens of
// microseconds); past 200 us ask the runtime, which also reports a launch that failed.
static int await_delivery(smt_ctx *ctx, const Delivery &dl)
{
    volatile unsigned long long *flag = dl.host_flag;
    const auto t0 = std::chrono::steady_clock::now();
    unsigned long long got = 0;
    for (unsigned spins = 1; (got = *flag) == 0; ++spins) {
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();   // (a polite spin: the sibling hyperthread keeps its issue slots)
#endif
        if ((spins & 63) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(200)) {
            SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
            got = *flag;
            break;
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (got != dl.seq) {
        (void)hipStreamSynchronize(ctx->stream);   // (whatever is left of the launch) -- and the block counter starts from zero again
        (void)hipMemsetAsync(ctx->d_status + 4, 0, sizeof(unsigned long long), ctx->stream);
        set_error("the select kernel did not deliver its answer (completion word %llu, expected %llu)", got, dl.seq);
        return SMT_E_HIP;
    }
    ++ctx->deliveries;
    return SMT_OK;
}

// ... and of any other launch: a D2H copy and a synchronise
static int fetch_answer(smt_ctx *ctx, void *host, const void *dev, size_t bytes)
{
    SMT_HIP_CHECK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return SMT_OK;
}

// ---------------- top-k <= SCAN_MAX_K (optionally with the workspace score threshold): K2 or K3, then the uncertain queries again
static int search_topk_small(const StagedCall &c, std::vector<LocalHits> &out)
{
    smt_ctx *ctx = c.ctx;
    const uint32_t nq = c.nq, k_eff = (uint32_t)c.rule.k;
    const size_t o_rows = (size_t)nq * k_eff * sizeof(uint64_t);
    const size_t o_dist = (size_t)nq * k_eff * sizeof(double);
    const size_t o_cnt = (size_t)2 * nq * sizeof(uint64_t);  // counts, then the "uncertain" flags
    const size_t o_bytes = o_rows + o_dist + o_cnt;
    uint64_t *d_ocnt = reinterpret_cast<uint64_t *>(c.d_out + o_rows + o_dist);
    ScanArgs a = staged_scan_args(c);
    a.out_rows = reinterpret_cast<uint64_t *>(c.d_out);
    a.out_dist = reinterpret_cast<double *>(c.d_out + o_rows);
    a.out_counts = d_ocnt;
    a.out_uncertain = d_ocnt + nq;
    int rc = ensure_pinned(ctx, 64 + o_bytes);
    if (rc) return rc;
    // the answers' place in the pinned buffer: behind a 64-byte line whose first word is the completion word of a delivered answer
    char *h_ans = reinterpret_cast<char *>(ctx->h_pinned) + 64;
    // A SMALL answer is delivered by the select kernel itself (common.h Delivery): its last block copies the device block
    // [rows | distances | counts | flags] into the pinned buffer and stores this call's sequence number behind it; the host waits
    // for that word -- no D2H copy command, no hipStreamSynchronize: ~10 us of every small call (profiles/r06_call_floor.json,
    // profiles/r06_small_calls.json).  One select launch answers the whole call (<= 32 queries: below the batched kernel's pass size).
    const bool direct = ctx->tune.direct_delivery != 0 && nq <= 32 && o_bytes <= 8192;
    Delivery dl;
    if (direct) {
        dl.dev_out = reinterpret_cast<const unsigned long long *>(c.d_out);
        dl.host_out = reinterpret_cast<unsigned long long *>(h_ans);
        dl.n_words = (uint32_t)(o_bytes / 8);
        dl.host_flag = reinterpret_cast<unsigned long long *>(ctx->h_pinned);
        dl.seq = ++ctx->deliver_seq;
        dl.done = ctx->d_status + 4;
        *reinterpret_cast<volatile unsigned long long *>(dl.host_flag) = 0;
        a.deliver = &dl;
    }
    if ((rc = topk_dispatch(ctx, c.corpus, a))) return rc;
    if ((rc = direct ? await_delivery(ctx, dl) : fetch_answer(ctx, h_ans, c.d_out, o_bytes))) return rc;
    const uint64_t *h_rows = reinterpret_cast<const uint64_t *>(h_ans);
    const double *h_dist = reinterpret_cast<const double *>(h_ans + o_rows);
    const uint64_t *h_cnt = reinterpret_cast<const uint64_t *>(h_ans + o_rows + o_dist);
    std::vector<uint32_t> redo;
    for (uint32_t q = 0; q < nq; ++q) {
        const uint64_t n = h_cnt[q];
        out[q].rows.assign(h_rows + (size_t)q * k_eff, h_rows + (size_t)q * k_eff + n);
        out[q].dist.assign(h_dist + (size_t)q * k_eff, h_dist + (size_t)q * k_eff + n);
        if (h_cnt[nq + q]) redo.push_back(q);  // (h_pinned is reused by the fallback: copy everything out first)
    }
    // queries whose f32 nomination could not be proven sufficient (a cluster of near-ties around the k-th
    // place that is wider than the guard band): answer them exhaustively -- several of them with ONE batched
    // threshold pass over the shard (batched_fallback), the rest (and whatever overflows there) one K4 scan each
    auto bound_of = [&](uint32_t q) {
        return out[q].rows.size() == k_eff ? out[q].dist.back() : 1.0 - (double)c.rule.thr_score;
    };
    if (c.plan.nr == 0 && redo.size() >= 2 && ctx->tune.gemm_bf16x3 && ctx->tune.gemm_rowreg &&
        c.corpus->rows >= (uint64_t)ctx->tune.fallback_batch_min_rows) {
        std::vector<double> bounds;
        for (uint32_t q : redo) bounds.push_back(bound_of(q));
        std::vector<uint32_t> left;
        if ((rc = batched_fallback(ctx, c.corpus, c.d_q, redo, bounds, c.rule, out, left))) return rc;
        redo.swap(left);
    }
    for (uint32_t q : redo)
        if ((rc = exact_fallback(ctx, c.corpus, c.d_q + (size_t)q * SMT_DIM, c.plan, bound_of(q), c.rule, out[q]))) return rc;
    return SMT_OK;
}

// 57 <= k <= 1024: the sampled-threshold route (topk_large.hip) answers every query of the call in three launches; proved[q] = 1
// where it could prove its answer (not: ties across tau, an overflowed buffer).  Lists [rows | distances | verdicts] in the stage
// behind the inputs, home through the pinned buffer.
static int largek_sampled(const StagedCall &c, std::vector<char> &proved, std::vector<LocalHits> &out)
{
    smt_ctx *ctx = c.ctx;
    const uint32_t nq = c.nq, k_eff = (uint32_t)c.rule.k;
    const size_t kw = (size_t)nq * k_eff, o_words = 2 * kw + nq;
    uint64_t *d_out = reinterpret_cast<uint64_t *>(c.d_out);
    ScanArgs a = staged_scan_args(c);
    a.out_rows = d_out;
    a.out_dist = reinterpret_cast<double *>(d_out + kw);
    a.out_uncertain = d_out + 2 * kw;
    int rc = largek_route(ctx, c.corpus, a);
    if (rc) return rc;
    if ((rc = ensure_pinned(ctx, o_words * sizeof(uint64_t)))) return rc;
    const uint64_t *h = reinterpret_cast<const uint64_t *>(ctx->h_pinned);
    if ((rc = fetch_answer(ctx, ctx->h_pinned, d_out, o_words * sizeof(uint64_t)))) return rc;
    for (uint32_t q = 0; q < nq; ++q) {
        if (h[2 * kw + q] != SMT_STATUS_PROVED) continue;
        proved[q] = 1;
        const uint64_t *r = h + (size_t)q * k_eff;
        const double *d = reinterpret_cast<const double *>(h + kw) + (size_t)q * k_eff;
        uint32_t n = 0;
        while (n < k_eff && r[n] != UINT64_MAX) ++n;
        out[q].rows.assign(r, r + n);
        out[q].dist.assign(d, d + n);
    }
    return SMT_OK;
}

// ONE query by the all-keys path (largek.hip): all keys + sort + exact rescoring of k + guard candidates, then the exactness
// certificate over them and the K4 re-answer where it fails.
static int largek_all_keys(const StagedCall &c, uint32_t q, LocalHits &out)
{
    const RangePlan &plan = c.plan;
    const uint64_t k_eff = c.rule.k;
    const uint64_t guard = std::max<uint64_t>(64, k_eff / 16);
    const uint64_t n_cand = std::min<uint64_t>(plan.n_virtual, k_eff + guard);
    const float *query_dev = c.d_q + (size_t)q * SMT_DIM;
    std::vector<uint32_t> c_rows;
    std::vector<double> c_dist;
    float next_d32 = 0.f;
    int rc = launch_largek_candidates(c.ctx, c.corpus->d_rows, query_dev, plan.d_r, plan.d_p, plan.nr, plan.n_virtual, n_cand, c_rows, c_dist,
                                      &next_d32);
    if (rc) return rc;
    order_hits(c_rows.data(), c_dist.data(), c_rows.size(), std::numeric_limits<double>::infinity(), false, /*sorted=*/false, c.rule, out);
    // exactness certificate (SelectArgs::f32_err): rows outside the candidates have exact distance >= floor_out
    const uint64_t n = out.rows.size();
    const double floor_out = (double)next_d32 - F32_ERR_SCAN;
    const bool certain = n == k_eff ? floor_out > out.dist[n - 1]
                                    : (c.rule.ws_thr ? !ws_score_passes(floor_out, c.rule.thr_score) : next_d32 == __builtin_inff());
    if (certain) return SMT_OK;
    const double bound = n == k_eff ? out.dist[n - 1] : 1.0 - (double)c.rule.thr_score;
    return exact_fallback(c.ctx, c.corpus, query_dev, plan, bound, c.rule, out);
}

// ---------------- top-k > SCAN_MAX_K (also k in 57..64, where the f32 scan's candidate lists have no room left for the guard band)
static int search_topk_large(const StagedCall &c, std::vector<LocalHits> &out)
{
    std::vector<char> proved(c.nq, 0);
    if (c.ctx->tune.largek_sampled && c.rule.k <= LARGEK_MAX_K)
        if (int rc = largek_sampled(c, proved, out)) return rc;
    for (uint32_t q = 0; q < c.nq; ++q)   // what the sampled route did not prove (or take) is answered exactly as before it existed
        if (!proved[q])
            if (int rc = largek_all_keys(c, q, out[q])) return rc;
    return SMT_OK;
}

// ---------------- all rows with distance < max_distance (mod.rs:88-89,115-116)
static int search_all_under(const StagedCall &c, std::vector<LocalHits> &out)
{
    smt_ctx *ctx = c.ctx;
    // several queries on a large unfiltered shard: ONE sweep of the batched kernel collects every query's hits (up to a
    // candidate buffer, 2048 rows, each); a query with more hits than that takes the streaming K4 scan below
    std::vector<uint32_t> todo(c.nq);
    for (uint32_t q = 0; q < c.nq; ++q) todo[q] = q;
    if (c.plan.nr == 0 && c.nq >= 2 && ctx->tune.gemm_bf16x3 && ctx->tune.gemm_rowreg && c.max_distance <= 2.5 &&
        c.corpus->rows >= (uint64_t)ctx->tune.fallback_batch_min_rows) {
        std::vector<double> bounds(c.nq, c.max_distance);
        std::vector<uint32_t> left;
        const HitRule every{~0ull, false, 0.f, c.rule.row_base};
        if (int rc = batched_fallback(ctx, c.corpus, c.d_q, todo, bounds, every, out, left, /*strict=*/true)) return rc;
        todo.swap(left);
    }
    for (uint32_t q : todo) {
        const ThresholdQuery t = threshold_query(c.corpus, c.d_q + (size_t)q * SMT_DIM, c.plan, c.max_distance);
        const uint32_t *h_rows = nullptr;
        const double *h_dist = nullptr;
        uint64_t n_ok = 0;
        if (int rc = run_threshold_query(ctx, t, &h_rows, &h_dist, &n_ok)) return rc;
        out[q].rows.resize(n_ok);
        for (uint64_t i = 0; i < n_ok; ++i) out[q].rows[i] = c.rule.row_base + h_rows[i];
        out[q].dist.assign(h_dist, h_dist + n_ok);
    }
    return SMT_OK;
}

// The search proper: argument checks, the range plan, ONE upload of everything the call reads, then one of the three bodies above.
static int search_local_host_impl(smt_corpus *corpus, const float *queries, uint32_t nq, uint32_t top_k, double max_distance, int mode,
                                  const smt_range *ranges, uint32_t n_ranges, uint64_t row_base, std::vector<LocalHits> &out)
{
    SMT_REQUIRE(corpus != nullptr, "corpus");
    SMT_REQUIRE(mode == SMT_MODE_DOCUMENTS || mode == SMT_MODE_WORKSPACE, "mode");
    SMT_REQUIRE(nq == 0 || queries, "null argument");
    SMT_REQUIRE(n_ranges == 0 || ranges != nullptr, "ranges");
    smt_ctx *ctx = corpus->ctx;
    int rc = bind_device(ctx);
    if (rc) return rc;
    out.assign(nq, LocalHits());
    if (nq == 0) return SMT_OK;
    if ((rc = require_queries_domain_host(queries, nq, "search"))) return rc;   // (domain.hip: finite, ordinary magnitudes)

    const bool has_thr = !std::isnan(max_distance);
    const bool all_under_threshold = (mode == SMT_MODE_DOCUMENTS) && has_thr;

    // drop empty ranges; total rows to scan.  A list searched before has its device copy (and tables) kept on the corpus.
    RangePlan plan;
    plan.n_virtual = corpus->rows;
    if (n_ranges && (rc = range_plan_find(corpus, ranges, n_ranges, plan))) return rc;
    if (plan.n_virtual == 0) return SMT_OK;
    if (!all_under_threshold && top_k == 0) return SMT_OK;  // take(0) / store.rs:489-491
    if ((rc = range_plan_finish(corpus, plan))) return rc;

    // ---- device staging: one persistent buffer per context, [queries | ranges | 3 prefixes | result lists] (no per-call hipMalloc/hipFree)
    const size_t q_bytes = (size_t)nq * SMT_DIM * sizeof(float);
    const size_t up_bytes = q_bytes + plan.upload_bytes();
    const size_t in_bytes = (q_bytes + plan.table_bytes() + 255) & ~(size_t)255;
    // (the result lists of the large-k route, 57 <= k <= 1024, are staged here too)
    const uint64_t k_eff = std::min<uint64_t>(top_k, plan.n_virtual);
    const bool largek_lists = ctx->tune.largek_sampled && k_eff > SCAN_MAX_K && k_eff <= LARGEK_MAX_K;
    const uint32_t k_stage = all_under_threshold ? 0u : (uint32_t)std::min<uint64_t>(k_eff, largek_lists ? LARGEK_MAX_K : 64);
    const size_t out_bytes_stage = (size_t)nq * k_stage * 16 + (size_t)2 * nq * sizeof(uint64_t);
    if ((rc = ensure_stage(ctx, in_bytes + out_bytes_stage + 64))) return rc;
    char *stage = reinterpret_cast<char *>(ctx->d_stage);
    // queries, ranges and the three prefixes are assembled in ONE pinned buffer (laid out like the device stage) and go up in one
    // copy: four pageable hipMemcpyAsync calls -- each staged by the runtime before it returns -- were ~50 us of a 0.6 ms call
    if ((rc = ensure_pinned_in(ctx, up_bytes))) return rc;
    char *pin = reinterpret_cast<char *>(ctx->h_pinned_in);
    memcpy(pin, queries, q_bytes);
    plan.write(pin + q_bytes);
    SMT_HIP_CHECK(hipMemcpyAsync(stage, pin, up_bytes, hipMemcpyHostToDevice, ctx->stream));
    plan.bind(stage + q_bytes);   // (a kept set: only the queries went up)

    const HitRule rule{k_eff, mode == SMT_MODE_WORKSPACE && has_thr, 1.0f - (float)max_distance /* store.rs:502-503 */, row_base};
    const StagedCall call{ctx, corpus, reinterpret_cast<const float *>(stage), nq, plan, stage + in_bytes, rule, max_distance};
    if (all_under_threshold) return search_all_under(call, out);
    return k_eff > SCAN_MAX_K ? search_topk_large(call, out) : search_topk_small(call, out);
}

// The body of smt_search with per-query result vectors instead of caller arrays: sharded_search.cpp runs it once per
// local shard (threshold mode / top_k > 64, whose result sizes are not known up front) and exchanges the lists.
// Store::search_line_embeddings with a ZERO query vector (an empty query, or one made of unknown tokens only: model2vec pools it to
// zeros).  qdrant's cosine_preprocess leaves a vector with |x|^2 < f32::EPSILON as it is, so the query scores 0 against EVERY point --
// distance 1.0 for all of them, zero rows included -- where simsimd's rule for search_documents says (zero, zero) -> distance 0
// (oracle: orc_search_line_embeddings against orc_cosine_*; src/workspace/store.rs:500-531).  The answer is a constant, so it is
// written here instead of being computed: with a threshold nothing unless 0 > 1 - max_distance (f32), else the first top_k rows of
// the subset in storage order (equal scores: earlier row first, as in the oracle), each at distance 1.0.
int search_local_host(smt_corpus *corpus, const float *queries, uint32_t nq, uint32_t top_k, double max_distance, int mode,
                      const smt_range *ranges, uint32_t n_ranges, uint64_t row_base, std::vector<LocalHits> &out)
{
    if (mode != SMT_MODE_WORKSPACE || !queries || nq == 0)
        return search_local_host_impl(corpus, queries, nq, top_k, max_distance, mode, ranges, n_ranges, row_base, out);
    // workspace mode: zero queries never reach the GPU (every row ties at distance 1.0: the kernels would flag the answer uncertain
    // and the exhaustive re-answer would collect the whole subset to order a constant)
    std::vector<uint32_t> live;
    for (uint32_t q = 0; q < nq; ++q)
        if (!query_is_zero(queries + (size_t)q * SMT_DIM)) live.push_back(q);
    if (live.size() == nq) return search_local_host_impl(corpus, queries, nq, top_k, max_distance, mode, ranges, n_ranges, row_base, out);
    SMT_REQUIRE(corpus != nullptr, "corpus");
    std::vector<float> packed(live.size() * (size_t)SMT_DIM);
    for (size_t j = 0; j < live.size(); ++j) memcpy(&packed[j * SMT_DIM], queries + (size_t)live[j] * SMT_DIM, SMT_DIM * sizeof(float));
    std::vector<LocalHits> part;
    // (an all-zero batch still goes through the argument checks of the search proper: ranges, mode, the corpus' device)
    int rc = search_local_host_impl(corpus, packed.empty() ? queries : packed.data(), packed.empty() ? 0u : (uint32_t)live.size(), top_k,
                                    max_distance, mode, ranges, n_ranges, row_base, part);
    if (rc) return rc;
    if (n_ranges) {   // (validated by the search proper only when it had a query to answer)
        uint64_t prev_end = 0;
        for (uint32_t i = 0; i < n_ranges; ++i) {
            SMT_REQUIRE(ranges[i].begin <= ranges[i].end && ranges[i].end <= corpus->rows && (i == 0 || ranges[i].begin >= prev_end),
                        "ranges must be sorted, disjoint and inside the corpus");
            prev_end = ranges[i].end;
        }
    }
    out.assign(nq, LocalHits());
    for (size_t j = 0; j < live.size(); ++j) out[live[j]] = std::move(part[j]);
    for (uint32_t q = 0; q < nq; ++q)
        if (query_is_zero(queries + (size_t)q * SMT_DIM))
            workspace_zero_query_hits(ranges, n_ranges, corpus->rows, top_k, !std::isnan(max_distance), max_distance, row_base, out[q]);
    return SMT_OK;
}

// Copy per-query hit lists into the caller's [nq x out_cap] arrays; counts hold the TRUE sizes.
int deliver_hits(const std::vector<LocalHits> &hits, uint64_t *out_rows, double *out_dist, uint64_t *out_counts, uint64_t out_cap)
{
    bool truncated = false;
    for (size_t q = 0; q < hits.size(); ++q) {
        const uint64_t n = hits[q].rows.size();
        out_counts[q] = n;
        const uint64_t w = std::min<uint64_t>(n, out_cap);
        if (n > out_cap) truncated = true;
        if (w) {
            SMT_REQUIRE(out_rows && out_dist, "null output");
            memcpy(out_rows + q * out_cap, hits[q].rows.data(), (size_t)w * sizeof(uint64_t));
            memcpy(out_dist + q * out_cap, hits[q].dist.data(), (size_t)w * sizeof(double));
        }
    }
    if (truncated) { set_error("out_cap smaller than the number of hits"); return SMT_E_TRUNCATED; }
    return SMT_OK;
}

// One shard's top-k with everything on the device (the exchange path of sharded_search.cpp).  queries_dev [nq x 256];
// ranges_local = sorted, disjoint LOCAL row ranges (host array); filtered && n_ranges == 0 means "the filter
// leaves this shard nothing to scan".  packed_dev [nq][2][k_pad] receives global rows, then f64 distance bit
// patterns, padded with (UINT64_MAX, +inf).  1 <= k_pad <= LARGEK_MAX_K (above SCAN_MAX_K: topk_large.hip).  Enqueued on the context's stream (the
// select stage on the aux stream when allow_async and the async_select tuning key say so); no host sync.
int search_topk_packed_local(smt_corpus *corpus, const float *queries_dev, uint32_t nq, uint32_t k_pad, int ws_threshold,
                             float ws_thr_score, const smt_range *ranges_local, uint32_t n_ranges, bool filtered,
                             uint64_t row_base, uint64_t *packed_dev, uint64_t *uncertain_dev, bool allow_async)
{
    SMT_REQUIRE(corpus && queries_dev && packed_dev, "null argument");
    smt_ctx *ctx = corpus->ctx;
    SMT_REQUIRE(k_pad >= 1 && k_pad <= (ctx->tune.largek_sampled ? LARGEK_MAX_K : SCAN_MAX_K),
                ctx->tune.largek_sampled ? "top_k of the device exchange path must be in [1, 1024]"
                                         : "top_k of the device exchange path must be in [1, 56] (largek_sampled = 0)");
    RangePlan plan;
    plan.n_virtual = corpus->rows;
    if (filtered)
        if (int rcv = range_plan_find(corpus, ranges_local, n_ranges, plan)) return rcv;
    const uint32_t k_eff = (uint32_t)std::min<uint64_t>(k_pad, plan.n_virtual);
    const bool async = allow_async && ctx->tune.async_select && nq == 1 && !filtered && k_eff == k_pad && k_pad <= SCAN_MAX_K;
    int rc = bind_device(ctx, !async);
    if (rc) return rc;
    if (k_eff < k_pad) {  // short or empty shard: padding first, the select then overwrites the head of each list
        if ((rc = launch_merge_topk_packed_on(ctx, ctx->stream, packed_dev, 0, nq, 1, k_pad, packed_dev))) return rc;
        if (k_eff == 0) {
            if (uncertain_dev) SMT_HIP_CHECK(hipMemsetAsync(uncertain_dev, 0, (size_t)nq * sizeof(uint64_t), ctx->stream));
            return SMT_OK;
        }
    }
    if ((rc = range_plan_finish(corpus, plan))) return rc;
    if (plan.upload_bytes() && (rc = ensure_stage(ctx, plan.upload_bytes() + 64))) return rc;
    plan.bind(reinterpret_cast<char *>(ctx->d_stage));
    if (plan.upload_bytes()) {
        SMT_HIP_CHECK(hipMemcpyAsync(const_cast<smt_range *>(plan.d_r), plan.rr.data(), plan.r_bytes(), hipMemcpyHostToDevice, ctx->stream));
        SMT_HIP_CHECK(hipMemcpyAsync(const_cast<uint64_t *>(plan.d_p), plan.prefixes.data(), plan.prefixes.size() * sizeof(uint64_t),
                                     hipMemcpyHostToDevice, ctx->stream));
        SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // the host vectors die with this frame
    }
    ScanArgs a = scan_args(corpus, queries_dev, nq, k_eff, row_base);
    plan.apply(a);
    a.ws_threshold = ws_threshold;
    a.ws_thr_score = ws_thr_score;
    a.out_rows = packed_dev;
    a.out_dist = reinterpret_cast<double *>(packed_dev + k_pad);
    a.out_uncertain = uncertain_dev;
    a.allow_async = async;
    a.out_stride = (uint64_t)2 * k_pad;
    return k_eff > SCAN_MAX_K ? largek_route(ctx, corpus, a) : topk_dispatch(ctx, corpus, a);
}

}  // namespace smt

extern "C" {

int smt_search(smt_corpus *corpus, const float *queries, uint32_t nq, uint32_t top_k, double max_distance, int mode,
               const smt_range *ranges, uint32_t n_ranges, uint64_t row_base, uint64_t *out_rows, double *out_dist,
               uint64_t *out_counts, uint64_t out_cap)
try {
    SMT_REQUIRE(nq == 0 || out_counts, "null argument");
    std::vector<LocalHits> hits;
    int rc = search_local_host(corpus, queries, nq, top_k, max_distance, mode, ranges, n_ranges, row_base, hits);
    if (rc) return rc;
    return deliver_hits(hits, out_rows, out_dist, out_counts, out_cap);
} catch (...) { return smt::api_catch(); }

int smt_debug_deliveries(smt_ctx *ctx, uint64_t *count)
try {
    SMT_REQUIRE(ctx != nullptr && count != nullptr, "null argument");
    *count = ctx->deliveries;
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

int smt_debug_range_sets(const smt_corpus *corpus, uint64_t *kept, uint64_t *hits, uint64_t *builds)
try {
    SMT_REQUIRE(corpus != nullptr, "corpus");
    if (kept) *kept = corpus->range_sets.size();
    if (hits) *hits = corpus->range_set_hits;
    if (builds) *builds = corpus->range_set_builds;
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

int smt_search_topk_device(smt_corpus *corpus, const float *queries_dev, uint32_t nq, uint32_t top_k, uint64_t row_base,
                           uint64_t *out_rows_dev, double *out_dist_dev)
try {
    return smt_search_topk_device_ex(corpus, queries_dev, nq, top_k, row_base, out_rows_dev, out_dist_dev, nullptr);
} catch (...) { return smt::api_catch(); }

int smt_search_topk_device_ex(smt_corpus *corpus, const float *queries_dev, uint32_t nq, uint32_t top_k, uint64_t row_base,
                              uint64_t *out_rows_dev, double *out_dist_dev, uint32_t *out_status_dev)
try {
    SMT_REQUIRE(corpus != nullptr, "corpus");
    SMT_REQUIRE(nq == 0 || (queries_dev && out_rows_dev && out_dist_dev), "null argument");
    smt_ctx *ctx = corpus->ctx;
    const bool large = top_k > SCAN_MAX_K;   // 57..1024: the sampled-threshold route (topk_large.hip; tuning key largek_sampled)
    SMT_REQUIRE(top_k >= 1 && top_k <= (ctx->tune.largek_sampled ? LARGEK_MAX_K : SCAN_MAX_K),
                ctx->tune.largek_sampled ? "top_k must be in [1, 1024]" : "top_k must be in [1, 56] (largek_sampled = 0)");
    const bool async = !large && ctx->tune.async_select && nq == 1 && corpus->rows > 0;  // launch_scan_topk keeps the pipeline going
    int rc = bind_device(ctx, !async);
    if (rc) return rc;
    if (nq == 0) return SMT_OK;
    ScanArgs a = scan_args(corpus, queries_dev, nq, top_k, row_base);
    a.out_rows = out_rows_dev;
    a.out_dist = out_dist_dev;
    a.out_status = out_status_dev;
    a.allow_async = async;
    a.allow_overlap = async;
    if (large) return largek_route(ctx, corpus, a);   // (also pads the lists of an empty corpus)
    if (corpus->rows == 0) {
        // nothing to scan: fill with padding through the merge kernel on zero lists (an empty answer is a proved one)
        if (out_status_dev) SMT_HIP_CHECK(hipMemsetAsync(out_status_dev, 0, (size_t)nq * sizeof(uint32_t), ctx->stream));
        return launch_merge_topk(ctx, out_rows_dev, out_dist_dev, 0, nq, 1, top_k, out_rows_dev, out_dist_dev);
    }
    return topk_dispatch(ctx, corpus, a);
} catch (...) { return smt::api_catch(); }

int smt_debug_batched_scores(smt_corpus *corpus, const float *queries, uint32_t nq, uint64_t first_row, uint32_t n_rows,
                             float *out)
try {
    SMT_REQUIRE(corpus && queries && out, "null argument");
    SMT_REQUIRE(first_row + n_rows <= corpus->rows, "row range outside the corpus");
    smt_ctx *ctx = corpus->ctx;
    int rc = bind_device(ctx, true);
    if (rc) return rc;
    const size_t b_q = (size_t)nq * 256 * 4, b_out = (size_t)n_rows * 32 * 4;
    if ((rc = ensure_scratch(ctx, b_q + b_out + 256))) return rc;
    float *d_q = reinterpret_cast<float *>(ctx->d_scratch);
    float *d_out = reinterpret_cast<float *>(reinterpret_cast<char *>(ctx->d_scratch) + ((b_q + 255) & ~(size_t)255));
    SMT_HIP_CHECK(hipMemcpyAsync(d_q, queries, b_q, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = launch_gemm_debug_scores(ctx, corpus->d_rows, first_row, n_rows, d_q, nq, d_out))) return rc;
    SMT_HIP_CHECK(hipMemcpyAsync(out, d_out, b_out, hipMemcpyDeviceToHost, ctx->stream));
    SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

// The ScanArgs of a real batched call of nq host queries over the whole corpus, for the K3 test hooks: ranges through the range plan,
// the operand image as topk_dispatch.  Staged: the queries, then nq_pad floats (tau, may be null), then the plan's tables.
static int debug_batch_args(smt_corpus *corpus, const float *queries, uint32_t nq, uint32_t top_k, const smt_range *ranges, uint32_t n_ranges,
                            const float *tau, RangePlan &plan, ScanArgs &a, const float **tau_dev)
{
    smt_ctx *ctx = corpus->ctx;
    const uint32_t nq_pad = (nq + 31) / 32 * 32;
    int rc;
    plan.n_virtual = corpus->rows;
    if (n_ranges && (rc = range_plan_find(corpus, ranges, n_ranges, plan))) return rc;
    SMT_REQUIRE(plan.n_virtual >= 1, "debug nominations: nothing to scan");
    if ((rc = range_plan_finish(corpus, plan))) return rc;
    const size_t q_bytes = (size_t)nq * SMT_DIM * sizeof(float), t_bytes = (size_t)nq_pad * sizeof(float);
    if ((rc = ensure_stage(ctx, q_bytes + t_bytes + plan.table_bytes() + 64))) return rc;
    char *stage = reinterpret_cast<char *>(ctx->d_stage);
    SMT_HIP_CHECK(hipMemcpyAsync(stage, queries, q_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (tau) { SMT_HIP_CHECK(hipMemcpyAsync(stage + q_bytes, tau, (size_t)nq * sizeof(float), hipMemcpyHostToDevice, ctx->stream)); }
    plan.bind(stage + q_bytes + t_bytes);
    if (plan.upload_bytes()) {
        SMT_HIP_CHECK(hipMemcpyAsync(const_cast<smt_range *>(plan.d_r), plan.rr.data(), plan.r_bytes(), hipMemcpyHostToDevice, ctx->stream));
        SMT_HIP_CHECK(hipMemcpyAsync(const_cast<uint64_t *>(plan.d_p), plan.prefixes.data(), plan.prefixes.size() * sizeof(uint64_t),
                                     hipMemcpyHostToDevice, ctx->stream));
    }
    a = scan_args(corpus, reinterpret_cast<const float *>(stage), nq, top_k, 0);
    plan.apply(a);
    if (ctx->tune.gemm_bf16x3 && ctx->tune.gemm_rowreg && (a.n_ranges == 0 || tiles_dense(a.n_virtual, a.n_vtiles))) {
        if ((rc = corpus_image_sync(corpus, a.nq, &a.image, &a.image_zero))) return rc;
    }
    *tau_dev = reinterpret_cast<const float *>(stage + q_bytes);
    return SMT_OK;
}

static int debug_nominations(smt_corpus *corpus, const float *queries, uint32_t nq, uint32_t top_k, const smt_range *ranges, uint32_t n_ranges,
                             const float *tau, int buffered, const GemmDebugLevel &level, float *out_dist, uint32_t *out_hits,
                             uint32_t *out_counts, uint32_t *out_route)
{
    SMT_REQUIRE(corpus && queries && tau && out_dist && out_hits && out_counts && out_route, "null argument");
    SMT_REQUIRE(n_ranges == 0 || ranges != nullptr, "ranges");
    SMT_REQUIRE(nq >= 1 && nq <= 64, "debug nominations: 1..64 queries");
    smt_ctx *ctx = corpus->ctx;
    int rc = bind_device(ctx, true);
    if (rc) return rc;
    const uint32_t nq_pad = (nq + 31) / 32 * 32;
    const uint64_t rows = corpus->rows;
    for (uint64_t i = 0; i < rows * nq; ++i) { out_dist[i] = std::numeric_limits<float>::quiet_NaN(); out_hits[i] = 0; }
    for (uint32_t q = 0; q < nq_pad; ++q) out_counts[q] = 0;
    *out_route = 0;
    RangePlan plan;
    ScanArgs a;
    const float *tau_dev = nullptr;
    if ((rc = debug_batch_args(corpus, queries, nq, top_k, ranges, n_ranges, tau, plan, a, &tau_dev))) return rc;
    const key_t64 *cand = nullptr;
    const unsigned int *counts = nullptr;
    if ((rc = launch_gemm_debug_nominations(ctx, a, tau_dev, buffered, level, &cand, &counts, out_route))) return rc;
    std::vector<key_t64> keys((size_t)nq_pad * 2048);
    SMT_HIP_CHECK(hipMemcpyAsync(keys.data(), cand, keys.size() * sizeof(key_t64), hipMemcpyDeviceToHost, ctx->stream));
    SMT_HIP_CHECK(hipMemcpyAsync(out_counts, counts, (size_t)nq_pad * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (uint32_t q = 0; q < nq; ++q) {
        SMT_REQUIRE(out_counts[q] <= 2048, "debug nominations: a query was nominated more often than rows were scanned");
        for (uint32_t i = 0; i < out_counts[q]; ++i) {
            const key_t64 key = keys[(size_t)q * 2048 + i];
            const uint64_t row = key & 0xFFFFFFFFull;
            if (row >= rows) {
                set_error("debug nominations: slot %u of query %u names row %llu (the corpus has %llu; 4294967295 = a counted slot nobody wrote)",
                          i, q, (unsigned long long)row, (unsigned long long)rows);
                return SMT_E_INVALID;
            }
            const uint32_t bits = (uint32_t)(key >> 32);
            memcpy(&out_dist[row * nq + q], &bits, sizeof(bits));
            ++out_hits[row * nq + q];
        }
    }
    return SMT_OK;
}

int smt_debug_nominations(smt_corpus *corpus, const float *queries, uint32_t nq, uint32_t top_k, const smt_range *ranges, uint32_t n_ranges,
                          const float *tau, int buffered, float *out_dist, uint32_t *out_hits, uint32_t *out_counts, uint32_t *out_route)
try {
    return debug_nominations(corpus, queries, nq, top_k, ranges, n_ranges, tau, buffered, GemmDebugLevel{}, out_dist, out_hits, out_counts, out_route);
} catch (...) { return smt::api_catch(); }

int smt_debug_level_nominations(smt_corpus *corpus, const float *queries, uint32_t nq, uint32_t top_k, const smt_range *ranges,
                                uint32_t n_ranges, const float *tau, int buffered, uint64_t stride, uint32_t skip, uint64_t tile_begin,
                                uint64_t tile_end, float *out_dist, uint32_t *out_hits, uint32_t *out_counts, uint32_t *out_route)
try {
    SMT_REQUIRE(skip <= 64 && tile_end != UINT64_MAX, "debug nominations: the level");
    GemmDebugLevel level;
    level.stride = stride;
    level.skip = (int)skip;
    level.tile_begin = tile_begin;
    level.tile_end = tile_end;
    return debug_nominations(corpus, queries, nq, top_k, ranges, n_ranges, tau, buffered, level, out_dist, out_hits, out_counts, out_route);
} catch (...) { return smt::api_catch(); }

int smt_debug_bootstrap_minima(smt_corpus *corpus, const float *queries, uint32_t nq, uint32_t top_k, const smt_range *ranges,
                               uint32_t n_ranges, float *out_tile_min, uint32_t *out_slots, uint64_t *out_stride, uint32_t *out_route)
try {
    SMT_REQUIRE(corpus && queries && out_tile_min && out_slots && out_stride && out_route, "null argument");
    SMT_REQUIRE(n_ranges == 0 || ranges != nullptr, "ranges");
    SMT_REQUIRE(nq >= 1 && nq <= 64, "debug bootstrap: 1..64 queries");
    smt_ctx *ctx = corpus->ctx;
    int rc = bind_device(ctx, true);
    if (rc) return rc;
    *out_slots = 0; *out_stride = 0; *out_route = 0;
    RangePlan plan;
    ScanArgs a;
    const float *unused = nullptr;
    if ((rc = debug_batch_args(corpus, queries, nq, top_k, ranges, n_ranges, nullptr, plan, a, &unused))) return rc;
    const float *tile_min = nullptr;
    if ((rc = launch_gemm_debug_bootstrap(ctx, a, &tile_min, out_slots, out_stride, out_route))) return rc;
    const uint32_t nq_pad = (nq + 31) / 32 * 32;
    SMT_HIP_CHECK(hipMemcpyAsync(out_tile_min, tile_min, (size_t)*out_slots * nq_pad * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

int smt_debug_bootstrap_tau(smt_ctx *ctx, const float *tile_min_dev, uint32_t n_slots, uint32_t nq, uint32_t nq_pad, uint32_t kp,
                            float *tau_dev, float *qconst_dev)
try {
    int rc = check_ctx(ctx);
    if (rc) return rc;
    SMT_REQUIRE(tile_min_dev && tau_dev && qconst_dev, "null argument");
    if ((rc = bind_device(ctx))) return rc;
    return launch_debug_bootstrap_tau(ctx, tile_min_dev, n_slots, nq, nq_pad, kp, tau_dev, qconst_dev);
} catch (...) { return smt::api_catch(); }

int smt_debug_level_select(smt_ctx *ctx, uint64_t *cand_dev, uint32_t *counts_dev, uint32_t *overflow_dev, float *tau_dev, float *qconst_dev,
                           uint32_t nq, uint32_t kp)
try {
    int rc = check_ctx(ctx);
    if (rc) return rc;
    SMT_REQUIRE(cand_dev && counts_dev && overflow_dev && tau_dev, "null argument");
    if ((rc = bind_device(ctx))) return rc;
    return launch_debug_level_select(ctx, reinterpret_cast<key_t64 *>(cand_dev), counts_dev, overflow_dev, tau_dev, qconst_dev, nq, kp);
} catch (...) { return smt::api_catch(); }

int smt_debug_gemm_plan(uint64_t plan_tiles, uint32_t nq, uint32_t kp, int family, int f16x1, uint32_t blocks, int gemm_bootstrap,
                        int gemm_boot_fine, int gemm_split_last, int gemm_qsplit, uint64_t *out, uint32_t out_cap, uint32_t *out_n)
try {
    SMT_REQUIRE(out_n != nullptr && (out != nullptr || out_cap == 0), "null argument");
    SMT_REQUIRE(plan_tiles >= 1 && plan_tiles < (1ull << 27) && nq >= 1 && nq <= 3584 && kp >= 1 && kp <= 64 && family >= 0 && family <= 2 &&
                    blocks >= 1 && blocks <= 65536,
                "debug plan: 1 .. 2^27 - 1 tiles, 1..3584 queries, k' in [1, 64], family 0..2, 1..65536 blocks");
    const std::vector<GemmPlanLaunch> plan = gemm_level_plan(GemmPlanInput{plan_tiles, nq, kp, family, f16x1 != 0, (int)blocks, gemm_bootstrap,
                                                                            gemm_boot_fine, gemm_split_last, gemm_qsplit});
    *out_n = (uint32_t)plan.size();
    SMT_REQUIRE(plan.size() <= out_cap, "debug plan: more launches than the output holds (out_n says how many)");
    for (size_t i = 0; i < plan.size(); ++i) {
        const GemmPlanLaunch &e = plan[i];
        uint64_t *w = out + i * SMT_GEMM_PLAN_WORDS;
        w[0] = e.bootstrap ? 0 : 1;
        w[1] = e.stride;
        w[2] = (uint64_t)e.skip;
        w[3] = e.tile_begin;
        w[4] = e.tile_end;
        w[5] = e.qsplit;
        w[6] = (uint64_t)e.nb;
        w[7] = e.slots;
        w[8] = e.select ? 1 : 0;
        w[9] = (e.thresholds ? 1u : 0u) | (e.buffer_fits ? 2u : 0u);
    }
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

int smt_debug_gemm_trace(smt_ctx *ctx, uint32_t *buf_dev, uint64_t cap_words, uint32_t *out_selects, uint64_t *out_words)
try {
    int rc = check_ctx(ctx);
    if (rc) return rc;
    SMT_REQUIRE(buf_dev == nullptr || cap_words >= 1, "debug trace: a buffer needs a capacity");
    if (out_selects) *out_selects = ctx->gemm_trace_selects;
    if (out_words) *out_words = ctx->gemm_trace_used;
    const bool truncated = ctx->d_gemm_trace != nullptr && ctx->gemm_trace_used > ctx->gemm_trace_cap;
    ctx->d_gemm_trace = buf_dev;
    ctx->gemm_trace_cap = buf_dev ? cap_words : 0;
    ctx->gemm_trace_used = 0;
    ctx->gemm_trace_selects = 0;
    if (truncated) { set_error("debug trace: the buffer was too small for what the calls recorded"); return SMT_E_INVALID; }
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

int smt_merge_topk(const uint64_t *rows, const double *dist, uint32_t n_lists, uint32_t nq, uint32_t k_in, uint32_t k_out,
                   uint64_t *out_rows, double *out_dist, uint64_t *out_counts)
try {
    SMT_REQUIRE((rows && dist) || n_lists == 0 || nq == 0 || k_in == 0, "null input");
    SMT_REQUIRE(nq == 0 || k_out == 0 || (out_rows && out_dist), "null output");
    std::vector<std::pair<double, uint64_t>> cand;
    for (uint32_t q = 0; q < nq; ++q) {
        cand.clear();
        for (uint32_t l = 0; l < n_lists; ++l)
            for (uint32_t i = 0; i < k_in; ++i) {
                const size_t idx = ((size_t)l * nq + q) * k_in + i;
                if (rows[idx] != UINT64_MAX) cand.emplace_back(dist[idx], rows[idx]);
            }
        std::sort(cand.begin(), cand.end());
        const uint64_t n = std::min<uint64_t>(cand.size(), k_out);
        for (uint32_t i = 0; i < k_out; ++i) {
            out_rows[(size_t)q * k_out + i] = i < n ? cand[i].second : UINT64_MAX;
            out_dist[(size_t)q * k_out + i] = i < n ? cand[i].first : std::numeric_limits<double>::infinity();
        }
        if (out_counts) out_counts[q] = n;
    }
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

int smt_merge_topk_device(smt_ctx *ctx, const uint64_t *rows_dev, const double *dist_dev, uint32_t n_lists, uint32_t nq,
                          uint32_t k_in, uint32_t k_out, uint64_t *out_rows_dev, double *out_dist_dev)
try {
    int rc = check_ctx(ctx);
    if (rc) return rc;
    SMT_REQUIRE(nq == 0 || (out_rows_dev && out_dist_dev), "null output");
    if ((rc = bind_device(ctx))) return rc;
    if (nq == 0 || k_out == 0) return SMT_OK;
    return launch_merge_topk(ctx, rows_dev, dist_dev, n_lists, nq, k_in, k_out, out_rows_dev, out_dist_dev);
} catch (...) { return smt::api_catch(); }

int smt_merge_topk_packed_device(smt_ctx *ctx, const uint64_t *packed_dev, uint32_t n_lists, uint32_t nq, uint32_t k_in,
                                 uint32_t k_out, uint64_t *out_packed_dev)
try {
    int rc = check_ctx(ctx);
    if (rc) return rc;
    SMT_REQUIRE(nq == 0 || k_out == 0 || (packed_dev && out_packed_dev), "null argument");
    if ((rc = bind_device(ctx, !(ctx->tune.merge_on_aux && ctx->aux_stream)))) return rc;
    if (nq == 0 || k_out == 0) return SMT_OK;
    return launch_merge_topk_packed(ctx, packed_dev, n_lists, nq, k_in, k_out, out_packed_dev);
} catch (...) { return smt::api_catch(); }

// Test hooks: the launchers of merge.hip as the exchange calls them (group_exchange.cpp), on constructed lists.  Nothing is checked
// here that the launchers check themselves: their refusals are what the tests look at.
int smt_debug_merge_sources(smt_ctx *ctx, const uint64_t *const *lists_dev, uint32_t n_lists, uint32_t nq, uint32_t k_in, uint32_t k_out,
                            uint64_t *out_packed_dev)
try {
    int rc = check_ctx(ctx);
    if (rc) return rc;
    SMT_REQUIRE(n_lists == 0 || lists_dev != nullptr, "null argument");
    SMT_REQUIRE(nq == 0 || k_out == 0 || out_packed_dev != nullptr, "null output");
    if ((rc = bind_device(ctx))) return rc;
    if (nq == 0 || k_out == 0) return SMT_OK;
    MergeSources src{};
    for (uint32_t l = 0; l < n_lists && l < SMT_MAX_MERGE_SOURCES; ++l) src.list[l] = lists_dev[l];   // (more than 64: refused below)
    return launch_merge_topk_sources_on(ctx->stream, src, n_lists, nq, k_in, k_out, out_packed_dev);
} catch (...) { return smt::api_catch(); }

int smt_debug_merge_packed_strided(smt_ctx *ctx, const uint64_t *packed_dev, uint64_t list_stride_words, uint32_t n_lists, uint32_t nq,
                                   uint32_t k_in, uint32_t k_out, uint64_t *out_packed_dev)
try {
    int rc = check_ctx(ctx);
    if (rc) return rc;
    SMT_REQUIRE(nq == 0 || k_out == 0 || (packed_dev && out_packed_dev), "null argument");
    SMT_REQUIRE(list_stride_words == 0 || list_stride_words >= (uint64_t)nq * 2 * k_in, "the list stride is shorter than a list");
    if ((rc = bind_device(ctx))) return rc;
    if (nq == 0 || k_out == 0) return SMT_OK;
    return launch_merge_topk_packed_on(ctx, ctx->stream, packed_dev, n_lists, nq, k_in, k_out, out_packed_dev, list_stride_words);
} catch (...) { return smt::api_catch(); }

int smt_debug_combine_status(smt_ctx *ctx, const uint64_t *const *words_dev, const uint64_t *base_dev, uint64_t stride_words, uint32_t n,
                             uint32_t nq, uint32_t *out_status_dev)
try {
    int rc = check_ctx(ctx);
    if (rc) return rc;
    SMT_REQUIRE(nq == 0 || out_status_dev != nullptr, "null output");
    SMT_REQUIRE(base_dev == nullptr || stride_words >= nq, "the stride is shorter than a block of status words");
    if ((rc = bind_device(ctx))) return rc;
    MergeSources src{};
    for (uint32_t j = 0; words_dev && j < n && j < SMT_MAX_MERGE_SOURCES; ++j) src.list[j] = words_dev[j];   // (more than 64: refused below)
    return launch_combine_status_on(ctx->stream, words_dev ? &src : nullptr, base_dev, stride_words, n, nq, out_status_dev);
} catch (...) { return smt::api_catch(); }

// Test hook: launch_select (select.hip) on constructed block lists, on the context's stream, with the f32 rows of `corpus` behind the
// keys.  No async step, no delivery.  The launcher's own refusals (list count, k', k_out) are what the tests look at.
int smt_debug_select_lists(smt_corpus *corpus, const float *queries_dev, uint32_t nq, const uint64_t *lists_dev, uint64_t list_stride,
                           uint32_t n_lists, uint32_t kp, uint32_t k_out, int ws_threshold, float ws_thr_score, uint64_t row_base,
                           double f32_err, const uint32_t *overflow_dev, uint64_t out_stride, uint64_t *out_rows_dev, double *out_dist_dev,
                           uint64_t *out_counts_dev, uint64_t *out_uncertain_dev, uint32_t *out_status_dev)
try {
    SMT_REQUIRE(corpus != nullptr, "corpus");
    SMT_REQUIRE(nq == 0 || (queries_dev && lists_dev && out_rows_dev && out_dist_dev), "null argument");
    SMT_REQUIRE(list_stride == 0 || list_stride >= (uint64_t)n_lists * kp, "the list stride is shorter than a query's lists");
    SMT_REQUIRE(out_stride == 0 || out_stride >= k_out, "the output stride is shorter than an output list");
    smt_ctx *ctx = corpus->ctx;
    int rc = bind_device(ctx);
    if (rc) return rc;
    if (nq == 0) return SMT_OK;
    SelectArgs s;
    s.corpus = corpus->d_rows;
    s.queries = queries_dev;
    s.nq = nq;
    s.lists = const_cast<key_t64 *>(reinterpret_cast<const key_t64 *>(lists_dev));
    s.n_lists = n_lists;
    s.kp = kp;
    s.list_stride = list_stride ? list_stride : (uint64_t)n_lists * kp;
    s.k_out = k_out;
    s.ws_threshold = ws_threshold;
    s.ws_thr_score = ws_thr_score;
    s.row_base = row_base;
    s.out_rows = out_rows_dev;
    s.out_dist = out_dist_dev;
    s.out_counts = out_counts_dev;
    s.out_stride = out_stride;
    s.f32_err = f32_err;
    s.out_uncertain = out_uncertain_dev;
    s.out_status = out_status_dev;
    s.overflow = overflow_dev;
    return launch_select(ctx, s);
} catch (...) { return smt::api_catch(); }

// Test hook: the block lists of the scan stage.  The ScanArgs of a real synchronous top_k call of nq host queries over the corpus --
// ranges through the range plan, as smt_debug_nominations -- handed to debug_scan_lists (scan_launch.hip), which runs the code
// launch_scan_topk runs up to the select.
int smt_debug_scan_lists(smt_corpus *corpus, const float *queries, uint32_t nq, uint32_t top_k, const smt_range *ranges, uint32_t n_ranges,
                         uint64_t *out_keys, uint64_t out_cap_keys, uint32_t *out_blocks, uint32_t *out_kp, uint32_t *out_route)
try {
    SMT_REQUIRE(corpus && queries && out_keys && out_blocks && out_kp && out_route, "null argument");
    SMT_REQUIRE(n_ranges == 0 || ranges != nullptr, "ranges");
    SMT_REQUIRE(nq >= 1 && nq <= 8, "debug scan lists: 1..8 queries");
    SMT_REQUIRE(top_k >= 1 && top_k <= SCAN_MAX_K, "debug scan lists: top_k in [1, 56]");
    smt_ctx *ctx = corpus->ctx;
    int rc = bind_device(ctx, true);
    if (rc) return rc;
    *out_blocks = 0; *out_kp = 0; *out_route = 0;
    RangePlan plan;
    plan.n_virtual = corpus->rows;
    if (n_ranges && (rc = range_plan_find(corpus, ranges, n_ranges, plan))) return rc;
    SMT_REQUIRE(plan.n_virtual >= 1, "debug scan lists: no row to scan");
    if ((rc = range_plan_finish(corpus, plan))) return rc;
    const size_t q_bytes = (size_t)nq * SMT_DIM * sizeof(float);
    if ((rc = ensure_stage(ctx, q_bytes + plan.table_bytes() + 64))) return rc;
    char *stage = reinterpret_cast<char *>(ctx->d_stage);
    SMT_HIP_CHECK(hipMemcpyAsync(stage, queries, q_bytes, hipMemcpyHostToDevice, ctx->stream));
    plan.bind(stage + q_bytes);
    if (plan.upload_bytes()) {
        SMT_HIP_CHECK(hipMemcpyAsync(const_cast<smt_range *>(plan.d_r), plan.rr.data(), plan.r_bytes(), hipMemcpyHostToDevice, ctx->stream));
        SMT_HIP_CHECK(hipMemcpyAsync(const_cast<uint64_t *>(plan.d_p), plan.prefixes.data(), plan.prefixes.size() * sizeof(uint64_t),
                                     hipMemcpyHostToDevice, ctx->stream));
    }
    ScanArgs a = scan_args(corpus, reinterpret_cast<const float *>(stage), nq, top_k, 0);
    plan.apply(a);
    return debug_scan_lists(ctx, a, reinterpret_cast<key_t64 *>(out_keys), out_cap_keys, out_blocks, out_kp, out_route);
} catch (...) { return smt::api_catch(); }

int smt_debug_scan_ring(smt_ctx *ctx, uint32_t calls_back, uint64_t n_keys, uint64_t *out_keys)
try {
    int rc = check_ctx(ctx);
    if (rc) return rc;
    SMT_REQUIRE(n_keys == 0 || out_keys != nullptr, "null output");
    if ((rc = bind_device(ctx, false))) return rc;
    return debug_scan_ring(ctx, calls_back, n_keys, reinterpret_cast<key_t64 *>(out_keys));
} catch (...) { return smt::api_catch(); }

}  // extern "C"
