// search_slab.cpp -- the search entry points over a WIDE corpus (rows of 512, 768 or 1024 floats) or a NARROW one (rows of 64
// floats, scan_narrow.hip: the same calls, no batched route) or a HALF corpus (rows of 256
// binary16 values, half_rows.h: the same calls with the row type handed on) or a BYTE corpus (rows of 256 int8, byte_rows.h: the
// same again) or a NIBBLE corpus (rows of 256 int4, nibble_rows.h: the same again): what smt_search and
// smt_search_topk_device[_ex] do before they would reach a 256 kernel.  Served: top-k (1 .. 56) in documents mode without a
// distance bound, workspace mode with or without one, ranges, row_base, any number of queries in passes of four, or -- from tuning
// key slab_batch_min (half rows: half_batch_min, byte rows: byte_batch_min, nibble rows: nibble_batch_min) queries on -- in batched
// passes on the MFMA pipe (batch_slab.hip, batch_half.hip, batch_byte.hip, batch_nibble.hip) whose unproved answers the host form
// runs again through the scan (not for byte and nibble rows: their batched bound is not wider than the scan's).  Also the test
// hooks of those routes (smt_debug_batch_slab_lists, smt_debug_batch_half_lists, smt_debug_batch_byte_lists,
// smt_debug_batch_nibble_lists).  Everything is
// enqueued on the context's stream directly: no one-query pipeline, no grouping, no operand image.  Also the two refusals every
// other entry point answers a wide corpus or model with.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "nibble_rows.h"

namespace smt {

int refuse_dim(uint32_t D)
{
    set_error("embedding dim %u unsupported (kernels are specialised for 256; wide rows: 512, 768, 1024; narrow rows: 64)", D);
    return SMT_E_UNSUPPORTED;
}

int refuse_wide(uint32_t D, const char *what)
{
    set_error("%s: not served for %u-dimensional rows yet (wide rows: top-k searches up to 56, ranges, workspace mode; everything else is 256 only)",
              what, D);
    return SMT_E_UNSUPPORTED;
}

int refuse_narrow(const char *what)
{
    set_error("%s: not served for 64-dimensional rows yet (narrow rows: f32 rows, plain models, append, write, read, truncate, save, "
              "load, embed into the corpus, top-k searches up to 56, ranges, workspace mode; everything else is 256 only)", what);
    return SMT_E_UNSUPPORTED;
}

int refuse_half(const char *what)
{
    set_error("%s: not served for half rows (SMT_ROWS_F16) yet (half rows: append, write, read, truncate, embed into the corpus, top-k "
              "searches up to 56, ranges, workspace mode; everything else needs f32 rows)", what);
    return SMT_E_UNSUPPORTED;
}

int refuse_byte(const char *what)
{
    set_error("%s: not served for byte rows (SMT_ROWS_I8) yet (byte rows: append, write, read, truncate, embed into the corpus, top-k "
              "searches up to 56, ranges, workspace mode; everything else needs f32 rows)", what);
    return SMT_E_UNSUPPORTED;
}

int refuse_nibble(const char *what)
{
    set_error("%s: not served for nibble rows (SMT_ROWS_I4) yet (nibble rows: append, write, read, truncate, embed into the corpus, "
              "top-k searches up to 56, ranges, workspace mode; everything else needs f32 rows)", what);
    return SMT_E_UNSUPPORTED;
}

static bool wide_query_is_zero(const float *q, uint32_t dim)
{
    for (uint32_t d = 0; d < dim; ++d)
        if (q[d] != 0.0f) return false;
    return true;
}

// The workspace score rule (store.rs:502-503), cut on the host: the rows over the threshold are a prefix of the ordered top-k
static void cut_at_score(LocalHits &h, float thr_score)
{
    size_t n = 0;
    while (n < h.rows.size() && (1.0 - h.dist[n]) > (double)thr_score) ++n;
    h.rows.resize(n);
    h.dist.resize(n);
}

int search_wide_host(smt_corpus *corpus, const float *queries, uint32_t nq, uint32_t top_k, double max_distance, int mode,
                     const smt_range *ranges, uint32_t n_ranges, uint64_t row_base, std::vector<LocalHits> &out)
{
    SMT_REQUIRE(mode == SMT_MODE_DOCUMENTS || mode == SMT_MODE_WORKSPACE, "mode");
    SMT_REQUIRE(nq == 0 || queries, "null argument");
    const uint32_t dim = corpus->dim;
    const bool has_thr = !std::isnan(max_distance);
    if (mode == SMT_MODE_DOCUMENTS && has_thr) return refuse_rows(corpus, "smt_search with max_distance in documents mode (the threshold kernel)");
    if (top_k > SCAN_MAX_K) return refuse_rows(corpus, "smt_search with top_k > 56 (the large-k route)");
    smt_ctx *ctx = corpus->ctx;
    int rc = bind_device(ctx);
    if (rc) return rc;
    if ((rc = validate_ranges(ranges, n_ranges, corpus->rows))) return rc;
    out.assign(nq, LocalHits());
    if (nq == 0) return SMT_OK;
    {
        const int64_t bad = first_outside_domain_host(queries, nq, dim);
        if (bad >= 0) {
            set_error("search: query %lld is outside the library's domain -- every component must be finite and the largest magnitude 0 or "
                      "within [2^-40, 2^40] (include/semtools_hip.h, \"Domain\")", (long long)bad);
            return SMT_E_INVALID;
        }
    }
    // the non-empty ranges and the chunks in front of each (range_tables.hip)
    std::vector<smt_range> rr;
    std::vector<uint64_t> chunk_prefix(1, 0);
    uint64_t n_virtual = n_ranges ? 0 : corpus->rows;
    for (uint32_t i = 0; i < n_ranges; ++i) {
        const uint64_t len = ranges[i].end - ranges[i].begin;
        if (!len) continue;
        rr.push_back(ranges[i]);
        chunk_prefix.push_back(chunk_prefix.back() + (len + FILTER_CHUNK - 1) / FILTER_CHUNK);
        n_virtual += len;
    }
    if (n_virtual == 0 || top_k == 0) return SMT_OK;
    const uint64_t n_chunks = chunk_prefix.back();
    const uint32_t k_eff = (uint32_t)std::min<uint64_t>(top_k, n_virtual);
    const float thr_score = 1.0f - (float)max_distance;
    const bool ws_thr = mode == SMT_MODE_WORKSPACE && has_thr;

    // workspace mode: a zero query has a constant answer and never reaches the GPU (search.cpp search_local_host)
    std::vector<uint32_t> live;
    for (uint32_t q = 0; q < nq; ++q) {
        if (mode == SMT_MODE_WORKSPACE && wide_query_is_zero(queries + (size_t)q * dim, dim))
            workspace_zero_query_hits(ranges, n_ranges, corpus->rows, top_k, has_thr, max_distance, row_base, out[q]);
        else live.push_back(q);
    }
    if (live.empty()) return SMT_OK;
    const uint32_t nl = (uint32_t)live.size();

    // the stage: [queries | ranges | chunk prefix | chunk table | rows | distances | counts | status]
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t q_bytes = al((size_t)nl * dim * sizeof(float)), r_bytes = al(rr.size() * sizeof(smt_range));
    const size_t cp_bytes = al(chunk_prefix.size() * sizeof(uint64_t)), t_bytes = al((size_t)n_chunks * sizeof(uint64_t));
    const size_t o_rows = (size_t)nl * k_eff * sizeof(uint64_t), o_cnt = (size_t)nl * sizeof(uint64_t), o_st = al((size_t)nl * sizeof(uint32_t));
    const size_t o_bytes = 2 * o_rows + o_cnt + o_st;
    const size_t up_bytes = q_bytes + r_bytes + cp_bytes;
    if ((rc = ensure_stage(ctx, up_bytes + t_bytes + o_bytes + 256))) return rc;
    if ((rc = ensure_pinned_in(ctx, up_bytes))) return rc;
    if ((rc = ensure_pinned(ctx, o_bytes))) return rc;
    char *stage = reinterpret_cast<char *>(ctx->d_stage), *pin = reinterpret_cast<char *>(ctx->h_pinned_in);
    for (uint32_t j = 0; j < nl; ++j) memcpy(pin + (size_t)j * dim * sizeof(float), queries + (size_t)live[j] * dim, (size_t)dim * sizeof(float));
    if (!rr.empty()) {
        memcpy(pin + q_bytes, rr.data(), rr.size() * sizeof(smt_range));
        memcpy(pin + q_bytes + r_bytes, chunk_prefix.data(), chunk_prefix.size() * sizeof(uint64_t));
    }
    SMT_HIP_CHECK(hipMemcpyAsync(stage, pin, up_bytes, hipMemcpyHostToDevice, ctx->stream));
    const float *d_q = reinterpret_cast<const float *>(stage);
    uint64_t *d_table = rr.empty() ? nullptr : reinterpret_cast<uint64_t *>(stage + up_bytes);
    if (d_table &&
        (rc = launch_build_chunk_table(ctx, reinterpret_cast<const smt_range *>(stage + q_bytes),
                                       reinterpret_cast<const uint64_t *>(stage + q_bytes + r_bytes), (uint32_t)rr.size(), n_chunks, d_table)))
        return rc;
    char *d_out = stage + up_bytes + t_bytes;

    SlabSearch a;
    a.corpus = corpus->d_rows;
    a.row_dtype = corpus->row_dtype;
    a.rows = corpus->rows;
    a.dim = dim;
    a.queries = d_q;
    a.nq = nl;
    a.k_out = k_eff;
    a.chunk_table = d_table;
    a.n_chunks = n_chunks;
    a.row_base = row_base;
    a.out_rows = reinterpret_cast<uint64_t *>(d_out);
    a.out_dist = reinterpret_cast<double *>(d_out + o_rows);
    a.out_counts = reinterpret_cast<uint64_t *>(d_out + 2 * o_rows);
    a.out_status = reinterpret_cast<uint32_t *>(d_out + 2 * o_rows + o_cnt);
    if ((rc = launch_search_slab(ctx, a))) return rc;
    char *h = reinterpret_cast<char *>(ctx->h_pinned);
    SMT_HIP_CHECK(hipMemcpyAsync(h, d_out, o_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    const uint64_t *h_rows = reinterpret_cast<const uint64_t *>(h);
    const double *h_dist = reinterpret_cast<const double *>(h + o_rows);
    const uint64_t *h_cnt = reinterpret_cast<const uint64_t *>(h + 2 * o_rows);
    const uint32_t *h_st = reinterpret_cast<const uint32_t *>(h + 2 * o_rows + o_cnt);
    std::vector<uint32_t> redo;
    for (uint32_t j = 0; j < nl; ++j) {
        LocalHits &hits = out[live[j]];
        if (h_st[j] != SMT_STATUS_PROVED) { redo.push_back(j); continue; }   // (the pinned buffer is reused below: copy first)
        hits.rows.assign(h_rows + (size_t)j * k_eff, h_rows + (size_t)j * k_eff + h_cnt[j]);
        hits.dist.assign(h_dist + (size_t)j * k_eff, h_dist + (size_t)j * k_eff + h_cnt[j]);
        if (ws_thr) cut_at_score(hits, thr_score);
    }
    if (redo.empty()) return SMT_OK;

    // What the batched route left unproved is first run again, together, through the scan route and its tighter f32_err_slab: the
    // queries move to the front of the stage (ascending, so none is overwritten before it has moved), `redo` then indexes them there.
    // Byte rows are left out: f32_err_batch_byte is UNDER the scan's f32_err_byte (byte_rows.h), the scan could prove no more.
    // Nibble rows too: f32_err_batch_nibble EQUALS the scan's f32_err_nibble (nibble_rows.h).
    if (batch_route_serves(ctx, a)) {
        const uint32_t nr = (uint32_t)redo.size();
        for (uint32_t i = 0; i < nr; ++i)
            if (redo[i] != i)
                SMT_HIP_CHECK(hipMemcpyAsync(const_cast<float *>(d_q) + (size_t)i * dim, d_q + (size_t)redo[i] * dim, (size_t)dim * sizeof(float),
                                             hipMemcpyDeviceToDevice, ctx->stream));
        for (uint32_t i = 0; i < nr; ++i) live[i] = live[redo[i]];
        a.nq = nr;
        a.scan_only = true;
        if ((rc = launch_search_slab(ctx, a))) return rc;
        SMT_HIP_CHECK(hipMemcpyAsync(h, d_out, o_bytes, hipMemcpyDeviceToHost, ctx->stream));
        SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        redo.clear();
        for (uint32_t i = 0; i < nr; ++i) {
            LocalHits &hits = out[live[i]];
            if (h_st[i] != SMT_STATUS_PROVED) { redo.push_back(i); continue; }
            hits.rows.assign(h_rows + (size_t)i * k_eff, h_rows + (size_t)i * k_eff + h_cnt[i]);
            hits.dist.assign(h_dist + (size_t)i * k_eff, h_dist + (size_t)i * k_eff + h_cnt[i]);
            if (ws_thr) cut_at_score(hits, thr_score);
        }
        if (redo.empty()) return SMT_OK;
    }

    // An unproved list is never returned: the exact f64 distance of EVERY allowed row (exact_all_slab_kernel), selected here by
    // (distance, row).  Slow, rare -- near-ties past the guard band -- and correct.
    const uint64_t n_slots = d_table ? n_chunks * FILTER_CHUNK : corpus->rows;
    std::vector<uint64_t> slot_row(n_virtual), slot_at(n_virtual);   // the allowed rows in order, and where their distance lands
    if (d_table) {
        uint64_t v = 0;
        for (size_t i = 0; i < rr.size(); ++i)
            for (uint64_t r = rr[i].begin; r < rr[i].end; ++r, ++v) { slot_row[v] = r; slot_at[v] = chunk_prefix[i] * FILTER_CHUNK + (r - rr[i].begin); }
    } else {
        for (uint64_t v = 0; v < n_virtual; ++v) slot_row[v] = slot_at[v] = v;
    }
    double *d_all = nullptr;
    SMT_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&d_all), n_slots * sizeof(double)));
    std::vector<double> all(n_slots);
    std::vector<uint64_t> order(n_virtual);
    for (uint32_t j : redo) {
        rc = launch_exact_all_slab(ctx, corpus->d_rows, corpus->row_dtype, corpus->rows, dim, d_q + (size_t)j * dim, d_table, n_chunks, d_all);
        hipError_t e = rc ? hipSuccess : hipMemcpyAsync(all.data(), d_all, n_slots * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
        if (!rc && e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (rc || e != hipSuccess) {
            (void)hipFree(d_all);
            if (!rc) { set_error("exhaustive re-answer: %s", hipGetErrorString(e)); rc = SMT_E_HIP; }
            return rc;
        }
        for (uint64_t v = 0; v < n_virtual; ++v) order[v] = v;
        auto before = [&](uint64_t x, uint64_t y) {
            const double dx = all[slot_at[x]], dy = all[slot_at[y]];
            return dx != dy ? dx < dy : slot_row[x] < slot_row[y];
        };
        std::partial_sort(order.begin(), order.begin() + k_eff, order.end(), before);
        LocalHits &hits = out[live[j]];
        hits.rows.resize(k_eff);
        hits.dist.resize(k_eff);
        for (uint32_t i = 0; i < k_eff; ++i) { hits.rows[i] = row_base + slot_row[order[i]]; hits.dist[i] = all[slot_at[order[i]]]; }
        if (ws_thr) cut_at_score(hits, thr_score);
    }
    SMT_HIP_CHECK(hipFree(d_all));
    return SMT_OK;
}

int search_wide_device(smt_corpus *corpus, const float *queries_dev, uint32_t nq, uint32_t top_k, uint64_t row_base, uint64_t *out_rows_dev,
                       double *out_dist_dev, uint32_t *out_status_dev)
{
    SMT_REQUIRE(nq == 0 || (queries_dev && out_rows_dev && out_dist_dev), "null argument");
    SMT_REQUIRE(top_k >= 1, "top_k must be at least 1");
    if (top_k > SCAN_MAX_K) return refuse_rows(corpus, "smt_search_topk_device with top_k > 56 (the large-k route)");
    int rc = bind_device(corpus->ctx);
    if (rc) return rc;
    if (nq == 0) return SMT_OK;
    SlabSearch a;
    a.corpus = corpus->d_rows;
    a.row_dtype = corpus->row_dtype;
    a.rows = corpus->rows;
    a.dim = corpus->dim;
    a.queries = queries_dev;
    a.nq = nq;
    a.k_out = top_k;
    a.row_base = row_base;
    a.out_rows = out_rows_dev;
    a.out_dist = out_dist_dev;
    a.out_status = out_status_dev;
    return launch_search_slab(corpus->ctx, a);
}

}  // namespace smt

using namespace smt;

// What the four list hooks share: nq host queries and the optional ranges (through the chunk table) onto the stage, then the
// route's debug_batch_*_lists (batch_slab.hip, batch_half.hip, batch_byte.hip, batch_nibble.hip) under the grid the current tuning
// gives.  `rows`: the element type the hook is for (SMT_ROWS_F32: the wide route).
static int debug_batch_lists_staged(smt_corpus *corpus, int rows, const float *queries, uint32_t nq, uint32_t top_k, const smt_range *ranges,
                                    uint32_t n_ranges, uint64_t *out_keys, uint64_t out_cap_keys, uint32_t *out_blocks, uint32_t *out_kp)
{
    SMT_REQUIRE(corpus && queries && out_keys && out_blocks && out_kp, "null argument");
    const bool half = rows == SMT_ROWS_F16, byte = rows == SMT_ROWS_I8, nibble = rows == SMT_ROWS_I4;
    if (rows_are_narrow(corpus)) return refuse_narrow("the list hooks of the batched routes (narrow rows have no batched route)");
    if (rows_are_nibble(corpus) && !nibble)
        return refuse_nibble(byte   ? "smt_debug_batch_byte_lists (the batched route of nibble rows has smt_debug_batch_nibble_lists)"
                             : half ? "smt_debug_batch_half_lists (the batched route of nibble rows has smt_debug_batch_nibble_lists)"
                                    : "smt_debug_batch_slab_lists (the batched route of nibble rows has smt_debug_batch_nibble_lists)");
    if (rows_are_byte(corpus) && !byte)
        return refuse_byte(nibble ? "smt_debug_batch_nibble_lists (the batched route of byte rows has smt_debug_batch_byte_lists)"
                           : half ? "smt_debug_batch_half_lists (the batched route of byte rows has smt_debug_batch_byte_lists)"
                                  : "smt_debug_batch_slab_lists (the batched route of byte rows has smt_debug_batch_byte_lists)");
    if (nibble) SMT_REQUIRE(rows_are_nibble(corpus), "debug batch lists: a nibble corpus (SMT_ROWS_I4)");
    else if (byte) SMT_REQUIRE(rows_are_byte(corpus), "debug batch lists: a byte corpus (SMT_ROWS_I8)");
    else if (half) SMT_REQUIRE(rows_are_half(corpus), "debug batch lists: a half corpus (SMT_ROWS_F16)");
    else SMT_REQUIRE(dim_is_wide(corpus->dim), "debug batch lists: a wide corpus (512, 768 or 1024 dimensions)");
    SMT_REQUIRE(top_k >= 1 && top_k <= SCAN_MAX_K, "debug batch lists: top_k in [1, 56]");
    SMT_REQUIRE(nq >= 1 && nq <= 256, "debug batch lists: 1 .. 256 queries");
    smt_ctx *ctx = corpus->ctx;
    int rc = bind_device(ctx);
    if (rc) return rc;
    *out_blocks = 0; *out_kp = 0;
    if ((rc = validate_ranges(ranges, n_ranges, corpus->rows))) return rc;
    const uint32_t dim = corpus->dim;
    std::vector<smt_range> rr;
    std::vector<uint64_t> chunk_prefix(1, 0);
    for (uint32_t i = 0; i < n_ranges; ++i) {
        const uint64_t len = ranges[i].end - ranges[i].begin;
        if (!len) continue;
        rr.push_back(ranges[i]);
        chunk_prefix.push_back(chunk_prefix.back() + (len + FILTER_CHUNK - 1) / FILTER_CHUNK);
    }
    SMT_REQUIRE(n_ranges ? !rr.empty() : corpus->rows > 0, "debug batch lists: no row to scan");
    const uint64_t n_chunks = chunk_prefix.back();
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t q_bytes = al((size_t)nq * dim * sizeof(float)), r_bytes = al(rr.size() * sizeof(smt_range));
    const size_t cp_bytes = al(chunk_prefix.size() * sizeof(uint64_t)), t_bytes = al((size_t)n_chunks * sizeof(uint64_t));
    if ((rc = ensure_stage(ctx, q_bytes + r_bytes + cp_bytes + t_bytes))) return rc;
    char *stage = reinterpret_cast<char *>(ctx->d_stage);
    SMT_HIP_CHECK(hipMemcpyAsync(stage, queries, (size_t)nq * dim * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    uint64_t *d_table = nullptr;
    if (!rr.empty()) {
        SMT_HIP_CHECK(hipMemcpyAsync(stage + q_bytes, rr.data(), rr.size() * sizeof(smt_range), hipMemcpyHostToDevice, ctx->stream));
        SMT_HIP_CHECK(hipMemcpyAsync(stage + q_bytes + r_bytes, chunk_prefix.data(), chunk_prefix.size() * sizeof(uint64_t), hipMemcpyHostToDevice,
                                     ctx->stream));
        d_table = reinterpret_cast<uint64_t *>(stage + q_bytes + r_bytes + cp_bytes);
        if ((rc = launch_build_chunk_table(ctx, reinterpret_cast<const smt_range *>(stage + q_bytes),
                                           reinterpret_cast<const uint64_t *>(stage + q_bytes + r_bytes), (uint32_t)rr.size(), n_chunks, d_table)))
            return rc;
    }
    SlabSearch a;
    a.corpus = corpus->d_rows;
    a.rows = corpus->rows;
    a.dim = dim;
    a.queries = reinterpret_cast<const float *>(stage);
    a.nq = nq;
    a.k_out = top_k;
    a.chunk_table = d_table;
    a.n_chunks = n_chunks;
    a.row_dtype = corpus->row_dtype;
    rc = (nibble ? debug_batch_nibble_lists : byte ? debug_batch_byte_lists : half ? debug_batch_half_lists : debug_batch_slab_lists)(ctx, a, reinterpret_cast<key_t64 *>(out_keys), out_cap_keys, out_blocks, out_kp);
    if (rc) (void)hipStreamSynchronize(ctx->stream);   // (the uploads read this frame's vectors)
    return rc;
}

extern "C" {

// Test hook: the block lists of the batched wide route (batch_slab_kernel, one launch per pass of the nq host queries)
int smt_debug_batch_slab_lists(smt_corpus *corpus, const float *queries, uint32_t nq, uint32_t top_k, const smt_range *ranges, uint32_t n_ranges,
                               uint64_t *out_keys, uint64_t out_cap_keys, uint32_t *out_blocks, uint32_t *out_kp)
try {
    return debug_batch_lists_staged(corpus, SMT_ROWS_F32, queries, nq, top_k, ranges, n_ranges, out_keys, out_cap_keys, out_blocks, out_kp);
} catch (...) { return smt::api_catch(); }

// ... and of the batched half route (batch_half_kernel)
int smt_debug_batch_half_lists(smt_corpus *corpus, const float *queries, uint32_t nq, uint32_t top_k, const smt_range *ranges, uint32_t n_ranges,
                               uint64_t *out_keys, uint64_t out_cap_keys, uint32_t *out_blocks, uint32_t *out_kp)
try {
    return debug_batch_lists_staged(corpus, SMT_ROWS_F16, queries, nq, top_k, ranges, n_ranges, out_keys, out_cap_keys, out_blocks, out_kp);
} catch (...) { return smt::api_catch(); }

// ... and of the batched byte route (batch_byte_kernel)
int smt_debug_batch_byte_lists(smt_corpus *corpus, const float *queries, uint32_t nq, uint32_t top_k, const smt_range *ranges, uint32_t n_ranges,
                               uint64_t *out_keys, uint64_t out_cap_keys, uint32_t *out_blocks, uint32_t *out_kp)
try {
    return debug_batch_lists_staged(corpus, SMT_ROWS_I8, queries, nq, top_k, ranges, n_ranges, out_keys, out_cap_keys, out_blocks, out_kp);
} catch (...) { return smt::api_catch(); }

// ... and of the batched nibble route (batch_nibble_kernel)
int smt_debug_batch_nibble_lists(smt_corpus *corpus, const float *queries, uint32_t nq, uint32_t top_k, const smt_range *ranges, uint32_t n_ranges,
                                 uint64_t *out_keys, uint64_t out_cap_keys, uint32_t *out_blocks, uint32_t *out_kp)
try {
    return debug_batch_lists_staged(corpus, SMT_ROWS_I4, queries, nq, top_k, ranges, n_ranges, out_keys, out_cap_keys, out_blocks, out_kp);
} catch (...) { return smt::api_catch(); }

}  // extern "C"
