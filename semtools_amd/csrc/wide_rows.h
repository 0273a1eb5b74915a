// wide_rows.h -- rows of D = 256 * S floats, S in {2, 3, 4}: what the wide units share (embed_slab.hip, scan_slab.hip,
// finish_slab.hip, search_slab.cpp).  A wide row is S SLABS of 1 KiB; D = 256 runs none of this.
#pragma once
#include "common.h"

namespace smt {

inline bool dim_is_wide(uint32_t D) { return D == 512 || D == 768 || D == 1024; }
// NARROW rows: 64 floats, 256 B, four rows per 1 KiB wave load (embed_narrow.hip, scan_narrow.hip); f32 rows only
inline bool dim_is_narrow(uint32_t D) { return D == 64; }
// a width of this family: its own K1 and K2, the finish stage and the entry points of search_slab.cpp; the 256 kernels never see it
inline bool dim_in_family(uint32_t D) { return dim_is_wide(D) || dim_is_narrow(D); }
inline bool dim_supported(uint32_t D) { return D == SMT_DIM || dim_in_family(D); }
// SMT_E_UNSUPPORTED for a width no kernel serves (the message names 256 and lists the five widths)
int refuse_dim(uint32_t D);
// SMT_E_UNSUPPORTED for a call wide rows do not serve yet: `what` names it, the message names the width
int refuse_wide(uint32_t D, const char *what);
// ... and for one narrow rows do not serve yet: the message names the 64 dimensions
int refuse_narrow(const char *what);
// whichever of the two fits a width of the family
inline int refuse_width(uint32_t D, const char *what) { return dim_is_narrow(D) ? refuse_narrow(what) : refuse_wide(D, what); }
// ... and for one half rows do not serve yet (half_rows.h): the message names the half rows
int refuse_half(const char *what);
// ... and for one byte rows do not serve yet (byte_rows.h): the message names the byte rows
int refuse_byte(const char *what);
// ... and for one nibble rows do not serve yet (nibble_rows.h): the message names the nibble rows
int refuse_nibble(const char *what);
// whichever of the five fits a corpus that is wide, narrow, half, byte or nibble
inline int refuse_rows(const smt_corpus *c, const char *what)
{
    return c->row_dtype == SMT_ROWS_I4   ? refuse_nibble(what)
           : c->row_dtype == SMT_ROWS_I8 ? refuse_byte(what)
           : c->row_dtype == SMT_ROWS_F16 ? refuse_half(what) : refuse_width(c->dim, what);
}
inline bool rows_are_narrow(const smt_corpus *c) { return dim_is_narrow(c->dim); }

// |f32 scan distance - exact distance| of scan_slab_kernel<S, .>, by the counting rule at F32_ERR_SCAN (common.h): a lane runs
// 4 S fused multiply-adds, the tree (wave_sum4 or wave_sum: six levels) is taken as eight steps as there, on terms whose absolute
// sum is <= 1, and two rsqrt and two multiplies follow: (4 S + 8 + 4) roundings of 2^-24 -- 1.19e-6, 1.43e-6, 1.67e-6 at
// S = 2, 3, 4 (the rule gives 9.5e-7 at S = 1, the "< 1e-6" written there).  The constant keeps the factor 4 that 4e-6 has over
// that figure: 4.8e-6, 5.8e-6, 6.7e-6.  (A count that also carries the error of |c|^2 and |q|^2 through their rsqrt comes to
// (8 S + 22) x 2^-24 = 3.2e-6 at S = 4: inside the margin.)  Not measured on keys yet, unlike the 256 kernels' bound.
constexpr double f32_err_slab(int S) { return 4.0 * (double)(4 * S + 12) / 16777216.0; }

// ... of batch_slab_kernel<S, .> (batch_slab.hip), by the rule for bf16 x 3 at F32_ERR_BF16X3 (common.h): representation
// 3 x 2^-16 |x||q| (4.6e-5), 48 S MFMA instructions at 2 ulp = 2^-23 each (2.3e-5, 3.4e-5, 4.6e-5), the two f32 scalings (1e-6),
// the whole times the 1.2 that took 5.8e-5 to 7e-5 there: 8.4e-5, 9.7e-5, 1.11e-4 at S = 2, 3, 4.
// MEASURED on every key tests/test_gpu_wide_batch.py reads through smt_debug_batch_slab_lists (profiles/wide_batch.json): at most
// 7.7e-7 on random rows, 2.6e-5 on the constructed worst-case rows (1024 dimensions).
constexpr double f32_err_batch_slab(int S) { return 1.2 * (3.0 / 65536.0 + 48.0 * S * 2.0 / 8388608.0 + 1e-6); }

// ... of scan_narrow_kernel (scan_narrow.hip), by the same rule: a lane runs four fused multiply-adds, the tree inside a 16-lane row
// (four levels) is taken as eight steps as there, two rsqrt and two multiplies follow: (4 + 8 + 4) roundings of 2^-24 = 9.5e-7 --
// the 256 kernel's own count, a row of 64 floats in 16 lanes is a row of 256 in 64 -- times the factor 4: 3.8e-6.
// DERIVED, not measured on keys.
constexpr double f32_err_narrow = 4.0 * 16.0 / 16777216.0;
constexpr int NARROW_STEP_ROWS = 16;   // rows a wave of scan_narrow_kernel takes per step: four 1 KiB loads of four rows each

constexpr int SLAB_MAX_LISTS = 256;  // block lists per query the finish kernel merges: the scan launches at most this many blocks

// K1 (embed_slab.hip): plain tables of `table_dtype`, rows of D elements
int launch_embed_slab(smt_ctx *ctx, const void *table, int table_dtype, uint64_t V, uint32_t D, int normalize, const uint32_t *ids,
                      const uint64_t *offsets, uint64_t n_lines, uint32_t max_tokens, float *out);

// the run table of the K1 kernels of this family (embed_slab.hip): ctx->d_embed_runs[g] = the first line of group g when the lines
// are cut by tokens + 4 per line into `groups` runs, [groups] = n_lines; grows the table, enqueues one launch
int launch_embed_runs(smt_ctx *ctx, const uint64_t *offsets, uint64_t n_lines, uint64_t groups);
// K1 for 64-wide tables (embed_narrow.hip): plain tables of `table_dtype`, rows of 64 elements
int launch_embed_narrow(smt_ctx *ctx, const void *table, int table_dtype, uint64_t V, int normalize, const uint32_t *ids,
                        const uint64_t *offsets, uint64_t n_lines, uint32_t max_tokens, float *out);

// K2 + finish for the queries of one call, in passes of up to four (scan_slab.hip, finish_slab.hip).  All pointers device; enqueued
// on the context's stream, nothing waits.  chunk_table / n_chunks: the range filter (range_tables.hip), nullptr / 0 without one.
struct SlabSearch {
    const float *corpus = nullptr;     // (binary16 values behind it when row_dtype is SMT_ROWS_F16, signed bytes when SMT_ROWS_I8, packed nibbles when SMT_ROWS_I4)
    int row_dtype = SMT_ROWS_F32;
    uint64_t rows = 0;                 // < 2^32 - 1
    uint32_t dim = 0;
    const float *queries = nullptr;    // [nq x dim]
    uint32_t nq = 0;
    uint32_t k_out = 0;                // 1 .. SCAN_MAX_K; slots beyond the rows there are hold (UINT64_MAX, +inf)
    const uint64_t *chunk_table = nullptr;
    uint64_t n_chunks = 0;
    uint64_t row_base = 0;
    uint64_t *out_rows = nullptr;      // [nq][k_out]
    double *out_dist = nullptr;        // [nq][k_out]
    uint64_t *out_counts = nullptr;    // [nq] or nullptr
    uint32_t *out_status = nullptr;    // [nq] or nullptr: SMT_STATUS_*
    bool scan_only = false;            // never the batched route (the host form's re-run of what that route left unproved)
};
int launch_search_slab(smt_ctx *ctx, const SlabSearch &a);
// what a K2 kernel of this family is launched with (scan_slab.hip, scan_narrow.hip, scan_half.hip, scan_byte.hip, scan_nibble.hip)
struct SlabScanParams {
    const float *corpus;
    uint64_t n_rows;
    const float *queries;          // the pass' first query
    uint32_t nq_active;            // 1 .. NQ
    uint32_t kp;
    const uint64_t *chunk_table;   // FILTERED
    uint64_t n_chunks;
    key_t64 *block_lists;          // [NQ][gridDim.x][kp]
};
using slab_scan_kernel_t = void (*)(SlabScanParams);
// scan_narrow.hip: scan_narrow_kernel<4, slots, filtered>, launched by launch_search_slab (scan_slab.hip) like the wide kernels
slab_scan_kernel_t narrow_scan_kernel_of(int slots, bool filtered);
// the finish stage alone (finish_slab.hip): lists [nq][n_lists][kp] of block lists -> answers, one block per query, certified under
// f32_err (0: the scan's f32_err_slab)
int launch_finish_slab(smt_ctx *ctx, const SlabSearch &a, const key_t64 *lists, uint32_t n_lists, uint32_t kp, uint32_t first_query,
                       uint32_t nq_pass, double f32_err = 0.0);
// The batched route (batch_slab.hip): calls of at least tuning key slab_batch_min queries (0: never) run passes of slab_batch_qb
// queries -- 64 at 512 dimensions, 32 at 768 and 1024 -- on the bf16 MFMA pipe, certified under f32_err_batch_slab.
inline bool slab_batch_serves(const smt_ctx *ctx, const SlabSearch &a)
{
    return !a.scan_only && a.row_dtype == SMT_ROWS_F32 && dim_is_wide(a.dim) && ctx->tune.slab_batch_min > 0 &&   // (narrow rows: the scan only)
           a.nq >= (uint32_t)ctx->tune.slab_batch_min;
}
uint32_t slab_batch_qb(uint32_t dim);
int launch_batch_slab(smt_ctx *ctx, const SlabSearch &a);
int debug_batch_slab_lists(smt_ctx *ctx, const SlabSearch &a, key_t64 *out_keys_host, uint64_t out_cap_keys, uint32_t *out_blocks,
                           uint32_t *out_kp);
// the exhaustive re-answer's kernel (finish_slab.hip): out[i] = exact f64 distance of row i (no table), or of row j of chunk c at
// out[4 c + j] (slots past a chunk's rows are not written)
int launch_exact_all_slab(smt_ctx *ctx, const float *corpus, int row_dtype, uint64_t rows, uint32_t dim, const float *query,
                          const uint64_t *chunk_table, uint64_t n_chunks, double *out);
// domain.hip: rows of `dim` floats (the whole row: every slab), as check_rows_domain does for 256
int check_rows_domain_dim(smt_ctx *ctx, const float *d_rows, uint64_t n_rows, uint32_t dim, uint64_t *n_bad, uint64_t *first_bad);
int require_rows_domain_dim(smt_ctx *ctx, const float *d_rows, uint64_t n_rows, uint32_t dim, const char *what, uint64_t base = 0);

// search_slab.cpp: what smt_search / smt_search_topk_device[_ex] do for a wide corpus
int search_wide_host(smt_corpus *corpus, const float *queries, uint32_t nq, uint32_t top_k, double max_distance, int mode,
                     const smt_range *ranges, uint32_t n_ranges, uint64_t row_base, std::vector<LocalHits> &out);
int search_wide_device(smt_corpus *corpus, const float *queries_dev, uint32_t nq, uint32_t top_k, uint64_t row_base, uint64_t *out_rows_dev,
                       double *out_dist_dev, uint32_t *out_status_dev);

}  // namespace smt
