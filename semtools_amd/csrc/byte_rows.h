// byte_rows.h -- corpora whose rows are stored as 256 signed bytes (SMT_ROWS_I8, 256 B a row): what rows_byte.hip, scan_byte.hip
// and the element-typed parts of finish_slab.hip, scan_slab.hip's launch and search_slab.cpp share.  Cosine distance does not depend
// on a row's length, so a row is an int8 DIRECTION and carries no scale.  The answers are defined over the STORED values: an int8
// widens to f32 exactly, and the exact distance is the f64 distance of the widened row.
//
// THE ROUNDING of a row that enters as f32, bit for bit this NumPy expression with every array float32:
//     amax = np.abs(X).max(1, keepdims=True);  s = np.where(amax > 0, np.float32(127) / amax, np.float32(0))
//     q = np.rint(X * s).astype(np.int8)
// one correctly rounded division per row, one f32 multiply per component that is contracted into nothing, round to nearest with
// ties to even.  NO CLIPPING is needed: fl(127 / amax) <= (127 / amax)(1 + 2^-24), so |x| s <= amax s <= 127 (1 + 2^-24), whose
// rounded product is <= 127 (1 + 2^-24)^2 < 127.5, and rint gives at most 127; -128 is never produced.  Inside the f32 domain
// (amax in [2^-40, 2^40]) s lies in [127 x 2^-40, 127 x 2^40]: always a normal f32.  A product in the subnormal range is below
// 2^-126 and rounds to 0 whether or not the device flushes it.  A zero row (amax = 0, s = 0) is stored as zeros.
#pragma once
#include "half_rows.h"

namespace smt {

inline bool rows_are_byte(const smt_corpus *c) { return c->row_dtype == SMT_ROWS_I8; }
// a corpus that is not f32 rows (half or byte): the 256 kernels never see it
inline bool rows_are_typed(const smt_corpus *c) { return c->row_dtype != SMT_ROWS_F32; }

constexpr int BYTE_STEP_ROWS = 16;   // rows a wave of scan_byte_kernel takes per step: four 1 KiB loads of four rows each
constexpr int BYTE_PASS_QUERIES = 4; // queries of a pass (scan_byte.hip: four slots in registers)

// |f32 scan distance - exact distance| of scan_byte_kernel, by the counting rule at F32_ERR_SCAN (common.h), as f32_err_slab and
// f32_err_half apply it.  The arithmetic shipped is the SIGNED form: a lane widens its sixteen bytes to f32 (exact) and runs one
// product and fifteen fused multiply-adds -- sixteen roundings -- on terms whose absolute sum is <= |c||q|; the tree inside a
// 16-lane row has four levels and is taken as eight steps as there; two rsqrt and two multiplies follow.  |c|^2 is an INTEGER sum
// (v_dot4_i32_i8, then integer adds: at most 256 x 128^2 = 2^22 < 2^24) that converts to f32 exactly and carries no rounding at
// all, so the count is generous by what the rule allots to it.  (16 + 8 + 4) roundings of 2^-24 = 1.67e-6, times the factor 4
// that 4e-6 has over the 256 kernel's figure: 6.7e-6 -- the figure of f32_err_slab(4), whose lane also runs sixteen.
// DERIVED, not measured on keys; profiles/byte_rows.json records what the tests saw on a GPU.
constexpr double f32_err_byte = 4.0 * 28.0 / 16777216.0;

// rows_byte.hip.  src_dev: n_rows x 256 f32 on the device; dst_dev receives the bytes.  Checks every row on the way: inside the f32
// domain (domain.hip), nothing more.  Synchronises; a bad row is SMT_E_INVALID, `what` names the entry point, the message the first
// bad row (+ base).  dst_dev is written either way: hand it memory that is not part of a corpus yet.
int rows_to_byte(smt_ctx *ctx, const float *src_dev, uint64_t n_rows, void *dst_dev, const char *what, uint64_t base = 0);
// n_rows byte rows widened into dst_dev (f32); enqueued on the context's stream
int launch_byte_to_f32(smt_ctx *ctx, const void *src_dev, uint64_t n_rows, float *dst_dev);

// |nominated distance - exact distance| of batch_byte_kernel (batch_byte.hip), by the rules f32_err_batch_half (half_rows.h) uses.
// The ROWS contribute nothing, a stored row is the operand, and the INSTRUCTIONS contribute nothing either: the three digit planes
// accumulate in i32, |A_d| <= 2^22, exact (where the half route counts 32 x 2^-22).  Representation, the query's alone: n_i =
// rint(2^22 u_i) is off by at most 1/2, that is |e_i| <= 2^-23 on u_i, and over a row |<e, c>| / |c| <= |e|_2 <= 16 x 2^-23 = 2^-19.
// The f32 scalings, in units of 2^-24 of the cosine, as built: |q|^2 -- four fused multiply-adds and the six levels of wave_sum,
// ten roundings, halved by the root -- 5; its rsqrt 1; u_i = q_i x that 1; x 2^22 exact; |c|^2 an exact integer, its rsqrt 1,
// x 2^-22 exact; the combination 256 A1 + A2 rounds at magnitude <= 2^19 |c| (|d1|_2, |d2|_2 <= 2^11), 1/8, and 65536 A0 + that 1;
// score x rxj 1; 1 - that 1: 11.2 x 2^-24 = 6.7e-7, inside the 1e-6 the half route allots to its two scalings.  The whole times the
// project's 1.2: 1.2 x (2^-19 + 1e-6) = 3.49e-6 -- UNDER the scan's f32_err_byte, so what this route leaves unproved the scan
// cannot prove either: search_wide_host does not run byte rows again through the scan, they fall to the exhaustive re-answer.
// DERIVED, not measured; profiles/byte_batch.json records the largest |d32 - d64| tests/test_gpu_byte_batch.py saw.
constexpr double f32_err_batch_byte = 1.2 * (1.0 / 524288.0 + 1e-6);

// The batched route (batch_byte.hip): calls of at least tuning key byte_batch_min queries (0: never) run passes of byte_batch_qb
// queries on the int8 MFMA pipe, certified under f32_err_batch_byte.
inline bool byte_batch_serves(const smt_ctx *ctx, const SlabSearch &a)
{
    return !a.scan_only && a.row_dtype == SMT_ROWS_I8 && ctx->tune.byte_batch_min > 0 && a.nq >= (uint32_t)ctx->tune.byte_batch_min;
}
uint32_t byte_batch_qb();
int launch_batch_byte(smt_ctx *ctx, const SlabSearch &a);
int debug_batch_byte_lists(smt_ctx *ctx, const SlabSearch &a, key_t64 *out_keys_host, uint64_t out_cap_keys, uint32_t *out_blocks,
                           uint32_t *out_kp);

// scan_byte.hip: scan_byte_kernel<slots, filtered>, launched by launch_search_slab (scan_slab.hip) like the wide and half kernels
slab_scan_kernel_t byte_scan_kernel_of(int slots, bool filtered);

}  // namespace smt
