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

// scan_byte.hip: scan_byte_kernel<slots, filtered>, launched by launch_search_slab (scan_slab.hip) like the wide and half kernels
slab_scan_kernel_t byte_scan_kernel_of(int slots, bool filtered);

}  // namespace smt
