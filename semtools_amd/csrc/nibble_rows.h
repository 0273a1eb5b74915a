// nibble_rows.h -- corpora whose rows are stored as 256 signed 4-bit integers (SMT_ROWS_I4, 128 B a row): what rows_nibble.hip,
// scan_nibble.hip and the element-typed parts of finish_slab.hip, scan_slab.hip's launch and search_slab.cpp share.  As for byte
// rows (byte_rows.h) a row is a DIRECTION without a scale, and the answers are defined over the STORED values: a nibble widens to
// f32 exactly, and the exact distance is the f64 distance of the widened row.
//
// THE LAYOUT.  Byte j of a row holds element 2 j in bits 0 .. 3 and element 2 j + 1 in bits 4 .. 7, two's complement, [-8, 7].  A
// little-endian dword therefore holds the eight consecutive elements 8 w .. 8 w + 7 in nibbles 0 .. 7: the order in which
// v_dot8_i32_i4 pairs the nibbles of its two operands.
//
// THE ROUNDING of a row that enters as f32, bit for bit this NumPy expression with every array float32:
//     amax = np.abs(X).max(1, keepdims=True);  s = np.where(amax > 0, np.float32(7) / amax, np.float32(0))
//     q = np.rint(X * s).astype(np.int8)
//     packed = ((q[:, 0::2] & 15) | ((q[:, 1::2] & 15) << 4)).astype(np.uint8)
// one correctly rounded division per row, one f32 multiply per component that is contracted into nothing, round to nearest with
// ties to even.  NO CLIPPING is needed, by the argument of byte_rows.h: fl(7 / amax) <= (7 / amax)(1 + 2^-24), so |x| s <= amax s
// <= 7 (1 + 2^-24), whose rounded product is <= 7 (1 + 2^-24)^2 < 7.5, and rint gives at most 7; -8 is never produced from f32.
// Inside the f32 domain (amax in [2^-40, 2^40]) s lies in [7 x 2^-40, 7 x 2^40]: always a normal f32.  A product in the subnormal
// range is below 2^-126 and rounds to 0 whether or not the device flushes it.  A zero row (amax = 0, s = 0) is stored as zeros.
// An ADOPTED corpus may hold any byte, -8 nibbles included; they are served like any other value.
#pragma once
#include "byte_rows.h"

namespace smt {

inline bool rows_are_nibble(const smt_corpus *c) { return c->row_dtype == SMT_ROWS_I4; }

// the element type finish_slab.hip's templates take for these rows: a tag, never loaded through (two elements share a byte)
struct nibble_t {
    uint8_t pair;
};

constexpr int NIBBLE_ROW_BYTES = 128;
constexpr int NIBBLE_STEP_ROWS = 32;   // rows a wave of scan_nibble_kernel takes per step: four 1 KiB loads of eight rows each
constexpr int NIBBLE_PASS_QUERIES = 4; // queries of a pass (scan_nibble.hip: four slots in registers)

// |f32 scan distance - exact distance| of scan_nibble_kernel, by the rules f32_err_batch_byte (byte_rows.h) uses: the kernel is
// that route's arithmetic on the scan's loads.  The ROWS contribute nothing, a stored row is the operand, and the INSTRUCTIONS
// contribute nothing: <c, n> and |c|^2 are exact i32 (scan_nibble.hip states the bounds).  Representation, the query's alone:
// n_i = rint(2^22 u_i) is off by at most 1/2, that is |e_i| <= 2^-23 on u_i, and over a row |<e, c>| / |c| <= |e|_2 <= 16 x 2^-23
// = 2^-19.  The f32 operations, in units of 2^-24 of the cosine, as built: |q|^2 -- a lane's product and three fused
// multiply-adds over its four components and the six levels of wave_sum, ten roundings, halved by the root -- 5; its rsqrt 1;
// u_i = q_i x that 1; x 2^22 exact; the ONE conversion of <c, n> (an integer of magnitude < 2^30) to f32 1; |c|^2 <= 2^14
// converts exactly, its rsqrt 1; x 2^-22 exact; x rsqrt(|c|^2) 1; 1 - that 1: 11 x 2^-24 = 6.6e-7, inside the 1e-6 the batched
// routes allot to their scalings.  The whole times the project's 1.2: 1.2 x (2^-19 + 1e-6) = 3.49e-6 -- the figure of
// f32_err_batch_byte, and about half of the byte scan's f32_err_byte.  DERIVED, not measured on keys;
// profiles/nibble_rows.json records the largest |d32 - d64| the tests saw on a GPU.
constexpr double f32_err_nibble = 1.2 * (1.0 / 524288.0 + 1e-6);

// rows_nibble.hip.  src_dev: n_rows x 256 f32 on the device; dst_dev receives the packed nibbles (128 B a row).  Checks every row
// on the way: inside the f32 domain (domain.hip), nothing more.  Synchronises; a bad row is SMT_E_INVALID, `what` names the entry
// point, the message the first bad row (+ base).  dst_dev is written either way: hand it memory that is not part of a corpus yet.
int rows_to_nibble(smt_ctx *ctx, const float *src_dev, uint64_t n_rows, void *dst_dev, const char *what, uint64_t base = 0);
// n_rows nibble rows widened into dst_dev (f32); enqueued on the context's stream
int launch_nibble_to_f32(smt_ctx *ctx, const void *src_dev, uint64_t n_rows, float *dst_dev);

// |nominated distance - exact distance| of batch_nibble_kernel (batch_nibble.hip), by the rules of f32_err_batch_byte
// (byte_rows.h), RECOUNTED for this kernel.  The ROWS contribute nothing: the operand is 16 x the stored nibble, exactly (a shift
// and a mask), and the 16 leaves as a power of two.  The INSTRUCTIONS contribute nothing: the three digit planes accumulate in
// i32, |A_d| <= 256 x 128 x 128 = 2^22 (a digit's 128 against 16 x 8), exact, and |c|^2 <= 2^14 is an exact v_dot8_i32_i4 sum.
// Representation, the query's alone: n_i = rint(2^22 u_i) is off by at most 1/2, |e_i| <= 2^-23 on u_i, and over a row
// |<e, c>| / |c| <= |e|_2 <= 16 x 2^-23 = 2^-19.  The f32 scalings, in units of 2^-24 of the cosine, as built: |q|^2 -- four fused
// multiply-adds and the six levels of wave_sum, ten roundings, halved by the root -- 5; its rsqrt 1; u_i = q_i x that 1; x 2^22
// exact; |c|^2 converts exactly, its rsqrt 1, x 2^-26 exact; the combination 256 A1 + A2 rounds at magnitude <= 2^19 x 16 |c|
// (|d1|_2, |d2|_2 <= 2^11) against a full scale of 2^22 x 16 |c|, 1/8, and 65536 A0 + that 1; score x rxj 1; 1 - that 1:
// 11.2 x 2^-24 = 6.7e-7, inside the 1e-6 the batched routes allot to their scalings.  The whole times the project's 1.2:
// 1.2 x (2^-19 + 1e-6) = 3.49e-6 -- EQUAL to the scan's f32_err_nibble, so what this route leaves unproved the scan cannot prove
// either: search_wide_host does not run nibble rows again through the scan, they fall to the exhaustive re-answer.
// DERIVED, not measured; profiles/nibble_batch.json records the largest |d32 - d64| tests/test_gpu_nibble_batch.py saw.
constexpr double f32_err_batch_nibble = 1.2 * (1.0 / 524288.0 + 1e-6);

// The batched route (batch_nibble.hip): calls of at least tuning key nibble_batch_min queries (0: never) run passes of
// nibble_batch_qb queries on the int8 MFMA pipe, certified under f32_err_batch_nibble.
inline bool nibble_batch_serves(const smt_ctx *ctx, const SlabSearch &a)
{
    return !a.scan_only && a.row_dtype == SMT_ROWS_I4 && ctx->tune.nibble_batch_min > 0 && a.nq >= (uint32_t)ctx->tune.nibble_batch_min;
}
uint32_t nibble_batch_qb();
int launch_batch_nibble(smt_ctx *ctx, const SlabSearch &a);
int debug_batch_nibble_lists(smt_ctx *ctx, const SlabSearch &a, key_t64 *out_keys_host, uint64_t out_cap_keys, uint32_t *out_blocks,
                             uint32_t *out_kp);

// scan_nibble.hip: scan_nibble_kernel<slots, filtered>, launched by launch_search_slab (scan_slab.hip) like the half and byte kernels
slab_scan_kernel_t nibble_scan_kernel_of(int slots, bool filtered);

}  // namespace smt
