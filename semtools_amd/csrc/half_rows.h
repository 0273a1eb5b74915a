// half_rows.h -- corpora whose rows are stored as 256 IEEE binary16 values (SMT_ROWS_F16, 512 B a row): what rows_half.hip,
// scan_half.hip, batch_half.hip and the element-typed parts of finish_slab.hip, scan_slab.hip's launch and search_slab.cpp share.  The answers are
// defined over the STORED values: a half widens to f32 exactly, and the exact distance is the f64 distance of the widened row.
#pragma once
#include "wide_rows.h"

namespace smt {

inline bool rows_are_half(const smt_corpus *c) { return c->row_dtype == SMT_ROWS_F16; }

constexpr int HALF_STEP_ROWS = 8;   // rows a wave of scan_half_kernel takes per step: four 1 KiB loads of two rows each

// |f32 scan distance - exact distance| of scan_half_kernel, by the counting rule at F32_ERR_SCAN (common.h), as f32_err_slab
// (wide_rows.h) applies it: a lane runs eight fused multiply-adds (the widening of a half is exact and adds none), the tree over a
// 32-lane half has five levels and is taken as eight steps as there, on terms whose absolute sum is <= 1, and two rsqrt and two
// multiplies follow: (8 + 8 + 4) roundings of 2^-24 = 1.19e-6, times the factor 4 that 4e-6 has over the 256 kernel's figure:
// 4.8e-6.  DERIVED, not measured on keys; profiles/half_rows.json records the largest |d32 - d64| the tests saw on a GPU.
constexpr double f32_err_half = 4.0 * 20.0 / 16777216.0;

// f32 -> binary16, round to nearest even, in integer arithmetic (no rounding or denormal mode of the device has a say): subnormal
// halves are produced, -0.0 and everything that rounds to zero keep their sign, |x| >= 65520 gives an infinity, NaN stays NaN.
// Bit for bit NumPy's astype(float16).
__host__ __device__ inline uint16_t half_bits_from_f32_bits(uint32_t x)
{
    const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
    if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                       // 65520 = 65504 + half an ulp: ties to even go up
    if (a >= 0x38800000u) return (uint16_t)(sign | ((a + 0x0fffu + ((a >> 13) & 1u) - 0x38000000u) >> 13));   // normal halves, >= 2^-14
    if (a < 0x33000000u) return (uint16_t)sign;                                    // < 2^-25
    const uint32_t shift = 126u - (a >> 23);                                       // 14 .. 24: the result counts units of 2^-24
    const uint32_t m = (a & 0x7fffffu) | 0x800000u, q = m >> shift, rem = m & ((1u << shift) - 1u), mid = 1u << (shift - 1);
    return (uint16_t)(sign | (q + ((rem > mid || (rem == mid && (q & 1u))) ? 1u : 0u)));
}
// binary16 -> f32, exact, subnormals included, in integer arithmetic but for the one exact product of a subnormal
__host__ __device__ inline float f32_from_half_bits(uint16_t h)
{
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    uint32_t bits;
    if (e == 0) {
        const float f = (float)m * 5.9604644775390625e-08f;   // m x 2^-24: a normal f32
        memcpy(&bits, &f, 4);
        bits |= sign;
    } else {
        bits = sign | (e == 31 ? 0x7f800000u : (e + 112u) << 23) | (m << 13);
    }
    float out;
    memcpy(&out, &bits, 4);
    return out;
}

// rows_half.hip.  src_dev: n_rows x 256 f32 on the device; dst_dev receives the halves.  Checks every row on the way: inside the f32
// domain (domain.hip) and no component that rounds to an infinity.  Synchronises; a bad row is SMT_E_INVALID, `what` names the entry
// point, the message the first bad row (+ base).  dst_dev is written either way: hand it memory that is not part of a corpus yet.
int rows_to_half(smt_ctx *ctx, const float *src_dev, uint64_t n_rows, void *dst_dev, const char *what, uint64_t base = 0);
// half rows already on the device (smt_corpus_from_device_typed): every value finite, or SMT_E_INVALID as above
int require_half_rows_domain(smt_ctx *ctx, const void *rows_dev, uint64_t n_rows, const char *what);
// n_rows half rows widened into dst_dev (f32); enqueued on the context's stream
int launch_half_to_f32(smt_ctx *ctx, const void *src_dev, uint64_t n_rows, float *dst_dev);

// |nominated distance - exact distance| of batch_half_kernel (batch_half.hip), by the rules at F32_ERR_BF16X3 (common.h, mfma_tile.h)
// and f32_err_batch_slab (wide_rows.h): the query's hi + lo carry 22 bits -- representation 2^-22 |x||u|; the ROWS contribute nothing,
// a stored half is the operand; 32 MFMA instructions at 2 ulp = 2^-23 each of an accumulator whose magnitude, scaled back, is <= 1:
// 32 x 2^-22 (the 7.6e-6 of the f16 x 2 note); the two f32 scalings 1e-6; the whole times the project's 1.2:
// 1.2 x (33 x 2^-22 + 1e-6) = 1.06e-5, an eighth of f32_err_batch_slab(2).  DERIVED, not measured; profiles/half_batch.json records
// the largest |d32 - d64| tests/test_gpu_half_batch.py saw on random, worst-case and subnormal rows.
constexpr double f32_err_batch_half = 1.2 * (33.0 / 4194304.0 + 1e-6);

// The batched route (batch_half.hip): calls of at least tuning key half_batch_min queries (0: never) run passes of half_batch_qb
// queries on the f16 MFMA pipe, certified under f32_err_batch_half.
inline bool half_batch_serves(const smt_ctx *ctx, const SlabSearch &a)
{
    return !a.scan_only && a.row_dtype == SMT_ROWS_F16 && ctx->tune.half_batch_min > 0 && a.nq >= (uint32_t)ctx->tune.half_batch_min;
}
// either batched route: what it leaves unproved, search_wide_host runs again through the scan
inline bool batch_route_serves(const smt_ctx *ctx, const SlabSearch &a) { return slab_batch_serves(ctx, a) || half_batch_serves(ctx, a); }
uint32_t half_batch_qb();
int launch_batch_half(smt_ctx *ctx, const SlabSearch &a);
int debug_batch_half_lists(smt_ctx *ctx, const SlabSearch &a, key_t64 *out_keys_host, uint64_t out_cap_keys, uint32_t *out_blocks,
                           uint32_t *out_kp);

// scan_half.hip: scan_half_kernel<slots, filtered>, launched by launch_search_slab (scan_slab.hip) like the wide kernels
slab_scan_kernel_t half_scan_kernel_of(int slots, bool filtered);

}  // namespace smt
