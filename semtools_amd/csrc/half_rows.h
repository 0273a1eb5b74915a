// half_rows.h -- corpora whose rows are stored as 256 IEEE binary16 values (SMT_ROWS_F16, 512 B a row): what rows_half.hip,
// scan_half.hip and the element-typed parts of finish_slab.hip, scan_slab.hip's launch and search_slab.cpp share.  The answers are
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

// scan_half.hip: scan_half_kernel<slots, filtered>, launched by launch_search_slab (scan_slab.hip) like the wide kernels
slab_scan_kernel_t half_scan_kernel_of(int slots, bool filtered);

}  // namespace smt
