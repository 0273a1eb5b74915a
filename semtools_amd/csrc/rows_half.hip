// rows_half.hip -- how rows enter and leave a HALF corpus (half_rows.h): f32 -> binary16 with the domain test on input and result,
// the test alone for half rows adopted from device memory, and binary16 -> f32 for smt_corpus_read_rows.
//
// One wave per row, lane l holds components [4 l, 4 l + 4) -- the layout of rows_domain_kernel (domain.hip), whose verdict this
// repeats for the f32 input: m = max |x| as an integer, in domain iff 0 or within [2^-40, 2^40]; NaN and Inf sort above every finite
// value.  On top of it the RESULT must be finite: a component of magnitude >= 65520 rounds to an infinity, and 65520 < 2^40, so
// the one comparison m < bits(65520) is both upper bounds.  The rounding itself is half_bits_from_f32_bits (integer arithmetic:
// subnormal halves kept, signs of zeros kept).  Bad rows are counted and the smallest index kept; the halves are stored either way,
// the callers convert into memory that is not part of a corpus yet.
#include "half_rows.h"
#include "device_utils.h"

namespace smt {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// FROM_F32: src = f32 rows, dst = the halves (stored).  Otherwise src = half rows, nothing is stored: the test alone.
template <bool FROM_F32>
__global__ void __launch_bounds__(256) rows_half_kernel(const void *src, uint64_t n_rows, u32x2 *dst, unsigned long long *out /* [count, first] */)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t r = wave; r < n_rows; r += n_waves) {
        bool bad;
        if constexpr (FROM_F32) {
            const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(src) + r * 64 + lane);
            const uint32_t m = wave_max_u32(max(max(v.x & 0x7fffffffu, v.y & 0x7fffffffu), max(v.z & 0x7fffffffu, v.w & 0x7fffffffu)));
            bad = !magnitude_in_domain(m) || m >= 0x477ff000u;
            u32x2 h;
            h.x = (uint32_t)half_bits_from_f32_bits(v.x) | ((uint32_t)half_bits_from_f32_bits(v.y) << 16);
            h.y = (uint32_t)half_bits_from_f32_bits(v.z) | ((uint32_t)half_bits_from_f32_bits(v.w) << 16);
            dst[r * 64 + lane] = h;
        } else {
            const u32x2 h = __builtin_nontemporal_load(reinterpret_cast<const u32x2 *>(src) + r * 64 + lane);
            // the largest magnitude among the four halves; an exponent of all ones (Inf, NaN) is 0x7c00 or more
            const uint32_t m = wave_max_u32(max(max(h.x & 0x7fffu, (h.x >> 16) & 0x7fffu), max(h.y & 0x7fffu, (h.y >> 16) & 0x7fffu)));
            bad = m >= 0x7c00u;
        }
        if (bad && lane == 0) {
            atomicAdd(out, 1ull);
            atomicMin(out + 1, (unsigned long long)r);
        }
    }
}

template <bool FROM_F32>
static int run_rows_half(smt_ctx *ctx, const void *src, uint64_t n_rows, void *dst, const char *what, uint64_t base)
{
    if (n_rows == 0) return SMT_OK;
    unsigned long long init[2] = {0ull, ~0ull}, got[2] = {0ull, ~0ull};
    unsigned long long *d = ctx->d_status + 2;   // (the words check_rows_domain uses: domain.hip)
    SMT_HIP_CHECK(hipMemcpyAsync(d, init, sizeof(init), hipMemcpyHostToDevice, ctx->stream));
    const int blocks = (int)std::min<uint64_t>((n_rows + 3) / 4, (uint64_t)(ctx->num_cus > 0 ? ctx->num_cus : 256) * 8);
    hipLaunchKernelGGL(rows_half_kernel<FROM_F32>, dim3(blocks), dim3(256), 0, ctx->stream, src, n_rows, reinterpret_cast<u32x2 *>(dst), d);
    SMT_HIP_CHECK(hipGetLastError());
    SMT_HIP_CHECK(hipMemcpyAsync(got, d, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
    SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (got[0] == 0) return SMT_OK;
    set_error("%s: %llu of %llu rows cannot be stored as half rows (first: row %llu) -- every component must be finite, the largest "
              "magnitude of a row 0 or at least 2^-40, and none may round to an infinity (|x| >= 65520) (include/semtools_hip.h, "
              "\"HALF ROWS\")", what, got[0], (unsigned long long)n_rows, (unsigned long long)(base + got[1]));
    return SMT_E_INVALID;
}

int rows_to_half(smt_ctx *ctx, const float *src_dev, uint64_t n_rows, void *dst_dev, const char *what, uint64_t base)
{
    return run_rows_half<true>(ctx, src_dev, n_rows, dst_dev, what, base);
}

int require_half_rows_domain(smt_ctx *ctx, const void *rows_dev, uint64_t n_rows, const char *what)
{
    return run_rows_half<false>(ctx, rows_dev, n_rows, nullptr, what, 0);
}

// four halves per thread, widened exactly
__global__ void __launch_bounds__(256) half_to_f32_kernel(const u32x2 *src, uint64_t n_quads, f32x4 *dst)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_quads) return;
    const u32x2 h = src[i];
    f32x4 v;
    v.x = f32_from_half_bits((uint16_t)h.x);
    v.y = f32_from_half_bits((uint16_t)(h.x >> 16));
    v.z = f32_from_half_bits((uint16_t)h.y);
    v.w = f32_from_half_bits((uint16_t)(h.y >> 16));
    dst[i] = v;
}

int launch_half_to_f32(smt_ctx *ctx, const void *src_dev, uint64_t n_rows, float *dst_dev)
{
    if (n_rows == 0) return SMT_OK;
    const uint64_t n_quads = n_rows * 64, blocks = (n_quads + 255) / 256;
    SMT_REQUIRE(blocks < (1ull << 31), "too many rows for one conversion launch");
    hipLaunchKernelGGL(half_to_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, reinterpret_cast<const u32x2 *>(src_dev), n_quads,
                       reinterpret_cast<f32x4 *>(dst_dev));
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

}  // namespace smt
