// rows_nibble.hip -- how rows enter and leave a NIBBLE corpus (nibble_rows.h): f32 -> packed int4 direction with the domain test
// on the input, and packed int4 -> f32 for smt_corpus_read_rows.  Adopted nibble rows need neither: any byte is a valid pair.
//
// One wave per row, lane l holds components [4 l, 4 l + 4) -- the layout of rows_domain_kernel (domain.hip) and rows_byte_kernel,
// whose verdict this repeats: m = max |x| as an integer, in domain iff 0 or within [2^-40, 2^40]; NaN and Inf sort above every
// finite value.  The bits of m ARE amax, so the row's scale is one __fdiv_rn(7, amax) -- the correctly rounded division, never a
// reciprocal -- and a component is rint(__fmul_rn(x, s)): the product is an intrinsic so that nothing contracts it, the rounding is
// v_rndne_f32 (ties to even).  The bound that makes clipping unnecessary is in nibble_rows.h.  A lane's four components are two
// bytes of the row, element 2 j in the low nibble of byte j: one 16-bit store per lane, 128 B per wave.  Bad rows are counted and
// the smallest index kept; they are stored as zeros, and the callers convert into memory that is not part of a corpus yet.
#include "nibble_rows.h"
#include "device_utils.h"

namespace smt {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t nibble_of(uint32_t x_bits, float s)
{
    return (uint32_t)(int)__builtin_rintf(__fmul_rn(__uint_as_float(x_bits), s)) & 0xfu;
}

__global__ void __launch_bounds__(256) rows_nibble_kernel(const u32x4 *src, uint64_t n_rows, uint16_t *dst, unsigned long long *out /* [count, first] */)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t r = wave; r < n_rows; r += n_waves) {
        u32x4 v = __builtin_nontemporal_load(src + r * 64 + lane);
        const uint32_t m = wave_max_u32(max(max(v.x & 0x7fffffffu, v.y & 0x7fffffffu), max(v.z & 0x7fffffffu, v.w & 0x7fffffffu)));
        const bool bad = !magnitude_in_domain(m);
        if (bad) v = u32x4{0u, 0u, 0u, 0u};
        const float s = (bad || m == 0u) ? 0.0f : __fdiv_rn(7.0f, __uint_as_float(m));
        dst[r * 64 + lane] = (uint16_t)(nibble_of(v.x, s) | (nibble_of(v.y, s) << 4) | (nibble_of(v.z, s) << 8) | (nibble_of(v.w, s) << 12));
        if (bad && lane == 0) {
            atomicAdd(out, 1ull);
            atomicMin(out + 1, (unsigned long long)r);
        }
    }
}

int rows_to_nibble(smt_ctx *ctx, const float *src_dev, uint64_t n_rows, void *dst_dev, const char *what, uint64_t base)
{
    if (n_rows == 0) return SMT_OK;
    unsigned long long init[2] = {0ull, ~0ull}, got[2] = {0ull, ~0ull};
    unsigned long long *d = ctx->d_status + 2;   // (the words check_rows_domain uses: domain.hip)
    SMT_HIP_CHECK(hipMemcpyAsync(d, init, sizeof(init), hipMemcpyHostToDevice, ctx->stream));
    const int blocks = (int)std::min<uint64_t>((n_rows + 3) / 4, (uint64_t)(ctx->num_cus > 0 ? ctx->num_cus : 256) * 8);
    hipLaunchKernelGGL(rows_nibble_kernel, dim3(blocks), dim3(256), 0, ctx->stream, reinterpret_cast<const u32x4 *>(src_dev), n_rows,
                       static_cast<uint16_t *>(dst_dev), d);
    SMT_HIP_CHECK(hipGetLastError());
    SMT_HIP_CHECK(hipMemcpyAsync(got, d, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
    SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (got[0] == 0) return SMT_OK;
    set_error("%s: %llu of %llu rows are outside the library's domain (first: row %llu) -- every component must be finite and the "
              "largest magnitude of a row 0 or within [2^-40, 2^40] (include/semtools_hip.h, \"Domain\")", what, got[0],
              (unsigned long long)n_rows, (unsigned long long)(base + got[1]));
    return SMT_E_INVALID;
}

// a dword -- eight elements -- per thread, widened exactly: a shift pair sign-extends each nibble, then an integer conversion
__global__ void __launch_bounds__(256) nibble_to_f32_kernel(const uint32_t *src, uint64_t n_words, f32x4 *dst)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_words) return;
    const uint32_t w = src[i];
    f32x4 lo, hi;
    lo.x = (float)((int)(w << 28) >> 28);
    lo.y = (float)((int)(w << 24) >> 28);
    lo.z = (float)((int)(w << 20) >> 28);
    lo.w = (float)((int)(w << 16) >> 28);
    hi.x = (float)((int)(w << 12) >> 28);
    hi.y = (float)((int)(w << 8) >> 28);
    hi.z = (float)((int)(w << 4) >> 28);
    hi.w = (float)((int)w >> 28);
    dst[2 * i] = lo;
    dst[2 * i + 1] = hi;
}

int launch_nibble_to_f32(smt_ctx *ctx, const void *src_dev, uint64_t n_rows, float *dst_dev)
{
    if (n_rows == 0) return SMT_OK;
    const uint64_t n_words = n_rows * (NIBBLE_ROW_BYTES / 4), blocks = (n_words + 255) / 256;
    SMT_REQUIRE(blocks < (1ull << 31), "too many rows for one conversion launch");
    hipLaunchKernelGGL(nibble_to_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, static_cast<const uint32_t *>(src_dev), n_words,
                       reinterpret_cast<f32x4 *>(dst_dev));
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

}  // namespace smt
