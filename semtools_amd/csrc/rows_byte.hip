// rows_byte.hip -- how rows enter and leave a BYTE corpus (byte_rows.h): f32 -> int8 direction with the domain test on the input,
// and int8 -> f32 for smt_corpus_read_rows.  Adopted byte rows need neither: any byte is a valid value.
//
// One wave per row, lane l holds components [4 l, 4 l + 4) -- the layout of rows_domain_kernel (domain.hip), whose verdict this
// repeats: m = max |x| as an integer, in domain iff 0 or within [2^-40, 2^40]; NaN and Inf sort above every finite value.  The
// bits of m ARE amax, so the row's scale is one __fdiv_rn(127, amax) -- the correctly rounded division, never a reciprocal -- and
// a component is rint(__fmul_rn(x, s)): the product is an intrinsic so that nothing contracts it, the rounding is v_rndne_f32
// (ties to even).  The bound that makes clipping unnecessary is in byte_rows.h.  Bad rows are counted and the smallest index kept;
// they are stored as zeros, and the callers convert into memory that is not part of a corpus yet.
#include "byte_rows.h"
#include "device_utils.h"

namespace smt {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t byte_of(uint32_t x_bits, float s)
{
    return (uint32_t)(int)__builtin_rintf(__fmul_rn(__uint_as_float(x_bits), s)) & 0xffu;
}

__global__ void __launch_bounds__(256) rows_byte_kernel(const u32x4 *src, uint64_t n_rows, uint32_t *dst, unsigned long long *out /* [count, first] */)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t r = wave; r < n_rows; r += n_waves) {
        u32x4 v = __builtin_nontemporal_load(src + r * 64 + lane);
        const uint32_t m = wave_max_u32(max(max(v.x & 0x7fffffffu, v.y & 0x7fffffffu), max(v.z & 0x7fffffffu, v.w & 0x7fffffffu)));
        const bool bad = !magnitude_in_domain(m);
        if (bad) v = u32x4{0u, 0u, 0u, 0u};
        const float s = (bad || m == 0u) ? 0.0f : __fdiv_rn(127.0f, __uint_as_float(m));
        dst[r * 64 + lane] = byte_of(v.x, s) | (byte_of(v.y, s) << 8) | (byte_of(v.z, s) << 16) | (byte_of(v.w, s) << 24);
        if (bad && lane == 0) {
            atomicAdd(out, 1ull);
            atomicMin(out + 1, (unsigned long long)r);
        }
    }
}

int rows_to_byte(smt_ctx *ctx, const float *src_dev, uint64_t n_rows, void *dst_dev, const char *what, uint64_t base)
{
    if (n_rows == 0) return SMT_OK;
    unsigned long long init[2] = {0ull, ~0ull}, got[2] = {0ull, ~0ull};
    unsigned long long *d = ctx->d_status + 2;   // (the words check_rows_domain uses: domain.hip)
    SMT_HIP_CHECK(hipMemcpyAsync(d, init, sizeof(init), hipMemcpyHostToDevice, ctx->stream));
    const int blocks = (int)std::min<uint64_t>((n_rows + 3) / 4, (uint64_t)(ctx->num_cus > 0 ? ctx->num_cus : 256) * 8);
    hipLaunchKernelGGL(rows_byte_kernel, dim3(blocks), dim3(256), 0, ctx->stream, reinterpret_cast<const u32x4 *>(src_dev), n_rows,
                       static_cast<uint32_t *>(dst_dev), d);
    SMT_HIP_CHECK(hipGetLastError());
    SMT_HIP_CHECK(hipMemcpyAsync(got, d, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
    SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (got[0] == 0) return SMT_OK;
    set_error("%s: %llu of %llu rows are outside the library's domain (first: row %llu) -- every component must be finite and the "
              "largest magnitude of a row 0 or within [2^-40, 2^40] (include/semtools_hip.h, \"Domain\")", what, got[0],
              (unsigned long long)n_rows, (unsigned long long)(base + got[1]));
    return SMT_E_INVALID;
}

// four bytes per thread, widened exactly (sign extension, then an integer conversion)
__global__ void __launch_bounds__(256) byte_to_f32_kernel(const uint32_t *src, uint64_t n_quads, f32x4 *dst)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_quads) return;
    const uint32_t w = src[i];
    f32x4 v;
    v.x = (float)(int8_t)w;
    v.y = (float)(int8_t)(w >> 8);
    v.z = (float)(int8_t)(w >> 16);
    v.w = (float)(int8_t)(w >> 24);
    dst[i] = v;
}

int launch_byte_to_f32(smt_ctx *ctx, const void *src_dev, uint64_t n_rows, float *dst_dev)
{
    if (n_rows == 0) return SMT_OK;
    const uint64_t n_quads = n_rows * 64, blocks = (n_quads + 255) / 256;
    SMT_REQUIRE(blocks < (1ull << 31), "too many rows for one conversion launch");
    hipLaunchKernelGGL(byte_to_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, static_cast<const uint32_t *>(src_dev), n_quads,
                       reinterpret_cast<f32x4 *>(dst_dev));
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

}  // namespace smt
