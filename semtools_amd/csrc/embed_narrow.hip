// embed_narrow.hip -- K1 for NARROW tables: model2vec pooling of rows of 64 elements (f32, IEEE half or int8 as stored: 256, 128 or
// 64 B a row), bit-identical to the oracle's pool_ids.  D = 256 keeps embed_kernels.hip, the wide tables embed_slab.hip; indexed
// models are not served here.
//
// The order of every rounding is the CPU code's: per dimension one f32 chain of adds in token order, the division by the token
// count, then ONE sequential f32 sum of the 64 squares in index order, sqrt, max(., 1e-12), the division.  Contraction is off.
//
// LAYOUT.  A 16-lane DPP row owns a LINE: lane a of the group holds the components 4 a .. 4 a + 3 of the pooled row -- FOUR
// accumulators -- whatever the table stores: one gather instruction reads a table row as 16 x 16 B (f32), 16 x 8 B (half) or
// 16 x 4 B (int8), contiguous, and the elements are widened in registers.  A wave pools four lines at once.
// IMBALANCE.  The groups do not take "the next four lines": the lines are cut into contiguous RUNS of equal work (tokens + 4 per
// line, the run table of embed_slab.hip / embed_kernels.hip) and a group walks its run, so a long line beside three empty ones
// costs its group that line and the others move on inside their own runs.
// LOADS.  A step takes TU = 4 tokens: their four table rows are requested together, and the ids of the NEXT step are loaded
// before this step's rows are added (the id -> row dependency is the latency of a line; one step ahead hides it as in K1).
// THE NORM.  The chain ((v_0^2 + v_1^2) + ...) + v_63^2 runs round the group with row_ror:1: at step a the true value sits in lane
// a, which adds its four squares in index order and hands it on -- 64 dependent adds, 15 rotations.
#include "wide_rows.h"

namespace smt {

constexpr int NARROW_DPP_ROW_ROR1 = 0x121;   // lane i of a 16-lane row receives lane (i - 1) mod 16
__device__ __forceinline__ float narrow_ror1(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), NARROW_DPP_ROW_ROR1, 0xF, 0xF, false));
}

typedef float narrow_float4 __attribute__((ext_vector_type(4)));
typedef _Float16 narrow_half4 __attribute__((ext_vector_type(4)));
typedef signed char narrow_char4 __attribute__((ext_vector_type(4)));
template <typename T> struct NarrowPiece;
template <> struct NarrowPiece<float> { using type = narrow_float4; };
template <> struct NarrowPiece<_Float16> { using type = narrow_half4; };
template <> struct NarrowPiece<signed char> { using type = narrow_char4; };

struct EmbedNarrowParams {
    const unsigned char *table;
    uint64_t V;
    const uint32_t *ids;
    const uint64_t *offsets;
    uint32_t max_tokens;
    int normalize;
    float *out;
    const uint64_t *run_start;   // [n_groups + 1]
    uint64_t n_groups;
};

template <typename T>
__global__ void __launch_bounds__(256) embed_narrow_kernel(EmbedNarrowParams p)
{
#pragma clang fp contract(off)
    using piece_t = typename NarrowPiece<T>::type;
    constexpr int D = 64;
    constexpr int TU = 4;   // tokens in flight per group
    const int lane = threadIdx.x & 63;
    const int a = lane & 15;
    const uint64_t group = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    if (group >= p.n_groups) return;   // (whole groups leave; the DPP row steps and the shuffle below stay inside a group's 16 lanes)
    const uint64_t line_end = p.run_start[group + 1];
    for (uint64_t line = p.run_start[group]; line < line_end; ++line) {
        const uint64_t t0 = p.offsets[line];
        uint64_t t1 = p.offsets[line + 1];
        if (p.max_tokens != 0 && t1 - t0 > (uint64_t)p.max_tokens) t1 = t0 + p.max_tokens;
        const float cnt = (float)(t1 > t0 ? t1 - t0 : 1);
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t idn[TU];
#pragma unroll
        for (int u = 0; u < TU; ++u) idn[u] = t0 + u < t1 ? p.ids[t0 + u] : 0u;
        for (uint64_t t = t0; t < t1; t += TU) {
            piece_t r[TU];
            bool on[TU];
#pragma unroll
            for (int u = 0; u < TU; ++u) {
                on[u] = t + u < t1;
                const uint64_t id = idn[u];
                const bool ok = on[u] && id < p.V;   // an id outside the table adds nothing and still counts in the mean
                r[u] = ok ? reinterpret_cast<const piece_t *>(p.table + id * (D * sizeof(T)))[a] : piece_t(0);
            }
#pragma unroll
            for (int u = 0; u < TU; ++u) idn[u] = t + TU + u < t1 ? p.ids[t + TU + u] : 0u;   // the next step's ids, behind this step's rows
#pragma unroll
            for (int u = 0; u < TU; ++u) {   // token order
                if (on[u]) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] = acc[e] + (float)r[u][e];
                }
            }
        }
        float mean[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) mean[e] = acc[e] / cnt;
        if (p.normalize) {
            float ss = 0.0f;
#pragma unroll
            for (int step = 0; step < 16; ++step) {
                ss = step == 0 ? 0.0f : narrow_ror1(ss);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float sq = mean[e] * mean[e];
                    ss = ss + sq;
                }
            }
            ss = __shfl(ss, (lane & 48) | 15);   // after the last step the whole chain is in lane 15 of the group
            float norm = sqrtf(ss);
            if (!(norm > 1e-12f)) norm = 1e-12f;
#pragma unroll
            for (int e = 0; e < 4; ++e) mean[e] = mean[e] / norm;
        }
        narrow_float4 v;
        v.x = mean[0]; v.y = mean[1]; v.z = mean[2]; v.w = mean[3];
        reinterpret_cast<narrow_float4 *>(p.out + line * D)[a] = v;
    }
}

int launch_embed_narrow(smt_ctx *ctx, const void *table, int table_dtype, uint64_t V, int normalize, const uint32_t *ids,
                        const uint64_t *offsets, uint64_t n_lines, uint32_t max_tokens, float *out)
{
    if (n_lines == 0) return SMT_OK;
    SMT_REQUIRE(table_dtype == SMT_TABLE_F32 || table_dtype == SMT_TABLE_F16 || table_dtype == SMT_TABLE_I8, "unknown table dtype");
    // enough groups to fill the chip (16 waves x 4 groups per CU), never more than lines
    const uint64_t groups = std::min<uint64_t>(n_lines, (uint64_t)std::max(ctx->num_cus, 1) * 64);
    const int rc = launch_embed_runs(ctx, offsets, n_lines, groups);   // (may move ctx->d_embed_runs: before it is read below)
    if (rc) return rc;
    prof_begin(ctx, "embed_narrow");
    EmbedNarrowParams p;
    p.table = static_cast<const unsigned char *>(table);
    p.V = V;
    p.ids = ids;
    p.offsets = offsets;
    p.max_tokens = max_tokens;
    p.normalize = normalize;
    p.out = out;
    p.run_start = ctx->d_embed_runs;
    p.n_groups = groups;
    const unsigned blocks = (unsigned)((groups + 15) / 16);   // 256 threads = 16 groups
    if (table_dtype == SMT_TABLE_F16) hipLaunchKernelGGL(embed_narrow_kernel<_Float16>, dim3(blocks), dim3(256), 0, ctx->stream, p);
    else if (table_dtype == SMT_TABLE_I8) hipLaunchKernelGGL(embed_narrow_kernel<signed char>, dim3(blocks), dim3(256), 0, ctx->stream, p);
    else hipLaunchKernelGGL(embed_narrow_kernel<float>, dim3(blocks), dim3(256), 0, ctx->stream, p);
    prof_end(ctx, "embed_narrow");
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

}  // namespace smt
