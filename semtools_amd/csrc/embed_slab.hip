// embed_slab.hip -- K1 for WIDE tables: model2vec pooling of rows of D = 256 S elements (S = 2, 3, 4; f32, IEEE half or int8 as
// stored), bit-identical to the oracle's pool_ids.  D = 256 keeps embed_kernels.hip; indexed models are not served here.
//
// The order of every rounding is the CPU code's: per dimension one f32 chain of adds in token order, the division by the token
// count, then ONE sequential f32 sum of all D squares in index order, sqrt, max(., 1e-12), the division.  Contraction is off.
//
// Shape: the 16-lanes-per-row gather of embed_kernels.hip -- a group of 16 lanes reads 16 x 16 B = 256 contiguous bytes per
// instruction -- and its work-balanced runs (a group walks a contiguous run of lines cut by tokens + 4 per line).  S enters as
// SLAB PASSES WITH A FINAL NORMALISE: a group pools its line one slab at a time (the line's tokens are walked S times, four in
// flight, 16 accumulators per lane exactly as for a 256 row; the ids come from L1/L2 after the first pass) and parks each slab's
// means in registers (S x 16); slabs are independent up to there.  Only the norm sees the whole row: its chain runs round the
// group with row_ror:1 through all S slabs in index order (S x 256 dependent adds), then every parked mean is divided and stored.
// Piece p of a slab in lane a holds the slab's dims (256 / NC) p + EPL a .. + EPL - 1 (NC = 4, 2, 1 pieces of EPL = 4, 8, 16
// elements for f32, half, int8): accumulator EPL p + e, as in embed_kernels.hip.
// Simpler than the 256 kernel on purpose: no id prefetch across steps, no parked-line batching.  Not measured.
#include "wide_rows.h"

namespace smt {

constexpr int SLAB_DPP_ROW_ROR1 = 0x121;   // lane i of a 16-lane row receives lane (i - 1) mod 16
__device__ __forceinline__ float slab_ror1(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), SLAB_DPP_ROW_ROR1, 0xF, 0xF, false));
}

typedef _Float16 slab_half8 __attribute__((ext_vector_type(8)));
typedef signed char slab_char16 __attribute__((ext_vector_type(16)));
typedef float slab_float4 __attribute__((ext_vector_type(4)));
template <typename T> struct SlabPiece;
template <> struct SlabPiece<float> { using type = slab_float4; static constexpr int NC = 4; };
template <> struct SlabPiece<_Float16> { using type = slab_half8; static constexpr int NC = 2; };
template <> struct SlabPiece<signed char> { using type = slab_char16; static constexpr int NC = 1; };

struct EmbedSlabParams {
    const unsigned char *table;
    uint64_t V;
    const uint32_t *ids;
    const uint64_t *offsets;
    uint64_t n_lines;
    uint32_t max_tokens;
    int normalize;
    float *out;
    const uint64_t *run_start;   // [n_groups + 1]
    uint64_t n_groups;
};

// run_start[g] = the first line whose key offsets[i] - offsets[0] + 4 i reaches g / n_groups of the total (embed_kernels.hip's rule)
__global__ void __launch_bounds__(256) embed_slab_runs_kernel(const uint64_t *__restrict__ offsets, uint64_t n_lines, uint64_t n_groups,
                                                              uint64_t *__restrict__ run_start)
{
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g > n_groups) return;
    const uint64_t o0 = offsets[0];
    const uint64_t total = offsets[n_lines] - o0 + 4 * n_lines;
    const uint64_t target = (uint64_t)(((unsigned __int128)total * g) / n_groups);
    uint64_t lo = 0, hi = n_lines;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] - o0 + 4 * mid >= target) hi = mid; else lo = mid + 1;
    }
    run_start[g] = g == n_groups ? n_lines : lo;
}

template <typename T, int S>
__global__ void __launch_bounds__(256) embed_slab_kernel(EmbedSlabParams p)
{
#pragma clang fp contract(off)
    using piece_t = typename SlabPiece<T>::type;
    constexpr int NC = SlabPiece<T>::NC;
    constexpr int EPL = 16 / NC;
    constexpr uint64_t SLAB_BYTES = 256 * sizeof(T), ROW_BYTES = S * SLAB_BYTES;
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
        float mean[S][16];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            float acc[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[k] = 0.0f;
            for (uint64_t t = t0; t < t1; t += TU) {
                piece_t r[TU][NC];
                bool on[TU];
#pragma unroll
                for (int u = 0; u < TU; ++u) {
                    on[u] = t + u < t1;
                    const uint64_t id = on[u] ? (uint64_t)p.ids[t + u] : 0;
                    const bool ok = on[u] && id < p.V;   // an id outside the table adds nothing and still counts in the mean
                    const piece_t *row = reinterpret_cast<const piece_t *>(p.table + (ok ? id : 0) * ROW_BYTES + s * SLAB_BYTES);
#pragma unroll
                    for (int c = 0; c < NC; ++c) r[u][c] = ok ? row[c * 16 + a] : piece_t(0);
                }
#pragma unroll
                for (int u = 0; u < TU; ++u) {   // token order
                    if (on[u]) {
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
#pragma unroll
                            for (int e = 0; e < EPL; ++e) acc[EPL * c + e] = acc[EPL * c + e] + (float)r[u][c][e];
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 16; ++k) mean[s][k] = acc[k] / cnt;
        }
        if (p.normalize) {
            // ss = ((0 + v_0^2) + v_1^2) + ... + v_{D-1}^2.  Step (s, c, a') adds the EPL squares of piece c of slab s in lane a';
            // the true chain value sits in that lane and moves on to lane a' + 1 (15 -> 0) with the rotation.
            float ss = 0.0f;
#pragma unroll
            for (int s = 0; s < S; ++s) {
#pragma unroll
                for (int c = 0; c < NC; ++c) {
#pragma unroll
                    for (int step = 0; step < 16; ++step) {
                        ss = (s == 0 && c == 0 && step == 0) ? 0.0f : slab_ror1(ss);
#pragma unroll
                        for (int e = 0; e < EPL; ++e) {
                            const float sq = mean[s][EPL * c + e] * mean[s][EPL * c + e];
                            ss = ss + sq;
                        }
                    }
                }
            }
            ss = __shfl(ss, (lane & 48) | 15);   // after the last step the whole chain is in lane 15 of the group
            float norm = sqrtf(ss);
            if (!(norm > 1e-12f)) norm = 1e-12f;
#pragma unroll
            for (int s = 0; s < S; ++s) {
#pragma unroll
                for (int k = 0; k < 16; ++k) mean[s][k] = mean[s][k] / norm;
            }
        }
        slab_float4 *o = reinterpret_cast<slab_float4 *>(p.out + line * (256 * S));
#pragma unroll
        for (int s = 0; s < S; ++s) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {   // accumulators 4 g .. 4 g + 3 = elements e0 .. e0 + 3 of piece c
                const int c = (4 * g) / EPL, e0 = (4 * g) % EPL;
                const int dim0 = (256 / NC) * c + EPL * a + e0;
                slab_float4 v;
                v.x = mean[s][4 * g]; v.y = mean[s][4 * g + 1]; v.z = mean[s][4 * g + 2]; v.w = mean[s][4 * g + 3];
                o[s * 64 + dim0 / 4] = v;
            }
        }
    }
}

template <typename T>
static void launch_embed_slab_typed(int S, unsigned blocks, hipStream_t st, const EmbedSlabParams &p)
{
    if (S == 2) hipLaunchKernelGGL((embed_slab_kernel<T, 2>), dim3(blocks), dim3(256), 0, st, p);
    else if (S == 3) hipLaunchKernelGGL((embed_slab_kernel<T, 3>), dim3(blocks), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((embed_slab_kernel<T, 4>), dim3(blocks), dim3(256), 0, st, p);
}

int launch_embed_runs(smt_ctx *ctx, const uint64_t *offsets, uint64_t n_lines, uint64_t groups)
{
    if (ctx->embed_runs_cap < groups + 1) {
        SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (ctx->d_embed_runs) SMT_HIP_CHECK(hipFree(ctx->d_embed_runs));
        ctx->d_embed_runs = nullptr;
        ctx->embed_runs_cap = 0;
        SMT_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&ctx->d_embed_runs), (groups + 1) * sizeof(uint64_t)));
        ctx->embed_runs_cap = groups + 1;
    }
    hipLaunchKernelGGL(embed_slab_runs_kernel, dim3((unsigned)((groups + 1 + 255) / 256)), dim3(256), 0, ctx->stream, offsets, n_lines, groups,
                       ctx->d_embed_runs);
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

int launch_embed_slab(smt_ctx *ctx, const void *table, int table_dtype, uint64_t V, uint32_t D, int normalize, const uint32_t *ids,
                      const uint64_t *offsets, uint64_t n_lines, uint32_t max_tokens, float *out)
{
    if (n_lines == 0) return SMT_OK;
    SMT_REQUIRE(dim_is_wide(D), "wide embed: 512, 768 or 1024 dimensions");
    SMT_REQUIRE(table_dtype == SMT_TABLE_F32 || table_dtype == SMT_TABLE_F16 || table_dtype == SMT_TABLE_I8, "unknown table dtype");
    // enough groups to fill the chip (16 waves x 4 groups per CU), never more than lines
    const uint64_t groups = std::min<uint64_t>(n_lines, (uint64_t)std::max(ctx->num_cus, 1) * 64);
    const int rc = launch_embed_runs(ctx, offsets, n_lines, groups);   // (may move ctx->d_embed_runs: before it is read below)
    if (rc) return rc;
    EmbedSlabParams p;
    p.table = static_cast<const unsigned char *>(table);
    p.V = V;
    p.ids = ids;
    p.offsets = offsets;
    p.n_lines = n_lines;
    p.max_tokens = max_tokens;
    p.normalize = normalize;
    p.out = out;
    p.run_start = ctx->d_embed_runs;
    p.n_groups = groups;
    const unsigned blocks = (unsigned)((groups + 15) / 16);   // 256 threads = 16 groups
    const int S = (int)(D / 256);
    prof_begin(ctx, "embed_slab");
    if (table_dtype == SMT_TABLE_F16) launch_embed_slab_typed<_Float16>(S, blocks, ctx->stream, p);
    else if (table_dtype == SMT_TABLE_I8) launch_embed_slab_typed<signed char>(S, blocks, ctx->stream, p);
    else launch_embed_slab_typed<float>(S, blocks, ctx->stream, p);
    prof_end(ctx, "embed_slab");
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

}  // namespace smt
