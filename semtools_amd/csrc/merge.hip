// merge.hip -- what runs after the shards' selects: the cross-shard top-k merges (gathered lists, or lists read in place
// over xGMI) and the combine of the shards' status words, with their launchers (called by api.cpp, sharded.cpp and
// group_exchange.cpp).
#include "common.h"
#include "device_utils.h"

namespace smt {

// ------------------------------------------------- cross-shard top-k merge
// Entry (list l, query qi, slot i): rows[l*list_stride + qi*query_stride + i], same for dist.
// Plain layout [n_lists][nq][k_in]: list_stride = nq*k_in, query_stride = k_in.  Packed layout
// [n_lists][nq][2][k_in] (rows then distance bits, one all-gather instead of two):
// list_stride = nq*2*k_in, query_stride = 2*k_in, dist = rows + k_in.  One block per query.
__global__ void merge_topk_kernel(const uint64_t *rows, const double *dist, uint32_t n_lists, uint64_t list_stride,
                                  uint64_t query_stride, uint32_t k_in, uint32_t k_out, uint64_t *out_rows,
                                  double *out_dist, uint64_t out_query_stride)
{
    const uint32_t qi = blockIdx.x;
    const uint32_t M = n_lists * k_in;
    uint64_t *orow = out_rows + (size_t)qi * out_query_stride;
    double *odist = out_dist + (size_t)qi * out_query_stride;
    for (uint32_t t = threadIdx.x; t < k_out; t += blockDim.x) {
        orow[t] = 0xFFFFFFFFFFFFFFFFull;
        odist[t] = __builtin_inf();
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < M; e += blockDim.x) {
        const size_t idx = (size_t)(e / k_in) * list_stride + (size_t)qi * query_stride + (e % k_in);
        const uint64_t r = rows[idx];
        if (r == 0xFFFFFFFFFFFFFFFFull) continue;
        const double d = dist[idx];
        uint32_t rank = 0;
        for (uint32_t f = 0; f < M; ++f) {
            const size_t jdx = (size_t)(f / k_in) * list_stride + (size_t)qi * query_stride + (f % k_in);
            const uint64_t rf = rows[jdx];
            if (rf == 0xFFFFFFFFFFFFFFFFull) continue;
            const double df = dist[jdx];
            if (df < d || (df == d && rf < r)) ++rank;
        }
        if (rank < k_out) { orow[rank] = r; odist[rank] = d; }
    }
}

// The same merge over lists that are NOT gathered: list l starts at src.list[l] -- for a one-process group the exchange buffer of
// rank l, read IN PLACE over xGMI (peer access) or on this device (logical ranks).  Nothing is copied between the ranks: the
// exchange is this kernel's loads (n_lists x k_in x 16 B per query -- 1280 B at 8 ranks, k = 10: latency-bound), ordered
// after the ranks' select kernels by one stream event per rank (group_exchange.cpp: peer transport).  The candidates are staged in LDS once
// (16 B each, M <= 4096) so that the M x M rank computation never goes back over the links.
__global__ void merge_topk_sources_kernel(MergeSources src, uint32_t n_lists, uint64_t query_stride, uint32_t k_in, uint32_t k_out,
                                          uint64_t *out_rows, double *out_dist, uint64_t out_query_stride)
{
    extern __shared__ unsigned char smem_raw[];
    uint64_t *s_row = reinterpret_cast<uint64_t *>(smem_raw);
    const uint32_t qi = blockIdx.x;
    const uint32_t M = n_lists * k_in;
    double *s_dist = reinterpret_cast<double *>(s_row + M);
    uint64_t *orow = out_rows + (size_t)qi * out_query_stride;
    double *odist = out_dist + (size_t)qi * out_query_stride;
    for (uint32_t t = threadIdx.x; t < k_out; t += blockDim.x) {
        orow[t] = 0xFFFFFFFFFFFFFFFFull;
        odist[t] = __builtin_inf();
    }
    for (uint32_t e = threadIdx.x; e < M; e += blockDim.x) {
        const uint64_t *l = src.list[e / k_in] + (size_t)qi * query_stride;
        const uint32_t i = e % k_in;
        s_row[e] = l[i];
        s_dist[e] = reinterpret_cast<const double *>(l + k_in)[i];
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < M; e += blockDim.x) {
        const uint64_t r = s_row[e];
        if (r == 0xFFFFFFFFFFFFFFFFull) continue;
        const double d = s_dist[e];
        uint32_t rank = 0;
        for (uint32_t f = 0; f < M; ++f) {
            const uint64_t rf = s_row[f];
            if (rf == 0xFFFFFFFFFFFFFFFFull) continue;
            const double df = s_dist[f];
            if (df < d || (df == d && rf < r)) ++rank;
        }
        if (rank < k_out) { orow[rank] = r; odist[rank] = d; }
    }
}

int launch_merge_topk(smt_ctx *ctx, const uint64_t *rows, const double *dist, uint32_t n_lists,
                      uint32_t nq, uint32_t k_in, uint32_t k_out, uint64_t *out_rows, double *out_dist)
{
    SMT_REQUIRE((uint64_t)n_lists * k_in <= 8192, "device merge handles up to 8192 candidates per query");
    hipLaunchKernelGGL(merge_topk_kernel, dim3(nq), dim3(256), 0, ctx->stream, rows, dist, n_lists, (uint64_t)nq * k_in,
                       (uint64_t)k_in, k_in, k_out, out_rows, out_dist, (uint64_t)k_out);
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

// Packed lists [n_lists][nq][2][k_in] (list_stride_words apart: the exchange buffers of group_exchange.cpp carry a few status
// words behind each rank's lists; 0 = dense) -> out_packed [nq][2][k_out], on stream `st`.  n_lists == 0 writes padding.
int launch_merge_topk_packed_on(smt_ctx *ctx, hipStream_t st, const uint64_t *packed, uint32_t n_lists, uint32_t nq, uint32_t k_in,
                                uint32_t k_out, uint64_t *out_packed, uint64_t list_stride_words)
{
    (void)ctx;
    SMT_REQUIRE((uint64_t)n_lists * k_in <= 8192, "device merge handles up to 8192 candidates per query");
    const uint64_t ls = list_stride_words ? list_stride_words : (uint64_t)nq * 2 * k_in;
    hipLaunchKernelGGL(merge_topk_kernel, dim3(nq), dim3(256), 0, st, packed, reinterpret_cast<const double *>(packed + k_in),
                       n_lists, ls, (uint64_t)2 * k_in, k_in, k_out, out_packed, reinterpret_cast<double *>(out_packed + k_out),
                       (uint64_t)2 * k_out);
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

// Packed lists [nq][2][k_in], one per source pointer (see merge_topk_sources_kernel) -> out_packed [nq][2][k_out] on stream `st`.
int launch_merge_topk_sources_on(hipStream_t st, const MergeSources &src, uint32_t n_lists, uint32_t nq, uint32_t k_in, uint32_t k_out,
                                 uint64_t *out_packed)
{
    SMT_REQUIRE(n_lists >= 1 && n_lists <= SMT_MAX_MERGE_SOURCES, "1..64 lists are merged in place");
    SMT_REQUIRE((uint64_t)n_lists * k_in <= 8192, "the in-place merge stages up to 8192 candidates per query");
    const size_t smem = (size_t)n_lists * k_in * 16;
    if (smem > 64 * 1024) {   // more than 4096 candidates (large k: up to 8 x 1024): 128 KiB of LDS, allowed once per device
        static bool big[64] = {};
        int dev = 0;
        SMT_HIP_CHECK(hipGetDevice(&dev));
        if (dev < 0 || dev >= 64) return SMT_E_INVALID;
        if (!big[dev]) {
            SMT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(merge_topk_sources_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                              8192 * 16));
            big[dev] = true;
        }
    }
    hipLaunchKernelGGL(merge_topk_sources_kernel, dim3(nq), dim3(256), smem, st, src, n_lists, (uint64_t)2 * k_in, k_in, k_out, out_packed,
                       reinterpret_cast<double *>(out_packed + k_out), (uint64_t)2 * k_out);
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

__global__ void combine_status_kernel(MergeSources src, const uint64_t *base, uint64_t stride_words, uint32_t n, uint32_t nq, uint32_t *out)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    uint64_t worst = 0;
    for (uint32_t j = 0; j < n; ++j) {
        const uint64_t v = base ? base[(size_t)j * stride_words + q] : src.list[j][q];
        worst = v > worst ? v : worst;
    }
    out[q] = (uint32_t)worst;
}

int launch_combine_status_on(hipStream_t st, const MergeSources *src, const uint64_t *base, uint64_t stride_words, uint32_t n, uint32_t nq,
                             uint32_t *out)
{
    SMT_REQUIRE((src != nullptr) != (base != nullptr), "status sources: pointers or a strided buffer");
    SMT_REQUIRE(src == nullptr || n <= SMT_MAX_MERGE_SOURCES, "1..64 status sources are read in place");
    if (nq == 0) return SMT_OK;
    MergeSources none{};
    hipLaunchKernelGGL(combine_status_kernel, dim3((nq + 255) / 256), dim3(256), 0, st, src ? *src : none, base, stride_words, n, nq, out);
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

int launch_merge_topk_packed(smt_ctx *ctx, const uint64_t *packed, uint32_t n_lists, uint32_t nq, uint32_t k_in,
                             uint32_t k_out, uint64_t *out_packed)
{
    // async pipeline: the merge follows the select it consumes on the aux stream (tuning key merge_on_aux)
    const bool on_aux = ctx->tune.merge_on_aux && ctx->aux_stream != nullptr;
    hipStream_t st = on_aux ? ctx->aux_stream : ctx->stream;  // (ctx->stream may itself be the null stream)
    if (on_aux) ctx->async_pending = true;
    return launch_merge_topk_packed_on(ctx, st, packed, n_lists, nq, k_in, k_out, out_packed, 0);
}

}  // namespace smt
