// range_tables.hip -- the descriptor tables of range-filtered searches, built on the device from the sorted range list:
// one descriptor per FILTER_CHUNK-row chunk for the streaming kernels (K2, K4, the large-k collect, the LDS-row batched
// kernel) and one per aligned 32-row tile for the MFMA kernel (gemm_rowreg_kernel).
#include "common.h"
#include "device_utils.h"

namespace smt {

// Range filter (path-subset search, src/workspace/store.rs:507-515): the rows to scan are the concatenation
// of sorted, disjoint row ranges.  Each range is cut into chunks of FILTER_CHUNK rows (the last one short),
// and ONE descriptor per chunk says where it starts and how many of its rows are valid, so the streaming
// kernels never search the range list: they read descriptor c (a wave-uniform 8-byte load, requested one
// pipeline stage before the rows) and stream row0 .. row0+cnt-1.  2 B per scanned row of extra traffic.
// (The first version binary-searched the ranges per ROW inside the scan loop: 3 dependent scalar loads in
// front of every row load made a 2-range search of 1 M rows 3x slower than the unfiltered one.)
__global__ void build_chunk_table_kernel(const smt_range *ranges, const uint64_t *chunk_prefix, uint32_t n_ranges,
                                         uint64_t n_chunks, uint64_t *table)
{
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    uint32_t lo = 0, hi = n_ranges;  // invariant: chunk_prefix[lo] <= c < chunk_prefix[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (chunk_prefix[mid] <= c) lo = mid; else hi = mid;
    }
    const uint64_t row0 = ranges[lo].begin + (c - chunk_prefix[lo]) * FILTER_CHUNK;
    const uint64_t cnt = ranges[lo].end - row0 < (uint64_t)FILTER_CHUNK ? ranges[lo].end - row0 : (uint64_t)FILTER_CHUNK;
    table[c] = row0 | (cnt << 32);
}

int launch_build_chunk_table(smt_ctx *ctx, const smt_range *ranges, const uint64_t *chunk_prefix, uint32_t n_ranges,
                             uint64_t n_chunks, uint64_t *table)
{
    if (n_chunks == 0) return SMT_OK;
    hipLaunchKernelGGL(build_chunk_table_kernel, dim3((unsigned)((n_chunks + 255) / 256)), dim3(256), 0, ctx->stream, ranges,
                       chunk_prefix, n_ranges, n_chunks, table);
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

// The same filter for the MFMA kernel (gemm_rowreg_kernel), whose unit is the ALIGNED 32-row tile -- the unit of the corpus' fp16
// operand image: one descriptor per tile that holds at least one wanted row, tile index | row mask << 32.  Ranges that meet
// inside a tile share its descriptor (tile_prefix counts a tile for the first range that touches it: search.cpp stage_ranges),
// so no tile is read twice however small the documents are.
__global__ void build_tile_table_kernel(const smt_range *ranges, const uint64_t *tile_prefix, uint32_t n_ranges, uint64_t n_vtiles,
                                        uint64_t *table)
{
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_vtiles) return;
    uint32_t lo = 0, hi = n_ranges;  // first range i with tile_prefix[i + 1] > v (ranges that own no tile are skipped)
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tile_prefix[mid + 1] > v) hi = mid; else lo = mid + 1;
    }
    const uint32_t i = lo;
    const uint64_t first = ranges[i].begin >> 5;
    const bool shared = i > 0 && ((ranges[i - 1].end - 1) >> 5) == first;   // (empty ranges were dropped by the host)
    const uint64_t tile = first + (shared ? 1 : 0) + (v - tile_prefix[i]);
    const uint64_t t0 = tile << 5, t1 = t0 + 32;
    uint32_t mask = 0;
    for (uint32_t k = i; k < n_ranges && ranges[k].begin < t1; ++k) {
        const uint64_t b = ranges[k].begin > t0 ? ranges[k].begin : t0, e = ranges[k].end < t1 ? ranges[k].end : t1;
        if (e > b) mask |= (uint32_t)((~0ull >> (64 - (e - b))) << (b - t0));
    }
    table[v] = tile | ((uint64_t)mask << 32);
}

int launch_build_tile_table(smt_ctx *ctx, const smt_range *ranges, const uint64_t *tile_prefix, uint32_t n_ranges, uint64_t n_vtiles,
                            uint64_t *table)
{
    if (n_vtiles == 0) return SMT_OK;
    hipLaunchKernelGGL(build_tile_table_kernel, dim3((unsigned)((n_vtiles + 255) / 256)), dim3(256), 0, ctx->stream, ranges,
                       tile_prefix, n_ranges, n_vtiles, table);
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

}  // namespace smt
