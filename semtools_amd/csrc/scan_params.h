// scan_params.h -- K2 (single/few-query cosine scan + per-wave top-k'): what its kernels have in common.  ScanParams, the start
// gate, and the row fetch of the grouped kernels.  The kernels: scan_topk_kernel (scan_topk.hip), and the grouped scan_pair_kernel
// (up to four calls per pass, scan_pair.hip), scan_wide_kernel (up to eight, scan_wide.hip) and scan_deep_kernel (up to sixteen,
// scan_deep.hip) with their host/device pairing protocol (scan_group.h).  launch_scan_topk (scan_launch.hip) runs the passes of a
// call and hands the block lists to the select stage (select.hip; optionally overlapped with the next scan: async
// select).  The chunk table of range-filtered scans is built in range_tables.hip, the cross-shard top-k merge
// lives in merge.hip, K4 (threshold mode) in threshold.hip.
// gfx950 only (wave64, DPP, 16 B/lane row loads).
//
// Replaces the `for doc / for line: f32::cosine(q, e)` loop and the
// sort/take of search_documents (reference src/search/mod.rs:84-119) and the
// exact filtered scan behind Store::search_line_embeddings
// (src/workspace/store.rs:481-546).
//
// Data layout: corpus row-major f32 [rows x 256]; one row = 1024 B = one
// wave-wide 16 B/lane load (perfectly coalesced).  A wave owns U rows per
// iteration (U independent 1 KiB loads in flight), reduces ab = <q,c> and
// b2 = <c,c> with DPP butterflies, and keeps its best k' candidates in a
// lane-distributed sorted list (lane i = i-th best).  The f32 scan only
// NOMINATES candidates: the merge stage recomputes the distance of the final
// k' rows with f64 accumulation in index order (simsimd "accurate" formula),
// so returned distances/ordering do not depend on the reduction tree.
#pragma once
#include "common.h"
#include "device_utils.h"
#include "device_flags.h"
#include "chunk_deal.h"

namespace smt {

struct ScanParams {
    const float *corpus;
    const float *queries;  // [NQ x 256] (device)
    uint64_t n_virtual;    // unfiltered: rows to scan
    const uint64_t *chunk_table;  // FILTERED: one descriptor per chunk (row0 | valid rows << 32), see build_chunk_table_kernel
    uint64_t n_chunks;     // chunks to scan (FILTERED: table entries; else ceil(n_virtual / U))
    uint32_t kp;           // candidates kept per wave / per block (<= 64)
    uint32_t nq_active;    // queries of this pass that exist (<= NQ): a pass of 3 runs the 4-query kernel, slot 3 repeats query 0 and writes no list
    key_t64 *block_lists;  // [NQ][gridDim.x][kp]
    unsigned long long *stamps;  // optional (tuning key scan_debug_ptr): wall_clock64 per wave [start, loop end], per block [end]
    unsigned long long *flags;   // async select (or nullptr): [0] scan_done step, [1] select_done step, [2] blocks done, [3] timeout
    unsigned long long step;     // this launch's step number (>= 1)
    unsigned int *steal_ctr;     // STEAL: this launch's group counter (zero at launch), see scan_topk_kernel
    uint32_t steal_lr;           // STEAL: log2 of the rounds per group
    uint32_t steal_static;       // STEAL: a block's first steal_static groups are dealt statically (group g of block b = g * blocks + b)
    // START GATE (tuning keys scan_overlap, scan_gate_pct; nullptr = none): consecutive one-query scans run on two streams and overlap.
    // Every block adds 1 to *gate once its waves have finished their rows (a block of scan_pair_kernel: the number of calls its pass
    // serves; an absorbed launch nothing: the counter counts calls served, in blocks), and thread 0 of every block waits, before any row load,
    // until *gate >= gate_open -- the predecessor scan has finished scan_gate_pct per cent of its blocks' rows -- or gate_ticks of the
    // 100 MHz wall clock have passed.  The counter only grows (the host keeps the running total), so a later launch reads as "open"
    // too.  Advisory: it orders no data (list buffers and selects meet in stream order), so it can cost time, never an answer.
    unsigned long long *gate;
    unsigned long long gate_open;   // 0: no wait
    unsigned long long gate_ticks;
};

__device__ __forceinline__ void gate_wait(const ScanParams &p)
{
    if (flag_load(p.gate) >= p.gate_open) return;
    const unsigned long long t0 = wall_clock64();
    while (flag_load(p.gate) < p.gate_open && wall_clock64() - t0 < p.gate_ticks) __builtin_amdgcn_s_sleep(8);
}

// ------------------------------------------------- the row fetch of the grouped kernels (unfiltered, four rows per chunk)
// Is row v a row of the corpus?
// (row numbers are far below 2^63: the sign of the difference is a scalar compare, where "<" on 64 bits takes the VALU and a
// vector register pair for n_virtual -- these kernels have none to spare)
// (... and the sign is asked of the high word behind an empty asm: the compiler folds "high word < 0" back into a 64-bit signed
// compare, for which the scalar unit has no instruction -- a v_cmp_lt_i64 of two scalar values, three times per chunk)
__device__ __forceinline__ bool rows_in_corpus(const ScanParams &p, uint64_t v)
{
    uint32_t hi = (uint32_t)((v - p.n_virtual) >> 32);
    asm("" : "+s"(hi));
    return (int32_t)hi < 0;
}
// A chunk's rows are 1024 B apart and the load's immediate offset reaches 3072: a full chunk is ONE wave-uniform base address
// in scalar registers, the lane's 16 B offset and four immediates -- no vector instruction.  Only the chunk that crosses
// n_virtual clamps its rows one by one.  (The base passes through an empty asm: otherwise the compiler regroups the sum as
// (corpus + 16 lane) + row offset, hoists the bracket into a vector register pair and adds the rest on the VALU, per row.  The
// ragged chunk's rows pass through one too: loads of the same kind on both sides of a branch are joined behind it, and the
// joined load is back at one address per row.)
// (the global address space by name: a pointer made from an integer is a generic one, and its loads flat_load)
typedef const f32x4 __attribute__((address_space(1))) *global_rows_ptr;
__device__ __forceinline__ global_rows_ptr rows_ptr(const ScanParams &p, uint64_t v, int lane)
{
    uint64_t base = (uint64_t)(uintptr_t)p.corpus + v * 1024u;
    asm volatile("" : "+s"(base));
    return (global_rows_ptr)(uintptr_t)base + lane;
}
template <bool NT, int U>
__device__ __forceinline__ void rows_issue(const ScanParams &p, uint64_t v0, f32x4 (&c)[U], int lane)
{
    if (rows_in_corpus(p, v0 + (U - 1))) {   // (uniform)
        const global_rows_ptr src = rows_ptr(p, v0, lane);
#pragma unroll
        for (int j = 0; j < U; ++j) c[j] = NT ? __builtin_nontemporal_load(src + 64 * j) : src[64 * j];
    } else {
#pragma unroll
        for (int j = 0; j < U; ++j) {
            uint64_t v = v0 + j;
            if (!rows_in_corpus(p, v)) v = p.n_virtual - 1;  // clamp (result discarded)
            const global_rows_ptr src = rows_ptr(p, (uint64_t)(uint32_t)v, lane);
            c[j] = NT ? __builtin_nontemporal_load(src) : *src;
            asm volatile("" : "+v"(c[j]));
        }
    }
}

// One pass of scan_topk_kernel (scan_topk.hip): `slots` query slots (1, 2, 4), of which p.nq_active hold a query, over chunks of U
// rows.  Enqueues only: the caller asks hipGetLastError.
void launch_scan_topk_kernel(int slots, int U, bool nt, bool filtered, int blocks, int threads, hipStream_t st, const ScanParams &p);

}  // namespace smt
