// ivfpq_compact.hip -- carry an IVF index through an in-place compaction of its corpus (smt_ivfpq_compact): instead of a rebuild
// (k-means, quantiser fit, encode, sort) one stable stream compaction over the index's 36-byte entries plus an id remap.  No
// reference counterpart (the reference's store has no index; ivfpq.h).
//
// What the index holds per row is a 4-byte position (ids) and a 32-byte code, both in LIST order; centroids, codebooks, per-list
// bases and scales do not depend on where a row sits and the code of a kept row does not change.  The keep list maps old rows to
// new rows monotonically (old row keep[i].begin + j -> prefix[i] + j), so dropping the dead entries and renaming the kept ones
// leaves every list ascending by row.  The update is OUT OF PLACE into fresh ids / codes / offsets sized for the kept count -- the
// idiom of smt_ivfpq_append: 36 B per kept row in transit, and the dropped entries' memory is given back.  Four kernels, all on the
// context's stream, no atomics anywhere (the result is deterministic); p = a list position < n_old, word w = positions [64 w, 64 w + 64):
//   (a) ivf_compact_mark_kernel   one lane per p: a coalesced load of ids[p], a binary search of the sorted kept ranges (staged in LDS
//       with their prefixes up to 1024 ranges, read from global memory beyond: ivf_range_mask_kernel's border), alive bit and P(id).
//       One ballot per wave IS one word of the alive bitmap, stored by one lane; a block of 4 waves x 16 words also leaves the number
//       of alive positions among its 4096.  P(id) of an alive lane goes to a 4 B per entry temporary.
//   (b) ivf_compact_scan_kernel   ONE block: exclusive prefix of the per-block counts (n_old / 4096 numbers: 2441 at 10 M rows);
//       ivf_compact_offsets_kernel: new offsets[l] = rank(old offsets[l]) = the block prefix + the popcounts of at most 63 words
//       + the partial word in front of the offset, one lane per list.
//   (c) ivf_compact_move_kernel   a block takes the 64 words (a) counted together: every wave loads them, one per lane, and a wave
//       prefix over their popcounts gives each word's first destination.  A word's kept entries land in ONE contiguous run:
//       the alive lane with r alive lanes below it stores its id at run + r (a coalesced, compacted store); the 2 x popcount
//       16-byte halves of the kept codes are dealt to the lanes in destination order -- lane pairs, both sides 16-byte accesses, the
//       stores contiguous over the wave -- and the source position of the e-th kept entry is the e-th set bit of the word, found
//       from the ballot word itself (six popcount steps in registers: wave-uniform data, so neither LDS nor ds_bpermute is needed).
//       Dead positions load no code bytes.  Destinations are checked against the kept count the HOST derived from the list: an
//       index that names a row twice cannot write past the new arrays (the host then finds offsets[nlist] off and refuses it).
// The remapped ids go through the temporary instead of being recomputed in (c): (c) then needs no range table and no LDS at all,
// the binary search runs once per entry, and the price is 8 B of coalesced traffic per entry beside the 72 B of a kept code's trip.
// Launch bounds: grids are sized from n_old and nlist only; every position is 64-bit arithmetic (n_old may exceed 2^31; a shard
// holds fewer than 2^32 - 1 rows, so the ids themselves stay 32-bit).
#include "ivfpq.h"

using namespace smt;

namespace smt {

constexpr int IC_THREADS = 256;                   // 4 waves
constexpr int IC_WORDS_PER_WAVE = 16;
constexpr int IC_BLOCK_WORDS = (IC_THREADS / 64) * IC_WORDS_PER_WAVE;   // 64 words = 4096 positions per block, in (a) and (c)
constexpr uint32_t IC_LDS_RANGES = 1024;          // 16 KiB of ranges + 8 KiB of prefixes
constexpr int IC_SCAN_THREADS = 1024;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// P(row) if the row lies in a kept range, else ~0: the last range with begin <= row is the only one that can hold it
template <typename R, typename P>
__device__ __forceinline__ uint32_t ic_remap(const R *r, const P *prefix, uint32_t n_ranges, uint64_t row)
{
    uint32_t lo = 0, hi = n_ranges;   // #(begin <= row) lies in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (r[mid].begin <= row) lo = mid + 1; else hi = mid;
    }
    if (lo == 0 || row >= r[lo - 1].end) return 0xFFFFFFFFu;
    return (uint32_t)(prefix[lo - 1] + (row - r[lo - 1].begin));
}

__global__ void __launch_bounds__(IC_THREADS) ivf_compact_mark_kernel(const uint32_t *ids, uint64_t n_old, const smt_range *ranges,
                                                                       const uint64_t *prefix, uint32_t n_ranges, uint64_t *mask,
                                                                       uint32_t *new_ids, uint32_t *block_count)
{
    __shared__ smt_range s_ranges[IC_LDS_RANGES];
    __shared__ uint64_t s_prefix[IC_LDS_RANGES];
    __shared__ uint32_t s_count[IC_THREADS / 64];
    const bool staged = n_ranges <= IC_LDS_RANGES;   // block-uniform
    if (staged) {
        for (uint32_t e = threadIdx.x; e < n_ranges; e += IC_THREADS) { s_ranges[e] = ranges[e]; s_prefix[e] = prefix[e]; }
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t n_words = (n_old + 63) >> 6;
    const uint64_t w0 = (uint64_t)blockIdx.x * IC_BLOCK_WORDS + (uint64_t)wave * IC_WORDS_PER_WAVE;
    uint32_t count = 0;
    for (int u = 0; u < IC_WORDS_PER_WAVE; ++u) {
        const uint64_t w = w0 + u;
        if (w >= n_words) break;   // wave-uniform
        const uint64_t p = w * 64 + lane;
        uint32_t to = 0xFFFFFFFFu;
        if (p < n_old) {
            const uint64_t row = ids[p];
            to = staged ? ic_remap(s_ranges, s_prefix, n_ranges, row) : ic_remap(ranges, prefix, n_ranges, row);
        }
        const bool alive = to != 0xFFFFFFFFu;
        const unsigned long long word = __ballot(alive);
        if (alive) new_ids[p] = to;
        if (lane == 0) mask[w] = word;
        count += (uint32_t)__popcll(word);
    }
    if (lane == 0) s_count[wave] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (int i = 0; i < IC_THREADS / 64; ++i) sum += s_count[i];
        block_count[blockIdx.x] = sum;
    }
}

// ONE block: block_prefix[b] = alive positions in front of block b of (a), block_prefix[n_blocks] = all of them
__global__ void __launch_bounds__(IC_SCAN_THREADS) ivf_compact_scan_kernel(const uint32_t *block_count, uint64_t n_blocks, uint64_t *block_prefix)
{
    __shared__ uint32_t s_wave[IC_SCAN_THREADS / 64];
    const int lane = threadIdx.x & 63;
    const uint32_t wave = threadIdx.x >> 6;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n_blocks; base += IC_SCAN_THREADS) {   // block-uniform
        const uint64_t i = base + threadIdx.x;
        const uint32_t v = i < n_blocks ? block_count[i] : 0u;
        uint32_t incl = v;   // (a chunk sums to at most 1024 x 4096)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t k = 0; k < IC_SCAN_THREADS / 64; ++k) {
            const uint32_t t = s_wave[k];
            before += k < wave ? t : 0u;
            total += t;
        }
        if (i < n_blocks) block_prefix[i] = carry + before + (incl - v);
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) block_prefix[n_blocks] = carry;
}

// new_off[l] = alive positions in front of old_off[l], l = 0 .. nlist (old_off[nlist] = n_old: the kept count)
__global__ void __launch_bounds__(256) ivf_compact_offsets_kernel(const uint64_t *old_off, uint32_t nlist, const uint64_t *mask,
                                                                   const uint64_t *block_prefix, uint64_t *new_off)
{
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l > nlist) return;
    const uint64_t o = old_off[l];
    const uint64_t blk = o / (64 * IC_BLOCK_WORDS), w_end = o >> 6;
    uint64_t r = block_prefix[blk];
    for (uint64_t w = blk * IC_BLOCK_WORDS; w < w_end; ++w) r += (uint64_t)__popcll(mask[w]);   // (at most 63 words, all < n_words)
    const uint32_t bit = (uint32_t)(o & 63);
    if (bit) r += (uint64_t)__popcll(mask[w_end] & ((1ull << bit) - 1));   // (bit != 0: o < 64 n_words, the word exists)
    new_off[l] = r;
}

// the position (0 .. 63) of the e-th set bit of `word`, e < popcount(word)
__device__ __forceinline__ uint32_t ic_select_bit(uint64_t word, uint32_t e)
{
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t s = 32; s; s >>= 1) {
        const uint32_t c = (uint32_t)__popcll((word >> pos) & ((1ull << s) - 1));
        if (e >= c) { e -= c; pos += s; }
    }
    return pos;
}

__global__ void __launch_bounds__(IC_THREADS) ivf_compact_move_kernel(const uint64_t *mask, const uint64_t *block_prefix, uint64_t n_words,
                                                                       const uint32_t *new_ids, const u32x4 *codes, uint64_t n_out,
                                                                       uint32_t *out_ids, u32x4 *out_codes)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t w_block = (uint64_t)blockIdx.x * IC_BLOCK_WORDS;
    // the block's 64 words, one per lane, and the exclusive prefix of their popcounts (every wave computes the same)
    const uint64_t mine = w_block + lane < n_words ? mask[w_block + lane] : 0ull;
    const uint32_t c = (uint32_t)__popcll(mine);
    uint32_t incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if (lane >= (uint32_t)d) incl += up;
    }
    const uint32_t excl = incl - c;
    const uint64_t run0 = block_prefix[blockIdx.x];
    for (int u = 0; u < IC_WORDS_PER_WAVE; ++u) {
        const uint32_t wi = wave * IC_WORDS_PER_WAVE + u;
        const uint64_t w = w_block + wi;
        if (w >= n_words) return;   // wave-uniform
        const uint64_t word = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(mine >> 32), (int)wi) << 32) |
                              (uint64_t)(uint32_t)__shfl((int)(uint32_t)mine, (int)wi);
        if (word == 0) continue;   // wave-uniform
        const uint64_t run = run0 + (uint32_t)__shfl((int)excl, (int)wi);   // first destination of the word's kept entries
        const uint32_t cnt = (uint32_t)__popcll(word);
        const uint64_t p0 = w * 64;
        if ((word >> lane) & 1ull) {
            const uint32_t r = (uint32_t)__popcll(word & ((1ull << lane) - 1));
            if (run + r < n_out) out_ids[run + r] = new_ids[p0 + lane];
        }
        // 2 x cnt halves of 16 bytes in destination order: item t = half (t & 1) of kept entry t >> 1
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t t = lane + 64u * h, e = t >> 1;
            if (e < cnt && run + e < n_out) {
                const uint64_t src = p0 + ic_select_bit(word, e);
                const u32x4 v = __builtin_nontemporal_load(codes + src * 2 + (t & 1u));
                __builtin_nontemporal_store(v, out_codes + (run + e) * 2 + (t & 1u));
            }
        }
    }
}

int ivfpq_compact_check(const smt_ivfpq *ix, const smt_range *keep, uint32_t n_keep, CompactPlan &plan, uint64_t &n_new)
{
    SMT_REQUIRE(ix != nullptr, "index");
    IVF_REQUIRE_FRESH(ix);
    const smt_corpus *c = ix->corpus;
    SMT_REQUIRE(c->rows >= ix->n_rows, "the corpus shrank since the index was built: rebuild");
    int rc = corpus_compact_plan(c, keep, n_keep, plan);
    if (rc) return rc;
    n_new = 0;   // the kept rows below the rows the index covers
    for (const smt_range &r : plan.ranges) {
        if (r.begin >= ix->n_rows) break;
        n_new += std::min<uint64_t>(r.end, ix->n_rows) - r.begin;
    }
    if (n_new == 0 && ix->n_rows != 0) {
        set_error("smt_ivfpq_compact: the list keeps no row the index covers; compact the corpus alone and rebuild the index");
        return SMT_E_UNSUPPORTED;
    }
    return SMT_OK;
}

int ivfpq_compact_apply(smt_ivfpq *ix, const CompactPlan &plan, uint64_t n_new, uint64_t *rows_moved, uint64_t *entries_dropped)
{
    if (rows_moved) *rows_moved = 0;
    if (entries_dropped) *entries_dropped = 0;
    smt_corpus *c = ix->corpus;
    smt_ctx *ctx = c->ctx;
    const uint64_t n_old = ix->n_rows;
    // nothing dropped at all (no kernel, no allocation), or only rows the index does not cover yet: P is the identity below n_old
    if (plan.new_rows == c->rows || n_new == n_old) return corpus_compact_run(c, plan, rows_moved);
    IVF_HIP(hipSetDevice(ctx->device));
    { int rc_drain = drain_async(ctx); if (rc_drain) return rc_drain; }
    const uint32_t nlist = ix->nlist, n_ranges = (uint32_t)plan.ranges.size();
    const uint64_t n_words = (n_old + 63) / 64, n_blocks = (n_words + IC_BLOCK_WORDS - 1) / IC_BLOCK_WORDS;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    // temporaries: [ranges | prefix | mask | block counts | block prefix] and the remapped ids; then the index's new arrays
    const size_t o_r = 0, b_r = al((size_t)n_ranges * sizeof(smt_range));
    const size_t o_p = o_r + b_r, b_p = al((size_t)n_ranges * 8);
    const size_t o_m = o_p + b_p, b_m = al((size_t)n_words * 8);
    const size_t o_bc = o_m + b_m, b_bc = al((size_t)n_blocks * 4);
    const size_t o_bp = o_bc + b_bc, b_bp = al((size_t)(n_blocks + 1) * 8);
    IvfDevBuf b_tab, b_to, b_ids, b_codes, b_off;
    int rc;
    if ((rc = ivf_dev_alloc(b_tab, o_bp + b_bp)) || (rc = ivf_dev_alloc(b_to, (size_t)n_old * 4)) || (rc = ivf_dev_alloc(b_ids, (size_t)n_new * 4)) ||
        (rc = ivf_dev_alloc(b_codes, (size_t)n_new * PQ_M)) || (rc = ivf_dev_alloc(b_off, (size_t)(nlist + 1) * 8)))
        return rc;   // (nothing has moved: the index stays as it is)
    char *tab = b_tab.as<char>();
    // the keep ranges and their prefixes go up once (the host vectors live in `plan` until the stream has been waited for below)
    IVF_HIP(hipMemcpyAsync(tab + o_r, plan.ranges.data(), (size_t)n_ranges * sizeof(smt_range), hipMemcpyHostToDevice, ctx->stream));
    IVF_HIP(hipMemcpyAsync(tab + o_p, plan.prefix.data(), (size_t)n_ranges * 8, hipMemcpyHostToDevice, ctx->stream));
    const smt_range *d_ranges = reinterpret_cast<const smt_range *>(tab + o_r);
    const uint64_t *d_prefix = reinterpret_cast<const uint64_t *>(tab + o_p);
    uint64_t *d_mask = reinterpret_cast<uint64_t *>(tab + o_m), *d_bp = reinterpret_cast<uint64_t *>(tab + o_bp);
    uint32_t *d_bc = reinterpret_cast<uint32_t *>(tab + o_bc);
    prof_begin(ctx, "ivf_compact");
    hipLaunchKernelGGL(ivf_compact_mark_kernel, dim3((unsigned)n_blocks), dim3(IC_THREADS), 0, ctx->stream, ix->d_ids, n_old, d_ranges, d_prefix,
                       n_ranges, d_mask, b_to.as<uint32_t>(), d_bc);
    hipLaunchKernelGGL(ivf_compact_scan_kernel, dim3(1), dim3(IC_SCAN_THREADS), 0, ctx->stream, d_bc, n_blocks, d_bp);
    hipLaunchKernelGGL(ivf_compact_offsets_kernel, dim3((nlist + 1 + 255) / 256), dim3(256), 0, ctx->stream, ix->d_offsets, nlist, d_mask, d_bp,
                       b_off.as<uint64_t>());
    hipLaunchKernelGGL(ivf_compact_move_kernel, dim3((unsigned)n_blocks), dim3(IC_THREADS), 0, ctx->stream, d_mask, d_bp, n_words,
                       b_to.as<uint32_t>(), reinterpret_cast<const u32x4 *>(ix->d_codes), n_new, b_ids.as<uint32_t>(), b_codes.as<u32x4>());
    prof_end(ctx, "ivf_compact");
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {   // (the corpus has not moved)
        (void)hipStreamSynchronize(ctx->stream);
        set_error("carrying the index: %s", hipGetErrorString(e));
        return SMT_E_HIP;
    }
    // the rows, behind the index kernels on the same stream (they read nothing of the corpus)
    rc = corpus_compact_run(c, plan, rows_moved);
    e = hipStreamSynchronize(ctx->stream);   // earlier _device searches may still read the old arrays: they are freed behind this
    std::vector<uint64_t> off(nlist + 1);
    if (rc == SMT_OK && e == hipSuccess) e = hipMemcpy(off.data(), b_off.p, off.size() * 8, hipMemcpyDeviceToHost);
    if (rc != SMT_OK) {   // refused behind the validation (memory: no row moved) or a HIP error (the rows are anybody's guess)
        if (rc == SMT_E_HIP) ix->stale = true;
        return rc;
    }
    if (e != hipSuccess || off[nlist] != n_new) {   // the corpus HAS moved: the index no longer describes it
        ix->stale = true;
        if (e != hipSuccess) set_error("carrying the index: %s", hipGetErrorString(e));
        else set_error("carrying the index: %llu entries kept where the list keeps %llu rows (the index did not name every row once): rebuild",
                       (unsigned long long)off[nlist], (unsigned long long)n_new);
        return e != hipSuccess ? SMT_E_HIP : SMT_E_INVALID;
    }
    // (the old arrays leave with the buffers, behind the synchronise above)
    { void *t = ix->d_ids; ix->d_ids = b_ids.as<uint32_t>(); b_ids.p = t; }
    { void *t = ix->d_codes; ix->d_codes = b_codes.as<uint8_t>(); b_codes.p = t; }
    { void *t = ix->d_offsets; ix->d_offsets = b_off.as<uint64_t>(); b_off.p = t; }
    ix->n_rows = n_new;
    ix->max_list = 0;
    for (uint32_t l = 0; l < nlist; ++l) ix->max_list = std::max<uint64_t>(ix->max_list, off[l + 1] - off[l]);
    if (entries_dropped) *entries_dropped = n_old - n_new;
    return SMT_OK;
}

}  // namespace smt

extern "C" {

int smt_ivfpq_compact(smt_ivfpq *ix, const smt_range *keep, uint32_t n_keep, uint64_t *rows_moved, uint64_t *entries_dropped)
try {
    if (rows_moved) *rows_moved = 0;
    if (entries_dropped) *entries_dropped = 0;
    CompactPlan plan;
    uint64_t n_new = 0;
    int rc = ivfpq_compact_check(ix, keep, n_keep, plan, n_new);
    if (rc) return rc;
    return ivfpq_compact_apply(ix, plan, n_new, rows_moved, entries_dropped);
} catch (...) { return smt::api_catch(); }

}  // extern "C"
