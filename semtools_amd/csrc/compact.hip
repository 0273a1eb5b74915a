// compact.hip -- drop dead rows of a corpus IN PLACE (smt_corpus_compact): keep a sorted, disjoint list of row ranges and close
// the gaps between them, so that virtual row v of the concatenated list ends at physical row v.  No reference counterpart as a
// function (qdrant's optimiser vacuums deleted points behind src/workspace/store.rs); the caller it serves is the workspace
// store's compaction (host/store.cpp compact_if_sparse), which until now carried every live row to the host and back.
//
// The source of v is src(v) >= v and src(v) - v never decreases: every row moves DOWN, rows before the first gap stay.  A single
// launch that reads and writes the same buffer would need blocks to wait for one another (a block may write what a later block
// still has to read).  No block of this kernel waits for anything: the HOST cuts the move into steps whose launches cannot
// overwrite their own sources, and order between steps comes from launch order on the context's stream alone.
//   v = next virtual row, delta = src(v) - v, B = bounce rows (tuning key compact_bounce_rows).
//   delta >= B  DIRECT step: one launch gathers W = min(delta, new_rows - v) rows to [v, v + W).  The destination ends at or below
//               src(v), the lowest source of the launch: nothing in the launch reads what the launch writes.
//   delta <  B  BOUNCED step: W = min(B, new_rows - v) rows are gathered into the bounce buffer (context scratch), then copied
//               to [v, v + W) -- two enqueues.
// Every step but the last advances at least B rows: at most 2 * ceil(new_rows / B) enqueues whatever the gap pattern.
//
// compact_gather_kernel: one wave moves one 1 KiB row per instruction (64 lanes x f32x4); a wave takes CP_RUN consecutive virtual
// rows, finds the range of the first by binary search in the prefix table (topk_large.hip lk_map_virtual, with 64-bit rows) and
// walks forward from there.  CP_UNROLL independent row loads are in flight before the first store (16 data VGPRs: a gather of
// whole 1 KiB rows reads at the chip's rate with 4 rows per wave and 16 waves per CU in flight); loads and stores are
// non-temporal -- nothing is read twice.  No LDS, no atomics, no inline assembly.
#include <algorithm>

#include "common.h"
#include "device_utils.h"

namespace smt {

namespace {

constexpr int CP_THREADS = 256;   // 4 waves
constexpr int CP_UNROLL = 4;      // rows in flight per wave
constexpr int CP_RUN = 16;        // consecutive virtual rows per wave: one binary search per 16 KiB moved
constexpr uint64_t CP_MAX_LAUNCH_ROWS = (uint64_t)1 << 30;   // (keeps the grid inside 32 bits; a longer direct step takes two launches)

struct CompactParams {
    const float *src;         // the corpus rows
    float *dst;               // where virtual row v0 goes: inside the corpus (direct step) or the bounce buffer
    const smt_range *ranges;  // device: the non-empty kept ranges
    const uint64_t *prefix;   // device: exclusive prefix of their lengths [n_ranges + 1]
    uint32_t n_ranges;
    uint64_t v0;              // first virtual row of the launch
    uint64_t n;               // rows of the launch; v0 + n <= prefix[n_ranges]
};

__global__ void __launch_bounds__(CP_THREADS) compact_gather_kernel(CompactParams p)
{
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint64_t i = ((uint64_t)blockIdx.x * (CP_THREADS / 64) + wave) * CP_RUN;
    if (i >= p.n) return;
    const uint64_t end = i + CP_RUN < p.n ? i + CP_RUN : p.n;
    // the last range whose prefix is <= the run's first virtual row
    uint32_t lo = 0, hi = p.n_ranges;
    {
        const uint64_t v = p.v0 + i;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (p.prefix[mid] <= v) lo = mid; else hi = mid;
        }
    }
    uint32_t ri = lo;
    uint64_t begin = p.ranges[ri].begin, pb = p.prefix[ri], pe = p.prefix[ri + 1];
    // (v < prefix[n_ranges] and no range is empty: the walk ends inside the table)
    auto source = [&](uint64_t v) -> const f32x4 * {
        while (v >= pe) { ++ri; begin = p.ranges[ri].begin; pb = pe; pe = p.prefix[ri + 1]; }
        return reinterpret_cast<const f32x4 *>(p.src + (begin + (v - pb)) * 256) + lane;
    };
    for (; i + CP_UNROLL <= end; i += CP_UNROLL) {
        const f32x4 *s[CP_UNROLL];
        f32x4 c[CP_UNROLL];
#pragma unroll
        for (int j = 0; j < CP_UNROLL; ++j) s[j] = source(p.v0 + i + j);
#pragma unroll
        for (int j = 0; j < CP_UNROLL; ++j) c[j] = __builtin_nontemporal_load(s[j]);
#pragma unroll
        for (int j = 0; j < CP_UNROLL; ++j) __builtin_nontemporal_store(c[j], reinterpret_cast<f32x4 *>(p.dst + (i + j) * 256) + lane);
    }
    for (; i < end; ++i) {   // (the last wave of a launch)
        const f32x4 c = __builtin_nontemporal_load(source(p.v0 + i));
        __builtin_nontemporal_store(c, reinterpret_cast<f32x4 *>(p.dst + i * 256) + lane);
    }
}

struct Step { uint64_t v, n; bool bounced; };

}  // namespace

int corpus_compact_plan(const smt_corpus *c, const smt_range *keep, uint32_t n_keep, CompactPlan &plan)
{
    SMT_REQUIRE(c != nullptr, "corpus");
    SMT_REQUIRE(keep || n_keep == 0, "keep");
    if (!c->owned) { set_error("smt_corpus_compact: a corpus adopted from device memory is the caller's to rearrange"); return SMT_E_UNSUPPORTED; }
    // validate, drop empty ranges, prefix; first_moved = the first virtual row whose source is not itself
    std::vector<smt_range> &rr = plan.ranges;
    std::vector<uint64_t> &prefix = plan.prefix;
    rr.clear();
    prefix.assign(1, 0);
    uint64_t prev_end = 0, new_rows = 0, first_moved = 0;
    bool gap = false;
    for (uint32_t k = 0; k < n_keep; ++k) {
        const uint64_t b = keep[k].begin, e = keep[k].end;
        SMT_REQUIRE(b <= e, "range begin > end");
        SMT_REQUIRE(e <= c->rows, "range extends past the corpus");
        SMT_REQUIRE(k == 0 || b >= prev_end, "ranges must be sorted and disjoint");
        prev_end = e;
        if (e == b) continue;
        if (!gap && b != new_rows) { gap = true; first_moved = new_rows; }
        rr.push_back(keep[k]);
        new_rows += e - b;
        prefix.push_back(new_rows);
    }
    if (!gap) first_moved = new_rows;
    plan.new_rows = new_rows;
    plan.first_moved = first_moved;
    return SMT_OK;
}

int corpus_compact(smt_corpus *c, const smt_range *keep, uint32_t n_keep, uint64_t *rows_moved)
{
    if (rows_moved) *rows_moved = 0;
    CompactPlan plan;
    int rc = corpus_compact_plan(c, keep, n_keep, plan);
    if (rc) return rc;
    return corpus_compact_run(c, plan, rows_moved);
}

int corpus_compact_run(smt_corpus *c, const CompactPlan &plan, uint64_t *rows_moved)
{
    if (rows_moved) *rows_moved = 0;
    const std::vector<smt_range> &rr = plan.ranges;
    const std::vector<uint64_t> &prefix = plan.prefix;
    const uint64_t new_rows = plan.new_rows, first_moved = plan.first_moved;
    smt_ctx *ctx = c->ctx;
    // a list that drops nothing covers [0, rows): no row moves, nothing is enqueued (and an index built on the corpus stays valid)
    if (new_rows == c->rows) { ++ctx->compact_calls; return SMT_OK; }
    // Ordered after everything already enqueued: bind_device waits for the one-query pipelines (their scans run on the two scan
    // streams, their selects there or on the aux stream); the context's own stream orders the rest.  Scans enqueued later start
    // behind an event on that stream, so they see the compacted rows.
    int rc = bind_device(ctx);
    if (rc) return rc;
    corpus_writer_drain(c);   // (a write-ahead job reads the rows where they are)
    const uint64_t moved = new_rows - first_moved;
    if (moved) {
        const uint64_t B = (uint64_t)std::max<int64_t>(64, ctx->tune.compact_bounce_rows);
        std::vector<Step> steps;
        bool any_bounced = false;
        {
            size_t ri = 0;
            for (uint64_t v = first_moved; v < new_rows;) {
                while (v >= prefix[ri + 1]) ++ri;
                const uint64_t delta = rr[ri].begin + (v - prefix[ri]) - v;
                Step s;
                s.v = v;
                s.bounced = delta < B;
                s.n = std::min(s.bounced ? B : std::min(delta, CP_MAX_LAUNCH_ROWS), new_rows - v);
                any_bounced |= s.bounced;
                steps.push_back(s);
                v += s.n;
            }
        }
        // one scratch block: [ranges | prefix | bounce]; the tables are staged ONCE per call, from pinned memory
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t nr = rr.size(), r_bytes = al(nr * sizeof(smt_range)), p_bytes = al((nr + 1) * sizeof(uint64_t));
        const size_t bounce_rows = any_bounced ? (size_t)std::min(B, moved) : 0;
        if ((rc = ensure_scratch(ctx, r_bytes + p_bytes + bounce_rows * 256 * sizeof(float)))) return rc;
        if ((rc = ensure_pinned_in(ctx, r_bytes + p_bytes))) return rc;
        char *pin = reinterpret_cast<char *>(ctx->h_pinned_in), *dev = reinterpret_cast<char *>(ctx->d_scratch);
        memcpy(pin, rr.data(), nr * sizeof(smt_range));
        memcpy(pin + r_bytes, prefix.data(), (nr + 1) * sizeof(uint64_t));
        SMT_HIP_CHECK(hipMemcpyAsync(dev, pin, r_bytes + p_bytes, hipMemcpyHostToDevice, ctx->stream));
        SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // (h_pinned_in is the next search's: the upload must have left it; the move itself is not waited for)
        float *bounce = reinterpret_cast<float *>(dev + r_bytes + p_bytes);
        CompactParams p;
        p.src = c->d_rows;
        p.ranges = reinterpret_cast<const smt_range *>(dev);
        p.prefix = reinterpret_cast<const uint64_t *>(dev + r_bytes);
        p.n_ranges = (uint32_t)nr;
        prof_begin(ctx, "compact");
        for (const Step &s : steps) {
            p.v0 = s.v;
            p.n = s.n;
            p.dst = s.bounced ? bounce : c->d_rows + (size_t)s.v * 256;
            const uint64_t rows_per_block = (uint64_t)(CP_THREADS / 64) * CP_RUN;
            hipLaunchKernelGGL(compact_gather_kernel, dim3((unsigned)((s.n + rows_per_block - 1) / rows_per_block)), dim3(CP_THREADS), 0,
                               ctx->stream, p);
            SMT_HIP_CHECK(hipGetLastError());
            if (s.bounced)
                SMT_HIP_CHECK(hipMemcpyAsync(c->d_rows + (size_t)s.v * 256, bounce, (size_t)s.n * 256 * sizeof(float),
                                             hipMemcpyDeviceToDevice, ctx->stream));
        }
        prof_end(ctx, "compact");
    }
    c->rows = new_rows;
    c->image_rows = std::min<uint64_t>(c->image_rows, first_moved / 32 * 32);   // derived data: corpus_image_sync packs the rest again
    ++ctx->compact_calls;
    ctx->compact_rows_moved += moved;
    if (rows_moved) *rows_moved = moved;
    return SMT_OK;
}

}  // namespace smt
