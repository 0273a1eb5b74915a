// scan_launch.hip -- K2, host side: launch_scan_topk plans a call's passes, enters the one-query pipeline, publishes the grouped
// kernels' slots, launches the passes through the units that hold the kernels (scan_topk.hip, scan_pair.hip, scan_wide.hip,
// scan_deep.hip) and hands the block lists to the select stage (select.hip).
#include "scan_group.h"

namespace smt {

// ------------------------------------------------------------------ launchers
static inline uint32_t candidates_per_list(const smt_ctx *ctx, uint32_t k_out)
{
    // guard band: 8 extra f32 candidates so that f32-vs-f64 rank flips at the k-th boundary do not drop a true
    // top-k row; the select stage PROVES per query that the band was wide enough (SelectArgs::f32_err) and flags
    // the query otherwise.  k_out <= SCAN_MAX_K = 56, so the band never shrinks below 8; tuning key guard_band widens
    // it (lists hold at most 64 keys) for corpora with many near-duplicate lines -- every proof that succeeds saves
    // the exhaustive re-answer, at the price of a longer select (256 lists x k' keys).
    return std::min<uint32_t>(64, k_out + (uint32_t)ctx->tune.guard_band);
}

// host_timing (tuning key, off by default; tools/ab_select_group.py): clock_gettime around the runtime calls of a pipeline call,
// summed per kind in smt_ctx::host_ns
struct HostTimer {
    smt_ctx *ctx;
    bool on;
    timespec t;
    explicit HostTimer(smt_ctx *c) : ctx(c), on(c->tune.host_timing != 0)
    {
        if (on) clock_gettime(CLOCK_MONOTONIC, &t);
    }
    void lap(int kind)
    {
        if (!on) return;
        timespec n;
        clock_gettime(CLOCK_MONOTONIC, &n);
        ctx->host_ns[kind] += (uint64_t)((n.tv_sec - t.tv_sec) * 1000000000ll + (n.tv_nsec - t.tv_nsec));
        t = n;
    }
};

// What the launches of one call have in common: plan_scan decides before anything is enqueued, the next two steps fill in the rest.
struct ScanPlan {
    bool filtered, nt;
    int blocks, threads, U;   // grid, block, rows per chunk
    uint32_t kp;              // candidates kept per list
    uint64_t n_chunks;
    bool async, overlap;      // the pipeline: async select (one query per call), and of those the two-stream overlap
    bool pair;                // scan_pair: one-query launches may share a corpus pass
    // enter_pipeline
    uint64_t step = 0;        // of the pipeline (0: synchronous)
    key_t64 *lists = nullptr; // this step's list set, and behind the sets the chunk table of a filtered call
    uint64_t *table = nullptr;
    // overlap_prologue
    hipStream_t st = nullptr;
    unsigned long long gate_open = 0, gate_ticks = 0;
    bool may_pair = false;    // scan_pair: this launch runs scan_pair_kernel (it looks for a partner, and may find itself absorbed)
    bool wide = false;        // scan_take: ... or scan_wide_kernel, when the limit exceeds what scan_pair_kernel serves
    bool deep = false;        // scan_deep: ... or scan_deep_kernel, when it exceeds what scan_wide_kernel serves
    unsigned int absorbable = 0;
    bool sel_group = false;   // select_group: the launch is followed by group_select_kernel, not by a select of its own
    SelSlot sel = {0, 0, 0, 0};   // ... and what a leader's launch of it needs of this call
    uint32_t sel_k_out = 0;
};

static ScanPlan plan_scan(const smt_ctx *ctx, const ScanArgs &a)
{
    ScanPlan pl;
    pl.filtered = a.n_ranges > 0;
    pl.nt = ctx->tune.scan_nontemporal != 0;
    pl.kp = candidates_per_list(ctx, a.k_out);
    pl.blocks = ctx->tune.scan_blocks > 0 ? ctx->tune.scan_blocks : ctx->num_cus;
    if (pl.blocks > SEL_MAX_LISTS) pl.blocks = SEL_MAX_LISTS;
    pl.threads = ctx->tune.scan_threads;
    pl.U = pl.filtered ? FILTER_CHUNK : ctx->tune.scan_unroll;
    pl.n_chunks = pl.filtered ? a.n_chunks : (a.n_virtual + (uint64_t)pl.U - 1) / (uint64_t)pl.U;
    const uint64_t waves_per_block = (uint64_t)(pl.threads / 64);
    if ((uint64_t)pl.blocks * waves_per_block > pl.n_chunks) {  // tiny inputs: do not launch idle blocks
        const uint64_t need = (pl.n_chunks + waves_per_block - 1) / waves_per_block;
        pl.blocks = (int)(need > 0 ? need : 1);
    }
    // async select (one query per call): two list buffers alternate, the select of step i reads buffer i&1 on
    // the aux stream while the scan of step i+1 fills the other one
    pl.async = a.allow_async && ctx->tune.async_select && a.nq == 1;
    // scan_overlap: scan AND select of step i on scan stream i&1, behind an event on the main stream (the caller's inputs).  List
    // buffer b belongs to stream b, so stream order protects it and no flag is needed; the two streams let scan i+1 start while
    // scan i drains, paced by the start gate (ScanParams::gate).  (Not with STEAL: its counter ring is reset in stream order.)
    pl.overlap = pl.async && a.allow_overlap && ctx->tune.scan_overlap && !pl.filtered && ctx->tune.scan_steal == 0;
    // scan_pair: the launch may share its corpus pass with the call two steps later, or be absorbed by the one two steps earlier
    // (scan_pair_kernel).  Not with wave stamps (profiling of the plain kernel).
    pl.pair = pl.overlap && ctx->tune.scan_pair && pl.U == 4 && ctx->tune.scan_debug_ptr == 0;
    // more than three calls taken along: scan_wide_kernel, whose shared lists hold 32 keys and whose launch bound is 8 waves
    pl.wide = pl.pair && ctx->tune.scan_pair > GROUP_MAX - 1 && pl.kp <= 32 && pl.threads <= 512;
    // more than seven: scan_deep_kernel, under the same two conditions (a launch is of ONE family: deep, else wide, else the four-call kernel)
    pl.deep = pl.wide && ctx->tune.scan_pair > WIDE_MAX - 1;
    if (pl.deep) pl.wide = false;
    pl.st = ctx->stream;
    return pl;
}

// Leaves the other pipeline if the last call ran it, makes this one's, takes the step number and carves up the scratch buffer.
static int enter_pipeline(smt_ctx *ctx, const ScanArgs &a, ScanPlan &pl)
{
    int rc = SMT_OK;
    if (pl.async && ctx->async_overlap != pl.overlap && (rc = drain_async(ctx))) return rc;   // the two pipelines share the list buffers
    if (pl.async && (rc = pl.overlap ? ensure_overlap(ctx) : ensure_async(ctx))) return rc;
    if (!pl.async && (rc = drain_async(ctx))) return rc;
    pl.step = pl.overlap ? ++ctx->ov_step : pl.async ? ++ctx->async_step : 0;
    ctx->ov_lists_live = pl.overlap;   // (any other scan carves the scratch up its own way: smt_debug_scan_ring)
    // (scan_overlap: scans of consecutive calls run at the same time, and their grids differ with the corpus -- the two buffers get a
    // fixed place, the largest one-query list set, or a small call's buffer 1 would lie inside a large call's buffer 0)
    const size_t list_bytes = pl.overlap ? (size_t)SEL_MAX_LISTS * 64 * sizeof(key_t64)
                                         : (((size_t)a.nq * pl.blocks * pl.kp * sizeof(key_t64)) + 255) & ~(size_t)255;
    const size_t table_bytes = pl.filtered ? (size_t)pl.n_chunks * sizeof(uint64_t) : 0;
    // (scan_overlap: a ring of thirty-two sets, step & 31, 8 MiB, whichever kernel runs.  A leading scan of step i fills the sets of
    // steps i, i + 2, ... at most i + 30, all on its own stream, and set s is shared by the steps s, s +- 32, s +- 64 ...: the last
    // readers of the sixteen sets it may write are the selects of steps i - 32, i - 30, ... i - 2, launched on the SAME stream before
    // scan i, so stream order alone has them finished.  The other stream's steps have the other parity and the other sixteen sets.
    // With fewer sets the scan of step i would write the set of step i + 30 into one that a select of the other stream, ordered
    // against nothing here, may be reading.  A leader with a shorter reach -- scan_wide_kernel's i + 14, scan_pair_kernel's i + 6 --
    // writes a subset of those sets: more sets than its reach needs only move a set's next writer further away.)
    const size_t n_sets = pl.overlap ? 2 * DEEP_MAX : 2;
    if ((rc = ensure_scratch(ctx, n_sets * list_bytes + table_bytes))) return rc;
    pl.lists = reinterpret_cast<key_t64 *>(reinterpret_cast<char *>(ctx->d_scratch) + (pl.step & (n_sets - 1)) * list_bytes);
    pl.table = reinterpret_cast<uint64_t *>(reinterpret_cast<char *>(ctx->d_scratch) + n_sets * list_bytes);
    return pl.pair ? ensure_pair(ctx) : SMT_OK;
}

// scan_overlap: the step's stream goes behind the caller's; timed-launch bracketing, may_pair / absorbable, the start gate.
static int overlap_prologue(smt_ctx *ctx, ScanPlan &pl)
{
    const uint64_t step = pl.step;
    hipStream_t st = pl.st = ctx->ov_stream[step & 1];
    // a predecessor that takes this call's query along reads it without waiting for ov_ready: only a query that no work queued on
    // the caller's stream can still be writing may be taken
    // ... and only a launch that queues up behind a predecessor on its stream can be absorbed by it, or has reason to look for a
    // partner itself (a call made while the GPU is idle must cost what it did: no look, no wait; scan_pair_wait_us: tests)
    // ov_skip_ready: the caller's stream is asked ONCE per call, and when it is empty there is nothing for the internal stream to be
    // ordered behind -- no event is recorded on the caller's stream and no barrier stands in front of the scan.  (Those markers were
    // also what the next call's query found on the caller's stream when the host ran far enough ahead of it.)  The answer serves as
    // `idle` too.  0: an event and a wait for every call, and the caller's stream asked only behind a predecessor, as before.
    const bool skip_ready = ctx->tune.ov_skip_ready != 0;
    HostTimer ht(ctx);
    bool caller_empty = false;
    if (skip_ready) caller_empty = hipStreamQuery(ctx->stream) == hipSuccess;
    if (pl.pair) {
        const bool behind = ctx->tune.scan_pair_wait_us > 0 || hipStreamQuery(st) != hipSuccess;
        const bool idle = behind && (skip_ready ? caller_empty : hipStreamQuery(ctx->stream) == hipSuccess);
        pl.absorbable = idle ? 1u : 0u;
        pl.may_pair = behind;
    }
    (void)hipGetLastError();   // (hipErrorNotReady is an answer here)
    ht.lap(0);
    if (!caller_empty) {
        SMT_HIP_CHECK(hipEventRecord(ctx->ov_ready[step & 1], ctx->stream));
        SMT_HIP_CHECK(hipStreamWaitEvent(st, ctx->ov_ready[step & 1], 0));
        ++ctx->ov_ready_records;
    }
    ht.lap(1);
    // a timed launch waits for its predecessor (and that one's select), and the launch after it waits for it: the events bracket a
    // kernel that has the part to itself, not a gate or an HBM shared with a neighbour
    const bool timed = prof_arms_next(ctx, "scan");
    if (timed || ctx->ov_after_timed) {
        SMT_HIP_CHECK(hipEventRecord(ctx->ov_done, ctx->ov_stream[(step & 1) ^ 1]));
        SMT_HIP_CHECK(hipStreamWaitEvent(st, ctx->ov_done, 0));
        // (a timed launch and its successor neither absorb nor get absorbed: the events keep bracketing a one-query pass)
        pl.may_pair = false;
        pl.absorbable = 0;
    }
    ctx->ov_after_timed = timed;
    // What the gate counts is CALLS served, in blocks: a plain launch's block adds 1 when its rows are done, a leader's block the
    // number of calls its pass serves, an absorbed launch nothing, and gate_total (launch_scan_topk, behind the passes) counts one grid per call.  So "gate_pct of
    // the predecessor" is: every call before the predecessor call is served, and gate_pct per cent of the predecessor call's
    // grid.  When that call is the m-th of n that one pass serves, the point lies at (m - 1 + gate_pct / 100) / n of the pass'
    // blocks: 75 % of a pair's pass and 87.5 % of a full group's at gate_pct = 50, while a leader still at its gate holds
    // successors back only until their bound.  The default by the sweeps: 50 for every mode.  (While the grouped
    // pass ran one tree per query, launches that take two or three calls along ran 4 us per step faster with no gate: two leaders
    // on a CU filled each other's stalls.  With the group reducer every gate from 5 to 100 measures 48.0 us per step and no gate
    // 50.1 with a spread of 3 us, profiles/scan_group_loop.json.)
    const int gate_pct = ctx->tune.scan_gate_pct >= 0 ? ctx->tune.scan_gate_pct : 50;
    if (gate_pct > 0 && ctx->gate_prev_blocks > 0) {
        pl.gate_open = ctx->gate_total - ctx->gate_prev_blocks + (ctx->gate_prev_blocks * (uint64_t)gate_pct + 99) / 100;
        // the bound: the predecessor's rows at 4 TB/s (half the part's HBM rate; 1 KiB rows, 10 ns ticks) + 20 us, at most 0.5 ms (a
        // grid that cannot be resident twice -- scan_blocks / scan_threads -- may hold back predecessor blocks while it waits)
        pl.gate_ticks = std::min<uint64_t>(ctx->gate_prev_rows / 39 + 2000, 50000);
    }
    return SMT_OK;
}

// The parameters of the pass over the queries q0 .. q0 + nq_active - 1 (STEAL: see steal_setup).
static ScanParams scan_params(const smt_ctx *ctx, const ScanArgs &a, const ScanPlan &pl, const uint64_t *chunk_table, uint32_t q0,
                              uint32_t nq_active)
{
    ScanParams p{};
    p.corpus = a.corpus;
    p.queries = a.queries + (size_t)q0 * 256;
    p.n_virtual = a.n_virtual;
    p.chunk_table = pl.filtered ? chunk_table : nullptr;
    p.n_chunks = pl.n_chunks;
    p.kp = pl.kp;
    p.nq_active = nq_active;
    p.block_lists = pl.lists + (size_t)q0 * pl.blocks * pl.kp;
    p.stamps = reinterpret_cast<unsigned long long *>(ctx->tune.scan_debug_ptr);
    p.flags = pl.async && !pl.overlap ? ctx->d_flags : nullptr;
    p.step = pl.step;
    p.gate = pl.overlap ? ctx->d_gate : nullptr;
    p.gate_open = pl.gate_open;
    p.gate_ticks = pl.gate_ticks;
    return p;
}

// Dynamic groups (scan_topk_kernel STEAL; tuning key scan_steal = rounds per group, 0 = the static deal): unfiltered scans of
// 8-wave blocks over enough rows that every block gets well past its static groups.  Each launch has its own counter: a ring
// of 64, zeroed together every 64th launch (one 256-byte memset in stream order).
static int steal_setup(smt_ctx *ctx, const ScanPlan &pl, ScanParams &p)
{
    if (pl.filtered || pl.U != 4 || pl.threads != 512 || ctx->tune.scan_steal <= 0 ||
        pl.n_chunks < (uint64_t)pl.blocks * 8u * (uint64_t)ctx->tune.scan_steal * 8u)
        return SMT_OK;
    if (!ctx->d_steal) SMT_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&ctx->d_steal), 64 * sizeof(unsigned int)));
    if (ctx->steal_seq % 64 == 0) SMT_HIP_CHECK(hipMemsetAsync(ctx->d_steal, 0, 64 * sizeof(unsigned int), ctx->stream));
    p.steal_ctr = ctx->d_steal + (ctx->steal_seq % 64);
    ++ctx->steal_seq;
    uint32_t lr = 0;
    while ((2 << lr) <= ctx->tune.scan_steal) ++lr;
    p.steal_lr = lr;
    // the dynamic share: scan_steal_pct per cent of the groups (at least STEAL_DEPTH + 1 per block stay static: scan_topk.hip)
    const uint64_t n_groups = (pl.n_chunks + (8ull << lr) - 1) / (8ull << lr);
    const uint64_t per_block = n_groups / (uint64_t)pl.blocks;
    const uint64_t n_static = per_block * (uint64_t)(100 - ctx->tune.scan_steal_pct) / 100;
    p.steal_static = (uint32_t)std::max<uint64_t>(n_static, 3);
    return SMT_OK;
}

int ensure_pair(smt_ctx *ctx)
{
    if (ctx->h_pair_ring) return SMT_OK;
    SMT_HIP_CHECK(hipMalloc(&ctx->d_pair_recs, PAIR_RECS * sizeof(PairRecord)));
    SMT_HIP_CHECK(hipMemset(ctx->d_pair_recs, 0, PAIR_RECS * sizeof(PairRecord)));
    SMT_HIP_CHECK(hipMalloc(&ctx->d_wide_recs, WIDE_RECS * sizeof(WideRecord)));
    SMT_HIP_CHECK(hipMemset(ctx->d_wide_recs, 0, WIDE_RECS * sizeof(WideRecord)));
    SMT_HIP_CHECK(hipMalloc(&ctx->d_deep_recs, DEEP_RECS * sizeof(DeepRecord)));
    SMT_HIP_CHECK(hipMemset(ctx->d_deep_recs, 0, DEEP_RECS * sizeof(DeepRecord)));
    SMT_HIP_CHECK(hipMalloc(&ctx->d_deep_sel_recs, DEEP_RECS * sizeof(DeepSelRecord)));
    SMT_HIP_CHECK(hipMemset(ctx->d_deep_sel_recs, 0, DEEP_RECS * sizeof(DeepSelRecord)));
    SMT_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&ctx->d_sel_groups), (GROUP_SEL_MAX + 1) * sizeof(unsigned long long)));
    SMT_HIP_CHECK(hipMemset(ctx->d_sel_groups, 0, (GROUP_SEL_MAX + 1) * sizeof(unsigned long long)));
    SMT_HIP_CHECK(hipHostMalloc(&ctx->h_sel_ring, PAIR_RING * sizeof(SelSlot), hipHostMallocDefault));
    memset(ctx->h_sel_ring, 0, PAIR_RING * sizeof(SelSlot));
    SMT_HIP_CHECK(hipHostMalloc(&ctx->h_pair_ring, PAIR_RING * sizeof(PairSlot), hipHostMallocDefault));
    memset(ctx->h_pair_ring, 0, PAIR_RING * sizeof(PairSlot));
    return SMT_OK;
}

// What the slot of a group-capable launch says beside k' and the grid: the kernel it runs, and (deep) the group select behind it.
static unsigned long long group_family(const ScanPlan &pl)
{
    if (pl.wide) return WIDE_FAMILY;
    if (!pl.deep) return 0ull;
    return DEEP_FAMILY | (pl.sel_group ? DEEP_SELGROUP | (unsigned long long)pl.sel_k_out << DEEP_KOUT_SHIFT : 0ull);
}

static unsigned long long pair_ring_mask(const smt_ctx *ctx)
{
    return (unsigned long long)std::min(ctx->tune.scan_pair_ring, PAIR_RING) - 1;
}

// Publishes this step's slot: what a predecessor needs to take the call along.  The step number goes last.
static void publish_slot(smt_ctx *ctx, const ScanParams &p, const ScanPlan &pl)
{
    const unsigned long long at = p.step & pair_ring_mask(ctx);
    PairSlot *slot = reinterpret_cast<PairSlot *>(ctx->h_pair_ring) + at;
    __atomic_store_n(&slot->step, 0ull, __ATOMIC_SEQ_CST);   // (a reader of the slot's previous use fails its second check)
    slot->corpus = (unsigned long long)(uintptr_t)p.corpus;
    slot->n_virtual = p.n_virtual;
    slot->query = (unsigned long long)(uintptr_t)p.queries;
    slot->lists = (unsigned long long)(uintptr_t)p.block_lists;
    if (pl.sel_group) reinterpret_cast<SelSlot *>(ctx->h_sel_ring)[at] = pl.sel;   // (between the two stores of slot->step)
    slot->kp_blocks = (unsigned long long)p.kp | group_family(pl) | (unsigned long long)pl.blocks << 32;
    slot->absorbable = pl.absorbable;
    __atomic_store_n(&slot->step, p.step, __ATOMIC_RELEASE);
}

// What the three kernels' second arguments have in common; `recs`: the records of the launched kernel's kind.
template <class PP>
static PP group_params(const smt_ctx *ctx, const ScanPlan &pl, void *recs, int max_take)
{
    PP pp{};
    pp.absorbable = pl.absorbable;
    pp.ring_mask = pair_ring_mask(ctx);
    pp.ring = reinterpret_cast<const PairSlot *>(ctx->h_pair_ring);
    pp.recs = reinterpret_cast<decltype(pp.recs)>(recs);
    pp.ctl = ctx->d_gate + 1;
    pp.wait_ticks = (unsigned long long)ctx->tune.scan_pair_wait_us * 100ull;
    pp.max_take = (unsigned int)std::min(std::max(ctx->tune.scan_pair, 1), max_take);
    return pp;
}

// The group-capable one-query scan: the slot, then scan_pair_kernel, scan_wide_kernel (pl.wide) or scan_deep_kernel (pl.deep).
static int launch_scan_pair(smt_ctx *ctx, const ScanParams &p, const ScanPlan &pl)
{
    publish_slot(ctx, p, pl);
    if (pl.deep) {
        DeepParams dp = group_params<DeepParams>(ctx, pl, ctx->d_deep_recs, DEEP_MAX - 1);
        dp.family = group_family(pl);
        if (pl.sel_group) {
            dp.sel_ring = reinterpret_cast<const SelSlot *>(ctx->h_sel_ring);
            dp.sel_recs = reinterpret_cast<DeepSelRecord *>(ctx->d_deep_sel_recs);
        }
        launch_scan_deep_kernel(pl.nt, pl.blocks, pl.threads, pl.st, p, dp);
    } else if (pl.wide) {
        launch_scan_wide_kernel(pl.nt, pl.blocks, pl.threads, pl.st, p, group_params<WideParams>(ctx, pl, ctx->d_wide_recs, WIDE_MAX - 1));
    } else {
        launch_scan_pair_kernel(pl.nt, pl.blocks, pl.threads, pl.st, p, group_params<PairParams>(ctx, pl, ctx->d_pair_recs, GROUP_MAX - 1));
    }
    SMT_HIP_CHECK(hipGetLastError());
    ctx->pair_live = true;
    return SMT_OK;
}

// One pass: `slots` query slots, of which p.nq_active hold a query.
static int launch_scan_pass(smt_ctx *ctx, const ScanPlan &pl, const ScanParams &p, int slots)
{
    if (slots == 1 && pl.pair) {
        if (pl.may_pair) return launch_scan_pair(ctx, p, pl);
        ++ctx->pair_alone_host;
    }
    launch_scan_topk_kernel(slots, pl.U, pl.nt, pl.filtered, pl.blocks, pl.threads, pl.st, p);
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

static SelectArgs select_args(const ScanArgs &a, const ScanPlan &pl)
{
    SelectArgs s;
    s.corpus = a.corpus;
    s.queries = a.queries;
    s.nq = a.nq;
    s.lists = pl.lists;
    s.n_lists = (uint32_t)pl.blocks;
    s.kp = pl.kp;
    s.list_stride = (uint64_t)pl.blocks * pl.kp;
    s.k_out = a.k_out;
    s.ws_threshold = a.ws_threshold;
    s.ws_thr_score = a.ws_thr_score;
    s.row_base = a.row_base;
    s.out_rows = a.out_rows;
    s.out_dist = a.out_dist;
    s.out_counts = a.out_counts;
    s.async_step = pl.overlap ? 0 : pl.step;
    s.stream = pl.st;
    s.out_stride = a.out_stride;
    s.f32_err = F32_ERR_SCAN;
    s.out_uncertain = a.out_uncertain;
    s.out_status = a.out_status;
    s.deliver = a.deliver;
    return s;
}

// The two halves of a call's scan that launch_scan_topk and the test hook debug_scan_lists share, so that the hook cannot drift from
// production.  scan_begin: the argument checks, the plan, the pipeline step and the list area.
static int scan_begin(smt_ctx *ctx, const ScanArgs &a, ScanPlan &pl)
{
    SMT_REQUIRE(a.k_out >= 1 && a.k_out <= SCAN_MAX_K, "top_k for the scan path must be in [1, 56]");
    SMT_REQUIRE(a.rows < 0xFFFFFFFFull, "a shard holds fewer than 2^32-1 rows");
    pl = plan_scan(ctx, a);
    return enter_pipeline(ctx, a, pl);
}

// scan_passes: the chunk table of a filtered call, then one pass per up to four queries.  `route` (the hook's; nullptr in production)
// receives what was launched: SMT_SCAN_ROUTE_* of semtools_hip.h.
static int scan_passes(smt_ctx *ctx, const ScanArgs &a, const ScanPlan &pl, uint32_t *route)
{
    int rc = SMT_OK;
    const uint64_t *chunk_table = pl.table;
    if (pl.filtered && (rc = range_chunk_table(ctx, a, pl.table, &chunk_table))) return rc;
    if (route) *route = (uint32_t)pl.U | (pl.nt ? 0x10u : 0u) | (pl.filtered ? 0x20u : 0u) | (uint32_t)pl.threads << 8;
    int pass = 0;
    for (uint32_t q0 = 0; q0 < a.nq; ++pass) {
        // (three queries ride in the four-query kernel: with the four rows of a chunk reduced together a pass costs 1.06 x / 1.4 x one
        // query's for two / four queries -- 172 / 230 us at 1 M rows -- against 335 us for a pass of two and a pass of one)
        const uint32_t left = a.nq - q0;
        const int slots = left >= 3 ? 4 : (int)left;
        ScanParams p = scan_params(ctx, a, pl, chunk_table, q0, std::min(left, 4u));
        if ((rc = steal_setup(ctx, pl, p)) || (rc = launch_scan_pass(ctx, pl, p, slots))) return rc;
        if (route && pass < 3) *route |= (p.steal_ctr ? 0x40u : 0u) | (uint32_t)slots << (20 + 4 * pass);
        q0 += p.nq_active;
    }
    return SMT_OK;
}

int launch_scan_topk(smt_ctx *ctx, const ScanArgs &a)
{
    ScanPlan pl;
    int rc = scan_begin(ctx, a, pl);
    if (rc != SMT_OK) return rc;
    HostTimer whole(ctx);
    if (pl.overlap && (rc = overlap_prologue(ctx, pl))) return rc;
    // select_group: a launch of scan_deep_kernel whose select is a plain one (rows, distances, status) is followed by ONE launch of
    // group_select_kernel for the calls its pass serves.  A call whose select carries more than the record holds keeps its own
    // select and is taken along by nobody.
    const SelectArgs sa = select_args(a, pl);
    if (pl.deep && pl.may_pair && ctx->tune.select_group) {
        pl.sel_group = group_select_serves(sa);
        if (pl.sel_group) {
            pl.sel = SelSlot{(unsigned long long)(uintptr_t)sa.out_rows, (unsigned long long)(uintptr_t)sa.out_dist,
                             (unsigned long long)(uintptr_t)sa.out_status, (unsigned long long)sa.row_base};
            pl.sel_k_out = sa.k_out;
        } else {
            pl.absorbable = 0;
        }
    }
    HostTimer ht(ctx);

    prof_begin_on(ctx, "scan", pl.st);
    if ((rc = scan_passes(ctx, a, pl, nullptr))) return rc;
    prof_end_on(ctx, "scan", pl.st);

    if (pl.overlap) {
        ctx->gate_total += (uint64_t)pl.blocks;
        ctx->gate_prev_blocks = (uint64_t)pl.blocks;
        ctx->gate_prev_rows = a.n_virtual;
        ctx->async_pending = true;
        ctx->async_overlap = true;
    } else if (pl.async) {
        ctx->async_overlap = false;
    }
    ht.lap(2);
    if (pl.sel_group) {
        GroupSelect gs;
        gs.rec = reinterpret_cast<const unsigned long long *>(reinterpret_cast<const DeepRecord *>(ctx->d_deep_recs) + pl.step % DEEP_RECS);
        gs.sel = reinterpret_cast<const unsigned long long *>(reinterpret_cast<const DeepSelRecord *>(ctx->d_deep_sel_recs) + pl.step % DEEP_RECS);
        gs.absorbed = (pl.step << PAIR_SHIFT) | PAIR_ABSORBED;
        gs.paired = (pl.step << PAIR_SHIFT) | PAIR_PAIRED;
        gs.hist = ctx->d_sel_groups;
        rc = launch_group_select(ctx, sa, gs);
    } else {
        rc = launch_select(ctx, sa);
    }
    ht.lap(3);
    // the aux stream's contract (smt_ctx_aux_stream): work a host chains there runs behind this call's select.  (select_group: the
    // select launch of an absorbed call does nothing, but it follows the leader's, which holds the call's answer, on this stream.)
    if (rc == SMT_OK && pl.overlap && ctx->aux_stream) {
        SMT_HIP_CHECK(hipEventRecord(ctx->ov_sel[pl.step & 1], pl.st));
        SMT_HIP_CHECK(hipStreamWaitEvent(ctx->aux_stream, ctx->ov_sel[pl.step & 1], 0));
    }
    ht.lap(4);
    if (pl.overlap) {
        whole.lap(5);
        if (whole.on) ++ctx->host_ns_calls;
    }
    return rc;
}

// ------------------------------------------------------------------ test hooks (smt_debug_scan_lists, smt_debug_scan_ring)
// The synchronous scan of `a` up to the select and no further, through scan_begin and scan_passes as launch_scan_topk runs them.  The
// list area of nq + 1 query sets is preset to the byte 0x5A in front of the first pass and copied out whole behind the last: the extra
// set is a guard no pass may touch (a pass of three queries rides in four slots).
int debug_scan_lists(smt_ctx *ctx, const ScanArgs &a, key_t64 *out_keys_host, uint64_t out_cap_keys, uint32_t *out_blocks, uint32_t *out_kp,
                     uint32_t *out_route)
{
    SMT_REQUIRE(!a.allow_async && !a.allow_overlap, "debug scan lists: the synchronous path");
    ScanPlan pl;
    int rc = scan_begin(ctx, a, pl);
    if (rc != SMT_OK) return rc;
    *out_blocks = (uint32_t)pl.blocks;
    *out_kp = pl.kp;
    const size_t n_keys = (size_t)(a.nq + 1) * pl.blocks * pl.kp;   // (inside the two list sets of enter_pipeline, in front of the chunk table)
    SMT_REQUIRE(out_cap_keys >= n_keys, "debug scan lists: the output holds fewer than (nq + 1) x blocks x k' keys");
    SMT_HIP_CHECK(hipMemsetAsync(pl.lists, 0x5A, n_keys * sizeof(key_t64), ctx->stream));
    if ((rc = scan_passes(ctx, a, pl, out_route))) return rc;
    SMT_HIP_CHECK(hipMemcpyAsync(out_keys_host, pl.lists, n_keys * sizeof(key_t64), hipMemcpyDeviceToHost, ctx->stream));
    SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return SMT_OK;
}

// The first n_keys keys of the list set of the one-query pipeline call made calls_back calls ago: set (ov_step - calls_back) & 31 at the
// fixed set stride of enter_pipeline.  Waits for the pipeline first.
int debug_scan_ring(smt_ctx *ctx, uint32_t calls_back, uint64_t n_keys, key_t64 *out_keys_host)
{
    const size_t set_keys = (size_t)SEL_MAX_LISTS * 64, n_sets = 2 * DEEP_MAX;
    SMT_REQUIRE(calls_back < n_sets, "debug scan ring: the ring holds the last 32 calls");
    SMT_REQUIRE(n_keys <= set_keys, "debug scan ring: a list set holds at most 512 x 64 keys");
    int rc = drain_async(ctx);
    if (rc != SMT_OK) return rc;
    SMT_REQUIRE(ctx->ov_lists_live && ctx->async_overlap, "debug scan ring: the last scan was not a call of the overlap pipeline");
    SMT_REQUIRE(ctx->ov_step > calls_back, "debug scan ring: no such call");
    SMT_REQUIRE(ctx->d_scratch && ctx->scratch_bytes >= n_sets * set_keys * sizeof(key_t64), "debug scan ring: no list ring");
    if (n_keys == 0) return SMT_OK;
    const key_t64 *set = reinterpret_cast<const key_t64 *>(ctx->d_scratch) + ((ctx->ov_step - calls_back) & (n_sets - 1)) * set_keys;
    SMT_HIP_CHECK(hipMemcpy(out_keys_host, set, n_keys * sizeof(key_t64), hipMemcpyDeviceToHost));
    return SMT_OK;
}

}  // namespace smt
