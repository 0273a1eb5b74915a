// group_exchange.cpp -- how lists move between the ranks of a group (group.h: "exchange").  Three transports: the RCCL all-gather
// (issued by group.cpp, which owns the binding), the event-ordered copy gather of logical ranks, and peer reads in place with their
// slot ring and the spread-waits hand-shake.  On top of them: the merge of the ranks' packed k-lists where an answer is wanted,
// the variable-length host-list exchange, and the copy-transport all-reduce of shared-centroid IVF builds.
#include <algorithm>

#include "group.h"

namespace smt {

int ensure_dev(smt_group *g, int i, size_t bytes)
{
    GroupBuf &b = g->buf[i];
    if (bytes <= b.dev_bytes) return SMT_OK;
    smt_ctx *c = g->ctx[i];
    int rc = drain_async(c);
    if (rc) return rc;
    SMT_HIP_CHECK(hipStreamSynchronize(c->stream));
    if ((rc = sync_side_streams(c))) return rc;
    if (b.dev) SMT_HIP_CHECK(hipFree(b.dev));
    b.dev = nullptr;
    b.dev_bytes = 0;
    const size_t want = std::max(bytes, (size_t)1 << 16);
    SMT_HIP_CHECK(hipMalloc(&b.dev, want));
    b.dev_bytes = want;
    return SMT_OK;
}

int ensure_host(smt_group *g, int i, size_t bytes)
{
    GroupBuf &b = g->buf[i];
    if (bytes <= b.pinned_bytes) return SMT_OK;
    SMT_HIP_CHECK(hipStreamSynchronize(g->ctx[i]->stream));
    if (b.pinned) SMT_HIP_CHECK(hipHostFree(b.pinned));
    b.pinned = nullptr;
    b.pinned_bytes = 0;
    const size_t want = std::max(bytes, (size_t)1 << 16);
    SMT_HIP_CHECK(hipHostMalloc(&b.pinned, want, hipHostMallocDefault));
    b.pinned_bytes = want;
    return SMT_OK;
}

// All-gather `words` u64 per rank: send_off/recv_off are BYTE offsets into each local device's exchange buffer.
// The streams are the contexts' main streams, or their aux streams where on_aux[i] (async select pipeline).
int allgather_words(smt_group *g, size_t send_off, size_t recv_off, size_t words, const std::vector<char> *on_aux)
{
    if (!g->copies) return rccl_allgather_words(g, send_off, recv_off, words, on_aux);
    // Copy transport (logical ranks of ONE process): gather into rank 0's receive buffer, then every other rank copies the
    // whole block -- 2 n copies and ~5 n event calls instead of the n x n copies of rounds 2-3 (192 HIP calls per exchange at 8
    // ranks: ~0.45 of the 0.58 ms one host thread needed to issue an 8-shard search, profiles/r04_group_issue.json).
    auto stream_of = [&](int i) { return exchange_stream(g, i, on_aux); };
    const int n = g->n_local;
    for (int j = 0; j < n; ++j) {
        SMT_HIP_CHECK(hipSetDevice(g->ctx[j]->device));
        SMT_HIP_CHECK(hipEventRecord(g->ev_ready[j], stream_of(j)));
    }
    SMT_HIP_CHECK(hipSetDevice(g->ctx[0]->device));
    char *dst0 = reinterpret_cast<char *>(g->buf[0].dev) + recv_off;
    for (int j = 0; j < n; ++j) {
        if (j != 0) SMT_HIP_CHECK(hipStreamWaitEvent(stream_of(0), g->ev_ready[j], 0));
        const char *src = reinterpret_cast<const char *>(g->buf[j].dev) + send_off;
        SMT_HIP_CHECK(hipMemcpyPeerAsync(dst0 + (size_t)j * words * 8, g->ctx[0]->device, src, g->ctx[j]->device, words * 8, stream_of(0)));
    }
    SMT_HIP_CHECK(hipEventRecord(g->ev_done[0], stream_of(0)));       // every send buffer has been read; rank 0 holds the block
    for (int i = 1; i < n; ++i) {
        SMT_HIP_CHECK(hipSetDevice(g->ctx[i]->device));
        SMT_HIP_CHECK(hipStreamWaitEvent(stream_of(i), g->ev_done[0], 0));   // (also: rank i may overwrite its send buffer after this)
        SMT_HIP_CHECK(hipMemcpyPeerAsync(reinterpret_cast<char *>(g->buf[i].dev) + recv_off, g->ctx[i]->device, dst0, g->ctx[0]->device,
                                         (size_t)n * words * 8, stream_of(i)));
        SMT_HIP_CHECK(hipEventRecord(g->ev_done[i], stream_of(i)));
    }
    // rank 0 may not overwrite its receive block (the next exchange) before every rank has copied it
    SMT_HIP_CHECK(hipSetDevice(g->ctx[0]->device));
    for (int i = 1; i < n; ++i) SMT_HIP_CHECK(hipStreamWaitEvent(stream_of(0), g->ev_done[i], 0));
    return SMT_OK;
}

int gather_host_words(smt_group *g, size_t w, const uint64_t *mine, std::vector<uint64_t> &all, bool every_local)
{
    const size_t R = (size_t)g->n_ranks;
    int rc;
    for (int i = 0; i < g->n_local; ++i) {
        if ((rc = group_bind(g, i)) || (rc = ensure_dev(g, i, (1 + R) * w * 8 + 64))) return rc;   // (no way left to tell the others)
        SMT_HIP_CHECK(hipMemcpyAsync(g->buf[i].dev, mine + (size_t)i * w, w * 8, hipMemcpyHostToDevice, g->ctx[i]->stream));
        SMT_HIP_CHECK(hipStreamSynchronize(g->ctx[i]->stream));
    }
    if ((rc = allgather_words(g, 0, w * 8, w))) return rc;
    const int readers = every_local ? g->n_local : 1;
    all.resize((size_t)readers * R * w);
    for (int i = 0; i < readers; ++i) {
        if ((rc = group_bind(g, i))) return rc;
        SMT_HIP_CHECK(hipMemcpyAsync(all.data() + (size_t)i * R * w, reinterpret_cast<char *>(g->buf[i].dev) + w * 8, R * w * 8,
                                     hipMemcpyDeviceToHost, g->ctx[i]->stream));
        if (every_local) SMT_HIP_CHECK(hipStreamSynchronize(g->ctx[i]->stream));
    }
    return every_local ? SMT_OK : group_sync_all(g);
}

// ---------------------------------------------------------------- peer transport (one-process groups)
int peer_publish(smt_group *g, int j, hipStream_t st)
{
    SMT_HIP_CHECK(hipEventRecord(g->ev_ready[j], st));
    g->pub_stream[j] = st;
    return SMT_OK;
}

// Rank j's issuer, right behind peer_publish(j): the merge that local device i will launch on `st_i` waits for rank j's list.
// (The wait names a stream of ANOTHER device when i != j: legal -- a stream carries its device -- and checked by the self-test.)
static int peer_await(smt_group *g, int j, int i, hipStream_t st_i)
{
    if (j == i && g->pub_stream[j] == st_i) return SMT_OK;   // stream order
    SMT_HIP_CHECK(hipStreamWaitEvent(st_i, g->ev_ready[j], 0));
    return SMT_OK;
}

uint64_t *exchange_list(smt_group *g, int j, const ExchangeLayout &L, int slot)
{
    char *base = slot < 0 ? reinterpret_cast<char *>(g->buf[j].dev) + L.loc_off
                          : reinterpret_cast<char *>(g->ring.dev[j]) + (size_t)slot * g->ring.slot_bytes;
    return reinterpret_cast<uint64_t *>(base);
}

int merge_ranks_on(smt_group *g, int i, hipStream_t st, const ExchangeLayout &L, int slot, uint32_t nq, uint32_t k, uint64_t *out_packed,
                   hipEvent_t done, bool waits_enqueued)
{
    const bool peer = g->transport == SMT_TRANSPORT_PEER;
    int rc = group_bind(g, i);
    if (rc) return rc;
    smt_ctx *c = g->ctx[i];
    MergeSources src;
    for (int j = 0; peer && j < g->n_local; ++j) {
        src.list[j] = exchange_list(g, j, L, slot);
        if (!waits_enqueued && (rc = peer_await(g, j, i, st))) return rc;
    }
    // profiling (smt_prof_enable on device i's context): "exchange" = from this rank's own list being ready to every list being there
    // (the skew between the ranks + what the transport costs), "merge" = the merge kernel
    prof_end_on(c, "exchange", st);
    prof_begin_on(c, "merge", st);
    if (peer) rc = launch_merge_topk_sources_on(st, src, (uint32_t)g->n_local, nq, k, k, out_packed);
    else rc = launch_merge_topk_packed_on(c, st, reinterpret_cast<const uint64_t *>(reinterpret_cast<char *>(g->buf[i].dev) + L.gath_off),
                                          (uint32_t)g->n_ranks, nq, k, k, out_packed, L.rank_words);
    if (rc) return rc;
    prof_end_on(c, "merge", st);
    if (done) SMT_HIP_CHECK(hipEventRecord(done, st));
    return SMT_OK;
}

int combine_ranks_status_on(smt_group *g, int i, hipStream_t st, const ExchangeLayout &L, int slot, uint32_t nq, uint32_t *out_status)
{
    if (g->transport != SMT_TRANSPORT_PEER) {
        const uint64_t *gath = reinterpret_cast<const uint64_t *>(reinterpret_cast<char *>(g->buf[i].dev) + L.gath_off);
        return launch_combine_status_on(st, nullptr, gath + L.list_words, L.rank_words, (uint32_t)g->n_ranks, nq, out_status);
    }
    MergeSources src;
    for (int j = 0; j < g->n_local; ++j) src.list[j] = exchange_list(g, j, L, slot) + L.list_words;
    return launch_combine_status_on(st, &src, nullptr, 0, (uint32_t)g->n_local, nq, out_status);
}

WaitBoard::WaitBoard(smt_group *g_, const std::vector<char> &on_aux_, uint64_t *const *out_packed)
    : g(g_), on_aux(on_aux_),
      active(g_->transport == SMT_TRANSPORT_PEER && g_->spread_waits && g_->workers != nullptr && g_->n_local <= MAX_RANKS)
{
    for (int i = 0; active && i < g->n_local; ++i) {
        if (out_packed[i]) merging |= 1ull << i;
        awaiting[i].store(0, std::memory_order_relaxed);
        issued[i].store(0, std::memory_order_relaxed);
    }
}

int WaitBoard::await_all(uint64_t ranks, int m)
{
    int rc = SMT_OK;
    for (int j = 0; ranks && !rc; ++j, ranks >>= 1)
        if (ranks & 1) rc = peer_await(g, j, m, exchange_stream(g, m, &on_aux));
    return rc;
}

int WaitBoard::own_work_issued(int i)
{
    if (!(merging >> i & 1)) return SMT_OK;
    int rc = peer_await(g, i, i, exchange_stream(g, i, &on_aux));   // (its own list: stream order, or the hop from its aux stream)
    if (rc) return rc;
    issued[i].store(1, std::memory_order_seq_cst);
    return await_all(awaiting[i].exchange(0, std::memory_order_seq_cst), i);
}

int WaitBoard::published(int i)
{
    const uint64_t mine = 1ull << i;
    for (int m = 0; m < g->n_local; ++m) {
        if (!(merging >> m & 1) || m == i) continue;
        awaiting[m].fetch_or(mine, std::memory_order_seq_cst);
        if (issued[m].load(std::memory_order_seq_cst) && (awaiting[m].fetch_and(~mine, std::memory_order_seq_cst) & mine))
            if (int rc = peer_await(g, i, m, exchange_stream(g, m, &on_aux))) return rc;
    }
    return SMT_OK;
}

int WaitBoard::sweep()
{
    int rc = SMT_OK;
    for (int m = 0; active && !rc && m < g->n_local; ++m) rc = await_all(awaiting[m].exchange(0, std::memory_order_seq_cst), m);
    return rc;
}

void ring_free(smt_group *g)
{
    smt_group::Ring &r = g->ring;
    for (int i = 0; i < (int)r.dev.size(); ++i)
        if (r.dev[i]) { (void)hipSetDevice(g->ctx[i]->device); (void)hipFree(r.dev[i]); }
    for (auto &row : r.done)
        for (hipEvent_t e : row)
            if (e) (void)hipEventDestroy(e);
    r = smt_group::Ring();
}

// The ring holds slots of at least `slot_bytes`; (re)made -- everything in flight finishes first -- when a call needs larger ones.
int ring_ensure(smt_group *g, size_t slot_bytes)
{
    smt_group::Ring &r = g->ring;
    if (!r.dev.empty() && slot_bytes <= r.slot_bytes) return SMT_OK;
    int rc = sync_every_stream(g);
    if (rc) return rc;
    ring_free(g);
    r.slot_bytes = align256(slot_bytes);
    r.slots = (int)std::min<size_t>(64, std::max<size_t>(2, ((size_t)16 << 20) / r.slot_bytes));
    r.dev.assign(g->n_local, nullptr);
    r.done.assign(r.slots, std::vector<hipEvent_t>(g->n_local, nullptr));
    r.merged.assign(r.slots, 0);
    for (int i = 0; i < g->n_local; ++i) {
        if ((rc = group_bind(g, i))) return rc;
        SMT_HIP_CHECK(hipMalloc(&r.dev[i], (size_t)r.slots * r.slot_bytes));
    }
    return SMT_OK;
}

// The slot of the next exchange, free to be written: the merges that read it `slots` exchanges ago are over (normally long since;
// otherwise the caller's thread waits here -- it may not run more than `slots` searches ahead of the devices).
int ring_next_slot(smt_group *g, int *slot_out)
{
    smt_group::Ring &r = g->ring;
    const int slot = (int)(r.seq % (uint64_t)r.slots);
    for (int i = 0; r.merged[slot] && i < g->n_local; ++i)
        if (r.merged[slot] >> i & 1) SMT_HIP_CHECK(hipEventSynchronize(r.done[slot][i]));
    r.merged[slot] = 0;
    ++r.seq;
    *slot_out = slot;
    return SMT_OK;
}

int ring_done_event(smt_group *g, int slot, int i, hipEvent_t *ev)
{
    smt_group::Ring &r = g->ring;
    if (!r.done[slot][i]) {
        // (an event belongs to the device that is current when it is made, and is recorded on a stream of THAT device)
        int rc = group_bind(g, i);
        if (rc) return rc;
        SMT_HIP_CHECK(hipEventCreateWithFlags(&r.done[slot][i], hipEventDisableTiming));
    }
    r.merged[slot] |= (uint64_t)1 << i;
    *ev = r.done[slot][i];
    return SMT_OK;
}

// The peer transport's self-test (smt_group_create, several devices): every rank's KERNEL writes a small list into its exchange
// buffer, device 0 merges the lists in place, the host checks the merge -- three rounds over the SAME addresses with different
// values, so that a reader serving stale lines from its own cache, or a writer whose lines have not left its L2 when its event
// fires, is caught here and not in an answer.  false = the group falls back to the ncclAllGather transport.
__global__ void peer_test_fill_kernel(uint64_t *list, uint32_t k, uint32_t rank, uint32_t n_ranks, uint32_t round)
{
    const uint32_t i = threadIdx.x;
    if (i >= k) return;
    list[i] = (uint64_t)round * 100000u + rank * 100u + i;                                  // "row"
    const double d = (double)(i * n_ranks + rank) + 0.001 * round;                            // interleaves the ranks' entries
    reinterpret_cast<double *>(list + k)[i] = d;
}

bool peer_self_test(smt_group *g)
{
    const uint32_t k = 4, n = (uint32_t)g->n_local;
    const size_t out_off = 4096;
    const ExchangeLayout L(1, k, 0, g->n_local, false, false);   // (the lists at the start of the exchange buffers)
    g->transport = SMT_TRANSPORT_PEER;   // (what merge_ranks_on is to test; the group's creator picks its transport after this)
    for (int i = 0; i < g->n_local; ++i)
        if (group_bind(g, i) || ensure_dev(g, i, out_off + 1024)) return false;
    for (uint32_t round = 0; round < 3; ++round) {
        for (int j = 0; j < g->n_local; ++j) {
            if (group_bind(g, j)) return false;
            hipLaunchKernelGGL(peer_test_fill_kernel, dim3(1), dim3(64), 0, g->ctx[j]->stream, exchange_list(g, j, L, -1), k, (uint32_t)j, n, round);
            if (hipGetLastError() != hipSuccess || peer_publish(g, j, g->ctx[j]->stream)) return false;
            // (with device j current, as rank j's issuing thread will have it)
            if (g->spread_waits && peer_await(g, j, 0, g->ctx[0]->stream)) {
                (void)hipGetLastError();
                g->spread_waits = false;
                return peer_self_test(g);   // once more from the start, every wait enqueued by the merging device's side
            }
        }
        uint64_t *merged = reinterpret_cast<uint64_t *>(reinterpret_cast<char *>(g->buf[0].dev) + out_off);
        if (merge_ranks_on(g, 0, g->ctx[0]->stream, L, -1, 1, k, merged, nullptr, g->spread_waits)) return false;
        uint64_t got[8];
        if (hipMemcpyAsync(got, merged, sizeof(got), hipMemcpyDeviceToHost, g->ctx[0]->stream) != hipSuccess) return false;
        if (group_sync_all(g)) return false;
        for (uint32_t e = 0; e < k; ++e) {   // the k smallest distances are entry 0 of ranks 0 .. k-1 (n >= k), else i * n + rank order
            const uint32_t i = e / n, r = e % n;
            double want_d = (double)(i * n + r) + 0.001 * round, got_d;
            memcpy(&got_d, &got[k + e], 8);
            if (got[e] != (uint64_t)round * 100000u + r * 100u + i || got_d != want_d) return false;
        }
    }
    return true;
}

// ---------------------------------------------------------------- generic (host-list) exchange
// Every local shard holds per-query hit lists of any length, sorted (distance asc, row asc), rows global.  All-gather
// of the counts, one all-gather of a max-count-padded buffer, host merge.  `keep` truncates after the merge
// (UINT64_MAX = keep all: search_documents with a threshold, src/search/mod.rs:115-116).
// One query's lists, each sorted by (distance, row), merged into the first `keep` entries of their union in that order: a
// cursor per list, the smallest head taken each time (R is the number of ranks: a linear scan of the heads beats a heap).
// (Round 5: this was std::sort over the union -- 3-4 ms per query with 65 k hits under a threshold.)
struct HitSpan { const uint64_t *rows; const double *dist; uint64_t n; };
static void merge_hit_spans(std::vector<HitSpan> &src, uint64_t keep, LocalHits &out)
{
    uint64_t total = 0;
    for (const HitSpan &sp : src) total += sp.n;
    const uint64_t n_out = std::min<uint64_t>(total, keep);
    out.rows.resize(n_out);
    out.dist.resize(n_out);
    size_t live = 0;
    for (size_t i = 0; i < src.size(); ++i)
        if (src[i].n) src[live++] = src[i];
    src.resize(live);
    for (uint64_t e = 0; e < n_out; ++e) {
        size_t best = 0;
        for (size_t i = 1; i < src.size(); ++i)
            if (src[i].dist[0] < src[best].dist[0] || (src[i].dist[0] == src[best].dist[0] && src[i].rows[0] < src[best].rows[0])) best = i;
        out.rows[e] = src[best].rows[0];
        out.dist[e] = src[best].dist[0];
        ++src[best].rows; ++src[best].dist;
        if (--src[best].n == 0) { src[best] = src.back(); src.pop_back(); }
    }
}

int exchange_host_lists(smt_group *g, const std::vector<std::vector<LocalHits>> &local /* [n_local][nq] */, uint32_t nq, uint64_t keep,
                        std::vector<LocalHits> &merged)
{
    merged.assign(nq, LocalHits());
    if (nq == 0) return SMT_OK;
    const int R = g->n_ranks;
    int rc;
    std::vector<HitSpan> src;
    // every rank lives in this process (one-process and logical groups): the lists are all here already -- nothing travels
    // ($SEMTOOLS_GROUP_HOST_LISTS=exchange sends them through the devices anyway: the tests' way to run the multi-process path below
    // on the logical ranks of one GPU)
    const char *force = getenv("SEMTOOLS_GROUP_HOST_LISTS");
    if (g->n_local == g->n_ranks && !(force && std::string(force) == "exchange")) {
        for (uint32_t q = 0; q < nq; ++q) {
            src.clear();
            for (int i = 0; i < g->n_local; ++i) src.push_back({local[i][q].rows.data(), local[i][q].dist.data(), local[i][q].rows.size()});
            merge_hit_spans(src, keep, merged[q]);
        }
        return SMT_OK;
    }
    // ---- counts
    std::vector<uint64_t> cnt((size_t)g->n_local * nq), counts;
    for (int i = 0; i < g->n_local; ++i)
        for (uint32_t q = 0; q < nq; ++q) cnt[(size_t)i * nq + q] = std::min<uint64_t>(local[i][q].rows.size(), keep);   // (nobody needs more than `keep` of a list)
    if ((rc = gather_host_words(g, nq, cnt.data(), counts))) return rc;
    std::vector<uint64_t> width(nq, 0), off(nq + 1, 0);
    for (uint32_t q = 0; q < nq; ++q) {
        for (int r = 0; r < R; ++r) width[q] = std::max(width[q], counts[(size_t)r * nq + q]);
        off[q + 1] = off[q] + 2 * width[q];
    }
    const size_t words = off[nq];  // per rank
    if (words == 0) return SMT_OK;
    // ---- padded payload: per query [rows | distance bits], width[q] each
    const size_t send_bytes = words * 8, recv_off = align256(send_bytes);
    for (int i = 0; i < g->n_local; ++i) {
        if ((rc = group_bind(g, i))) return rc;
        if ((rc = ensure_dev(g, i, recv_off + (size_t)R * send_bytes + 64))) return rc;
        if ((rc = ensure_host(g, i, std::max(send_bytes, i == 0 ? (size_t)R * send_bytes : (size_t)0)))) return rc;
        uint64_t *h = reinterpret_cast<uint64_t *>(g->buf[i].pinned);
        for (uint32_t q = 0; q < nq; ++q) {
            const LocalHits &l = local[i][q];
            const uint64_t mine = cnt[(size_t)i * nq + q];
            uint64_t *rows = h + off[q], *bits = rows + width[q];
            for (uint64_t e = 0; e < width[q]; ++e) {
                if (e < mine) { rows[e] = l.rows[e]; memcpy(bits + e, &l.dist[e], 8); }
                else { rows[e] = UINT64_MAX; bits[e] = 0x7FF0000000000000ull; }
            }
        }
        SMT_HIP_CHECK(hipMemcpyAsync(g->buf[i].dev, h, send_bytes, hipMemcpyHostToDevice, g->ctx[i]->stream));
    }
    if ((rc = allgather_words(g, 0, recv_off, words))) return rc;
    if ((rc = group_bind(g, 0))) return rc;
    uint64_t *all = reinterpret_cast<uint64_t *>(g->buf[0].pinned);
    SMT_HIP_CHECK(hipMemcpyAsync(all, reinterpret_cast<char *>(g->buf[0].dev) + recv_off, (size_t)R * send_bytes,
                                 hipMemcpyDeviceToHost, g->ctx[0]->stream));
    if ((rc = group_sync_all(g))) return rc;
    // ---- merge.  Shards are ascending contiguous row ranges (or pieces dealt in insertion order) and every list is (distance, row)-
    // sorted, so the (distance, row) merge of the lists reproduces the reference's stable sort over the whole corpus (mod.rs:107-111).
    for (uint32_t q = 0; q < nq; ++q) {
        src.clear();
        for (int r = 0; r < R; ++r) {
            const uint64_t *rows = all + (size_t)r * words + off[q];
            src.push_back({rows, reinterpret_cast<const double *>(rows + width[q]), counts[(size_t)r * nq + q]});
        }
        merge_hit_spans(src, keep, merged[q]);
    }
    return SMT_OK;
}

// ---------------------------------------------------------------- all-reduce for shared-centroid IVF builds
__global__ void sum_ranks_i64_kernel(const long long *const *ptrs, int n_ranks, size_t n, long long *out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    long long acc = 0;
    for (int r = 0; r < n_ranks; ++r) acc += ptrs[r][i];
    out[i] = acc;
}
__global__ void sum_ranks_u32_kernel(const unsigned int *const *ptrs, int n_ranks, size_t n, unsigned int *out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned int acc = 0;
    for (int r = 0; r < n_ranks; ++r) acc += ptrs[r][i];
    out[i] = acc;
}

static void thread_barrier(smt_group *g)
{
    std::unique_lock<std::mutex> lk(g->ar_mu);
    const uint64_t gen = g->ar_generation;
    if (++g->ar_waiting == g->n_local) {
        g->ar_waiting = 0;
        ++g->ar_generation;
        g->ar_cv.notify_all();
    } else {
        g->ar_cv.wait(lk, [&] { return g->ar_generation != gen; });
    }
}

// IvfBuildShare::allreduce for one local rank (called from that rank's host thread)
int group_allreduce_sums(void *user, long long *sums, size_t n_sums, unsigned int *counts, size_t n_counts)
{
    ShareCtx *sc = static_cast<ShareCtx *>(user);
    smt_group *g = sc->g;
    const int i = sc->local;
    smt_ctx *c = g->ctx[i];
    if (!g->copies) return rccl_allreduce_sums(g, i, sums, n_sums, counts, n_counts);
    // copy transport: every rank lives in this process (one thread each): meet, sum everybody's buffer, meet, copy back.
    // A rank whose HIP calls fail still passes BOTH barriers (its siblings would wait for it forever) and then reports.
    const size_t b_sums = align256(n_sums * 8), b_cnt = align256(n_counts * 4), b_ptr = align256((size_t)g->n_local * 16);
    int rc = ensure_dev(g, i, b_sums + b_cnt + b_ptr + 64);
    auto hip_ok = [&](hipError_t e, const char *what) {
        if (e != hipSuccess && !rc) { set_error("%s: %s", what, hipGetErrorString(e)); rc = SMT_E_HIP; }
    };
    hip_ok(hipStreamSynchronize(c->stream), "all-reduce (sync)");
    {
        std::lock_guard<std::mutex> lk(g->ar_mu);
        g->ar_sums[i] = sums;
        g->ar_counts[i] = counts;
    }
    thread_barrier(g);
    long long *t_sums = nullptr;
    unsigned int *t_cnt = nullptr;
    if (!rc) {
        char *base = reinterpret_cast<char *>(g->buf[i].dev);
        t_sums = reinterpret_cast<long long *>(base);
        t_cnt = reinterpret_cast<unsigned int *>(base + b_sums);
        const long long **d_ps = reinterpret_cast<const long long **>(base + b_sums + b_cnt);
        const unsigned int **d_pc = reinterpret_cast<const unsigned int **>(base + b_sums + b_cnt + (size_t)g->n_local * 8);
        hip_ok(hipMemcpyAsync(d_ps, g->ar_sums.data(), (size_t)g->n_local * 8, hipMemcpyHostToDevice, c->stream), "all-reduce (pointers)");
        hip_ok(hipMemcpyAsync(d_pc, g->ar_counts.data(), (size_t)g->n_local * 8, hipMemcpyHostToDevice, c->stream), "all-reduce (pointers)");
        if (!rc) {
            hipLaunchKernelGGL(sum_ranks_i64_kernel, dim3((unsigned)((n_sums + 255) / 256)), dim3(256), 0, c->stream, d_ps, g->n_local, n_sums, t_sums);
            hipLaunchKernelGGL(sum_ranks_u32_kernel, dim3((unsigned)((n_counts + 255) / 256)), dim3(256), 0, c->stream, d_pc, g->n_local, n_counts, t_cnt);
            hip_ok(hipGetLastError(), "all-reduce (sum kernels)");
        }
        hip_ok(hipStreamSynchronize(c->stream), "all-reduce (sum)");
    }
    thread_barrier(g);   // nobody overwrites its buffer before everybody has read it
    if (rc) return rc;
    SMT_HIP_CHECK(hipMemcpyAsync(sums, t_sums, n_sums * 8, hipMemcpyDeviceToDevice, c->stream));
    SMT_HIP_CHECK(hipMemcpyAsync(counts, t_cnt, n_counts * 4, hipMemcpyDeviceToDevice, c->stream));
    return SMT_OK;
}

// IvfBuildShare::agree: the ranks meet and share a status before the first collective of a build, so that a rank whose
// set-up failed (out of memory ...) takes the others with it instead of leaving them in the all-reduce.
int group_share_agree(void *user, int rc)
{
    ShareCtx *sc = static_cast<ShareCtx *>(user);
    smt_group *g = sc->g;
    if (!rc && sc->local == 0) rc = group_debug_fail(g, SMT_DEBUG_FAIL_BUILD);
    if (g->n_local == 1) return group_agree(g, rc);
    const std::string mine = rc ? smt_last_error() : "";
    {
        std::lock_guard<std::mutex> lk(g->ar_mu);
        if (rc && !g->ar_failed) g->ar_failed = rc;
    }
    thread_barrier(g);
    const int all = g->ar_failed;
    thread_barrier(g);             // everybody has read the verdict ...
    if (sc->local == 0) g->ar_failed = 0;   // ... before it is cleared for the next build
    thread_barrier(g);
    if (rc) { set_error("%s", mine.c_str()); return rc; }
    if (all) { set_error("another shard of the group failed to set up its index build"); return all; }
    return SMT_OK;
}

}  // namespace smt
