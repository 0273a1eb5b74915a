// sharded_search.cpp -- searches over a corpus row-sharded across the ranks of a group: per-shard scan + select, the exchange of the
// packed k-lists (group_exchange.cpp), the merge where the answer is wanted; host lists where the lists have no fixed size.  Also the
// sharded IVF-PQ index: one index per shard, built alone or around shared centroids, searched through the same exchange.
#include <cmath>
#include <new>

#include "group.h"
#include "ivfpq.h"

using namespace smt;

namespace smt {

// Per-shard host search of a query subset on every local device (one host thread per device when there are
// several: the K4 / large-k paths synchronise internally and would otherwise serialise the GPUs).
static int local_host_search(smt_sharded_corpus *sc, const float *queries, uint32_t nq, uint32_t top_k, double max_distance,
                             int mode, const smt_range *ranges, uint32_t n_ranges, std::vector<std::vector<LocalHits>> &local)
{
    smt_group *g = sc->group;
    local.assign(g->n_local, std::vector<LocalHits>(nq));
    RankStatuses st(g->n_local);
    auto work = [&](int i) {
        const int r = g->first_rank + i;
        std::vector<smt_range> lr;
        if (n_ranges) {
            layout_localize(sc, r, ranges, n_ranges, lr);
            if (lr.empty()) return;  // the filter leaves this shard nothing
        }
        // a shard cut as ONE range returns global rows by adding its base; a shard of several pieces returns local rows
        // (already in global order: pieces ascend in both numberings) which are mapped piece by piece
        st.record(i, search_local_host(sc->shard[i], queries, nq, top_k, max_distance, mode, lr.empty() ? nullptr : lr.data(),
                                       (uint32_t)lr.size(), sc->contiguous ? sc->rank_base[r] : 0, local[i]));
        if (!st.rcs[i] && !sc->contiguous)
            for (LocalHits &h : local[i])
                for (uint64_t &row : h.rows) row = layout_to_global(sc, r, row);
    };
    if (g->n_local == 1) work(0);
    else if (!run_on_threads(g->n_local, work)) return SMT_E_NOMEM;
    return st.report(g);
}

// Packed lists [nq][2][k] on the host (rows | f64 bits, short lists padded with UINT64_MAX rows) -> per-query hits; queries with
// skip[q] set are left alone.
static void unpack_packed_hits(const uint64_t *h, uint32_t nq, uint32_t k, std::vector<LocalHits> &hits, const char *skip = nullptr)
{
    for (uint32_t q = 0; q < nq; ++q) {
        if (skip && skip[q]) continue;
        const uint64_t *rws = h + (size_t)q * 2 * k, *bits = rws + k;
        for (uint32_t e = 0; e < k && rws[e] != UINT64_MAX; ++e) {
            double d;
            memcpy(&d, bits + e, 8);
            hits[q].rows.push_back(rws[e]);
            hits[q].dist.push_back(d);
        }
    }
}

// The sharded index search, over everything (`filtered` off) or inside GLOBAL row ranges: validated once, localised per rank; a rank
// the ranges leave nothing still takes part and contributes an empty list.  `wide`: top_k up to LARGEK_MAX_K -- every shard answers
// 57 and above from its candidate pool (ivfpq_search.hip), and the exchange carries lists of that length as it does for
// smt_sharded_search_topk_device_ex.  Every argument is checked before anything is enqueued.
static int sharded_ivfpq_search_impl(smt_sharded_ivfpq *six, const float *queries, uint32_t nq, uint32_t top_k, uint32_t nprobe,
                                     uint32_t rerank, const smt_range *ranges, uint32_t n_ranges, bool filtered, bool wide, const char *who,
                                     uint64_t *out_rows, double *out_dist, uint64_t *out_counts, uint64_t out_cap)
{
    SMT_REQUIRE(six != nullptr, "index");
    SMT_REQUIRE(nq == 0 || (queries && out_rows && out_dist && out_counts), "null argument");
    SMT_REQUIRE(n_ranges == 0 || ranges != nullptr, "ranges");
    if (wide) SMT_REQUIRE(top_k >= 1 && top_k <= LARGEK_MAX_K, "top_k must be in [1, 1024]");
    else SMT_REQUIRE(top_k >= 1 && top_k <= SCAN_MAX_K, "top_k must be in [1, 56]");
    smt_sharded_corpus *sc = six->corpus;
    smt_group *g = sc->group;
    SMT_REQUIRE((uint64_t)g->n_ranks * top_k <= 8192, "device merge handles up to 8192 candidates per query");
    int rc;
    if (n_ranges && (rc = validate_ranges(ranges, n_ranges, sc->total()))) return rc;   // (before anything is enqueued)
    if (nq == 0) return SMT_OK;
    if (int rcq = require_queries_domain_host(queries, nq, who)) return rcq;   // (domain.hip; SPMD: all ranks alike)
    if (wide) {   // (a shard would refuse these itself, but only after the first one's work was enqueued)
        for (smt_ivfpq *ix : six->shard) {
            SMT_REQUIRE(nprobe >= 1 && nprobe <= ix->nlist && nprobe <= 512, "nprobe must be in [1, min(nlist, 512)]");
            IVF_REQUIRE_FRESH(ix);
            SMT_REQUIRE(ix->corpus->rows >= ix->n_rows, "the corpus shrank after the index was built: rebuild");
        }
        SMT_REQUIRE(rerank == 0 || (rerank >= 4 && rerank <= 512), "rerank (full-precision re-scored ADC candidates per probed list) must be in [4, 512]");
    }
    if (g->n_ranks == 1) {
        if (wide)
            return smt_ivfpq_search_wide(six->shard[0], queries, nq, top_k, nprobe, rerank, ranges, n_ranges, 0, out_rows, out_dist, out_counts, out_cap);
        return n_ranges ? smt_ivfpq_search_ranges(six->shard[0], queries, nq, top_k, nprobe, rerank, ranges, n_ranges, 0, out_rows, out_dist,
                                                  out_counts, out_cap)
                        : smt_ivfpq_search(six->shard[0], queries, nq, top_k, nprobe, rerank, 0, out_rows, out_dist, out_counts, out_cap);
    }
    const ExchangeLayout L(nq, top_k, 0, g->n_ranks, true, true);
    const size_t list_words = L.list_words;
    const bool peer = g->transport == SMT_TRANSPORT_PEER;
    static_assert(SMT_MAX_MERGE_SOURCES * SCAN_MAX_K == 3584, "a peer group's n_ranks x top_k candidates always fit the in-place merge");
    for (int i = 0; i < g->n_local; ++i) {
        const int r = g->first_rank + i;
        if ((rc = group_bind(g, i))) return rc;
        if ((rc = ensure_dev(g, i, L.dev_bytes))) return rc;
        char *base = reinterpret_cast<char *>(g->buf[i].dev);
        uint64_t *loc = exchange_list(g, i, L, -1);
        if ((rc = drain_async(g->ctx[i]))) return rc;   // (see smt_sharded_search: the buffer may still be read on the aux stream)
        SMT_HIP_CHECK(hipMemcpyAsync(base, queries, (size_t)nq * SMT_DIM * 4, hipMemcpyHostToDevice, g->ctx[i]->stream));
        std::vector<smt_range> lr;
        if (n_ranges) layout_localize(sc, r, ranges, n_ranges, lr);
        if ((rc = ivfpq_search_packed(six->shard[i], reinterpret_cast<const float *>(base), nq, top_k, nprobe, rerank, lr.data(),
                                      (uint32_t)lr.size(), filtered, sc->contiguous ? sc->rank_base[r] : 0, loc, wide)))
            return rc;
        if (!sc->contiguous && (rc = layout_translate_packed(sc, i, g->ctx[i]->stream, loc, nq, top_k))) return rc;
        if (peer && (rc = peer_publish(g, i, g->ctx[i]->stream))) return rc;
    }
    if (!peer && (rc = allgather_words(g, L.loc_off, L.gath_off, list_words))) return rc;
    uint64_t *merged = reinterpret_cast<uint64_t *>(reinterpret_cast<char *>(g->buf[0].dev) + L.out_off);
    if ((rc = merge_ranks_on(g, 0, g->ctx[0]->stream, L, -1, nq, top_k, merged))) return rc;
    if ((rc = ensure_host(g, 0, list_words * 8))) return rc;
    uint64_t *h = reinterpret_cast<uint64_t *>(g->buf[0].pinned);
    SMT_HIP_CHECK(hipMemcpyAsync(h, merged, list_words * 8, hipMemcpyDeviceToHost, g->ctx[0]->stream));
    if ((rc = group_sync_all(g))) return rc;
    std::vector<LocalHits> hits(nq);
    unpack_packed_hits(h, nq, top_k, hits);
    return deliver_hits(hits, out_rows, out_dist, out_counts, out_cap);
}

}  // namespace smt

extern "C" {

/* ----------------------------------------------------------------- search ---- */

int smt_sharded_search(smt_sharded_corpus *sc, const float *queries, uint32_t nq, uint32_t top_k, double max_distance, int mode,
                       const smt_range *ranges, uint32_t n_ranges, uint64_t *out_rows, double *out_dist, uint64_t *out_counts,
                       uint64_t out_cap)
try {
    SMT_REQUIRE(sc != nullptr, "corpus");
    SMT_REQUIRE(mode == SMT_MODE_DOCUMENTS || mode == SMT_MODE_WORKSPACE, "mode");
    SMT_REQUIRE(nq == 0 || (queries && out_counts), "null argument");
    SMT_REQUIRE(n_ranges == 0 || ranges != nullptr, "ranges");
    smt_group *g = sc->group;
    if (nq == 0) return SMT_OK;
    // (domain.hip; SPMD callers pass the same host arguments, so every rank refuses together, before any collective)
    if (int rcq = require_queries_domain_host(queries, nq, "smt_sharded_search")) return rcq;
    if (g->n_ranks == 1)   // one shard: the single-GPU call, nothing to exchange
        return smt_search(sc->shard[0], queries, nq, top_k, max_distance, mode, ranges, n_ranges, 0, out_rows, out_dist, out_counts, out_cap);
    for (uint32_t q = 0; q < nq; ++q) out_counts[q] = 0;
    const uint64_t total = sc->total();
    int rc;
    if (n_ranges && (rc = validate_ranges(ranges, n_ranges, total))) return rc;
    uint64_t n_virtual = total;
    if (n_ranges) {
        n_virtual = 0;
        for (uint32_t i = 0; i < n_ranges; ++i) n_virtual += ranges[i].end - ranges[i].begin;
    }
    const bool has_thr = !std::isnan(max_distance);
    const bool all_under_threshold = (mode == SMT_MODE_DOCUMENTS) && has_thr;
    if (n_virtual == 0) return SMT_OK;
    if (!all_under_threshold && top_k == 0) return SMT_OK;

    std::vector<LocalHits> hits(nq);
    const uint32_t K = (uint32_t)std::min<uint64_t>(top_k, n_virtual);
    const bool device_exchange = !all_under_threshold && K <= SCAN_MAX_K && (uint64_t)g->n_ranks * K <= 8192;
    std::vector<uint32_t> redo;  // queries answered through the host-list exchange
    if (device_exchange) {
        // ---- per-shard scan + select -> packed lists -> ONE all-gather -> device merge
        // per rank: the lists, one "uncertain" word per query, one STATUS word -- a rank whose local stage failed still
        // takes part in the all-gather and says so there, so that every process returns the error together (a rank
        // that simply left would strand the others inside the collective)
        const ExchangeLayout L(nq, K, (size_t)nq + 1, g->n_ranks, true, true);
        const size_t list_words = L.list_words;
        const int ws = (mode == SMT_MODE_WORKSPACE && has_thr) ? 1 : 0;
        const float thr_score = 1.0f - (float)max_distance;  // store.rs:502-503
        // Pinned staging per local device: [queries][status word] (+ device 0: the merged lists and every rank's flags).  A device's
        // share only ENQUEUES -- upload, scan, select, status -- and the shares of a one-process group are issued at once by the
        // group's issuing threads (group_for_each_local), so the shards scan concurrently and the caller's thread pays for one.
        // (a stack status word once forced a stream sync per device here, i.e. the SUM of the shard times.)
        const size_t flag_words = (size_t)g->n_ranks * (nq + 1);
        const size_t pin_status_off = L.loc_off, pin_res_off = L.loc_off + 64;
        // peer transport (one-process groups): no gather -- device 0's merge reads the ranks' lists in place, every rank copies
        // its own flag words to its own pinned block on its own stream (issued by its thread)
        const bool peer = g->transport == SMT_TRANSPORT_PEER;
        RankStatuses stage(g->n_local);
        rc = group_for_each_local(g, [&](int i) -> int {
            const int r = g->first_rank + i;
            int rc_i;
            if ((rc_i = group_bind(g, i))) return rc_i;
            if ((rc_i = ensure_dev(g, i, L.dev_bytes))) return rc_i;   // (no exchange buffer: nothing to report through)
            if ((rc_i = ensure_host(g, i, pin_res_off + (i == 0 ? (list_words + flag_words) * 8 : (size_t)(nq + 1) * 8)))) return rc_i;
            char *base = reinterpret_cast<char *>(g->buf[i].dev);
            char *pin = reinterpret_cast<char *>(g->buf[i].pinned);
            uint64_t *loc = exchange_list(g, i, L, -1);
            // a pipelined smt_sharded_search_topk_device (rccl / copy transport) may still be gathering out of this buffer on the aux stream
            if ((rc_i = drain_async(g->ctx[i]))) return rc_i;
            const int stage_rc = [&]() -> int {
                memcpy(pin, queries, (size_t)nq * SMT_DIM * 4);
                SMT_HIP_CHECK(hipMemcpyAsync(base, pin, (size_t)nq * SMT_DIM * 4, hipMemcpyHostToDevice, g->ctx[i]->stream));
                std::vector<smt_range> lr;
                if (n_ranges) layout_localize(sc, r, ranges, n_ranges, lr);
                int rc2 = search_topk_packed_local(sc->shard[i], reinterpret_cast<const float *>(base), nq, K, ws, thr_score, lr.data(),
                                                   (uint32_t)lr.size(), n_ranges != 0, sc->contiguous ? sc->rank_base[r] : 0, loc,
                                                   loc + list_words, false);
                if (!rc2 && !sc->contiguous) rc2 = layout_translate_packed(sc, i, g->ctx[i]->stream, loc, nq, K);
                if (!rc2 && i == 0) rc2 = group_debug_fail(g, SMT_DEBUG_FAIL_STAGE);
                return rc2;
            }();
            stage.record(i, stage_rc);
            uint64_t *status = reinterpret_cast<uint64_t *>(pin + pin_status_off);   // lives in the pinned buffer until group_sync_all
            *status = (uint64_t)(uint32_t)(stage_rc < 0 ? -stage_rc : stage_rc);
            SMT_HIP_CHECK(hipMemcpyAsync(loc + list_words + nq, status, 8, hipMemcpyHostToDevice, g->ctx[i]->stream));
            if (peer) {
                uint64_t *my_flags = reinterpret_cast<uint64_t *>(pin + pin_res_off) + (i == 0 ? list_words : 0);
                SMT_HIP_CHECK(hipMemcpyAsync(my_flags, loc + list_words, (size_t)(nq + 1) * 8, hipMemcpyDeviceToHost, g->ctx[i]->stream));
                if ((rc_i = peer_publish(g, i, g->ctx[i]->stream))) return rc_i;
            }
            return SMT_OK;
        }, g->workers != nullptr);
        if (rc) return rc;
        const int local_rc = stage.failed();
        if (!peer && (rc = allgather_words(g, L.loc_off, L.gath_off, L.rank_words))) return rc;
        // the caller is one host thread and needs ONE copy of the answer: merge on local device 0
        // (this entry point ends with every stream drained: the next call may overwrite the lists without asking)
        if ((rc = group_bind(g, 0))) return rc;
        char *base0 = reinterpret_cast<char *>(g->buf[0].dev);
        uint64_t *gath = reinterpret_cast<uint64_t *>(base0 + L.gath_off), *merged = reinterpret_cast<uint64_t *>(base0 + L.out_off);
        uint64_t *h = reinterpret_cast<uint64_t *>(reinterpret_cast<char *>(g->buf[0].pinned) + pin_res_off);
        if (!local_rc && (rc = merge_ranks_on(g, 0, g->ctx[0]->stream, L, -1, nq, K, merged))) return rc;
        for (int r = 0; !peer && r < g->n_ranks; ++r)  // every rank's flags + status: all processes take the same decisions
            SMT_HIP_CHECK(hipMemcpyAsync(h + list_words + (size_t)r * (nq + 1), gath + (size_t)r * L.rank_words + list_words, (size_t)(nq + 1) * 8,
                                         hipMemcpyDeviceToHost, g->ctx[0]->stream));
        if (!local_rc) SMT_HIP_CHECK(hipMemcpyAsync(h, merged, list_words * 8, hipMemcpyDeviceToHost, g->ctx[0]->stream));
        if ((rc = group_sync_all(g))) return rc;
        if (local_rc) return stage.report(g, false);
        // rank r's [nq uncertain flags][status]: gathered into device 0's block, or (peer) in rank r's own pinned block
        auto flags_of = [&](int r) -> const uint64_t * {
            if (!peer || r == 0) return h + list_words + (size_t)r * (nq + 1);
            return reinterpret_cast<const uint64_t *>(reinterpret_cast<const char *>(g->buf[r].pinned) + pin_res_off);
        };
        for (int r = 0; r < g->n_ranks; ++r) {
            const uint64_t st = flags_of(r)[nq];
            if (st) { set_error("rank %d failed with status -%llu; this rank gives up with it", r, (unsigned long long)st); return -(int)st; }
        }
        std::vector<char> uncertain(nq, 0);
        for (uint32_t q = 0; q < nq; ++q) {
            for (int r = 0; r < g->n_ranks; ++r) uncertain[q] |= flags_of(r)[q] != 0;
            if (uncertain[q]) redo.push_back(q);
        }
        unpack_packed_hits(h, nq, K, hits, uncertain.data());
    } else {
        for (uint32_t q = 0; q < nq; ++q) redo.push_back(q);
    }
    if (!redo.empty()) {
        // threshold mode, top_k > 56, or queries whose exactness certificate failed on some shard: per-shard host
        // lists (each shard's own search is exact, fallback included), exchanged at their true sizes
        std::vector<float> sub((size_t)redo.size() * SMT_DIM);
        for (size_t j = 0; j < redo.size(); ++j) memcpy(&sub[j * SMT_DIM], queries + (size_t)redo[j] * SMT_DIM, SMT_DIM * 4);
        std::vector<std::vector<LocalHits>> local;
        rc = local_host_search(sc, sub.data(), (uint32_t)redo.size(), top_k, max_distance, mode, ranges, n_ranges, local);
        if ((rc = group_agree(g, rc))) return rc;   // (a rank whose shard search failed must not leave the others in the exchange)
        std::vector<LocalHits> merged;
        if ((rc = exchange_host_lists(g, local, (uint32_t)redo.size(), all_under_threshold ? UINT64_MAX : (uint64_t)top_k, merged)))
            return rc;
        for (size_t j = 0; j < redo.size(); ++j) hits[redo[j]] = std::move(merged[j]);
    }
    if (mode == SMT_MODE_WORKSPACE)   // (a zero query's answer is a constant: search.cpp workspace_zero_query_hits -- the same on every rank)
        for (uint32_t q = 0; q < nq; ++q)
            if (query_is_zero(queries + (size_t)q * SMT_DIM))
                workspace_zero_query_hits(ranges, n_ranges, total, top_k, has_thr, max_distance, 0, hits[q]);
    return deliver_hits(hits, out_rows, out_dist, out_counts, out_cap);
} catch (...) { return smt::api_catch(); }

int smt_sharded_search_topk_device(smt_sharded_corpus *sc, const float *const *queries_dev, uint32_t nq, uint32_t top_k,
                                   uint64_t *const *out_packed)
try {
    return smt_sharded_search_topk_device_ex(sc, queries_dev, nq, top_k, out_packed, nullptr);
} catch (...) { return smt::api_catch(); }

int smt_sharded_search_topk_device_ex(smt_sharded_corpus *sc, const float *const *queries_dev, uint32_t nq, uint32_t top_k,
                                      uint64_t *const *out_packed, uint32_t *const *out_status)
try {
    SMT_REQUIRE(sc && queries_dev && out_packed, "null argument");
    smt_group *g = sc->group;
    // 57 <= top_k <= 1024: every shard takes the large-k route (topk_large.hip, tuning key largek_sampled); the buffers below follow
    // rank_words, the merges take n_ranks x top_k <= 8192 candidates
    const bool largek = g->ctx[0]->tune.largek_sampled != 0;
    SMT_REQUIRE(top_k >= 1 && top_k <= (largek ? LARGEK_MAX_K : SCAN_MAX_K),
                largek ? "top_k must be in [1, 1024]" : "top_k must be in [1, 56] (largek_sampled = 0)");
    SMT_REQUIRE((uint64_t)g->n_ranks * top_k <= 8192, "device merge handles up to 8192 candidates per query");
    // (refused here, before a ring slot is taken and any rank's scan is enqueued)
    for (int i = 0; out_status && i < g->n_local; ++i)
        SMT_REQUIRE(!out_status[i] || out_packed[i], "a device that wants the verdicts takes the answer too");
    if (nq == 0) return SMT_OK;
    // with per-query verdicts wanted, every rank's nq status words (SMT_STATUS_* codes written by its select) travel behind its lists
    bool want_status = false;
    for (int i = 0; out_status && i < g->n_local; ++i) want_status = want_status || out_status[i] != nullptr;
    const ExchangeLayout L(nq, top_k, want_status ? nq : 0, g->n_ranks, false, false);
    std::vector<char> on_aux(g->n_local, 0);
    const bool peer = g->transport == SMT_TRANSPORT_PEER;
    int rc;
    for (int i = 0; i < g->n_local; ++i) SMT_REQUIRE(queries_dev[i] != nullptr, "queries_dev");
    // the select of a single query may run on the aux stream while the NEXT call's scan streams (async select); the exchange and
    // the merge then follow it there, and the main stream carries nothing but scans
    for (int i = 0; i < g->n_local; ++i) on_aux[i] = g->ctx[i]->tune.async_select && nq == 1 && sc->shard[i]->rows >= top_k && top_k <= SCAN_MAX_K ? 1 : 0;
    // (the aux streams exist before anything names them: the first async scan of a context would make its own only inside the
    // rank's search below, after exchange_stream had answered with a null stream -- the list was then published, and awaited by
    // the other ranks' issuers, on the default stream, which orders nothing against the select)
    for (int i = 0; i < g->n_local; ++i)
        if (on_aux[i] && ((rc = group_bind(g, i)) || (rc = ensure_async(g->ctx[i])))) return rc;
    WaitBoard board(g, on_aux, out_packed);   // (peer transport with issuing threads: the ranks' issuers enqueue the merges' waits)
    int slot = -1;
    if (peer) {   // rank j writes its list into slot `slot` of its ring; whoever needs the answer reads the slots in place
        if ((rc = ring_ensure(g, L.rank_words * 8))) return rc;
        if ((rc = ring_next_slot(g, &slot))) return rc;
    }
    // every device's scan + select is issued by its own thread (group_for_each_local); the collective follows on this one
    rc = group_for_each_local(g, [&](int i) -> int {
        const int r = g->first_rank + i;
        int rc_i;
        if ((rc_i = group_bind(g, i))) return rc_i;
        if (!peer && (rc_i = ensure_dev(g, i, L.dev_bytes))) return rc_i;
        smt_ctx *c = g->ctx[i];
        const bool async = on_aux[i] != 0;
        const hipStream_t st = exchange_stream(g, i, &on_aux);
        uint64_t *list = exchange_list(g, i, L, slot);
        rc_i = search_topk_packed_local(sc->shard[i], queries_dev[i], nq, top_k, 0, 0.f, nullptr, 0, false,
                                        sc->contiguous ? sc->rank_base[r] : 0, list, want_status ? list + L.list_words : nullptr, async);
        if (rc_i) return rc_i;
        if (!sc->contiguous && (rc_i = layout_translate_packed(sc, i, st, list, nq, top_k))) return rc_i;
        if (async) c->async_pending = true;
        if (out_packed[i]) prof_begin_on(c, "exchange", st);   // this rank's list is ready: the wait for the others starts
        if (peer && (rc_i = peer_publish(g, i, st))) return rc_i;
        if (board.active && ((rc_i = board.own_work_issued(i)) || (rc_i = board.published(i)))) return rc_i;
        return SMT_OK;
    }, g->workers != nullptr);
    if (!rc) rc = board.sweep();   // (a merging device whose issuer failed before raising its flag leaves bits behind: the call fails anyway)
    if (rc) return rc;
    if (!peer && (rc = allgather_words(g, 0, L.gath_off, L.rank_words, &on_aux))) return rc;
    for (int i = 0; i < g->n_local; ++i) {
        uint32_t *status_i = out_status ? out_status[i] : nullptr;
        if (!out_packed[i]) continue;
        const hipStream_t st = exchange_stream(g, i, &on_aux);
        // (peer: an answer wanted on ONE device -- the one-thread caller of SURVEY 8(b) -- costs n - 1 waits + a launch + a record here;
        //  the verdicts are read in place like the lists, by a second small kernel between the merge and the slot's `done` record)
        hipEvent_t done = nullptr;
        if (peer && (rc = ring_done_event(g, slot, i, &done))) return rc;
        if ((rc = merge_ranks_on(g, i, st, L, slot, nq, top_k, out_packed[i], status_i ? nullptr : done, board.active))) return rc;
        if (status_i) {
            if ((rc = combine_ranks_status_on(g, i, st, L, slot, nq, status_i))) return rc;
            if (done) SMT_HIP_CHECK(hipEventRecord(done, st));
        }
        if (peer && on_aux[i]) g->ctx[i]->async_pending = true;
    }
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

/* ------------------------------------------------------------ sharded IVF ---- */

int smt_sharded_ivfpq_build(smt_sharded_corpus *sc, const smt_ivfpq_params *params, int shared_centroids, smt_sharded_ivfpq **out)
try {
    SMT_REQUIRE(sc && params && out, "null argument");
    *out = nullptr;
    smt_group *g = sc->group;
    for (int r = 0; r < g->n_ranks; ++r)  // checked on EVERY rank's size: a rank bailing out alone would leave the others in the all-reduce
        SMT_REQUIRE(sc->rank_rows[r] >= params->nlist, "every shard needs at least nlist rows");
    smt_sharded_ivfpq *six = new (std::nothrow) smt_sharded_ivfpq();
    if (!six) { set_error("out of host memory"); return SMT_E_NOMEM; }
    six->corpus = sc;
    six->shared_centroids = shared_centroids ? 1 : 0;
    six->shard.assign(g->n_local, nullptr);
    RankStatuses st(g->n_local);
    std::vector<ShareCtx> sctx(g->n_local);
    // one host thread per local rank: the all-reduce inside the k-means loop needs every rank in it at once
    auto work = [&](int i) {
        IvfBuildShare share;
        share.rank = (uint32_t)(g->first_rank + i);
        share.n_ranks = (uint32_t)g->n_ranks;
        share.allreduce = group_allreduce_sums;
        share.agree = group_share_agree;
        sctx[i] = ShareCtx{g, i};
        share.user = &sctx[i];
        st.record(i, ivfpq_build_shared(sc->shard[i], params, shared_centroids ? &share : nullptr, &six->shard[i]));
    };
    if (g->n_local == 1) work(0);
    else if (!run_on_threads(g->n_local, work)) { smt_sharded_ivfpq_destroy(six); return SMT_E_NOMEM; }
    if (const int rc = st.report(g)) { smt_sharded_ivfpq_destroy(six); return rc; }
    *out = six;
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

void smt_sharded_ivfpq_destroy(smt_sharded_ivfpq *six)
{
    if (!six) return;
    for (smt_ivfpq *ix : six->shard) smt_ivfpq_destroy(ix);
    delete six;
}

smt_ivfpq *smt_sharded_ivfpq_shard(smt_sharded_ivfpq *six, int local_index)
{
    if (!six || local_index < 0 || local_index >= (int)six->shard.size()) return nullptr;
    return six->shard[local_index];
}

int smt_sharded_ivfpq_search(smt_sharded_ivfpq *six, const float *queries, uint32_t nq, uint32_t top_k, uint32_t nprobe, uint32_t rerank,
                             uint64_t *out_rows, double *out_dist, uint64_t *out_counts, uint64_t out_cap)
try {
    return sharded_ivfpq_search_impl(six, queries, nq, top_k, nprobe, rerank, nullptr, 0, false, false, "smt_sharded_ivfpq_search", out_rows,
                                     out_dist, out_counts, out_cap);
} catch (...) { return smt::api_catch(); }

int smt_sharded_ivfpq_search_ranges(smt_sharded_ivfpq *six, const float *queries, uint32_t nq, uint32_t top_k, uint32_t nprobe,
                                    uint32_t rerank, const smt_range *ranges, uint32_t n_ranges, uint64_t *out_rows, double *out_dist,
                                    uint64_t *out_counts, uint64_t out_cap)
try {
    return sharded_ivfpq_search_impl(six, queries, nq, top_k, nprobe, rerank, ranges, n_ranges, n_ranges != 0, false,
                                     "smt_sharded_ivfpq_search_ranges", out_rows, out_dist, out_counts, out_cap);
} catch (...) { return smt::api_catch(); }

int smt_sharded_ivfpq_search_wide(smt_sharded_ivfpq *six, const float *queries, uint32_t nq, uint32_t top_k, uint32_t nprobe,
                                  uint32_t rerank, const smt_range *ranges, uint32_t n_ranges, uint64_t *out_rows, double *out_dist,
                                  uint64_t *out_counts, uint64_t out_cap)
try {
    return sharded_ivfpq_search_impl(six, queries, nq, top_k, nprobe, rerank, ranges, ranges ? n_ranges : 0, ranges != nullptr, true,
                                     "smt_sharded_ivfpq_search_wide", out_rows, out_dist, out_counts, out_cap);
} catch (...) { return smt::api_catch(); }

}  // extern "C"
