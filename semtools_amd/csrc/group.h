// group.h -- internal declarations shared by group.cpp (the RCCL binding, group life cycle, issuing threads, barriers),
// group_exchange.cpp (the transports that move lists between ranks, and the merges on top of them), sharded_search.cpp (the sharded
// search entry points and the sharded IVF index) and sharded.cpp (the sharded corpus' row layout and storage, the replicated
// model + sharded embed).
#pragma once
#include <rccl/rccl.h>

#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "common.h"

// One exchange workspace per local device, grown on demand.
struct GroupBuf {
    void *dev = nullptr;
    size_t dev_bytes = 0;
    void *pinned = nullptr;
    size_t pinned_bytes = 0;
};

// What every local rank made of one step: its status and, where it failed, the message of the thread that ran it.
struct smt_group;
struct RankStatuses {
    std::vector<int> rcs;
    std::vector<std::string> errs;
    explicit RankStatuses(int n = 0) : rcs(n, SMT_OK), errs(n) {}
    void record(int i, int rc);   // rank i's status, with the calling thread's last error when it failed
    int failed() const;           // the first failing rank's status, 0 if none
    // the first failing rank's status and its message, as "shard %d: ..." with `prefix`, as this thread's error; 0 if none
    int report(const smt_group *g, bool prefix = true) const;
};

// Issuing threads: one per local device of a single-process group.  The caller is ONE synchronous host thread
// (src/bin/semtools.rs:134-135); issuing a search for 8 shards from it costs 8 x (bind + upload + scan + select launches) in a row --
// measured 16 us per shard (profiles/r04_group_issue.json), i.e. about one shard's whole 150 us scan at 1 M rows.  The workers issue
// every device's share at once; collectives stay on the caller's thread (ncclGroupStart / End needs all local ranks in one thread).
struct GroupWorkers {
    std::vector<std::thread> threads;
    int n_threads = 0;               // thread t issues the shares of local ranks t, t + n_threads, ...
    std::mutex mu;
    std::condition_variable cv_go, cv_done;
    const std::function<int(int)> *work = nullptr;
    // A search arrives every ~100 us in a pipelined caller: a thread that blocks in the kernel between two of them pays a futex wake
    // each way, and what that costs is the HOST's business (idle states): the same binary issued an 8-shard search in 56-67 us on
    // some leases and 85-95 on others.  So both sides SPIN first -- a worker for `spin_ns` after its last share, the caller while the
    // shares are being issued -- and only then block on the condition variables (the usual two-flag hand-over: whoever is about to
    // block says so, seq_cst, before its last look at the other side's counter).
    std::atomic<uint64_t> epoch{0};
    std::atomic<int> pending{0};
    std::atomic<int> sleepers{0};        // workers blocked (or about to block) on cv_go
    std::atomic<int> caller_blocked{0};  // the caller is blocked (or about to block) on cv_done
    std::atomic<bool> stop{false};
    long long spin_ns = 100000;          // $SEMTOOLS_GROUP_SPIN_US (0: block at once)
    RankStatuses status;                 // [n_local] slot i belongs to rank i's thread until `pending` reaches 0
};

struct smt_group {
    GroupWorkers *workers = nullptr; // n_local > 1: persistent issuing threads (group_for_each_local)
    int n_ranks = 0;
    int n_local = 0;
    int first_rank = 0;              // local device i is rank first_rank + i
    std::vector<smt_ctx *> ctx;      // [n_local], owned unless `borrowed`
    bool borrowed = false;           // smt_group_from_ctx: a one-rank group around a context the caller keeps
    std::vector<ncclComm_t> comm;    // [n_local]
    std::vector<GroupBuf> buf;       // [n_local]
    int rccl_version = 0;
    // Copy transport (smt_group_create_logical): every rank is a context of THIS process, possibly several on one
    // device; the all-gather is n x n device copies ordered by events instead of an RCCL collective.
    bool copies = false;
    std::vector<hipEvent_t> ev_ready;   // [n_local] rank j's send buffer is complete
    std::vector<hipEvent_t> ev_done;    // [n_local] rank i has finished reading everybody's send buffer
    // Peer transport (SMT_TRANSPORT_PEER, the default of every one-process group whose devices can read each other's memory):
    // the per-shard k-lists are not moved at all -- the merge kernel of the device that needs the answer loads them from the
    // ranks' exchange buffers where they lie (merge_topk_sources_kernel), ordered by ONE event per rank: ev_ready[j] after rank j's
    // select.  An answer costs n - 1 stream waits (enqueued by the ranks' issuers, see spread_waits) + one launch + one record; an RCCL all-gather of the same
    // 960 B costs ncclGroupStart + n ncclAllGather + ncclGroupEnd there.
    int transport = SMT_TRANSPORT_RCCL;
    bool peer_ok = false;               // every local device may read every other local device's memory
    std::vector<hipStream_t> pub_stream;   // [n_local] the stream ev_ready[j] was last recorded on
    // Who enqueues the n - 1 waits in front of a merge: the issuer of rank j, right behind its own event record (`spread_waits`: the
    // waits of one answer are spread over the issuing threads instead of queueing on the caller's thread -- ~3-5 us each), or the
    // caller's thread in peer_merge.  Checked by the self-test at creation: a runtime that refuses a wait enqueued on another
    // device's stream turns it off.  $SEMTOOLS_GROUP_WAITS=caller turns it off too (A/B).
    bool spread_waits = true;
    // The pipelined entry point (smt_sharded_search_topk_device: nothing synchronises) writes rank j's list of exchange e into slot
    // e % slots of rank j's RING, so that no rank ever waits for a reader on the device: a slot is reused `slots` exchanges later,
    // and the caller's thread first makes sure -- hipEventSynchronize on an event that has long completed, or real back-pressure
    // when the host runs `slots` searches ahead of the GPUs -- that the merges which read it are over.  (One cross-stream
    // hipStreamWaitEvent costs ~3-5 us of host time: a per-rank wait for the previous merge would double the exchange's cost.)
    struct Ring {
        std::vector<void *> dev;                    // [n_local] slots x slot_bytes
        size_t slot_bytes = 0;
        int slots = 0;
        uint64_t seq = 0;                           // exchanges issued
        std::vector<std::vector<hipEvent_t>> done;  // [slots][n_local], made on first use: device i's merge of the slot's exchange is over
        std::vector<uint64_t> merged;               // [slots] bit i: done[slot][i] was recorded for the slot's last exchange
    } ring;
    // copy-transport all-reduce (shared-centroid IVF builds run one host thread per local rank): a thread barrier
    // and the ranks' buffer addresses
    std::mutex ar_mu;
    std::condition_variable ar_cv;
    int ar_waiting = 0;
    uint64_t ar_generation = 0;
    int ar_failed = 0;               // first failure reported to group_share_agree by a rank's thread
    std::vector<const long long *> ar_sums;
    std::vector<const unsigned int *> ar_counts;
    // smt_debug_group_fail_next (test hook): the next local step of kind `debug_fail_where` on THIS process's ranks fails with
    // `debug_fail_code` -- how the tests make ONE rank of a multi-process group fail and check that all of them return together
    std::atomic<int> debug_fail_where{0};
    int debug_fail_code = 0;
};

struct smt_sharded_ivfpq {
    smt_sharded_corpus *corpus = nullptr;
    std::vector<smt_ivfpq *> shard;     // [n_local]
    int shared_centroids = 0;
};

// A run of consecutive GLOBAL rows held by one rank as consecutive LOCAL rows.
struct ShardPiece {
    uint64_t global_begin = 0, n_rows = 0, local_begin = 0;
    int rank = 0;
};

// Global rows are INSERTION ORDER over the whole corpus (the reference's tie order: document, then line --
// src/search/mod.rs:84-85,107-111).  A corpus built in one go is cut into one contiguous range per rank
// (rows_per_rank = ceil(N / n_ranks)).  A corpus that GROWS (the workspace store) deals every append over the
// ranks so that all GPUs keep embedding and scanning equal shares: the numbering is then a list of pieces.  Inside one
// rank pieces ascend in both numberings, so "local row asc" == "global row asc" there and every per-shard list is
// already in the reference's order; across ranks the merge compares (distance, global row).
struct smt_sharded_corpus {
    smt_group *group = nullptr;
    uint32_t dim = SMT_DIM;
    std::vector<smt_corpus *> shard;   // [n_local], owned handles (rows themselves may be adopted device memory)
    std::vector<uint64_t> rank_rows;   // [n_ranks]
    std::vector<uint64_t> rank_base;   // [n_ranks + 1] exclusive prefix of rank_rows; the ranks' first GLOBAL rows iff `contiguous`
    std::vector<ShardPiece> pieces;    // ascending global_begin, covering [0, total) exactly
    std::vector<std::vector<uint32_t>> rank_pieces;   // [n_ranks] indices into `pieces`, ascending (local and global)
    bool contiguous = true;            // one piece per non-empty rank, in rank order
    // device copies of the local ranks' piece tables ([n][3] u64: local_begin, n_rows, global_begin) for layout_translate_packed
    std::vector<void *> d_table;       // [n_local]
    std::vector<size_t> d_table_cap;   // [n_local] entries allocated
    std::vector<uint64_t> d_table_version;   // [n_local] layout_version the copy was made from
    uint64_t layout_version = 1;
    uint64_t total() const { return rank_base.empty() ? 0 : rank_base.back(); }
};

// The embedding table replicated on every local device ("K1 shards by line with a replicated table").
struct smt_sharded_model {
    smt_group *group = nullptr;
    std::vector<smt_model *> model;    // [n_local]
};

namespace smt {

// ---- groups (group.cpp)
int group_bind(smt_group *g, int i);
int group_sync_all(smt_group *g);
int sync_every_stream(smt_group *g);   // group_sync_all + the aux streams
// the RCCL halves of allgather_words and group_allreduce_sums (the binding is private to group.cpp)
int rccl_allgather_words(smt_group *g, size_t send_off, size_t recv_off, size_t words, const std::vector<char> *on_aux);
int rccl_allreduce_sums(smt_group *g, int i, long long *sums, size_t n_sums, unsigned int *counts, size_t n_counts);
// fn(i) for i in [0, n) on n threads that all exist before any starts; false (error set) = they could not be had and nothing ran
bool run_on_threads(int n, const std::function<void(int)> &fn);
int group_barrier(smt_group *g);
// Barrier that carries a status: every rank contributes `rc` and all of them return the first non-zero one (0 if none).
// Error paths of collective operations go through this so that no rank leaves while the others wait.
int group_agree(smt_group *g, int rc);
// the test hook's trigger: non-zero (an error status, message set) once if a failure of kind `where` is armed on the group
int group_debug_fail(smt_group *g, int where);
// run work(i) for every local device, on one host thread per device when there are several; first error wins
int group_for_each_local(smt_group *g, const std::function<int(int)> &work, bool threads = true);

// ---- exchange (group_exchange.cpp)
constexpr size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
// One exchange buffer: [queries | local list + `extra_words` (flags, statuses) | gathered: n_ranks of those | merged list], every
// region 256-byte aligned.  Host-in searches have all four; the device form has neither queries nor a merged list.
struct ExchangeLayout {
    size_t list_words, rank_words;       // per rank: the [nq][2][k] lists; the same + the words behind them
    size_t loc_off, gath_off, out_off;   // BYTE offsets of the local list, the gathered block, the merged list (0: none)
    size_t dev_bytes;
    constexpr ExchangeLayout(uint32_t nq, uint32_t k, size_t extra_words, int n_ranks, bool has_queries, bool has_merged)
        : list_words((size_t)nq * 2 * k), rank_words(list_words + extra_words),
          loc_off(has_queries ? align256((size_t)nq * SMT_DIM * 4) : 0), gath_off(loc_off + align256(rank_words * 8)),
          out_off(has_merged ? gath_off + align256((size_t)n_ranks * rank_words * 8) : 0),
          dev_bytes((has_merged ? out_off + list_words * 8 : gath_off + (size_t)n_ranks * rank_words * 8) + 64) {}
};
static_assert(ExchangeLayout(3, 56, 4, 8, true, true).out_off == 3072 + 2816 + 21760 && ExchangeLayout(3, 56, 4, 8, true, true).dev_bytes == 27648 + 2688 + 64 &&
              ExchangeLayout(1, 10, 1, 3, false, false).dev_bytes == 256 + 3 * 168 + 64, "exchange layout");

int ensure_dev(smt_group *g, int i, size_t bytes);
int ensure_host(smt_group *g, int i, size_t bytes);
inline hipStream_t exchange_stream(const smt_group *g, int i, const std::vector<char> *on_aux)
{
    return (on_aux && (*on_aux)[i]) ? g->ctx[i]->aux_stream : g->ctx[i]->stream;
}
// All-gather `words` u64 per rank: send_off / recv_off are BYTE offsets into each local device's exchange buffer.
int allgather_words(smt_group *g, size_t send_off, size_t recv_off, size_t words, const std::vector<char> *on_aux = nullptr);
// Every local rank i contributes the `w` host words mine[i * w ..]; all-gather; `all` = the n_ranks x w words as local device 0
// received them, every stream drained -- or (`every_local`) as each local device did, [n_local][n_ranks][w], each read synchronised.
int gather_host_words(smt_group *g, size_t w, const uint64_t *mine, std::vector<uint64_t> &all, bool every_local = false);
// Rank j's list of an exchange: in its exchange buffer at L.loc_off (slot < 0), or in slot `slot` of its ring.
uint64_t *exchange_list(smt_group *g, int j, const ExchangeLayout &L, int slot);
// Peer transport, rank j, after the last kernel that writes its list on `st`.
int peer_publish(smt_group *g, int j, hipStream_t st);
// The caller's thread, after every local rank has published (peer) or after allgather_words: local device i merges the ranks'
// packed lists [nq][2][k] into out_packed on its stream `st` -- read in place (peer transport; `waits_enqueued`: the ranks' issuers
// have enqueued the waits, WaitBoard) or from the gathered block; `done` (may be null) is recorded behind the merge.  Records the
// "exchange" / "merge" profiling pairs.  combine_ranks_status_on: the same sources' nq status words, worst of the ranks.
int merge_ranks_on(smt_group *g, int i, hipStream_t st, const ExchangeLayout &L, int slot, uint32_t nq, uint32_t k, uint64_t *out_packed,
                   hipEvent_t done = nullptr, bool waits_enqueued = false);
int combine_ranks_status_on(smt_group *g, int i, hipStream_t st, const ExchangeLayout &L, int slot, uint32_t nq, uint32_t *out_status);
void ring_free(smt_group *g);
int ring_ensure(smt_group *g, size_t slot_bytes);
int ring_next_slot(smt_group *g, int *slot_out);
int ring_done_event(smt_group *g, int slot, int i, hipEvent_t *ev);
bool peer_self_test(smt_group *g);
// per-rank host lists of any length -> the first `keep` of their (distance, row) merge, per query
int exchange_host_lists(smt_group *g, const std::vector<std::vector<LocalHits>> &local, uint32_t nq, uint64_t keep, std::vector<LocalHits> &merged);
// IvfBuildShare::allreduce / ::agree for local rank `local` of g (user = a ShareCtx), called from that rank's host thread
struct ShareCtx { smt_group *g; int local; };
int group_allreduce_sums(void *user, long long *sums, size_t n_sums, unsigned int *counts, size_t n_counts);
int group_share_agree(void *user, int rc);

// The spread-waits hand-shake of one pipelined search (peer transport, smt_group::spread_waits).  Every merge that will want a
// rank's list waits for it, enqueued off the caller's thread -- but never AHEAD of the merging device's own scan: a wait for rank
// i's event that lands on device m's stream before m's issuer has put its scan and select there makes shard m's whole share queue
// up behind shard i's (twice the latency, by timing).  So a wait is enqueued by whoever comes SECOND: rank i posts its
// bit in awaiting[m] and then looks at issued[m]; if m's own work is on its stream already, i takes the bit back and, if it still
// had it, enqueues the wait itself; m, once its own work is issued, raises issued[m] and enqueues the waits of every bit it finds.
// Each bit is claimed exactly once (every access seq_cst).
struct WaitBoard {
    static constexpr int MAX_RANKS = 64;   // one bit per rank in a 64-bit mask: larger groups leave the waits to the caller's thread
    smt_group *g;
    const std::vector<char> &on_aux;       // [n_local] device m merges on its aux stream
    const bool active;                     // false: every operation is a no-op and merge_ranks_on enqueues the waits
    uint64_t merging = 0;                  // bit m: local device m wants the answer
    WaitBoard(smt_group *g, const std::vector<char> &on_aux, uint64_t *const *out_packed);
    int own_work_issued(int i);   // rank i's issuer: my own work is on my stream -- I enqueue the waits posted for me so far
    int published(int i);         // rank i's issuer, behind peer_publish: post to every merging device, or enqueue where it has issued
    int sweep();                  // the caller's thread, after every issuer: enqueue what is left
private:
    std::atomic<uint64_t> awaiting[MAX_RANKS];   // [m]: ranks whose list is published and whose wait on m's stream nobody has enqueued yet
    std::atomic<int> issued[MAX_RANKS];          // [m]: m's own scan + select + publish are on its stream
    int await_all(uint64_t ranks, int m);
};

// ---- row layout of a sharded corpus (sharded.cpp)
void layout_set_contiguous(smt_sharded_corpus *sc, const std::vector<uint64_t> &rank_rows);
// n new rows (global rows total .. total + n) dealt to the ranks: add[r] consecutive rows each, in rank order
void layout_append(smt_sharded_corpus *sc, const std::vector<uint64_t> &add);
// sharded.cpp: smt_sharded_embed's append path for a token CSR in device memory (one-rank groups; waits for the stream)
int sharded_embed_device_append(smt_sharded_model *model, const uint32_t *ids_dev, const uint64_t *offsets_dev, uint64_t n_lines,
                                smt_sharded_corpus *append_to);
// how an append of n rows is dealt: the emptier shards are filled first (water level), small appends go to one shard
void layout_deal(const smt_sharded_corpus *sc, uint64_t n, std::vector<uint64_t> &add);
// global ranges (sorted, disjoint) -> the LOCAL row ranges of rank r
void layout_localize(const smt_sharded_corpus *sc, int rank, const smt_range *ranges, uint32_t n, std::vector<smt_range> &out);
// local row of rank r -> global row
uint64_t layout_to_global(const smt_sharded_corpus *sc, int rank, uint64_t local_row);
// rewrite the rows of a packed [nq][2][k] list of local device i (local rows of its shard -> global rows) on `st`
int layout_translate_packed(smt_sharded_corpus *sc, int local_index, hipStream_t st, uint64_t *packed_dev, uint32_t nq, uint32_t k);

}  // namespace smt
