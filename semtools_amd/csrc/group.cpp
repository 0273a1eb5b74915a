// group.cpp -- the multi-GPU half of libsemtools_hip.so: a GROUP of GPUs behind the C ABI, a corpus row-sharded
// over them, and searches whose only collective is one RCCL all-gather of the per-shard top-k lists.  This file holds the RCCL
// binding and every nccl* call, the group life cycle, the issuing threads and the barriers; the transports that move lists
// between ranks are group_exchange.cpp, the sharded searches sharded_search.cpp, the sharded corpus sharded.cpp.
//
// No reference counterpart: the reference is single-process CPU code (src/bin/semtools.rs:134-135 runs the whole
// search synchronously from one task).  That caller is what this file is shaped for: ONE host thread calls
// smt_init / smt_sharded_search and the library drives every GPU of the node from it --
//   * single process:     smt_group_create(devices, n)  -> ncclCommInitAll, one context + stream per device;
//   * one rank per process (torchrun, MPI): smt_group_unique_id on rank 0, broadcast the 128 bytes by any
//     means, smt_group_create_rank(device, rank, n_ranks, id) -> ncclCommInitRank.  Calls are then SPMD: every
//     process makes the same calls with the same host arguments.
// Partitioning: contiguous row ranges, rows_per_rank = ceil(N / n_ranks), so a document's lines and
// the path-subset ranges of workspace searches stay ranges.  Exchange: rank r's select stage writes its k best
// (global row, exact f64 distance) pairs into one packed buffer; ncclAllGather moves k x 16 B per query per rank
// (latency-bound: xGMI bandwidth is irrelevant); merge_topk_kernel reduces the n_ranks lists to the global
// top-k.  Threshold mode (variable result sizes): all-gather of the counts, then ONE all-gather of a
// max-count-padded buffer, then a host merge of the sorted lists.
//
// RCCL is loaded lazily (dlopen) when the first group is created: single-GPU users -- the `semtools search` CLI
// -- never pay for mapping it.
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <stdexcept>

#include "group.h"

namespace smt {

// ------------------------------------------------------------------ RCCL, loaded on demand
struct RcclApi {
    void *handle = nullptr;
    decltype(&ncclGetVersion) GetVersion = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;
    decltype(&ncclCommUserRank) CommUserRank = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
};
static RcclApi g_rccl;

static int load_rccl()
{
    if (g_rccl.handle) return SMT_OK;
    // An RCCL already mapped into the process (PyTorch ships its own copy under the same SONAME) wins: two RCCLs
    // in one process would each own a set of IPC handles and proxy threads.
    void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) { set_error("cannot load RCCL (librccl.so.1): %s", dlerror()); return SMT_E_HIP; }
#define SMT_RCCL_SYM(name)                                                                  \
    g_rccl.name = reinterpret_cast<decltype(g_rccl.name)>(dlsym(h, "nccl" #name));          \
    if (!g_rccl.name) { set_error("RCCL lacks nccl" #name); dlclose(h); return SMT_E_HIP; }
    SMT_RCCL_SYM(GetVersion)
    SMT_RCCL_SYM(GetUniqueId)
    SMT_RCCL_SYM(CommInitRank)
    SMT_RCCL_SYM(CommInitAll)
    SMT_RCCL_SYM(CommDestroy)
    SMT_RCCL_SYM(CommCount)
    SMT_RCCL_SYM(CommUserRank)
    SMT_RCCL_SYM(AllGather)
    SMT_RCCL_SYM(AllReduce)
    SMT_RCCL_SYM(GroupStart)
    SMT_RCCL_SYM(GroupEnd)
    SMT_RCCL_SYM(GetErrorString)
#undef SMT_RCCL_SYM
    g_rccl.handle = h;
    return SMT_OK;
}

#define SMT_NCCL_CHECK(expr)                                                                   \
    do {                                                                                       \
        ncclResult_t _r = (expr);                                                              \
        if (_r != ncclSuccess) {                                                               \
            smt::set_error("%s failed: %s (%s:%d)", #expr, g_rccl.GetErrorString(_r), __FILE__, __LINE__); \
            return SMT_E_HIP;                                                                  \
        }                                                                                      \
    } while (0)

}  // namespace smt

using namespace smt;

namespace smt {

static smt_group *g_default_group = nullptr;

int group_bind(smt_group *g, int i)
{
    SMT_HIP_CHECK(hipSetDevice(g->ctx[i]->device));
    return SMT_OK;
}

// All-gather / all-reduce through the communicator (group_exchange.cpp: allgather_words, group_allreduce_sums)
int rccl_allgather_words(smt_group *g, size_t send_off, size_t recv_off, size_t words, const std::vector<char> *on_aux)
{
    SMT_NCCL_CHECK(g_rccl.GroupStart());
    for (int i = 0; i < g->n_local; ++i) {
        (void)hipSetDevice(g->ctx[i]->device);
        char *base = reinterpret_cast<char *>(g->buf[i].dev);
        ncclResult_t r = g_rccl.AllGather(base + send_off, base + recv_off, words, ncclUint64, g->comm[i], exchange_stream(g, i, on_aux));
        if (r != ncclSuccess) {
            (void)g_rccl.GroupEnd();
            set_error("ncclAllGather failed: %s", g_rccl.GetErrorString(r));
            return SMT_E_HIP;
        }
    }
    SMT_NCCL_CHECK(g_rccl.GroupEnd());
    return SMT_OK;
}

int rccl_allreduce_sums(smt_group *g, int i, long long *sums, size_t n_sums, unsigned int *counts, size_t n_counts)
{
    SMT_NCCL_CHECK(g_rccl.AllReduce(sums, sums, n_sums, ncclInt64, ncclSum, g->comm[i], g->ctx[i]->stream));
    SMT_NCCL_CHECK(g_rccl.AllReduce(counts, counts, n_counts, ncclUint32, ncclSum, g->comm[i], g->ctx[i]->stream));
    return SMT_OK;
}

int sync_every_stream(smt_group *g)
{
    int rc = group_sync_all(g);
    if (rc) return rc;
    for (int i = 0; i < g->n_local; ++i) {
        if ((rc = group_bind(g, i))) return rc;
        if (g->ctx[i]->aux_stream) SMT_HIP_CHECK(hipStreamSynchronize(g->ctx[i]->aux_stream));
    }
    return SMT_OK;
}

static int group_make_events(smt_group *g)
{
    g->ev_ready.assign(g->n_local, nullptr);
    g->ev_done.assign(g->n_local, nullptr);
    g->pub_stream.assign(g->n_local, nullptr);
    if (const char *w = getenv("SEMTOOLS_GROUP_WAITS")) g->spread_waits = std::string(w) != "caller";
    for (int i = 0; i < g->n_local; ++i) {
        // (the default system-scope release of an event record is what makes a rank's list visible to a reader on another device)
        hipError_t e = hipSetDevice(g->ctx[i]->device);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&g->ev_ready[i], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&g->ev_done[i], hipEventDisableTiming);
        if (e != hipSuccess) { set_error("hipEventCreate: %s", hipGetErrorString(e)); return SMT_E_HIP; }
    }
    return SMT_OK;
}

// Every device of a one-process group may read every other's memory?  Enables peer access both ways (RCCL may have done so already).
static bool group_enable_peers(const int *devices, int n)
{
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            if (i == j) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, devices[i], devices[j]) != hipSuccess || !can) { (void)hipGetLastError(); return false; }
        }
    for (int i = 0; i < n; ++i) {
        if (hipSetDevice(devices[i]) != hipSuccess) { (void)hipGetLastError(); return false; }
        for (int j = 0; j < n; ++j) {
            if (i == j) continue;
            const hipError_t e = hipDeviceEnablePeerAccess(devices[j], 0);
            (void)hipGetLastError();
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return false;
        }
    }
    return true;
}

// $SEMTOOLS_GROUP_TRANSPORT over the default `def`, where the group can use it
static int pick_transport(const smt_group *g, int def)
{
    const char *e = getenv("SEMTOOLS_GROUP_TRANSPORT");
    if (!e || !*e) return def;
    const std::string v(e);
    if (v == "peer" && g->peer_ok) return SMT_TRANSPORT_PEER;
    if (v == "rccl" && !g->copies) return SMT_TRANSPORT_RCCL;
    if (v == "copy" && g->copies) return SMT_TRANSPORT_COPY;
    return def;
}

int group_sync_all(smt_group *g)
{
    for (int i = 0; i < g->n_local; ++i) {
        int rc = group_bind(g, i);
        if (rc) return rc;
        SMT_HIP_CHECK(hipStreamSynchronize(g->ctx[i]->stream));
        if ((rc = drain_async(g->ctx[i]))) return rc;
    }
    return SMT_OK;
}

// A barrier across ranks that also proves the communicator works: all-gather one word per rank, checked on every local device.
int group_barrier(smt_group *g)
{
    std::vector<uint64_t> me(g->n_local), got;
    for (int i = 0; i < g->n_local; ++i) me[i] = (uint64_t)(g->first_rank + i);
    int rc = gather_host_words(g, 1, me.data(), got, true);
    if (rc) return rc;
    for (size_t e = 0; e < got.size(); ++e) {
        const int r = (int)(e % (size_t)g->n_ranks);
        if (got[e] != (uint64_t)r) { set_error("RCCL all-gather returned rank %llu in slot %d", (unsigned long long)got[e], r); return SMT_E_HIP; }
    }
    return SMT_OK;
}

int group_debug_fail(smt_group *g, int where)
{
    int armed = where;
    if (!g->debug_fail_where.compare_exchange_strong(armed, 0)) return SMT_OK;
    set_error("injected failure (smt_debug_group_fail_next, kind %d) on rank %d", where, g->first_rank);
    return g->debug_fail_code;
}

int group_agree(smt_group *g, int rc)
{
    if (!rc) rc = group_debug_fail(g, SMT_DEBUG_FAIL_AGREE);
    if (g->n_local == g->n_ranks) return rc;   // every rank is in this process: nothing to agree on
    const std::string mine = rc ? smt_last_error() : "";
    // (a rank that failed takes part all the same: the others are waiting in this all-gather)
    std::vector<uint64_t> word(g->n_local, (uint64_t)(uint32_t)(rc < 0 ? -rc : rc)), got;
    if (int rc2 = gather_host_words(g, 1, word.data(), got)) return rc2;   // (no way left to tell the others: HIP itself is failing)
    if (rc) { set_error("%s", mine.c_str()); return rc; }
    for (int r = 0; r < g->n_ranks; ++r)
        if (got[r]) { set_error("rank %d failed with status -%llu; this rank gives up with it", r, (unsigned long long)got[r]); return -(int)got[r]; }
    return SMT_OK;
}

// fn(i) for i in [0, n) on n threads that ALL exist before any of them starts: a thread that cannot be created must not leave the
// others waiting for it inside a collective.  false = the threads could not be had and nothing ran.
bool run_on_threads(int n, const std::function<void(int)> &fn)
{
    std::mutex mu;
    std::condition_variable cv;
    int go = 0;   // 0: wait, 1: run, -1: leave
    std::vector<std::thread> th;
    auto body = [&](int i) {
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return go != 0; });
        }
        if (go == 1) fn(i);
    };
    bool ok = true;
    try {   // (reserve first: a bad_alloc from the vector's growth, like a system_error from the thread, must find every started thread
            //  still joinable HERE -- unwinding past them would end in std::terminate inside ~thread)
        th.reserve((size_t)n);
        for (int i = 0; i < n; ++i) th.emplace_back(body, i);
    } catch (...) { ok = false; }
    {
        std::lock_guard<std::mutex> lk(mu);
        go = ok ? 1 : -1;
    }
    cv.notify_all();
    for (auto &t : th) t.join();
    if (!ok) set_error("cannot start a host thread per device");
    return ok;
}

static inline void cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#else
    std::this_thread::yield();
#endif
}

static inline long long mono_ns()
{
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// issuing thread t of T: it issues the shares of local ranks t, t + T, ... (T = one per device for a group of real GPUs)
static void worker_main(smt_group *g, int t)
{
    GroupWorkers *w = g->workers;
    const int T = w->n_threads;
    (void)hipSetDevice(g->ctx[t]->device);   // the thread's current device (every entry point binds again: cheap when unchanged)
    uint64_t seen = 0;
    for (;;) {
        // the next call: spin for a while (GroupWorkers), then block
        bool got = false;
        if (w->spin_ns > 0) {
            const long long t0 = mono_ns();
            for (unsigned spins = 1;; ++spins) {
                if (w->epoch.load(std::memory_order_acquire) != seen || w->stop.load(std::memory_order_acquire)) { got = true; break; }
                cpu_relax();
                if ((spins & 127) == 0 && mono_ns() - t0 > w->spin_ns) break;
            }
        }
        if (!got) {
            std::unique_lock<std::mutex> lk(w->mu);
            w->sleepers.fetch_add(1, std::memory_order_seq_cst);
            w->cv_go.wait(lk, [&] { return w->stop.load(std::memory_order_seq_cst) || w->epoch.load(std::memory_order_seq_cst) != seen; });
            w->sleepers.fetch_sub(1, std::memory_order_seq_cst);
        }
        if (w->stop.load(std::memory_order_acquire)) return;
        seen = w->epoch.load(std::memory_order_acquire);
        const std::function<int(int)> *work = w->work;   // (written before the epoch moved)
        for (int i = t; i < g->n_local; i += T) {
            int rc;
            try { rc = (*work)(i); }   // (an exception must reach the caller as a status, not std::terminate the process from this thread)
            catch (const std::bad_alloc &) { set_error("out of host memory"); rc = SMT_E_NOMEM; }
            catch (const std::exception &e) { set_error("%s", e.what()); rc = SMT_E_INVALID; }
            w->status.record(i, rc);   // (the message is thread-local: carried back to the caller's thread)
        }
        if (w->pending.fetch_sub(1, std::memory_order_seq_cst) == 1 && w->caller_blocked.load(std::memory_order_seq_cst)) {
            std::lock_guard<std::mutex> lk(w->mu);
            w->cv_done.notify_one();
        }
    }
}

static void group_stop_workers(smt_group *g);

static int group_start_workers(smt_group *g)
{
    if (g->n_local <= 1 || g->workers) return SMT_OK;
    // SEMTOOLS_GROUP_THREADS=0: the caller's thread issues every device's share itself (A/B, debugging); =1: one thread per local rank;
    // =N >= 2: N issuing threads, each serving every N-th rank.  Default: one per device for a group of real GPUs; FOUR for logical
    // ranks, which share one device, i.e. one runtime lock and one set of hardware queues -- measured on 8 logical shards, host us per
    // search (tools/ab_group_threads.sh, one box): no threads 83, 2 threads 70, 3: 67, 4: 65, 8: 73.  (With the per-rank stream waits of
    // the first peer protocol eight threads were SLOWER than none: 125-170 against 104 us -- the waits serialised on the device's lock.)
    const char *e = getenv("SEMTOOLS_GROUP_THREADS");
    if (e && e[0] == '0') return SMT_OK;
    int n_threads = g->copies ? (g->n_local >= 4 ? 4 : 0) : g->n_local;   // (2 logical ranks: 24 us from the caller's thread, 32 with two threads)
    if (e && atoi(e) >= 2) n_threads = std::min(g->n_local, atoi(e));
    else if (e && e[0] == '1') n_threads = g->n_local;
    if (n_threads < 2) return SMT_OK;
    g->workers = new (std::nothrow) GroupWorkers();
    if (!g->workers) { set_error("out of host memory"); return SMT_E_NOMEM; }
    g->workers->n_threads = n_threads;
    if (const char *sp = getenv("SEMTOOLS_GROUP_SPIN_US")) g->workers->spin_ns = std::max(0LL, atoll(sp)) * 1000;
    g->workers->status = RankStatuses(g->n_local);
    try {
        g->workers->threads.reserve((size_t)n_threads);
        for (int t = 0; t < n_threads; ++t) g->workers->threads.emplace_back(worker_main, g, t);
    } catch (...) {
        group_stop_workers(g);   // (the ones that exist leave; the group then issues from threads made per call, or from the caller's)
    }
    return SMT_OK;
}

static void group_stop_workers(smt_group *g)
{
    GroupWorkers *w = g->workers;
    if (!w) return;
    {
        std::lock_guard<std::mutex> lk(w->mu);
        w->stop.store(true, std::memory_order_seq_cst);
    }
    w->cv_go.notify_all();
    for (auto &t : w->threads) t.join();
    delete w;
    g->workers = nullptr;
}

// work(i) for every local device: on the group's issuing threads when it has them (n_local > 1), else on threads made for
// the call (`threads`), else in a row on the caller's thread.  First error wins.
int group_for_each_local(smt_group *g, const std::function<int(int)> &work, bool threads)
{
    if (GroupWorkers *w = (g->n_local > 1 && threads) ? g->workers : nullptr) {
        // (one caller at a time per group, as for every entry point that takes it)
        w->work = &work;
        w->pending.store(w->n_threads, std::memory_order_relaxed);
        w->epoch.fetch_add(1, std::memory_order_seq_cst);
        if (w->sleepers.load(std::memory_order_seq_cst) > 0) {
            std::lock_guard<std::mutex> lk(w->mu);
            w->cv_go.notify_all();
        }
        bool done = false;
        if (w->spin_ns > 0) {   // the shares of a search are issued in tens of microseconds: wait for them here
            const long long t0 = mono_ns();
            for (unsigned spins = 1;; ++spins) {
                if (w->pending.load(std::memory_order_acquire) == 0) { done = true; break; }
                cpu_relax();
                if ((spins & 127) == 0 && mono_ns() - t0 > 20 * w->spin_ns) break;
            }
        }
        if (!done) {
            std::unique_lock<std::mutex> lk(w->mu);
            w->caller_blocked.store(1, std::memory_order_seq_cst);
            w->cv_done.wait(lk, [&] { return w->pending.load(std::memory_order_seq_cst) == 0; });
            w->caller_blocked.store(0, std::memory_order_seq_cst);
        }
        w->work = nullptr;
        return w->status.report(g, g->n_ranks > 1);
    }
    RankStatuses st(g->n_local);
    auto run = [&](int i) {
        int rc;
        try { rc = work(i); }
        catch (const std::bad_alloc &) { set_error("out of host memory"); rc = SMT_E_NOMEM; }
        catch (const std::exception &e) { set_error("%s", e.what()); rc = SMT_E_INVALID; }
        st.record(i, rc);
    };
    if (g->n_local == 1 || !threads) {
        for (int i = 0; i < g->n_local; ++i) run(i);
    } else if (!run_on_threads(g->n_local, run)) return SMT_E_NOMEM;
    return st.report(g, g->n_ranks > 1);
}

static void group_free(smt_group *g)
{
    if (!g) return;
    group_stop_workers(g);
    for (int i = 0; i < (int)g->ctx.size(); ++i) {
        if (!g->ctx[i]) continue;
        (void)hipSetDevice(g->ctx[i]->device);
        (void)hipStreamSynchronize(g->ctx[i]->stream);
        if (g->ctx[i]->aux_stream) (void)hipStreamSynchronize(g->ctx[i]->aux_stream);
    }
    ring_free(g);
    for (int i = 0; i < (int)g->ctx.size(); ++i) {
        if (!g->ctx[i]) continue;
        (void)hipSetDevice(g->ctx[i]->device);
        (void)hipStreamSynchronize(g->ctx[i]->stream);
        (void)drain_async(g->ctx[i]);
        if (i < (int)g->comm.size() && g->comm[i] && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(g->comm[i]);
        if (i < (int)g->ev_ready.size() && g->ev_ready[i]) (void)hipEventDestroy(g->ev_ready[i]);
        if (i < (int)g->ev_done.size() && g->ev_done[i]) (void)hipEventDestroy(g->ev_done[i]);
        if (i < (int)g->buf.size()) {
            if (g->buf[i].dev) (void)hipFree(g->buf[i].dev);
            if (g->buf[i].pinned) (void)hipHostFree(g->buf[i].pinned);
        }
        if (!g->borrowed) smt_ctx_destroy(g->ctx[i]);
    }
    delete g;
}

static int group_make_contexts(smt_group *g, const int *devices, int n)
{
    g->ctx.assign(n, nullptr);
    g->comm.assign(n, nullptr);
    g->buf.assign(n, GroupBuf());
    g->ar_sums.assign(n, nullptr);
    g->ar_counts.assign(n, nullptr);
    for (int i = 0; i < n; ++i) {
        int rc = smt_ctx_create(devices[i], &g->ctx[i]);
        if (rc) return rc;
    }
    return SMT_OK;
}

}  // namespace smt

void RankStatuses::record(int i, int rc)
{
    rcs[i] = rc;
    if (rc) errs[i] = smt_last_error();
    else errs[i].clear();
}

int RankStatuses::failed() const
{
    for (int rc : rcs)
        if (rc) return rc;
    return SMT_OK;
}

int RankStatuses::report(const smt_group *g, bool prefix) const
{
    for (size_t i = 0; i < rcs.size(); ++i)
        if (rcs[i]) {
            if (prefix) set_error("shard %d: %s", g->first_rank + (int)i, errs[i].c_str());
            else set_error("%s", errs[i].c_str());
            return rcs[i];
        }
    return SMT_OK;
}

extern "C" {

/* ------------------------------------------------------------------ group ---- */

int smt_group_create(const int *devices, int n_dev, smt_group **out)
try {
    SMT_REQUIRE(out != nullptr, "out");
    *out = nullptr;
    SMT_REQUIRE(devices != nullptr && n_dev >= 1, "device list");
    for (int i = 0; i < n_dev; ++i)
        for (int j = 0; j < i; ++j) SMT_REQUIRE(devices[i] != devices[j], "a device may appear once in a group");
    int rc = load_rccl();
    if (rc) return rc;
    smt_group *g = new (std::nothrow) smt_group();
    if (!g) { set_error("out of host memory"); return SMT_E_NOMEM; }
    g->n_ranks = g->n_local = n_dev;
    g->first_rank = 0;
    if ((rc = group_make_contexts(g, devices, n_dev))) { group_free(g); return rc; }
    (void)g_rccl.GetVersion(&g->rccl_version);
    ncclResult_t r = g_rccl.CommInitAll(g->comm.data(), n_dev, devices);
    if (r != ncclSuccess) { set_error("ncclCommInitAll(%d devices): %s", n_dev, g_rccl.GetErrorString(r)); group_free(g); return SMT_E_HIP; }
    if ((rc = group_barrier(g))) { group_free(g); return rc; }  // channel set-up happens on the first collective: do it now
    // the k-lists of a top-k search are read in place by the merging device when every device can map every other's memory
    // (one hive of xGMI-linked GPUs: always, in practice); otherwise they travel through ncclAllGather
    if ((rc = group_make_events(g))) { group_free(g); return rc; }
    g->peer_ok = n_dev <= SMT_MAX_MERGE_SOURCES && (n_dev == 1 || group_enable_peers(devices, n_dev));
    if (g->peer_ok && n_dev > 1 && !peer_self_test(g)) {
        // (never seen; a node whose devices map each other's memory but do not serve it coherently to a reader's kernel)
        fprintf(stderr, "libsemtools_hip: peer reads between the devices of this group failed their self-test: using ncclAllGather\n");
        (void)hipGetLastError();
        g->peer_ok = false;
    }
    g->transport = pick_transport(g, g->peer_ok ? SMT_TRANSPORT_PEER : SMT_TRANSPORT_RCCL);
    if ((rc = group_start_workers(g))) { group_free(g); return rc; }
    *out = g;
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

int smt_group_create_logical(int device, int n_shards, smt_group **out)
try {
    SMT_REQUIRE(out != nullptr, "out");
    *out = nullptr;
    SMT_REQUIRE(n_shards >= 1 && n_shards <= 64, "1..64 logical shards");
    smt_group *g = new (std::nothrow) smt_group();
    if (!g) { set_error("out of host memory"); return SMT_E_NOMEM; }
    g->n_ranks = g->n_local = n_shards;
    g->first_rank = 0;
    g->copies = true;
    std::vector<int> devs(n_shards, device);
    int rc = group_make_contexts(g, devs.data(), n_shards);
    if (rc) { group_free(g); return rc; }
    if ((rc = group_make_events(g))) { group_free(g); return rc; }
    g->peer_ok = true;   // one device
    if (n_shards > 1 && !peer_self_test(g)) { set_error("the peer-read self-test failed on logical ranks of one device"); group_free(g); return SMT_E_HIP; }
    g->transport = pick_transport(g, SMT_TRANSPORT_PEER);
    if ((rc = group_barrier(g))) { group_free(g); return rc; }
    if ((rc = group_start_workers(g))) { group_free(g); return rc; }
    *out = g;
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

int smt_group_from_ctx(smt_ctx *ctx, smt_group **out)
try {
    SMT_REQUIRE(ctx && out, "null argument");
    *out = nullptr;
    smt_group *g = new (std::nothrow) smt_group();
    if (!g) { set_error("out of host memory"); return SMT_E_NOMEM; }
    g->n_ranks = g->n_local = 1;
    g->first_rank = 0;
    g->copies = true;      // no communicator: a one-rank group never exchanges anything
    g->borrowed = true;    // the caller keeps (and later destroys) the context
    g->ctx.assign(1, ctx);
    g->comm.assign(1, nullptr);
    g->buf.assign(1, GroupBuf());
    g->ar_sums.assign(1, nullptr);
    g->ar_counts.assign(1, nullptr);
    g->transport = SMT_TRANSPORT_COPY;
    if (int rc = group_make_events(g)) { group_free(g); return rc; }
    *out = g;
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

int smt_group_unique_id(void *id_out)
try {
    SMT_REQUIRE(id_out != nullptr, "id_out");
    int rc = load_rccl();
    if (rc) return rc;
    static_assert(sizeof(ncclUniqueId) == SMT_UNIQUE_ID_BYTES, "ncclUniqueId is 128 bytes");
    ncclUniqueId id;
    SMT_NCCL_CHECK(g_rccl.GetUniqueId(&id));
    memcpy(id_out, &id, sizeof(id));
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

int smt_group_create_rank(int device, int rank, int n_ranks, const void *unique_id, smt_group **out)
try {
    SMT_REQUIRE(out != nullptr, "out");
    *out = nullptr;
    SMT_REQUIRE(unique_id != nullptr, "unique_id");
    SMT_REQUIRE(n_ranks >= 1 && rank >= 0 && rank < n_ranks, "rank / n_ranks");
    int rc = load_rccl();
    if (rc) return rc;
    smt_group *g = new (std::nothrow) smt_group();
    if (!g) { set_error("out of host memory"); return SMT_E_NOMEM; }
    g->n_ranks = n_ranks;
    g->n_local = 1;
    g->first_rank = rank;
    if ((rc = group_make_contexts(g, &device, 1))) { group_free(g); return rc; }
    (void)g_rccl.GetVersion(&g->rccl_version);
    ncclUniqueId id;
    memcpy(&id, unique_id, sizeof(id));
    (void)hipSetDevice(device);
    ncclResult_t r = g_rccl.CommInitRank(&g->comm[0], n_ranks, id, rank);
    if (r != ncclSuccess) { set_error("ncclCommInitRank(rank %d of %d): %s", rank, n_ranks, g_rccl.GetErrorString(r)); group_free(g); return SMT_E_HIP; }
    if ((rc = group_barrier(g))) { group_free(g); return rc; }
    *out = g;
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

void smt_group_destroy(smt_group *group)
{
    if (group == g_default_group) g_default_group = nullptr;
    group_free(group);
}

int smt_group_info(const smt_group *group, int *n_ranks, int *n_local, int *first_rank, int *rccl_ranks, int *rccl_version)
try {
    SMT_REQUIRE(group != nullptr, "group");
    if (n_ranks) *n_ranks = group->n_ranks;
    if (n_local) *n_local = group->n_local;
    if (first_rank) *first_rank = group->first_rank;
    if (rccl_version) *rccl_version = group->rccl_version;
    if (rccl_ranks) {
        int count = 0;  // copy transport: no communicator
        if (!group->copies) SMT_NCCL_CHECK(g_rccl.CommCount(group->comm[0], &count));  // what the communicator itself reports
        *rccl_ranks = count;
    }
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

smt_ctx *smt_group_ctx(smt_group *group, int local_index)
{
    if (!group || local_index < 0 || local_index >= group->n_local) return nullptr;
    return group->ctx[local_index];
}

int smt_group_synchronize(smt_group *group)
try {
    SMT_REQUIRE(group != nullptr, "group");
    return group_sync_all(group);
} catch (...) { return smt::api_catch(); }

int smt_group_barrier(smt_group *group)
try {
    SMT_REQUIRE(group != nullptr, "group");
    int rc = group_sync_all(group);
    if (rc) return rc;
    return group_barrier(group);
} catch (...) { return smt::api_catch(); }

int smt_group_set_transport(smt_group *group, int transport)
try {
    SMT_REQUIRE(group != nullptr, "group");
    SMT_REQUIRE(transport == SMT_TRANSPORT_RCCL || transport == SMT_TRANSPORT_COPY || transport == SMT_TRANSPORT_PEER, "transport");
    SMT_REQUIRE(transport != SMT_TRANSPORT_PEER || group->peer_ok, "peer transport needs a one-process group whose devices can read each other's memory");
    SMT_REQUIRE(transport != SMT_TRANSPORT_RCCL || !group->copies, "this group has no RCCL communicator");
    SMT_REQUIRE(transport != SMT_TRANSPORT_COPY || group->copies, "copy transport is the all-gather of logical groups");
    int rc = sync_every_stream(group);   // nothing of an earlier exchange is in flight when the protocol changes
    if (rc) return rc;
    group->transport = transport;
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

int smt_debug_group_fail_next(smt_group *group, int where, int code)
try {
    SMT_REQUIRE(group != nullptr, "group");
    SMT_REQUIRE(where == 0 || where == SMT_DEBUG_FAIL_STAGE || where == SMT_DEBUG_FAIL_AGREE || where == SMT_DEBUG_FAIL_BUILD, "where");
    SMT_REQUIRE(where == 0 || code < 0, "code must be an SMT_E_* status");
    group->debug_fail_code = code;
    group->debug_fail_where.store(where);
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

int smt_group_transport(const smt_group *group)
try {
    SMT_REQUIRE(group != nullptr, "group");
    return group->transport;
} catch (...) { return smt::api_catch(); }

int smt_init(const int *devices, int n_dev)
try {
    if (g_default_group) {
        // idempotent for the same device list
        bool same = g_default_group->n_local == n_dev;
        for (int i = 0; same && i < n_dev; ++i) same = devices && g_default_group->ctx[i]->device == devices[i];
        if (same) return SMT_OK;
        set_error("smt_init was already called with a different device list (call smt_shutdown first)");
        return SMT_E_INVALID;
    }
    std::vector<int> all;
    if (!devices || n_dev <= 0) {  // NULL / 0 = every visible GPU
        const int n = smt_device_count();
        if (n <= 0) { if (n == 0) set_error("no HIP device visible: libsemtools_hip has no CPU fallback"); return SMT_E_HIP; }
        for (int i = 0; i < n; ++i) all.push_back(i);
        devices = all.data();
        n_dev = n;
    }
    return smt_group_create(devices, n_dev, &g_default_group);
} catch (...) { return smt::api_catch(); }

int smt_shutdown(void)
try {
    smt_group *g = g_default_group;
    g_default_group = nullptr;
    group_free(g);
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

smt_group *smt_default_group(void) { return g_default_group; }

}  // extern "C"
