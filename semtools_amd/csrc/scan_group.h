// scan_group.h -- K2, grouped: the take-along protocol of scan_pair_kernel (scan_pair.hip), scan_wide_kernel (scan_wide.hip) and
// scan_deep_kernel (scan_deep.hip), stated once: the slots, the records, the decision, and the frame the three kernels stand in
// around their reducers.  The host side -- slot publication, which family a launch is of -- is scan_launch.hip.
#pragma once
#include "scan_params.h"
#include "shared_list.h"

namespace smt {

// ------------------------------------------------------------- K2, grouped (tuning key scan_pair)
// Queued one-query scans of the scan_overlap pipeline share a corpus pass.  Every call still launches its scan and its select at
// once; the scan of step i decides ON THE DEVICE, when it starts, how many of the steps i + 2, i + 4, i + 6 -- the next calls on its
// own stream -- it takes along: then it runs the row loop over up to four queries and writes up to four list sets, its own and the
// others', and the scans of the steps it took find themselves ABSORBED and exit before their gate and before any row load.  The
// selects run where they always did, each on its own list set with its own query, outputs and status word: the scan only
// nominates, so no answer changes.
//   host -> device: a ring of PairSlot in pinned host memory, indexed by step; the host fills slot i before it launches scan i and
//     writes the step number last (release); the reader checks the number before and after the fields (a slot reused PAIR_RING
//     steps later fails that check).
//   block -> block: one PairRecord per step in device memory, state = step << 3 | code.  One block wins a CAS on it, decides, and
//     publishes the record -- the group size and the (query, lists) of the calls taken -- with one agent-scope release; the others
//     wait for it with a bounded wait (PairParams::ctl[0] is raised when one runs out, and drain_async turns that into an error
//     code).
//   leader -> absorbed: the deciding block MARKS the records of the steps it takes (state = that step << 3 | PAIR_ABSORBED) before
//     it publishes its own, and a launch learns its fate from its OWN record, the one it reads anyway: marked, it exits; anything
//     else, it leads.  The marks are complete by stream order: leader and absorbed launch are on one stream.  (The other way round,
//     an absorbed step looking for its leader, needs the records of steps i - 2, i - 4 and i - 6.)  Record reuse: the record of
//     step s is that of s - PAIR_RECS, a launch of the same stream that finished long ago, and is touched by the leader of s and
//     by s alone; a mark for a step whose slot check failed is never written, so a cut descriptor ring (scan_pair_ring = 64, the
//     host more than 64 calls ahead) only ends groups early.
// The group is a PREFIX: a refused step i + 2 ends it, so the calls of a group are consecutive on their stream.
// WHEN a launch looks is decided by the host: only a launch that queues up behind a predecessor on its internal stream
// (hipStreamQuery at the call) runs this kernel at all -- a call made while the GPU keeps up, a launch bracketed by profiling events
// and the one after it run scan_topk_kernel as before, so their latency and the profiled kernel time are the plain kernel's.  The
// deciding block reads the slots before it waits at its gate, the others learn the decision after they have requested their first
// rows (the same rows either way): no row load starts later than in scan_topk_kernel.  (Looking only when the block had to wait
// at its gate was measured too: 78.7 instead of 78.2 us per step, and under counter collection, which serialises kernels, nothing
// pairs at all -- profiles/scan_pairing.json.)
// THREE FAMILIES of one protocol: scan_pair_kernel reaches steps i + 2 .. i + 6 (up to four calls per pass), scan_wide_kernel
// i + 2 .. i + 14 (eight), scan_deep_kernel i + 2 .. i + 30 (sixteen).  A launch says in its slot which kernel it runs (the family
// bits of kp_blocks) and has a record of its own kind, in an array of its own: a leader takes launches of its own kernel only, and
// the other two refuse them by the same compare.
constexpr int PAIR_RING = 4096;   // slots: the host may run this many calls ahead of the GPU and still be found (256 KiB, pinned; tuning key scan_pair_ring uses fewer)
constexpr int PAIR_RECS = 64;     // records: record i is written by the leader of step i (a mark) and by step i, and read by step i
constexpr int GROUP_MAX = 4;      // calls one corpus pass serves: the leader's and up to three taken along
constexpr int WIDE_MAX = 8;       // calls one corpus pass of scan_wide_kernel serves: the leader's and up to seven taken along
constexpr int WIDE_RECS = 64;     // records (reuse distance 64 > 14, as PAIR_RECS)
constexpr int DEEP_MAX = 16;      // calls one corpus pass of scan_deep_kernel serves: the leader's and up to fifteen taken along
constexpr int DEEP_RECS = 64;     // records (reuse distance 64 > 30, as PAIR_RECS)
constexpr unsigned long long WIDE_FAMILY = 1ull << 16;   // PairSlot::kp_blocks of a scan_wide_kernel launch (kp <= 64 below it, the grid above)
constexpr unsigned long long DEEP_FAMILY = 1ull << 17;   // PairSlot::kp_blocks of a scan_deep_kernel launch (next to WIDE_FAMILY)
struct PairSlot {   // 64 bytes of pinned host memory
    unsigned long long step;        // written last
    unsigned long long corpus, n_virtual, query, lists;
    unsigned long long kp_blocks;   // kp | grid size << 32
    unsigned long long absorbable;
    unsigned long long pad;
};
template <int MAX>
struct GroupRecord {   // 16 MAX bytes: 64 (pair), 128 (wide), 256 (deep)
    unsigned long long state;       // step << 3 | PAIR_DECIDING / PAIR_ALONE / PAIR_PAIRED / PAIR_ABSORBED (any other step: undecided)
    unsigned long long taken;       // PAIR_PAIRED: calls taken along (1 .. MAX - 1) ...
    unsigned long long query[MAX - 1], lists[MAX - 1];   // ... and theirs
};
using PairRecord = GroupRecord<GROUP_MAX>;
using WideRecord = GroupRecord<WIDE_MAX>;
using DeepRecord = GroupRecord<DEEP_MAX>;
static_assert(sizeof(PairRecord) == 64 && sizeof(WideRecord) == 128, "a record is state, taken and MAX - 1 (query, lists) pairs");
static_assert(sizeof(DeepRecord) == 256, "DeepRecord: state, taken and fifteen (query, lists) pairs");
enum : unsigned long long { PAIR_DECIDING = 1, PAIR_ALONE = 2, PAIR_PAIRED = 3, PAIR_ABSORBED = 4 };
constexpr int PAIR_SHIFT = 3;
// select_group (select.hip group_select_kernel): ONE select launch behind the leader serves every call of its pass, so the leader
// also needs each member's output buffers, status word and row base.  They travel as (query, lists) do: the host writes them into a
// second pinned ring beside the PairSlot ring (same index, same length, between the two stores of PairSlot::step, so the step checks
// around the fields cover them; PairSlot keeps its 64 bytes and the two older kernels never see the ring), the deciding wave copies
// them AT THE DECISION into a device record beside DeepRecord (same index, same reuse distance), and the select reads that copy --
// never the pinned slot, which the host may have lapped by then (scan_pair_ring = 64).  A launch that is followed by a group select
// says so in its slot (DEEP_SELGROUP, and its k_out above it: k' alone does not fix k_out when the guard band changes between
// calls), so a leader takes only calls whose select it will run, and calls that will run none of their own.
constexpr unsigned long long DEEP_SELGROUP = 1ull << 18;   // PairSlot::kp_blocks: the launch is followed by group_select_kernel ...
constexpr int DEEP_KOUT_SHIFT = 24;                        // ... and k_out (<= 56) in bits 24 .. 29
struct SelSlot {   // 32 bytes of pinned host memory, slot i beside PairSlot i
    unsigned long long out_rows, out_dist, out_status, row_base;
};
struct DeepSelRecord {   // 512 bytes
    SelSlot member[DEEP_MAX];   // [0 .. DEEP_MAX - 2]: the calls taken along, as DeepRecord::query
};
static_assert(DEEP_MAX == GROUP_SEL_MAX && offsetof(DeepRecord, state) == 8 * GROUP_REC_STATE && offsetof(DeepRecord, taken) == 8 * GROUP_REC_TAKEN &&
                  offsetof(DeepRecord, query) == 8 * GROUP_REC_QUERY && offsetof(DeepRecord, lists) == 8 * GROUP_REC_LISTS && sizeof(SelSlot) == 32,
              "group_select_kernel reads these records as 8-byte words (common.h GroupSelect)");

// The kernels' second argument.  (Three named types in one field order each: their names are in the kernel symbols and their layout
// is the kernarg layout.)
struct PairParams {
    const PairSlot *ring;
    PairRecord *recs;
    unsigned long long *ctl;        // [0] a bounded wait ran out; launches that [1] took calls along, [2] ran alone, [3] were absorbed, [4..6] served 2, 3, 4 calls
    unsigned int absorbable;        // this launch's own slot says so: only then can a leader have marked its record
    unsigned int max_take;          // tuning key scan_pair: calls a launch may take along (1 .. GROUP_MAX - 1)
    unsigned long long wait_ticks;  // tuning key scan_pair_wait_us, in 10 ns ticks
    unsigned long long ring_mask;   // slots in use - 1 (tuning key scan_pair_ring)
};
struct WideParams {
    const PairSlot *ring;
    WideRecord *recs;
    unsigned long long *ctl;        // PairParams::ctl, and behind it [7..10] launches that served 5, 6, 7, 8 calls
    unsigned int absorbable;
    unsigned int max_take;          // tuning key scan_take: calls a launch may take along (1 .. WIDE_MAX - 1)
    unsigned long long wait_ticks;
    unsigned long long ring_mask;
};
struct DeepParams {
    const PairSlot *ring;
    const SelSlot *sel_ring;        // select_group: the ring beside `ring`, or nullptr ...
    DeepSelRecord *sel_recs;        // ... and the records beside `recs`
    unsigned long long family;      // what a slot's kp_blocks holds beside k' and the grid: DEEP_FAMILY, and with select_group DEEP_SELGROUP | k_out << DEEP_KOUT_SHIFT
    DeepRecord *recs;
    unsigned long long *ctl;        // PairParams::ctl; [11..26] launches of this kernel that served 1 .. 16 calls
    unsigned int absorbable;
    unsigned int max_take;          // tuning key scan_deep: calls a launch may take along (1 .. DEEP_MAX - 1)
    unsigned long long wait_ticks;
    unsigned long long ring_mask;
};
constexpr int DEEP_CTL_BY_SIZE = 11;

// dynamic LDS of a scan_pair_kernel launch: the four key regions, the waves' key counts, the query images, the block's control words
static inline size_t pair_smem_bytes(int threads)
{
    return (size_t)GROUP_MAX * (threads / 64) * 64 * sizeof(key_t64) + 256 + (size_t)GROUP_MAX * 1024 + 9 * 8 + 16;
}
// dynamic LDS of a scan_wide_kernel launch: the eight lists (32 keys each, whatever the block's size), the queries' records, the
// lock words, the query images, the block's control words
static inline size_t wide_smem_bytes(int threads)
{
    return (size_t)WIDE_MAX * 32 * sizeof(key_t64) + (size_t)WIDE_MAX * 16 + 64 + (size_t)WIDE_MAX * 1024 + 18 * 8 + 16;
}
// dynamic LDS of a scan_deep_kernel launch: the sixteen lists (32 keys each, whatever the block's size), the queries' records, the
// lock words, the query images, the block's control words (3 + 16 list sets + 15 query addresses) and the chunk counter
static inline size_t deep_smem_bytes(int threads)
{
    return (size_t)DEEP_MAX * 32 * sizeof(key_t64) + (size_t)DEEP_MAX * 16 + 64 + (size_t)DEEP_MAX * 1024 + 34 * 8 + 16;
}

// Each unit launches its own kernel: `blocks` blocks of `threads` threads with its *_smem_bytes of LDS on `st`.  Enqueues only: the
// caller asks hipGetLastError.
void launch_scan_pair_kernel(bool nt, int blocks, int threads, hipStream_t st, const ScanParams &p, const PairParams &pp);
void launch_scan_wide_kernel(bool nt, int blocks, int threads, hipStream_t st, const ScanParams &p, const WideParams &pp);
void launch_scan_deep_kernel(bool nt, int blocks, int threads, hipStream_t st, const ScanParams &p, const DeepParams &pp);

__device__ __forceinline__ unsigned long long sys_load(const unsigned long long *f)
{
    return __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The deciding block: the slots of step + 2, + 4, + 6 -> how many of them this launch takes along (their queries and list sets
// go into the record), the longest prefix that passes.  scan_pair_wait_us bounds the waits for all of them together.
// (FAMILY: which group-capable kernel the leader runs, in spare bits of PairSlot::kp_blocks -- a leader takes launches of its own
// kernel only, their records are of its kind; RECS: the records of that kind)
template <unsigned long long FAMILY, int RECS, class PP, class REC>
__device__ __forceinline__ unsigned int group_decide(const ScanParams &p, const PP &pp, REC *rec)
{
    const unsigned long long t0 = wall_clock64();
    unsigned int taken = 0;
    while (taken < pp.max_take) {
        const unsigned long long want = p.step + 2ull * (taken + 1);
        const PairSlot *s = pp.ring + (want & pp.ring_mask);
        unsigned long long s1 = __hip_atomic_load(&s->step, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
        if (s1 < want && pp.wait_ticks) {   // (tests: corpora that scan faster than the host issues calls; a LATER step's number: the slot was reused)
            while (s1 < want && wall_clock64() - t0 < pp.wait_ticks) {
                __builtin_amdgcn_s_sleep(32);
                s1 = __hip_atomic_load(&s->step, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        if (s1 != want) break;
        const unsigned long long corpus = sys_load(&s->corpus), n_virtual = sys_load(&s->n_virtual), kp_blocks = sys_load(&s->kp_blocks);
        const unsigned long long absorbable = sys_load(&s->absorbable);
        const unsigned long long query = sys_load(&s->query), lists = sys_load(&s->lists);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        if (sys_load(&s->step) != want) break;   // the host was rewriting the slot (a ring's length ahead)
        const bool same = corpus == (unsigned long long)(uintptr_t)p.corpus && n_virtual == p.n_virtual &&
                          kp_blocks == ((unsigned long long)p.kp | FAMILY | (unsigned long long)gridDim.x << 32);
        if (!(absorbable && same)) break;
        flag_store(&rec->query[taken], query);
        flag_store(&rec->lists[taken], lists);
        flag_store(&pp.recs[want % RECS].state, (want << PAIR_SHIFT) | PAIR_ABSORBED);   // the mark
        ++taken;
    }
    flag_store(&rec->taken, (unsigned long long)taken);
    return taken;
}

// ------------------------------------------------------------- the frame of the three kernels
// A grouped kernel runs:  [set up LDS, the leader's query] -> thread 0: group_look -> barrier -> absorbed? count the launch (ctl[3],
// once) and return -> [request the first rows] -> thread 0: group_await -> barrier -> [the queries taken along] -> the row loop
// (SMT_GROUP_ROW_LOOP around the kernel's reducer) -> barrier -> [the gate, the lists out].  scan_deep_kernel looks and awaits with
// a whole wave (scan_deep.hip: fifteen slots side by side), the other two with thread 0, here.
// The gate add behind the loop: a leader's block counts for the blocks of the calls it serves, the host's running totals count
// every launch (thread 0 by wave and lane: threadIdx.x itself would be one more register alive across the loop).

// Thread 0, before any row load: the gate and this step's record, two independent reads in one round trip (scan_topk_kernel reads
// its gate here).  Marked by its leader, the launch is absorbed (the code returned; 0 otherwise).  Else the first block to get here
// wins the record and looks for calls to take along while the others wait at the gate.  cur: the record's state as this block
// leaves it -- this step's: the block has won the CAS and decided, or lost it.
template <unsigned long long FAMILY, int RECS, class PP, class REC>
__device__ __forceinline__ unsigned long long group_look(const ScanParams &p, const PP &pp, REC *rec, unsigned long long tag,
                                                         unsigned long long &cur)
{
    const unsigned long long g = p.gate_open ? flag_load(p.gate) : 0ull;
    cur = flag_load(&rec->state);
    unsigned long long code = 0;
    if (pp.absorbable && cur == (tag | PAIR_ABSORBED)) {
        code = PAIR_ABSORBED;   // (marked by the leader, an earlier launch of this stream)
    } else {
        if ((cur >> PAIR_SHIFT) != p.step &&
            __hip_atomic_compare_exchange_strong(&rec->state, &cur, tag | PAIR_DECIDING, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT)) {
            const unsigned int taken = group_decide<FAMILY, RECS>(p, pp, rec);
            cur = tag | (taken ? PAIR_PAIRED : PAIR_ALONE);
            __hip_atomic_store(&rec->state, cur, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_add(pp.ctl + (taken ? 1 : 2), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (taken) (void)__hip_atomic_fetch_add(pp.ctl + 3 + taken, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (g < p.gate_open) gate_wait(p);
    }
    return code;
}

// Thread 0, behind the first row requests: the bounded wait for the deciding block's answer (bounded like flag_wait: a decision
// that never comes ends in an error code), then the (query, lists) of the calls taken along into LDS.  Returns the calls this pass
// serves, 1 .. NQ.
template <int NQ, class PP, class REC>
__device__ __forceinline__ unsigned long long group_await(const PP &pp, const REC *rec, unsigned long long tag, unsigned long long cur,
                                                          unsigned long long *s_qptr, unsigned long long *s_lists)
{
    if (cur == (tag | PAIR_DECIDING)) {
        const unsigned long long t0 = wall_clock64();
        while ((cur = flag_load(&rec->state)) == (tag | PAIR_DECIDING)) {
            __builtin_amdgcn_s_sleep(8);
            if (flag_load(pp.ctl) != 0ull) break;
            if (wall_clock64() - t0 > 200000000ull) { flag_store(pp.ctl, 1ull); break; }
        }
    }
    unsigned long long served = 1;
    if (cur == (tag | PAIR_PAIRED)) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        unsigned long long taken = flag_load(&rec->taken);
        if (taken > (unsigned long long)(NQ - 1)) taken = NQ - 1;   // (never: the record is this step's)
        for (unsigned long long j = 0; j < taken; ++j) {
            s_qptr[j] = flag_load(&rec->query[j]);
            s_lists[j] = flag_load(&rec->lists[j]);
        }
        served = 1 + taken;
    } else if (cur != (tag | PAIR_ALONE)) {
        flag_store(pp.ctl, 1ull);   // (a wait that ran out, or a record that is not this step's: alone, and the context reports it)
    }
    return served;
}

// ------------------------------------------------------------- shared lists (scan_wide_kernel, scan_deep_kernel)
// The block keeps ONE sorted list per query in LDS (shared_list.h: 32 keys, so these kernels serve kp <= 32) and one 16-byte record
// per query, {1 / |q|, q is zero, threshold distance, threshold row}.  Wave 0 sets up the lists, the locks and the records; the
// kernel's barriers stand between its stores and the row loop.
template <int NQ>
__device__ __forceinline__ void group_lists_setup(key_t64 *s_list, f32x4 *s_rec, unsigned int *s_lock, int wave, int lane)
{
    if (wave == 0) {
#pragma unroll
        for (int i = 0; i < NQ * SHARED_LIST_KEYS / 64; ++i) s_list[64 * i + lane] = KEY_PAD;
        if (lane < NQ) {
            f32x4 r;   // a query that is not there: zero, nothing under its threshold
            r.x = 0.0f;
            r.y = 1.0f;
            r.z = __builtin_inff();               // (SHARED_LIST_OPEN)
            r.w = __uint_as_float(0xFFFFFFFFu);
            s_rec[lane] = r;
            s_lock[lane] = 0u;
        }
    }
}
// One wave: its 16 bytes per lane of query n go into image `slot`, the norm half of the query's record follows (the norms are not
// held in registers: sixteen scalar registers for eight norms are not there).
__device__ __forceinline__ void group_query_norm(f32x4 *s_q, f32x4 *s_rec, int slot, int n, const f32x4 &qn, int lane)
{
    s_q[slot * 64 + lane] = qn;
    const float a2 = wave_sum(qn.x * qn.x + qn.y * qn.y + qn.z * qn.z + qn.w * qn.w);
    const bool qz = readlane_f(a2, 0) == 0.0f;
    const float rq = qz ? 0.0f : readlane_f(__frsqrt_rn(a2), 0);
    if (lane == 0) { s_rec[n].x = rq; s_rec[n].y = qz ? 1.0f : 0.0f; }
}
// Behind the row loop, its barrier and the gate add.  The block's lists are its answer, sorted and padded: there is no merge.  Wave
// w writes those of queries w, w + waves, ... to the list sets s_sets[0 .. n_on - 1], the launch's own first.
// (The gate add and the absorbed launch's counter bump stay in the kernels: their "wave == 0 && lane == 0" shares its two compares
// with the kernel's other uses only when it is written there -- inside a function it is folded to one compare of an OR first, and
// the code behind the row loop comes out different.)
__device__ __forceinline__ void group_lists_out(const key_t64 *s_list, const unsigned long long *s_sets, int n_on, int kp, int wave,
                                                int waves_per_block, int lane)
{
    for (int n = wave; n < n_on; n += waves_per_block) {
        key_t64 *out = reinterpret_cast<key_t64 *>((uintptr_t)uniform_u64(s_sets[n])) + (size_t)blockIdx.x * kp;
        if (lane < kp) out[lane] = s_list[n * SHARED_LIST_KEYS + lane];
    }
}

// ------------------------------------------------------------- the reducers' common ground
// The per-lane product of a row with a query, spelled out as the compiler contracts "x qx + y qy + z qz + w qw" in the one-query
// loop -- y qy, then fused adds of x, z, w -- so that no vectoriser's regrouping can move a rounding; SMT_OPAQUE keeps a tree's
// value a scalar: left to itself the SLP vectoriser pairs the trees into v_pk_add_f32, which cannot carry a DPP operand.
#define SMT_ROW_DOT(cj, qv) __builtin_fmaf((cj).w, (qv).w, __builtin_fmaf((cj).z, (qv).z, __builtin_fmaf((cj).x, (qv).x, (cj).y * (qv).y)))
#define SMT_OPAQUE(v) asm volatile("" : "+v"(v))

// The row loop.  The software pipeline of scan_topk_kernel -- the next chunk's rows are requested once the current chunk's have
// arrived and fly during its reduction -- without the register copy: the loop is unrolled by two and the two row buffers swap names.
// The empty wait on `cur` stands where the copy stood: it keeps the request timing (ONE chunk in flight per wave; two, the ping-pong,
// measured slower), and the claims come in the same order, so every wave takes the chunks it took.
// Two macros, so that every kernel's loop is the text it was.  SMT_GROUP_ROWS_BEGIN stands in front of group_await: it declares
// the pipeline (of the kernel's p, U, NT, s_next, wave, lane, waves_per_block: the chunk deal of chunk_deal.h, the scalar row test
// and row addresses of scan_params.h, the chunk numbers v0 / v0n, the first buffer cn) and requests the first rows before the
// decision is known -- they are the same rows either way.  SMT_GROUP_ROW_LOOP(REDUCE) runs it.
// REDUCE(rows, first row, real rows): the kernel's reducer; the chunk's real rows are a wave-uniform count, asked the scalar way.
#define SMT_GROUP_ROWS_BEGIN                                                                                      \
    auto chunk_v0 = [&](uint32_t t) -> uint64_t { return deal_chunk(t, waves_per_block) * U; };                   \
    auto claim = [&]() -> uint32_t { return deal_claim(s_next, lane); };                                          \
    auto in_corpus = [&](uint64_t v) -> bool { return rows_in_corpus(p, v); };                                    \
    auto issue_rows = [&](uint64_t v0, f32x4 (&c)[U]) { rows_issue<NT>(p, v0, c, lane); };                        \
    f32x4 cn[U];                                                                                                  \
    uint64_t v0 = chunk_v0((uint32_t)wave);                                                                       \
    uint64_t v0n = 0;                                                                                             \
    if (in_corpus(v0)) {                                                                                          \
        issue_rows(v0, cn);                                                                                       \
        v0n = chunk_v0(claim());                                                                                  \
    }
#define SMT_GROUP_STEP(cur, nxt, REDUCE)                                                                        \
    do {                                                                                                          \
        asm volatile("s_waitcnt vmcnt(0)" : "+v"((cur)[0]), "+v"((cur)[1]), "+v"((cur)[2]), "+v"((cur)[3]) : : "memory"); \
        if (in_corpus(v0n)) issue_rows(v0n, nxt);                                                                 \
        const uint64_t v0nn = chunk_v0(claim());                                                                  \
        REDUCE(cur, (uint32_t)v0, in_corpus(v0 + (U - 1)) ? 4u : (uint32_t)(p.n_virtual - v0));                   \
        v0 = v0n;                                                                                                 \
        v0n = v0nn;                                                                                               \
    } while (0)
#define SMT_GROUP_ROW_LOOP(REDUCE)                                                                                \
    f32x4 cm[U];                                                                                                  \
    while (in_corpus(v0)) {                                                                                       \
        SMT_GROUP_STEP(cn, cm, REDUCE);                                                                           \
        if (!in_corpus(v0)) break;                                                                                \
        SMT_GROUP_STEP(cm, cn, REDUCE);                                                                           \
    }

}  // namespace smt
