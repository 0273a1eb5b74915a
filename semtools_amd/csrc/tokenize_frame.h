// tokenize_frame.h -- the frame every device tokenizer stands in (wordpiece_kernels.hip: WordPiece, unigram_kernels.hip: Unigram),
// internal to the library and defined in tokenize_kernels.hip: the hash the vocabulary tables are built with, the table builder and
// its upload, the scratch between the two passes, the launch code of pass 2 (per-line counts, the one-block prefix sums, the chunk
// bases, wp_emit_kernel, the patch copy), and the handle base with the three calls written on it -- scan, emit and the host-array
// tokenize.  A family adds its table, its pass-1 kernel behind TokHandle::pass1, its create and six thin entry points.
//
// The contract of the scratch: slot s of ids_tmp holds a token id or TOK_NONE; line i owns the slots [slot_begin[i], slot_begin[i + 1])
// (the last line: up to n_slots), its tokens stand there in token order, and raw_count[i] is the number of its used slots.
#pragma once

#include <cstdint>
#include <utility>
#include <vector>

#include "common.h"

namespace smt {

constexpr uint32_t TOK_NONE = 0xFFFFFFFFu;   // an ids_tmp slot that holds no token
constexpr unsigned TOK_EMIT_THREADS = 256;   // pass 2: four slots per thread
constexpr unsigned TOK_EMIT_CHUNK = TOK_EMIT_THREADS * 4;

// the hash the device tables are built with and probed by: FNV-1a, 64 bits, carried byte by byte
constexpr uint64_t TOK_HASH_SEED = 0xcbf29ce484222325ull;
constexpr uint64_t TOK_HASH_MUL = 0x100000001b3ull;
inline uint64_t tok_hash_bytes(const char *b, size_t n, uint64_t h = TOK_HASH_SEED)
{
    for (size_t i = 0; i < n; ++i) h = (h ^ (uint8_t)b[i]) * TOK_HASH_MUL;
    return h;
}

// the number of i in [0, hi) with begin[i] <= p, given that every i < lo has
__device__ __forceinline__ uint64_t tok_count_le(const uint64_t *__restrict__ begin, uint64_t lo, uint64_t hi, uint64_t p)
{
    for (int step = 0; step < 64 && lo < hi; ++step) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (begin[mid] <= p) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the added tokens of a family's table, as pass 1 tests them
struct TokAdded {
    const uint8_t *pool;
    const uint32_t *off;               // [n + 1]: token t is pool[off[t], off[t + 1])
    uint32_t n;
    unsigned long long first[2];       // bit c: an added token starts with byte c
};

// What a pass-1 kernel starts with, one lane per text byte in blocks of `threads`: the block's line window into s_win behind the
// kernel's ONLY barrier (the kernel fills its own LDS tables in front of this call, and every lane of the block reaches the barrier),
// the lane's line by binary search, the looked-at end under keep_bytes, and the two flag checks.  False: the lane leaves -- it stands
// outside every line's looked-at bytes, or at a byte >= 0x80, which flags the line.  True: the lane stands at byte c of `line`, looked
// at in [lb, le); an added token standing there has flagged the line, and the lane still goes on with its family's work.
__device__ __forceinline__ bool tok_scan_lane(const TokAdded &A, unsigned threads, uint64_t *s_win, const uint8_t *__restrict__ text,
                                              uint64_t text_bytes, const uint64_t *__restrict__ line_begin, const uint32_t *__restrict__ line_len,
                                              uint64_t n_lines, uint32_t keep_bytes, uint8_t *__restrict__ flags, uint64_t &line, uint64_t &lb,
                                              uint64_t &le, uint8_t &c)
{
    const uint64_t first = (uint64_t)blockIdx.x * threads;
    if (threadIdx.x < 2) {
        const uint64_t last = first + threads - 1 < text_bytes ? first + threads - 1 : text_bytes - 1;
        s_win[threadIdx.x] = tok_count_le(line_begin, 0, n_lines, threadIdx.x == 0 ? first : last);
    }
    __syncthreads();
    const uint64_t p = first + threadIdx.x;
    if (p >= text_bytes) return false;
    const uint64_t n_le = tok_count_le(line_begin, s_win[0], s_win[1], p);
    if (n_le == 0) return false;                 // in front of the first line
    line = n_le - 1;
    lb = line_begin[line];
    const uint32_t ll = line_len[line];
    const uint64_t le_line = lb + (keep_bytes && keep_bytes < ll ? keep_bytes : ll);
    le = le_line < text_bytes ? le_line : text_bytes;   // the end of what is looked at
    if (p < lb || p >= le) return false;         // behind the cut, or between two lines
    c = text[p];
    if (c >= 0x80) { flags[line] = 1; return false; }
    if (((c < 64 ? A.first[0] : A.first[1]) >> (c & 63)) & 1) {
        for (uint32_t t = 0; t < A.n; ++t) {
            const uint32_t a = A.off[t], tl = A.off[t + 1] - a;
            if (tl == 0 || p + tl > le) continue;
            bool same = true;
            for (uint32_t j = 0; j < tl && same; ++j) same = text[p + j] == A.pool[a + j];
            if (same) { flags[line] = 1; break; }
        }
    }
    return true;
}

// one piece for the table: [off, off + len) of the pool, its id, a kind the owner defines (entries of different kinds never merge),
// its hash, and the caller's own index (a repeated piece: the LATER entry wins, and `src` says which one that was)
struct TokEntry { uint32_t off, len, id, kind; uint64_t h; uint64_t src; };
// open addressing at load <= 0.5: slots[i] = (hash tag << 32) | index into ents + 1, 0 = empty; ents[j] = {off, len, id, kind} of
// the entry that won, winner[j] = its `src`
struct TokTable {
    std::vector<unsigned long long> slots;
    std::vector<uint4> ents;
    std::vector<uint64_t> winner;
    uint32_t mask = 0;
};
void tok_build_table(const char *pool, const std::vector<TokEntry> &in, TokTable &out);
// the parts (pointer, bytes) back to back in ONE device allocation, each 16-byte aligned with room behind it: *d_table owns it, at[i]
// is the device address of part i.  SMT_E_NOMEM with nothing allocated when it does not fit.
int tok_upload_table(const char *family, const std::vector<std::pair<const void *, size_t>> &parts, void **d_table, const uint8_t **at);
// a family's added tokens (the params' added_pool / added_off / n_added): all ASCII, or SMT_E_INVALID; A.n and A.first from them
template <class Params> int tok_added_first(const Params *p, TokAdded &A)
{
    A.n = p->n_added;
    A.first[0] = A.first[1] = 0;
    for (uint32_t t = 0; t < p->n_added; ++t) {
        const uint32_t a = p->added_off[t], tl = p->added_off[t + 1] - a;
        for (uint32_t j = 0; j < tl; ++j) SMT_REQUIRE((uint8_t)p->added_pool[a + j] < 0x80, "added tokens must be ASCII");
        if (tl) A.first[(uint8_t)p->added_pool[a] >> 6] |= 1ull << ((uint8_t)p->added_pool[a] & 63);
    }
    return SMT_OK;
}

// the state between pass 1 and pass 2; owned by a tokenizer handle
struct TokScratch {
    uint32_t *d_ids_tmp = nullptr;    // [slots_cap]
    uint64_t slots_cap = 0;
    void *d_lines = nullptr;          // raw_count u32 [n] | final_count u32 [n] | raw_base u64 [n + 1] | slot_begin u64 [n]
    uint64_t lines_cap = 0;
    void *d_chunks = nullptr;         // chunk_count u32 [c] | chunk_base u64 [c + 1]
    uint64_t chunks_cap = 0;
    void *d_long = nullptr;           // a family's work list between two pass-1 kernels (Unigram's long pieces): a 32-byte header | 16-byte records [long_cap]
    uint64_t long_cap = 0;

    uint32_t *raw_count() const { return static_cast<uint32_t *>(d_lines); }
    uint32_t *final_count() const { return raw_count() + lines_cap; }
    uint64_t *raw_base() const { return reinterpret_cast<uint64_t *>(final_count() + lines_cap); }
    uint64_t *slot_begin() const { return raw_base() + lines_cap + 1; }
    uint32_t *chunk_count() const { return static_cast<uint32_t *>(d_chunks); }
    uint64_t *chunk_base() const { return reinterpret_cast<uint64_t *>(chunk_count() + chunks_cap); }
    static uint64_t chunks_of(uint64_t n_slots) { return (n_slots + TOK_EMIT_CHUNK - 1) / TOK_EMIT_CHUNK; }
};
// room for n_slots slots (padded to whole chunks), n_lines lines and n_long work-list records; waits for the stream before a buffer is
// replaced
int tok_scratch_reserve(smt_ctx *ctx, TokScratch &s, uint64_t n_slots, uint64_t n_lines, uint64_t n_long = 0);
// enqueues what every scan starts with: all slots empty, raw_count zero, the work list's header (where there is one) zero
int tok_scratch_clear(smt_ctx *ctx, TokScratch &s, uint64_t n_slots, uint64_t n_lines);
void tok_scratch_free(TokScratch &s);

// the frame's one-block prefix sum: out[i] = in[0] + ... + in[i - 1] for i in [0, n] (n == 0: out[0] = 0, `in` is not read).  Enqueued.
int tok_exscan(smt_ctx *ctx, const uint32_t *in_dev, uint64_t n, uint64_t *out_dev);
// counts[i] = flagged ? 0 : min(raw_count[i], max_tokens); *n_flagged += flagged lines.  pre_flags_dev (nullptr: none): flags an
// earlier step raised, ORed into flags_dev first.  Enqueued.
int tok_line_counts(smt_ctx *ctx, const TokScratch &s, uint64_t n_lines, uint8_t *flags_dev, uint32_t max_tokens, uint32_t *counts_dev,
                    uint32_t *n_flagged_dev, const uint8_t *pre_flags_dev = nullptr);
// pass 2 on a scratch that pass 1 filled: offsets_out = prefix sum of the (capped, or patched) counts, the ids to their place, the
// patch lines copied in.  slot_begin_dev: the first slot of every line.  Enqueued.
int tok_pass2(smt_ctx *ctx, const TokScratch &s, uint64_t n_slots, const uint64_t *slot_begin_dev, uint64_t n_lines, const uint32_t *counts_dev,
              const uint8_t *flags_dev, const uint64_t *patch_line_dev, const uint64_t *patch_off_dev, const uint32_t *patch_ids_dev,
              uint64_t n_patch, uint64_t n_patch_ids, uint32_t *ids_out_dev, uint64_t ids_cap, uint64_t *offsets_out_dev);

// what a family words in its own way, as last_error shows it
struct TokWords {
    const char *no_scan;        // emit without a scan
    const char *emit_cap;       // emit: ids_cap below the scan's bound + the patch ids
    const char *tokenize_cap;   // tokenize: ids_cap below the lines' bound, with the condition in parentheses
};

// what smt_wordpiece and smt_unigram are: the device table, the scratch and the state of the last scan.  A line owns its looked-at
// bytes as slots -- slot_begin is then the caller's line_begin -- or, with extra_slot, one more: pass1 fills S.slot_begin().
struct TokHandle {
    smt_ctx *const ctx;
    const bool extra_slot;
    const TokWords &words;
    void *d_table = nullptr;
    TokScratch S;
    bool scanned = false;
    uint64_t text_bytes = 0, n_lines = 0, ids_bound = 0;
    const uint64_t *slot_begin = nullptr;
    const uint32_t *counts = nullptr;
    const uint8_t *flags = nullptr;

    TokHandle(smt_ctx *c, bool extra, const TokWords &w) : ctx(c), extra_slot(extra), words(w) {}
    virtual ~TokHandle() = default;
    uint64_t slots_of(uint64_t bytes, uint64_t lines) const { return bytes + (extra_slot ? lines : 0); }
    // the work-list records the family's pass 1 can fill for a text of that many bytes (0: it keeps no list)
    virtual uint64_t long_records(uint64_t) const { return 0; }
    // the family's pass 1 on a cleared scratch: ids into S.d_ids_tmp, counts into S.raw_count(), flags raised.  Enqueued.
    virtual int pass1(const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev, const uint32_t *line_len_dev, uint64_t n_lines,
                      uint32_t keep_bytes, int drop_unk, uint8_t *flags_dev) = 0;
};
TokHandle *tok_handle(smt_wordpiece *tok);
TokHandle *tok_handle(smt_unigram *tok);
void tok_destroy(TokHandle *tok);   // waits for the context's stream; null is fine

// the bodies of smt_*_scan_device, smt_*_emit_device and smt_*_tokenize (include/semtools_hip.h), behind the entry's null check.
// pre_flags_dev (nullptr: none): [n_lines] flags an earlier step raised -- the lower-casing's, for lines it left as they were; a line
// flagged there is flagged here whatever pass 1 finds in its looked-at bytes (count 0, counted in *n_flagged_dev, patched like the others)
int tok_scan_device(TokHandle *tok, const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev, const uint32_t *line_len_dev,
                    uint64_t n_lines, uint32_t keep_bytes, uint32_t max_tokens, int drop_unk, uint32_t *counts_dev, uint8_t *flags_dev,
                    uint32_t *n_flagged_dev, const uint8_t *pre_flags_dev = nullptr);
int tok_emit_device(TokHandle *tok, uint64_t n_lines, const uint64_t *patch_line_dev, const uint64_t *patch_off_dev, const uint32_t *patch_ids_dev,
                    uint64_t n_patch, uint64_t n_patch_ids, uint32_t *ids_out_dev, uint64_t ids_cap, uint64_t *offsets_out_dev);
int tok_tokenize(TokHandle *tok, const char *text, const uint64_t *line_begin, const uint32_t *line_len, uint64_t n_lines, uint32_t keep_bytes,
                 uint32_t max_tokens, int drop_unk, uint32_t *ids_out, uint64_t ids_cap, uint64_t *offsets_out, uint8_t *flags_out);

// a compute entry point handed a null handle: SMT_E_HIP on a machine without a device, SMT_E_INVALID otherwise
int tok_null_handle(const char *what);

}  // namespace smt
