// tokenize_pass2.h -- what the device tokenizers (tokenize_kernels.hip: WordPiece, unigram_kernels.hip: Unigram) share, internal to
// the library: the hash the vocabulary tables are built with, the table builder, the scratch between the two passes, and the launch
// code of pass 2 (per-line counts, the one-block prefix sums, the chunk bases, wp_emit_kernel, the patch copy).  The kernels of
// pass 2 live in tokenize_kernels.hip; a tokenizer's own pass 1 fills the scratch and calls tokenize_pass2 on it.
//
// The contract of the scratch: slot s of ids_tmp holds a token id or TOK_NONE; line i owns the slots [slot_begin[i], slot_begin[i + 1])
// (the last line: up to n_slots), its tokens stand there in token order, and raw_count[i] is the number of its used slots.
#pragma once

#include <cstdint>
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

// the state between pass 1 and pass 2; owned by a tokenizer handle
struct TokScratch {
    uint32_t *d_ids_tmp = nullptr;    // [slots_cap]
    uint64_t slots_cap = 0;
    void *d_lines = nullptr;          // raw_count u32 [n] | final_count u32 [n] | raw_base u64 [n + 1] | slot_begin u64 [n]
    uint64_t lines_cap = 0;
    void *d_chunks = nullptr;         // chunk_count u32 [c] | chunk_base u64 [c + 1]
    uint64_t chunks_cap = 0;

    uint32_t *raw_count() const { return static_cast<uint32_t *>(d_lines); }
    uint32_t *final_count() const { return raw_count() + lines_cap; }
    uint64_t *raw_base() const { return reinterpret_cast<uint64_t *>(final_count() + lines_cap); }
    uint64_t *slot_begin() const { return raw_base() + lines_cap + 1; }
    uint32_t *chunk_count() const { return static_cast<uint32_t *>(d_chunks); }
    uint64_t *chunk_base() const { return reinterpret_cast<uint64_t *>(chunk_count() + chunks_cap); }
    static uint64_t chunks_of(uint64_t n_slots) { return (n_slots + TOK_EMIT_CHUNK - 1) / TOK_EMIT_CHUNK; }
};
// room for n_slots slots (padded to whole chunks) and n_lines lines; waits for the stream before a buffer is replaced
int tok_scratch_reserve(smt_ctx *ctx, TokScratch &s, uint64_t n_slots, uint64_t n_lines);
// enqueues what every scan starts with: all slots empty, raw_count zero
int tok_scratch_clear(smt_ctx *ctx, TokScratch &s, uint64_t n_slots, uint64_t n_lines);
void tok_scratch_free(TokScratch &s);

// counts[i] = flagged ? 0 : min(raw_count[i], max_tokens); *n_flagged += flagged lines.  Enqueued.
int tok_line_counts(smt_ctx *ctx, const TokScratch &s, uint64_t n_lines, const uint8_t *flags_dev, uint32_t max_tokens, uint32_t *counts_dev,
                    uint32_t *n_flagged_dev);
// pass 2 on a scratch that pass 1 filled: offsets_out = prefix sum of the (capped, or patched) counts, the ids to their place, the
// patch lines copied in.  slot_begin_dev: the first slot of every line (WordPiece: the line's first byte).  Enqueued.
int tok_pass2(smt_ctx *ctx, const TokScratch &s, uint64_t n_slots, const uint64_t *slot_begin_dev, uint64_t n_lines, const uint32_t *counts_dev,
              const uint8_t *flags_dev, const uint64_t *patch_line_dev, const uint64_t *patch_off_dev, const uint32_t *patch_ids_dev,
              uint64_t n_patch, uint64_t n_patch_ids, uint32_t *ids_out_dev, uint64_t ids_cap, uint64_t *offsets_out_dev);

// a compute entry point handed a null handle: SMT_E_HIP on a machine without a device, SMT_E_INVALID otherwise
int tok_null_handle(const char *what);

}  // namespace smt
