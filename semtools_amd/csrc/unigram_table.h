// unigram_table.h -- what the two pass-1 kernels of the Unigram device tokenizer share (unigram_kernels.hip: pure-ASCII lines,
// unigram_utf8_kernels.hip: UTF-8 lines): the device table, the constants of a lattice node, the handle, and the launch
// of the slot starts.  Internal to the library.
#pragma once

#include "common.h"
#include "tokenize_frame.h"
#include "wordpiece_table.h"

namespace smt {

constexpr unsigned UG_THREADS = 256;                       // pass 1: one position per thread
constexpr unsigned UG_NODES = UG_THREADS + SMT_UG_MAX_WORD;
constexpr uint8_t UG_DROP = 0xFF;                          // byte_map: the byte is dropped
constexpr uint32_t KEY_START = 0, KEY_R = 1;               // a node's start: the piece's start, the node behind R, or 2 + (node - owner's node)
constexpr uint16_t FROM_UNSET = 0xFFFF, FROM_UNK = 0x8000;
constexpr uint32_t UG_RULE_COLLAPSE = 1, UG_RULE_DROP_TRAILING = 2;   // smt_unigram_set_space_rules (unigram_rules_kernels.hip)

// ---- long pieces (unigram_long_kernels.hip): with the switch on, the owner of a piece whose measure passes SMT_UG_MAX_WORD appends one
// record to the work list in the handle's scratch instead of flagging its line, and ug_long_kernel tokenizes the piece with a wave.
// The list: a header of UG_LONG_HEADER bytes -- the record counter (u32 at byte 0), and the witness of smt_unigram_long_stats: the
// pieces ug_long_kernel measured to their end within the limit (u64 at byte 8) and the sum of their measures (u64 at byte 16) --,
// then the records {owner position low, high, line, bit 0: the piece starts at a SPACE | bit 1: nothing but dropped characters stands
// in front of the owner (the line's first piece; set by the scan kernels under the space rules only, for drop_trailing)}.  Pieces are
// disjoint and a handed-over piece holds at least SMT_UG_MAX_WORD raw bytes -- under the space rules too: absorbed spaces are raw
// bytes of the piece in front --, so text_bytes / SMT_UG_MAX_WORD + 1 records always suffice.
constexpr uint32_t UG_LONG_HEADER = 32;
struct UgLongList {
    uint32_t *head;                    // nullptr: the switch is off, and the owner flags the line as ever
    uint4 *rec;
    uint32_t cap;
};
__device__ __forceinline__ void ug_hand_over(const UgLongList &W, uint64_t p, uint64_t line, bool at_space, uint8_t *__restrict__ flags,
                                             bool first_piece = false)
{
    const uint32_t i = W.head ? atomicAdd(W.head, 1u) : W.cap;
    if (i < W.cap) W.rec[i] = make_uint4((uint32_t)p, (uint32_t)(p >> 32), (uint32_t)line, (at_space ? 1u : 0u) | (first_piece ? 2u : 0u));
    else flags[line] = 1;              // (the switch is off; a full list cannot be)
}

struct UgTable {
    const unsigned long long *slots;   // (tag << 32) | entry + 1; 0 = empty
    const uint4 *ent;                  // {pool offset of the piece, its length, its id, 1 = the piece starts with R}
    const double *score;               // per entry
    const uint8_t *pool;
    const uint8_t *map;                // [128]: the normalised byte, UG_DROP
    uint32_t mask;                     // capacity - 1
    uint32_t max_piece;                // longest piece of the vocabulary, in bytes
    uint32_t unk;                      // TOK_NONE: none
    uint32_t rlen;                     // bytes of R
    uint32_t prepend;                  // 0 always, 1 first, 2 never
    uint32_t r_id, r_unk;              // the edge over R alone: the piece R, or the unknown edge
    double r_score;
    double unk_score;
    unsigned long long r_state;        // the hash after R
    smt::TokAdded added;
};

}  // namespace smt

struct smt_unigram : smt::TokHandle {   // every line has one slot more than bytes
    smt::UgTable T{};                 // points into d_table: slots | entries | scores | pool | byte map | added pool | added offsets [| code points]
    smt::WpCodepoints U{};            // the UTF-8 form only: the code points >= U+0080, the table of wordpiece_table.h
    bool utf8 = false;
    uint64_t table_bytes = 0, codepoint_bytes = 0;   // of d_table: all of it, and its code-point part
    uint32_t max_long = 0;            // smt_unigram_set_long_pieces: 0 = off
    uint32_t rules = 0;               // smt_unigram_set_space_rules: UG_RULE_* bits; 0 = the kernels without the rules
    bool long_rules = false;          // smt_unigram_set_long_rules: under a space rule the scan kernels hand long pieces over too
    bool long_scanned = false;        // the last scan ran with the switch on: the list's header holds its witness
    explicit smt_unigram(smt_ctx *c);   // (unigram_kernels.hip, with the family's wording of the frame's errors)
    int pass1(const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev, const uint32_t *line_len_dev, uint64_t n_lines,
              uint32_t keep_bytes, int drop_unk, uint8_t *flags_dev) override;
    uint64_t long_records(uint64_t text_bytes) const override { return max_long ? text_bytes / SMT_UG_MAX_WORD + 1 : 0; }
    bool hands_over() const { return max_long != 0 && (!rules || long_rules); }   // the scan kernels of the next scan leave records
    smt::UgLongList long_list() const
    {
        if (!hands_over() || !S.d_long) return {nullptr, nullptr, 0};
        return {static_cast<uint32_t *>(S.d_long), reinterpret_cast<uint4 *>(static_cast<uint8_t *>(S.d_long) + smt::UG_LONG_HEADER), (uint32_t)S.long_cap};
    }
};

namespace smt {
// slot_begin[i] = line_begin[i] + i into the handle's scratch (unigram_kernels.hip: ug_slot_begin_kernel on the context's stream)
int ug_slot_begin_launch(smt_unigram *tok, const uint64_t *line_begin_dev, uint64_t n_lines);
// pass 1 of the UTF-8 form (unigram_utf8_kernels.hip): ug_scan_utf8_kernel on the context's stream
int ug_scan_utf8_launch(smt_unigram *tok, const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev,
                        const uint32_t *line_len_dev, uint64_t n_lines, uint32_t keep_bytes, int drop_unk, uint8_t *flags_dev);
// pass 1 of either form while a space rule is on (unigram_rules_kernels.hip); a piece over SMT_UG_MAX_WORD flags its line, or goes
// to the handle's work list while tok->hands_over()
int ug_scan_rules_launch(smt_unigram *tok, const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev,
                         const uint32_t *line_len_dev, uint64_t n_lines, uint32_t keep_bytes, int drop_unk, uint8_t *flags_dev);
// the long pieces of the scan just enqueued (unigram_long_kernels.hip): ug_long_kernel on the context's stream, a fixed grid over the
// work list; nothing waits for the count
int ug_long_launch(smt_unigram *tok, const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev, const uint32_t *line_len_dev,
                   uint64_t n_lines, uint32_t keep_bytes, int drop_unk, uint8_t *flags_dev);
// the same behind ug_scan_rules_launch (unigram_long_rules_kernels.hip): ug_long_rules_kernel, which knows the space rules
int ug_long_rules_launch(smt_unigram *tok, const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev,
                         const uint32_t *line_len_dev, uint64_t n_lines, uint32_t keep_bytes, int drop_unk, uint8_t *flags_dev);
}  // namespace smt
