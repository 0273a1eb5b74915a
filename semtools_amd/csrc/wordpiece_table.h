// wordpiece_table.h -- what the two pass-1 kernels of the WordPiece device tokenizer share (wordpiece_kernels.hip: pure-ASCII lines,
// wordpiece_utf8_kernels.hip: UTF-8 lines): the device table, the code-point table of the UTF-8 form, and the handle.
// Internal to the library.
#pragma once

#include <vector>

#include "common.h"
#include "tokenize_frame.h"
#include "wordpiece_bytes.h"

namespace smt {

struct WpTable {
    TokAdded added;                    // (in front: of three places measured, the one where pass 1 is no slower than before the struct)
    const unsigned long long *slots;   // (tag << 32) | entry + 1; 0 = empty
    const uint4 *ent;                  // {pool offset of the piece, its length, its id, 1 = continuing piece}
    const uint8_t *pool;
    const uint8_t *bytes;              // cls[128] | nrm[128]
    uint32_t mask;                     // capacity - 1
    uint32_t prefix_len;
    uint32_t max_piece;                // longest piece, in bytes: no match can be longer
    uint32_t max_chars;
    uint32_t unk;                      // WP_NONE: none
    unsigned long long prefix_state;   // the hash after the continuing prefix
};

// ---- the code points >= U+0080 of the UTF-8 form: a two-level table.  page[cp >> 8] names a page of 256 entries (pages of equal
// content are stored once); an entry is  class | characters << 3 | bytes << 6 | pool offset << 11  of what the code point becomes.
// bytes == 0 on a class that has output: the code point stays itself (its own UTF-8 bytes, one character).
constexpr uint8_t WP_FLAG = 4;                      // beside WP_ORDINARY .. WP_DROPPED of wordpiece_bytes.h (WP_PUNCT is "ALONE")
constexpr uint32_t WP_CP_PAGES = 0x110000 >> 8;     // 4352
constexpr uint32_t WP_CP_MAX_OUT = 16;              // at most 4 characters of at most 4 bytes
constexpr uint32_t WP_CP_MAX_POOL = 1u << 21;
__host__ __device__ inline uint32_t wp_cp_class(uint32_t e) { return e & 7u; }
__host__ __device__ inline uint32_t wp_cp_chars(uint32_t e) { return (e >> 3) & 7u; }
__host__ __device__ inline uint32_t wp_cp_bytes(uint32_t e) { return (e >> 6) & 31u; }
__host__ __device__ inline uint32_t wp_cp_off(uint32_t e) { return e >> 11; }

struct WpCodepoints {
    const uint16_t *page;     // [WP_CP_PAGES]: index of the page, < n_pages
    const uint32_t *ent;      // [n_pages * 256]
    const uint8_t *out;       // the explicit outputs, back to back
    uint32_t n_pages;
    uint32_t out_bytes;
};

// the host image of that table, built and VALIDATED from the caller's ranges (SMT_E_INVALID with a message; nothing is uploaded before)
struct WpCodepointImage {
    std::vector<uint16_t> page;
    std::vector<uint32_t> ent;
    std::vector<uint8_t> out;
};
int wp_codepoint_image(const smt_wordpiece_codepoints *cp, WpCodepointImage &img);

}  // namespace smt

struct smt_wordpiece : smt::TokHandle {
    smt::WpTable T{};                 // points into d_table: slots | entries | pool | byte tables | added pool | added offsets [| code points]
    smt::WpCodepoints U{};            // the UTF-8 form only
    bool utf8 = false;
    uint64_t table_bytes = 0, codepoint_bytes = 0;   // of d_table: all of it, and its code-point part
    smt_wordpiece(smt_ctx *c, const smt::TokWords &w) : smt::TokHandle(c, false, w) {}
    int pass1(const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev, const uint32_t *line_len_dev, uint64_t n_lines,
              uint32_t keep_bytes, int drop_unk, uint8_t *flags_dev) override;
};

namespace smt {
// pass 1 of the UTF-8 form (wordpiece_utf8_kernels.hip): wp_scan_utf8_kernel on the context's stream
int wp_scan_utf8_launch(smt_wordpiece *tok, const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev,
                        const uint32_t *line_len_dev, uint64_t n_lines, uint32_t keep_bytes, int drop_unk, uint8_t *flags_dev);
}  // namespace smt
