// wordpiece_bytes.h -- the byte rules of a pure-ASCII line through BertNormalizer -> BertPreTokenizer -> WordPiece, stated once as a
// 128-entry table (hf_tokenizer.cpp encode_ascii states the same rules as code; tests/wordpiece_ref.py restates them in Python).
// Host-only: the device reads the table wordpiece_kernels.hip uploads.
#pragma once

#include <cstdint>

#include "../../include/semtools_hip.h"

namespace smt {

enum : uint8_t {
    WP_ORDINARY = 0,   // a character of a word
    WP_SPACE = 1,      // white space: ends a word, yields nothing (\t \n \r are mapped to ' ' by clean_text: the same class)
    WP_PUNCT = 2,      // ASCII punctuation: a word of its own
    WP_DROPPED = 3,    // removed by clean_text (NUL, the controls, DEL): JOINS its neighbours, counts for nothing
};

// cls[c]: the class of byte c; nrm[c]: the byte it becomes in a word (A-Z lowered under LOWERCASE, every other byte itself)
inline void wordpiece_byte_table(uint32_t flags, uint8_t cls[128], uint8_t nrm[128])
{
    const bool norm = (flags & SMT_WP_NORMALIZER) != 0;
    const bool clean = norm && (flags & SMT_WP_CLEAN_TEXT) != 0;
    const bool lower = norm && (flags & SMT_WP_LOWERCASE) != 0;
    for (int c = 0; c < 128; ++c) {
        uint8_t k = WP_ORDINARY;
        if (clean && (c == '\t' || c == '\n' || c == '\r')) k = WP_SPACE;          // -> ' '
        else if (clean && (c < 0x20 || c == 0x7F)) k = WP_DROPPED;                 // VT and FF among them
        else if ((c >= 0x9 && c <= 0xD) || c == 0x20) k = WP_SPACE;                // without clean_text VT and FF are white space
        else if ((c >= 0x21 && c <= 0x2F) || (c >= 0x3A && c <= 0x40) || (c >= 0x5B && c <= 0x60) || (c >= 0x7B && c <= 0x7E)) k = WP_PUNCT;
        cls[c] = k;
        nrm[c] = (uint8_t)(lower && c >= 'A' && c <= 'Z' ? c + 32 : c);
    }
}

}  // namespace smt
