// utf8_cursor.h -- what the pass-1 kernels over UTF-8 lines share (wordpiece_utf8_kernels.hip, unigram_utf8_kernels.hip):
// one character of the text and what it becomes -- the strict decode, the lookup in the two-level code-point table of
// wordpiece_table.h --, the cursor over the normalised bytes (raw position of a character, byte within its output), and the lane
// prologue.  Device code only; internal to the library.
//
// Bounds: every decode is handed the end it may read to and checks it before the read; page and pool indices are checked against the
// table's sizes.
#pragma once

#include "tokenize_frame.h"
#include "wordpiece_bytes.h"
#include "wordpiece_table.h"

namespace smt {

enum : uint32_t { AT_BYTE = 0, AT_POOL = 1, AT_TEXT = 2 };

// one character of the text and what it becomes
struct WpChar {
    uint32_t src;     // its bytes in the text (>= 1)
    uint32_t cls;     // WP_ORDINARY .. WP_FLAG; malformed UTF-8 is WP_FLAG with src 1
    uint32_t n;       // bytes of its output (0 for SPACE, DROPPED and FLAG)
    uint32_t chars;   // characters of its output
    uint32_t where;   // the output: AT_BYTE: the one byte `at`; AT_POOL: U.out[at ..]; AT_TEXT: the character's own bytes
    uint32_t at;
};

// the character that starts at q and ends at or before `end` (q < end; nothing outside [q, end) is read)
__device__ __forceinline__ void wp_char_at(const WpCodepoints &U, const uint8_t *cls, const uint8_t *nrm, const uint8_t *__restrict__ text,
                                           uint64_t q, uint64_t end, WpChar &ch)
{
    const uint32_t b0 = text[q];
    ch.src = 1;
    ch.n = 1;
    ch.chars = 1;
    ch.where = AT_BYTE;
    if (b0 < 0x80) {
        ch.cls = cls[b0];
        ch.at = nrm[b0];
        ch.n = ch.chars = (ch.cls == smt::WP_ORDINARY || ch.cls == smt::WP_PUNCT) ? 1u : 0u;
        return;
    }
    ch.cls = smt::WP_FLAG;
    ch.n = 0;
    ch.at = 0;
    uint32_t len, cp;
    if (b0 >= 0xC2 && b0 <= 0xDF) { len = 2; cp = b0 & 0x1Fu; }
    else if ((b0 & 0xF0u) == 0xE0u) { len = 3; cp = b0 & 0x0Fu; }
    else if (b0 >= 0xF0 && b0 <= 0xF4) { len = 4; cp = b0 & 0x07u; }
    else return;                                   // a continuation byte, 0xC0 / 0xC1 (overlong), 0xF5 .. 0xFF
    if (q + len > end) return;                     // cut by the line's end
    for (uint32_t k = 1; k < len; ++k) {
        const uint32_t b = text[q + k];
        if ((b & 0xC0u) != 0x80u) return;
        cp = (cp << 6) | (b & 0x3Fu);
    }
    if (len == 3 && (cp < 0x800u || (cp >= 0xD800u && cp <= 0xDFFFu))) return;
    if (len == 4 && (cp < 0x10000u || cp > 0x10FFFFu)) return;
    const uint32_t pg = U.page[cp >> 8];           // cp <= U+10FFFF: inside the WP_CP_PAGES entries
    if (pg >= U.n_pages) return;
    const uint32_t e = U.ent[pg * 256u + (cp & 255u)];
    const uint32_t k = smt::wp_cp_class(e), nb = smt::wp_cp_bytes(e);
    if (k >= smt::WP_FLAG) return;
    ch.src = len;
    ch.cls = k;
    if (k == smt::WP_SPACE || k == smt::WP_DROPPED) { ch.chars = 0; return; }
    if (nb == 0) { ch.n = len; ch.where = AT_TEXT; return; }          // itself
    if (smt::wp_cp_off(e) + nb > U.out_bytes) { ch.cls = smt::WP_FLAG; ch.src = 1; return; }
    ch.n = nb;
    ch.chars = smt::wp_cp_chars(e);
    ch.where = AT_POOL;
    ch.at = smt::wp_cp_off(e);
}

// byte k (< ch.n) of what the character at q becomes
__device__ __forceinline__ uint32_t wp_byte(const WpCodepoints &U, const uint8_t *__restrict__ text, uint64_t q, const WpChar &ch, uint32_t k)
{
    if (ch.where == AT_BYTE) return ch.at;
    if (ch.where == AT_POOL) return U.out[ch.at + k];
    return text[q + k];
}

// q moves to the first character at or behind it, in front of we, that has output; q >= we: there is none.  (Inside a word every
// character was decoded before: a FLAG here cannot be, and ends the walk.)
__device__ __forceinline__ void wp_next_char(const WpCodepoints &U, const uint8_t *cls, const uint8_t *nrm, const uint8_t *__restrict__ text,
                                             uint64_t &q, uint64_t we, WpChar &ch)
{
    while (q < we) {
        wp_char_at(U, cls, nrm, text, q, we, ch);
        if (ch.cls == smt::WP_FLAG) { q = we; return; }
        if (ch.n) return;
        q += ch.src;
    }
}

// The sibling of tok_scan_lane (tokenize_frame.h) for UTF-8 text: the block's line window behind the kernel's only barrier, the lane's
// line, the looked-at end, and what a lane can decide from its own byte.  False: the lane leaves -- outside every line's looked-at
// bytes; at a byte >= 0x80 of a line longer than keep_bytes (flagged: the host cuts by characters); at a continuation byte (flagged
// unless a lead byte at most three bytes in front, inside the line, covers it).  True: the lane stands at an ASCII or a lead byte c;
// an added token standing there has flagged the line.
__device__ __forceinline__ bool wp_scan_lane_utf8(const smt::TokAdded &A, unsigned threads, uint64_t *s_win, const uint8_t *__restrict__ text,
                                                  uint64_t text_bytes, const uint64_t *__restrict__ line_begin, const uint32_t *__restrict__ line_len,
                                                  uint64_t n_lines, uint32_t keep_bytes, uint8_t *__restrict__ flags, uint64_t &line, uint64_t &lb,
                                                  uint64_t &le, uint8_t &c)
{
    const uint64_t first = (uint64_t)blockIdx.x * threads;
    if (threadIdx.x < 2) {
        const uint64_t last = first + threads - 1 < text_bytes ? first + threads - 1 : text_bytes - 1;
        s_win[threadIdx.x] = smt::tok_count_le(line_begin, 0, n_lines, threadIdx.x == 0 ? first : last);
    }
    __syncthreads();
    const uint64_t p = first + threadIdx.x;
    if (p >= text_bytes) return false;
    const uint64_t n_le = smt::tok_count_le(line_begin, s_win[0], s_win[1], p);
    if (n_le == 0) return false;                 // in front of the first line
    line = n_le - 1;
    lb = line_begin[line];
    const uint32_t ll = line_len[line];
    const bool cut = keep_bytes && keep_bytes < ll;
    const uint64_t le_line = lb + (cut ? keep_bytes : ll);
    le = le_line < text_bytes ? le_line : text_bytes;   // the end of what is looked at
    if (p < lb || p >= le) return false;         // behind the cut, or between two lines
    c = text[p];
    if (c >= 0x80) {
        if (cut) { flags[line] = 1; return false; }
        if ((c & 0xC0) != 0x80) return true;     // a lead byte (or a byte that leads nothing: the decode flags it)
        bool covered = false;
        for (uint32_t d = 1; d <= 3 && p - lb >= d; ++d) {
            const uint32_t b = text[p - d];
            if ((b & 0xC0u) == 0x80u) continue;
            const uint32_t len = (b >= 0xC2 && b <= 0xDF) ? 2u : (b & 0xF0u) == 0xE0u ? 3u : (b >= 0xF0 && b <= 0xF4) ? 4u : 0u;
            covered = len > d;
            break;
        }
        if (!covered) flags[line] = 1;
        return false;
    }
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

}  // namespace smt
