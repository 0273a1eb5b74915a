// unigram_utf8_kernels.hip -- Unigram over UTF-8 lines on the device (DESIGN.md 4.9 "Unigram over UTF-8 lines"): pass 1 of the handle
// smt_unigram_create_utf8 makes.  The decomposition of unigram_kernels.hip -- one lane per text BYTE, the line by the block-narrowed
// binary search, one barrier, the lattice in LDS, nothing in global memory beyond the id slots -- with the rules stated on CHARACTERS
// (utf8_cursor.h: the strict decode, the two-level code-point table, the cursor over the normalised bytes):
//
//   * a lane at a continuation byte only checks that a lead byte in front of it covers it, and leaves;
//   * a lane at a lead byte decodes its character strictly and looks it up; a FLAG code point or malformed UTF-8 flags the line;
//   * the OWNER of a piece is the lane at a SPACE character's lead byte, or at the line's first byte; its walk to the piece's end steps
//     by characters and stops at a SPACE character or the looked-at end;
//   * the piece's measure stays in RAW BYTES against SMT_UG_MAX_WORD, with the SPACE character counted as one whatever its length, so
//     ASCII lines are flagged exactly as by ug_scan_kernel (or, with long pieces on, handed to ug_long_kernel exactly as there);
//   * a lattice position is a normalised CHARACTER.  The node of output character j of the source character at raw byte q is the node
//     of raw byte q + j: an output has no more characters than its source has bytes, so the nodes of two source characters never
//     meet.  A SPACE character of s bytes shifts its piece's nodes down by s - 1, into its own bytes, so that the nodes a block's
//     pieces use stay inside UG_NODES and inside the raw bytes of their own piece: pieces are disjoint, no two lanes share a node.
//   * edges: one forward walk per start over the normalised-byte cursor, the FNV state carried byte by byte; a candidate is probed
//     only where the next normalised byte starts a character, and the probe's compare walks the same cursor.  The unknown edge covers
//     one normalised character of any byte length, offered only where no piece covers exactly it.  The sums, the tie rule (the
//     smallest start wins, a comparison of keys) and the fusing of unknowns are ug_scan_kernel's.
//
// Slots: a piece's tokens <= its normalised characters (+ 1 for R) <= its raw bytes, so line i still owns [begin_i + i, begin_{i+1} +
// i + 1) and slot order is token order; a slot is written only below the piece's raw end.
//
// Every loop advances at least one byte towards the piece's end or is bounded by the table's capacity; every decode is handed the
// end it may read to.
#include "common.h"
#include "tokenize_frame.h"
#include "unigram_probe.h"
#include "unigram_table.h"
#include "utf8_cursor.h"

namespace {

using smt::FROM_UNK;
using smt::FROM_UNSET;
using smt::KEY_R;
using smt::KEY_START;
using smt::UG_DROP;
using smt::UG_NODES;
using smt::UG_THREADS;
using smt::UgTable;
using smt::UgCursor;
using smt::ug_probe_utf8;
using smt::WpChar;
using smt::WpCodepoints;
using smt::wp_byte;
using smt::wp_char_at;
using smt::wp_next_char;

__global__ void __launch_bounds__(UG_THREADS) ug_scan_utf8_kernel(UgTable T, WpCodepoints U, const uint8_t *__restrict__ text, uint64_t text_bytes,
                                                                  const uint64_t *__restrict__ line_begin, const uint32_t *__restrict__ line_len,
                                                                  uint64_t n_lines, uint32_t keep_bytes, int drop_unk, uint32_t *__restrict__ ids_tmp,
                                                                  uint32_t *__restrict__ raw_count, uint8_t *__restrict__ flags, smt::UgLongList W)
{
    __shared__ uint8_t s_bytes[256];   // cls[128] | nrm[128] of the ASCII bytes, from the byte map
    __shared__ uint64_t s_win[2];
    __shared__ double s_score[UG_NODES];
    __shared__ uint32_t s_id[UG_NODES];
    __shared__ uint16_t s_from[UG_NODES];
    {
        const uint8_t m = T.map[threadIdx.x & 127];
        s_bytes[threadIdx.x] = threadIdx.x >= 128 ? m : m == ' ' ? (uint8_t)smt::WP_SPACE : m == UG_DROP ? (uint8_t)smt::WP_DROPPED : (uint8_t)smt::WP_ORDINARY;
    }
    uint64_t line, lb, le;
    uint8_t c;
    // (the only barrier is in there: lanes leave freely below)
    if (!smt::wp_scan_lane_utf8(T.added, UG_THREADS, s_win, text, text_bytes, line_begin, line_len, n_lines, keep_bytes, flags, line, lb, le, c)) return;
    const uint8_t *cls = s_bytes, *nrm = s_bytes + 128;
    const uint64_t first = (uint64_t)blockIdx.x * UG_THREADS, p = first + threadIdx.x;
    WpChar me;
    wp_char_at(U, cls, nrm, text, p, le, me);
    if (me.cls == smt::WP_FLAG) { flags[line] = 1; return; }   // a FLAG code point, or malformed UTF-8
    const bool at_space = me.cls == smt::WP_SPACE;
    if (!at_space && p != lb) return;            // no piece starts here
    // ---- the piece: [R] + the normalised characters of [run, end); its measure is its raw bytes, the SPACE character (or a prepended
    // R) counted as one
    const bool has_r = at_space || T.prepend != 2;
    const uint64_t run = at_space ? p + me.src : p;
    const uint64_t base = at_space ? p + line + 1 : lb + line;   // the piece's first slot
    const uint32_t rel = (uint32_t)(p - first);
    // node of output character j of the source character at q: q - origin + j (origin = first + the bytes of the SPACE character
    // beyond its first); its key: 2 + node - rel
    const uint64_t origin = first + (at_space ? me.src - 1 : 0);
    uint32_t measure = has_r ? 1 : 0, n_kept = 0, last_key = KEY_R;
    uint64_t end = run;
    while (end < le) {
        WpChar nc;
        wp_char_at(U, cls, nrm, text, end, le, nc);
        if (nc.cls == smt::WP_FLAG) return;      // (the line is flagged by that character's lane: nothing of it is used)
        if (nc.cls == smt::WP_SPACE) break;
        measure += nc.src;
        if (measure > SMT_UG_MAX_WORD) { smt::ug_hand_over(W, p, line, at_space, flags); return; }   // a long piece: flagged, or ug_long_kernel's
        for (uint32_t j = 0; j < nc.chars; ++j) s_from[end - origin + j] = FROM_UNSET;   // (chars <= src: inside the character's own bytes)
        if (nc.chars) last_key = 2 + (uint32_t)(end - origin) + nc.chars - 1 - rel;
        n_kept += nc.chars;
        end += nc.src;
    }
    if (!at_space && n_kept == 0 && end < le) return;   // the normalised text starts with R: that character's lane owns the first piece
    if (!has_r && n_kept == 0) return;                   // nothing is left of the line
    // ---- the lattice
    const double r_score = T.r_score + 0.0;
    // every edge out of one start: the pieces of `kind` found while the end walks forward from the cursor s (at a character that has
    // output, or at the piece's end), the unknown edge over the first character when no piece covers exactly it (the walk from the
    // piece's start through R offers none: R's own edge is T.r_*)
    auto relax = [&](double here, uint32_t key, unsigned long long h, uint32_t kind, const UgCursor &s) {
        bool single = false;
        uint32_t clen = 0, len = kind ? T.rlen : 0, n_char = 0;
        UgCursor w = s;
        while (w.q < end) {
            if (len >= T.max_piece) break;
            h = (h ^ wp_byte(U, text, w.q, w.c, w.k)) * smt::TOK_HASH_MUL;
            ++clen;
            ++len;
            ++w.k;
            const bool last = w.k >= w.c.n;      // of the source character's output
            if (last || (wp_byte(U, text, w.q, w.c, w.k) & 0xC0u) != 0x80u) {   // the next normalised byte starts a character
                ++n_char;
                const uint32_t e = ug_probe_utf8(T, U, text, cls, nrm, h, kind, s, end, clen);
                if (e) {
                    if (n_char == 1) single = true;
                    const double cand = T.score[e - 1] + here;
                    const uint32_t n = (uint32_t)(w.q - origin) + w.j;
                    const uint16_t f = s_from[n];
                    if (f == FROM_UNSET || cand > s_score[n] || (cand == s_score[n] && key < (uint32_t)(f & 0x7FFF))) {
                        s_score[n] = cand;
                        s_id[n] = T.ent[e - 1].z;
                        s_from[n] = (uint16_t)key;
                    }
                }
                ++w.j;
            }
            if (last) { w.q += w.c.src; w.k = 0; w.j = 0; wp_next_char(U, cls, nrm, text, w.q, end, w.c); }
        }
        if (kind == 0 && !single && s.q < end) {
            const double cand = T.unk_score + here;
            const uint32_t n = (uint32_t)(s.q - origin) + s.j;
            const uint16_t f = s_from[n];
            if (f == FROM_UNSET || cand > s_score[n] || (cand == s_score[n] && key < (uint32_t)(f & 0x7FFF))) {
                s_score[n] = cand;
                s_id[n] = T.unk == smt::TOK_NONE ? 0u : T.unk;
                s_from[n] = (uint16_t)(key | FROM_UNK);
            }
        }
    };
    UgCursor at;
    at.q = run;
    at.k = at.j = 0;
    at.c = me;
    wp_next_char(U, cls, nrm, text, at.q, end, at.c);
    if (has_r) {
        relax(0.0, KEY_START, T.r_state, 1, at);
        relax(r_score, KEY_R, smt::TOK_HASH_SEED, 0, at);
    } else {
        relax(0.0, KEY_START, smt::TOK_HASH_SEED, 0, at);
    }
    while (at.q < end) {   // `at` stands at the start of an output character: its node is final, the edges out of it start behind it
        const uint32_t n = (uint32_t)(at.q - origin) + at.j;
        do ++at.k; while (at.k < at.c.n && (wp_byte(U, text, at.q, at.c, at.k) & 0xC0u) == 0x80u);
        ++at.j;
        if (at.k >= at.c.n) { at.q += at.c.src; at.k = at.j = 0; wp_next_char(U, cls, nrm, text, at.q, end, at.c); }
        relax(s_score[n], 2 + n - rel, smt::TOK_HASH_SEED, 0, at);
    }
    // ---- back along the best path, twice: count what stays (consecutive unknowns fuse, the unk id is dropped), then write
    const uint32_t end_key = n_kept ? last_key : KEY_R;
    const bool dropping = drop_unk && T.unk != smt::TOK_NONE;
    const uint64_t room = end + line + 1 - base;   // the piece's slots end below its raw end
    uint32_t n_tok = 0;
    for (int pass = 0; pass < 2; ++pass) {
        uint32_t key = end_key, k = n_tok;
        for (uint32_t step = 0; step <= SMT_UG_MAX_WORD && key != KEY_START; ++step) {
            uint32_t id, from;
            bool unk;
            if (key == KEY_R) { id = T.r_id; unk = T.r_unk != 0; from = KEY_START; }
            else { const uint32_t n = rel + key - 2; const uint16_t f = s_from[n]; id = s_id[n]; unk = (f & FROM_UNK) != 0; from = f & 0x7FFF; }
            bool pred_unk = false;
            if (from == KEY_R) pred_unk = T.r_unk != 0;
            else if (from != KEY_START) pred_unk = (s_from[rel + from - 2] & FROM_UNK) != 0;
            if (unk && T.unk == smt::TOK_NONE) { flags[line] = 1; return; }   // (first pass: nothing is written yet)
            if (!(unk && pred_unk) && !(dropping && id == T.unk)) {
                if (pass == 0) ++n_tok;
                else ids_tmp[base + --k] = id;
            }
            key = from;
        }
        if (pass == 0 && n_tok > room) { flags[line] = 1; return; }   // (cannot be: tokens <= characters <= raw bytes; nothing is written yet)
    }
    if (n_tok) atomicAdd(&raw_count[line], n_tok);
}

}  // namespace

namespace smt {

int ug_scan_utf8_launch(smt_unigram *tok, const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev,
                        const uint32_t *line_len_dev, uint64_t n_lines, uint32_t keep_bytes, int drop_unk, uint8_t *flags_dev)
{
    hipLaunchKernelGGL(ug_scan_utf8_kernel, dim3((unsigned)((text_bytes + UG_THREADS - 1) / UG_THREADS)), dim3(UG_THREADS), 0, tok->ctx->stream,
                       tok->T, tok->U, text_dev, text_bytes, line_begin_dev, line_len_dev, n_lines, keep_bytes, drop_unk, tok->S.d_ids_tmp,
                       tok->S.raw_count(), flags_dev, tok->long_list());
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

}  // namespace smt
