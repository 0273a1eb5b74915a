// unigram_rules_kernels.hip -- pass 1 of the Unigram device tokenizer while a space rule of smt_unigram_set_space_rules is on (DESIGN.md
// 4.9 "Behind a Precompiled normalizer"): ug_scan_kernel (unigram_kernels.hip) and ug_scan_utf8_kernel (unigram_utf8_kernels.hip) with
// the two rules an XLM-R-style chain adds around Metaspace.  With both rules off the launch takes those kernels, which stay as they
// are; what is said there about the lattice, the nodes, the slots and the tie rule holds here word for word.
//
//   collapse_runs   a SPACE character whose nearest earlier not-dropped character of the line is a SPACE too is ABSORBED: its lane
//                   looks back over dropped characters (at most SMT_UG_MAX_WORD raw bytes of them -- more flag the line, as the
//                   measure of the piece they stand in does without long pieces), finds the SPACE and leaves.  It owns no piece and ends none:
//                   the owner in front skips the absorbed spaces and the dropped characters between them on its way to the piece's
//                   first kept character, and counts their raw bytes into the measure like dropped bytes.
//   drop_trailing   a piece that is the replacement alone and ends at the line's looked-at end emits nothing.  When that piece is the
//                   line's only one (nothing but spaces and dropped characters) the line is FLAGGED: a chain that strips gives the
//                   host tokenizer's lone replacement there, one that splits at white space gives nothing.
//
// Bounds: a piece's raw bytes -- the owner's SPACE, the absorbed ones, dropped and kept characters -- stay within SMT_UG_MAX_WORD by the
// measure, so its nodes stay inside UG_NODES, its keys below 2 + SMT_UG_MAX_WORD, and its tokens (<= 1 + its kept characters) inside
// the slots of its own raw bytes: absorbed spaces only add raw bytes.  The look-back reads inside [line begin, p).  LONG PIECES: a
// piece over SMT_UG_MAX_WORD flags its line (the host tokenizer takes it, the ids are its either way) -- unless the launch hands the
// kernels the handle's work list (W.head != nullptr: smt_unigram_set_long_pieces set a limit and smt_unigram_set_long_rules is on).
// Then the owner leaves a record {position, line, at a SPACE | the line's first piece} where its measure passes the bound, in the
// absorbed run or in the piece, and ug_long_rules_kernel (unigram_long_rules_kernels.hip) tokenizes the piece with a wave.  The
// look-back of a SPACE lane stays bounded either way: more than SMT_UG_MAX_WORD raw bytes of dropped characters directly in front of
// a SPACE flag the line -- a rule of the device form, no longer implied by the measure of the piece they stand in.
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
using smt::UgCursor;
using smt::UgTable;
using smt::WpChar;
using smt::WpCodepoints;
using smt::ug_probe;
using smt::ug_probe_utf8;
using smt::wp_byte;
using smt::wp_char_at;
using smt::wp_next_char;

enum : uint32_t { FRONT_NONE = 0, FRONT_SPACE = 1, FRONT_KEPT = 2 };   // the nearest not-dropped character in front of a SPACE

__global__ void __launch_bounds__(UG_THREADS) ug_scan_rules_kernel(UgTable T, uint32_t rules, const uint8_t *__restrict__ text, uint64_t text_bytes,
                                                             const uint64_t *__restrict__ line_begin, const uint32_t *__restrict__ line_len,
                                                             uint64_t n_lines, uint32_t keep_bytes, int drop_unk, uint32_t *__restrict__ ids_tmp,
                                                             uint32_t *__restrict__ raw_count, uint8_t *__restrict__ flags, smt::UgLongList W)
{
    __shared__ uint8_t s_map[128];
    __shared__ uint64_t s_win[2];
    __shared__ double s_score[UG_NODES];
    __shared__ uint32_t s_id[UG_NODES];
    __shared__ uint16_t s_from[UG_NODES];
    if (threadIdx.x < 128) s_map[threadIdx.x] = T.map[threadIdx.x];
    uint64_t line, lb, le;
    uint8_t c;
    // (the only barrier is in there: lanes leave freely below)
    if (!smt::tok_scan_lane(T.added, UG_THREADS, s_win, text, text_bytes, line_begin, line_len, n_lines, keep_bytes, flags, line, lb, le, c)) return;
    const uint64_t first = (uint64_t)blockIdx.x * UG_THREADS, p = first + threadIdx.x;
    const bool at_space = s_map[c] == ' ';
    if (!at_space && p != lb) return;            // no piece starts here
    // ---- the space rules: what stands in front of a SPACE, dropped bytes skipped (at most SMT_UG_MAX_WORD of them: more flag
    // the line -- the look-back bound)
    const bool collapse = (rules & smt::UG_RULE_COLLAPSE) != 0;
    bool first_piece = !at_space;                // nothing of the line but dropped bytes stands in front of the owner
    if (at_space) {
        uint32_t front = FRONT_NONE, back = 0;
        for (uint64_t q = p; q > lb && front == FRONT_NONE;) {
            const uint8_t b = text[--q];
            if (b >= 0x80) return;               // (the line is flagged by that byte's lane)
            const uint8_t m = s_map[b];
            if (m == UG_DROP) { if (++back > SMT_UG_MAX_WORD) { flags[line] = 1; return; } }
            else front = m == ' ' ? FRONT_SPACE : FRONT_KEPT;
        }
        if (collapse && front == FRONT_SPACE) return;   // absorbed: the space in front (or its owner) has this one in its piece
        first_piece = front == FRONT_NONE;
    }
    // ---- the piece: [R] + the kept bytes of [run, end); its measure is its raw bytes (+ 1 for a prepended R)
    const bool has_r = at_space || T.prepend != 2;
    uint64_t run = at_space ? p + 1 : p;
    const uint64_t base = at_space ? p + line + 1 : lb + line;   // the piece's first slot
    const uint32_t rel = (uint32_t)(p - first);  // node of raw byte q: q - first; its key: 2 + q - p
    uint32_t measure = has_r ? 1 : 0, n_kept = 0;
    if (collapse && at_space)                    // the absorbed spaces (and dropped bytes) in front of the piece's first kept byte
        for (; run < le; ++run) {
            const uint8_t b = text[run];
            if (b >= 0x80) return;
            const uint8_t m = s_map[b];
            if (m != ' ' && m != UG_DROP) break;
            if (++measure > SMT_UG_MAX_WORD) { smt::ug_hand_over(W, p, line, at_space, flags, first_piece); return; }   // flagged, or ug_long_rules_kernel's
        }
    uint64_t end = run, last_q = run;
    for (; end < le; ++end) {
        const uint8_t b = text[end];
        if (b >= 0x80) return;                   // (the line is flagged by that byte's lane: nothing of it is used)
        const uint8_t m = s_map[b];
        if (m == ' ') break;
        if (++measure > SMT_UG_MAX_WORD) { smt::ug_hand_over(W, p, line, at_space, flags, first_piece); return; }   // a long piece: flagged, or ug_long_rules_kernel's
        if (m == UG_DROP) continue;
        s_from[end - first] = FROM_UNSET;
        last_q = end;
        ++n_kept;
    }
    if (!at_space && n_kept == 0 && end < le) return;   // the normalised text starts with R: that byte's lane owns the first piece
    if (!has_r && n_kept == 0) return;                   // nothing is left of the line
    if ((rules & smt::UG_RULE_DROP_TRAILING) && n_kept == 0 && end == le) {   // R alone at the line's end emits nothing; as the line's
        if (first_piece) flags[line] = 1;                                     // only piece it is the host's (the chains differ there)
        return;
    }
    // ---- the lattice
    const double r_score = T.r_score + 0.0;
    // every edge out of one start: the pieces of `kind` found while the end walks forward from q0, the unknown edge over the first
    // character when no piece covers exactly it (the walk from the piece's start through R offers none: R's own edge is T.r_*)
    auto relax = [&](double here, uint32_t key, unsigned long long h, uint32_t kind, uint64_t q0) {
        bool single = false;
        uint32_t clen = 0, len = kind ? T.rlen : 0;
        uint64_t first_q = end;
        for (uint64_t q = q0; q < end; ++q) {
            const uint8_t m = s_map[text[q]];
            if (m == UG_DROP) continue;
            if (clen == 0) first_q = q;
            if (len >= T.max_piece) break;
            h = (h ^ m) * smt::TOK_HASH_MUL;
            ++clen;
            ++len;
            const uint32_t e = ug_probe(T, text, s_map, h, kind, q0, clen);
            if (!e) continue;
            if (clen == 1) single = true;
            const double cand = T.score[e - 1] + here;
            const uint32_t n = (uint32_t)(q - first);
            const uint16_t f = s_from[n];
            if (f == FROM_UNSET || cand > s_score[n] || (cand == s_score[n] && key < (uint32_t)(f & 0x7FFF))) {
                s_score[n] = cand;
                s_id[n] = T.ent[e - 1].z;
                s_from[n] = (uint16_t)key;
            }
        }
        if (kind == 0 && !single && first_q < end) {
            const double cand = T.unk_score + here;
            const uint32_t n = (uint32_t)(first_q - first);
            const uint16_t f = s_from[n];
            if (f == FROM_UNSET || cand > s_score[n] || (cand == s_score[n] && key < (uint32_t)(f & 0x7FFF))) {
                s_score[n] = cand;
                s_id[n] = T.unk == smt::TOK_NONE ? 0u : T.unk;
                s_from[n] = (uint16_t)(key | FROM_UNK);
            }
        }
    };
    if (has_r) {
        relax(0.0, KEY_START, T.r_state, 1, run);
        relax(r_score, KEY_R, smt::TOK_HASH_SEED, 0, run);
    } else {
        relax(0.0, KEY_START, smt::TOK_HASH_SEED, 0, run);
    }
    for (uint64_t q = run; q < end; ++q) {
        if (s_map[text[q]] == UG_DROP) continue;
        relax(s_score[q - first], 2 + (uint32_t)(q - p), smt::TOK_HASH_SEED, 0, q + 1);
    }
    // ---- back along the best path, twice: count what stays (consecutive unknowns fuse, the unk id is dropped), then write
    const uint32_t end_key = n_kept ? 2 + (uint32_t)(last_q - p) : KEY_R;
    const bool dropping = drop_unk && T.unk != smt::TOK_NONE;
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
    }
    if (n_tok) atomicAdd(&raw_count[line], n_tok);
}

__global__ void __launch_bounds__(UG_THREADS) ug_scan_utf8_rules_kernel(UgTable T, WpCodepoints U, uint32_t rules, const uint8_t *__restrict__ text, uint64_t text_bytes,
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
    // ---- the space rules: what stands in front of a SPACE character, dropped characters skipped (at most SMT_UG_MAX_WORD raw bytes of
    // them: more flag the line -- the look-back bound).  A character in front that does not end exactly here is
    // malformed, and its own lanes flag the line.
    const bool collapse = (rules & smt::UG_RULE_COLLAPSE) != 0;
    bool first_piece = !at_space;                // nothing of the line but dropped characters stands in front of the owner
    if (at_space) {
        uint32_t front = FRONT_NONE, back = 0;
        for (uint64_t cur = p; cur > lb && front == FRONT_NONE;) {
            uint64_t q = cur - 1;
            for (uint32_t d = 1; d < 4 && q > lb && (text[q] & 0xC0u) == 0x80u; ++d) --q;
            WpChar pc;
            wp_char_at(U, cls, nrm, text, q, le, pc);
            if (pc.cls == smt::WP_FLAG || q + pc.src != cur) return;
            if (pc.cls == smt::WP_DROPPED) { back += pc.src; if (back > SMT_UG_MAX_WORD) { flags[line] = 1; return; } }
            else front = pc.cls == smt::WP_SPACE ? FRONT_SPACE : FRONT_KEPT;
            cur = q;
        }
        if (collapse && front == FRONT_SPACE) return;   // absorbed: the space in front (or its owner) has this one in its piece
        first_piece = front == FRONT_NONE;
    }
    // ---- the piece: [R] + the normalised characters of [run, end); its measure is its raw bytes, the SPACE character (or a prepended
    // R) counted as one
    const bool has_r = at_space || T.prepend != 2;
    uint64_t run = at_space ? p + me.src : p;
    const uint64_t base = at_space ? p + line + 1 : lb + line;   // the piece's first slot
    const uint32_t rel = (uint32_t)(p - first);
    // node of output character j of the source character at q: q - origin + j (origin = first + the bytes of the SPACE character
    // beyond its first); its key: 2 + node - rel
    const uint64_t origin = first + (at_space ? me.src - 1 : 0);
    uint32_t measure = has_r ? 1 : 0, n_kept = 0, last_key = KEY_R;
    if (collapse && at_space)                    // the absorbed spaces (and dropped characters) in front of the piece's first kept one
        while (run < le) {
            WpChar nc;
            wp_char_at(U, cls, nrm, text, run, le, nc);
            if (nc.cls == smt::WP_FLAG) return;
            if (nc.cls != smt::WP_SPACE && nc.cls != smt::WP_DROPPED) break;
            measure += nc.src;
            if (measure > SMT_UG_MAX_WORD) { smt::ug_hand_over(W, p, line, at_space, flags, first_piece); return; }   // flagged, or ug_long_rules_kernel's
            run += nc.src;
        }
    uint64_t end = run;
    while (end < le) {
        WpChar nc;
        wp_char_at(U, cls, nrm, text, end, le, nc);
        if (nc.cls == smt::WP_FLAG) return;      // (the line is flagged by that character's lane: nothing of it is used)
        if (nc.cls == smt::WP_SPACE) break;
        measure += nc.src;
        if (measure > SMT_UG_MAX_WORD) { smt::ug_hand_over(W, p, line, at_space, flags, first_piece); return; }   // a long piece: flagged, or ug_long_rules_kernel's
        for (uint32_t j = 0; j < nc.chars; ++j) s_from[end - origin + j] = FROM_UNSET;   // (chars <= src: inside the character's own bytes)
        if (nc.chars) last_key = 2 + (uint32_t)(end - origin) + nc.chars - 1 - rel;
        n_kept += nc.chars;
        end += nc.src;
    }
    if (!at_space && n_kept == 0 && end < le) return;   // the normalised text starts with R: that character's lane owns the first piece
    if (!has_r && n_kept == 0) return;                   // nothing is left of the line
    if ((rules & smt::UG_RULE_DROP_TRAILING) && n_kept == 0 && end == le) {   // R alone at the line's end emits nothing; as the line's
        if (first_piece) flags[line] = 1;                                     // only piece it is the host's (the chains differ there)
        return;
    }
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

int ug_scan_rules_launch(smt_unigram *tok, const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev,
                         const uint32_t *line_len_dev, uint64_t n_lines, uint32_t keep_bytes, int drop_unk, uint8_t *flags_dev)
{
    const dim3 grid((unsigned)((text_bytes + UG_THREADS - 1) / UG_THREADS));
    const smt::UgLongList W = tok->long_list();   // head == nullptr unless smt_unigram_set_long_pieces and _set_long_rules are both on
    if (tok->utf8)
        hipLaunchKernelGGL(ug_scan_utf8_rules_kernel, grid, dim3(UG_THREADS), 0, tok->ctx->stream, tok->T, tok->U, tok->rules, text_dev, text_bytes,
                           line_begin_dev, line_len_dev, n_lines, keep_bytes, drop_unk, tok->S.d_ids_tmp, tok->S.raw_count(), flags_dev, W);
    else
        hipLaunchKernelGGL(ug_scan_rules_kernel, grid, dim3(UG_THREADS), 0, tok->ctx->stream, tok->T, tok->rules, text_dev, text_bytes, line_begin_dev,
                           line_len_dev, n_lines, keep_bytes, drop_unk, tok->S.d_ids_tmp, tok->S.raw_count(), flags_dev, W);
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

}  // namespace smt

extern "C" {

int smt_unigram_set_space_rules(smt_unigram *tok, int collapse_runs, int drop_trailing)
try {
    if (!tok) return smt::tok_null_handle("smt_unigram_set_space_rules");
    SMT_REQUIRE((collapse_runs == 0 || collapse_runs == 1) && (drop_trailing == 0 || drop_trailing == 1), "collapse_runs and drop_trailing are 0 or 1");
    tok->rules = (collapse_runs ? smt::UG_RULE_COLLAPSE : 0u) | (drop_trailing ? smt::UG_RULE_DROP_TRAILING : 0u);
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

}  // extern "C"
