// unigram_kernels.hip -- Unigram over pure-ASCII lines on the device ("Unigram"): a per-byte normalizer table, Metaspace
// and the Viterbi of hf_tokenizer.cpp's unigram(), the same ids, as the CSR K1 reads.
//
// Pass 1 is dealt by TEXT POSITION, one lane per byte, as wp_scan_kernel: the lane finds its line (the block-narrowed binary search),
// flags the line for a byte >= 0x80 or an added token standing there, and OWNS a piece when it stands at the piece's start: a byte
// the table maps to ' ' (it becomes the replacement character R, and every R starts a piece), or the line's first byte (the piece in
// front of the first R, with R prepended unless the scheme is `never`).  The owner walks to the piece's end, then runs the lattice
// over the piece's characters: from every character position one forward walk carries the FNV state byte by byte and probes every
// end up to the longest piece (no candidate is hashed twice), f64 sums formed as score[piece] + best[at], one add per edge.  THE TIE
// RULE: among candidates of equal sum for one end position the one with the SMALLEST START wins (the unknown edge has the largest
// start its end can have); it is stated in relax() as a comparison of starts, not left to the visiting order.
//
// The lattice lives in LDS: a node (best sum f64, id u32, start + unknown bit u16 = 14 bytes) per raw byte the block's pieces can
// reach -- a piece is at most SMT_UG_MAX_WORD raw bytes, so the pieces that start in a block of 256 bytes end within 256 +
// SMT_UG_MAX_WORD bytes, pieces are disjoint, and no two lanes share a node.  The node behind a leading R is held in registers.  No
// global scratch besides the id slots: 4 bytes per text byte + 4 per line (+ 8 per line for the slots' line starts).
//
// A line of n looked-at bytes can hold n + 1 tokens (the prepended R), so line i owns the slots [begin_i + i, begin_{i+1} + i + 1): the
// first piece writes from begin_i + i, the piece of a space at p from p + i + 1.  A piece has no more tokens than characters, so no two
// pieces share a slot and slot order is token order; pass 2 is the shared one (tokenize_frame.h) on these slots.
//
// Every loop is bounded: probes by the table's capacity, walks by the longest piece and the piece's end, pieces by SMT_UG_MAX_WORD.
// A piece whose measure passes SMT_UG_MAX_WORD flags its line -- or, while smt_unigram_set_long_pieces has the switch on, its owner
// leaves a record in the work list of unigram_table.h and ug_long_kernel (unigram_long_kernels.hip) tokenizes it with a wave.
//
// While a space rule of smt_unigram_set_space_rules is on, pass 1 of either form is unigram_rules_kernels.hip's -- followed by
// ug_long_rules_kernel (unigram_long_rules_kernels.hip) while smt_unigram_set_long_rules lets those kernels hand long pieces over; the
// vocabulary probe the kernels share is in unigram_probe.h.
//
// Also here: the create of both forms of the handle.  The UTF-8 form's pass 1 is unigram_utf8_kernels.hip; the table and the handle
// the two share are in unigram_table.h.
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "common.h"
#include "tokenize_frame.h"
#include "unigram_probe.h"
#include "unigram_table.h"

namespace {

using smt::FROM_UNK;
using smt::FROM_UNSET;
using smt::KEY_R;
using smt::KEY_START;
using smt::UG_DROP;
using smt::UG_NODES;
using smt::UG_THREADS;
using smt::UgTable;
using smt::ug_probe;

__global__ void __launch_bounds__(256) ug_slot_begin_kernel(const uint64_t *__restrict__ line_begin, uint64_t n_lines, uint64_t *__restrict__ slot_begin)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_lines) slot_begin[i] = line_begin[i] + i;
}

__global__ void __launch_bounds__(UG_THREADS) ug_scan_kernel(UgTable T, const uint8_t *__restrict__ text, uint64_t text_bytes,
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
    // ---- the piece: [R] + the kept bytes of [run, end); its measure is its raw bytes (+ 1 for a prepended R)
    const bool has_r = at_space || T.prepend != 2;
    const uint64_t run = at_space ? p + 1 : p;
    const uint64_t base = at_space ? p + line + 1 : lb + line;   // the piece's first slot
    const uint32_t rel = (uint32_t)(p - first);  // node of raw byte q: q - first; its key: 2 + q - p
    uint32_t measure = has_r ? 1 : 0, n_kept = 0;
    uint64_t end = run, last_q = run;
    for (; end < le; ++end) {
        const uint8_t b = text[end];
        if (b >= 0x80) return;                   // (the line is flagged by that byte's lane: nothing of it is used)
        const uint8_t m = s_map[b];
        if (m == ' ') break;
        if (++measure > SMT_UG_MAX_WORD) { smt::ug_hand_over(W, p, line, at_space, flags); return; }   // a long piece: flagged, or ug_long_kernel's
        if (m == UG_DROP) continue;
        s_from[end - first] = FROM_UNSET;
        last_q = end;
        ++n_kept;
    }
    if (!at_space && n_kept == 0 && end < le) return;   // the normalised text starts with R: that byte's lane owns the first piece
    if (!has_r && n_kept == 0) return;                   // nothing is left of the line
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

constexpr smt::TokWords UG_WORDS = {"no scan to emit (smt_unigram_scan_device comes first)",
                                    "ids_cap is below the looked-at bytes of all lines + one per line + the patch ids",
                                    "ids_cap is below the looked-at bytes of all lines + one per line (ids_cap >= looked + n_lines)"};

}  // namespace

smt_unigram::smt_unigram(smt_ctx *c) : smt::TokHandle(c, true, UG_WORDS) {}

int smt::ug_slot_begin_launch(smt_unigram *tok, const uint64_t *line_begin_dev, uint64_t n_lines)
{
    hipLaunchKernelGGL(ug_slot_begin_kernel, dim3((unsigned)((n_lines + 255) / 256)), dim3(256), 0, tok->ctx->stream, line_begin_dev, n_lines,
                       tok->S.slot_begin());
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

int smt_unigram::pass1(const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev, const uint32_t *line_len_dev, uint64_t n_lines,
                       uint32_t keep_bytes, int drop_unk, uint8_t *flags_dev)
{
    long_scanned = hands_over();
    if (!n_lines) return SMT_OK;
    int rc = smt::ug_slot_begin_launch(this, line_begin_dev, n_lines);
    if (rc) return rc;
    if (!text_bytes) return SMT_OK;
    if (rules) {
        if ((rc = smt::ug_scan_rules_launch(this, text_dev, text_bytes, line_begin_dev, line_len_dev, n_lines, keep_bytes, drop_unk, flags_dev))) return rc;
        return hands_over() ? smt::ug_long_rules_launch(this, text_dev, text_bytes, line_begin_dev, line_len_dev, n_lines, keep_bytes, drop_unk, flags_dev) : SMT_OK;
    }
    if (utf8) {
        if ((rc = smt::ug_scan_utf8_launch(this, text_dev, text_bytes, line_begin_dev, line_len_dev, n_lines, keep_bytes, drop_unk, flags_dev))) return rc;
        return max_long ? smt::ug_long_launch(this, text_dev, text_bytes, line_begin_dev, line_len_dev, n_lines, keep_bytes, drop_unk, flags_dev) : SMT_OK;
    }
    hipLaunchKernelGGL(ug_scan_kernel, dim3((unsigned)((text_bytes + UG_THREADS - 1) / UG_THREADS)), dim3(UG_THREADS), 0, ctx->stream, T, text_dev,
                       text_bytes, line_begin_dev, line_len_dev, n_lines, keep_bytes, drop_unk, S.d_ids_tmp, S.raw_count(), flags_dev, long_list());
    SMT_HIP_CHECK(hipGetLastError());
    if (max_long) return smt::ug_long_launch(this, text_dev, text_bytes, line_begin_dev, line_len_dev, n_lines, keep_bytes, drop_unk, flags_dev);
    return SMT_OK;
}

using namespace smt;

TokHandle *smt::tok_handle(smt_unigram *tok) { return tok; }

// the body of both creates.  cp == nullptr: the ASCII form (a byte >= 0x80 flags its line, pieces with such a byte cannot match and
// are left out); otherwise the UTF-8 form: all pieces enter, the code points come from *cp
static int ug_create(smt_ctx *ctx, const smt_unigram_params *p, const smt_wordpiece_codepoints *cp, smt_unigram **out)
{
    SMT_REQUIRE(p != nullptr && out != nullptr, "null argument");
    *out = nullptr;
    SMT_REQUIRE(p->n_pieces == 0 || (p->pool && p->piece_off && p->piece_id && p->scores), "vocabulary arrays");
    SMT_REQUIRE(p->n_pieces < 0x7FFFFFFFull, "too many pieces");
    SMT_REQUIRE(p->unk_id >= -1 && p->unk_id < 0xFFFFFFFFll, "unk_id");
    SMT_REQUIRE(p->replacement != nullptr && p->replacement_len >= 2 && p->replacement_len <= 4, "the replacement must be one character >= U+0080");
    SMT_REQUIRE((uint8_t)p->replacement[0] >= 0xC0, "the replacement must be one character >= U+0080");
    for (uint32_t i = 1; i < p->replacement_len; ++i) SMT_REQUIRE(((uint8_t)p->replacement[i] & 0xC0) == 0x80, "the replacement must be one UTF-8 character");
    SMT_REQUIRE(p->prepend <= 2, "prepend");
    SMT_REQUIRE(p->byte_map != nullptr, "byte_map");
    for (int c = 0; c < 128; ++c) SMT_REQUIRE(p->byte_map[c] < 0x80 || p->byte_map[c] == UG_DROP, "byte_map entries are ASCII bytes or 0xFF");
    SMT_REQUIRE(p->n_added == 0 || (p->added_pool && p->added_off), "added tokens");
    for (uint64_t i = 0; i < p->n_pieces; ++i) SMT_REQUIRE(p->piece_off[i] <= p->piece_off[i + 1], "piece_off must be non-decreasing");
    for (uint32_t i = 0; i < p->n_added; ++i) SMT_REQUIRE(p->added_off[i] <= p->added_off[i + 1], "added_off must be non-decreasing");
    WpCodepointImage img;
    int rc = SMT_OK;
    if (cp) {   // (validated before anything is uploaded)
        TokAdded probe;
        if ((rc = tok_added_first(p, probe))) return rc;
        for (uint64_t i = 0; i < cp->n && cp->cls; ++i)
            SMT_REQUIRE(cp->cls[i] != SMT_WP_CP_ALONE, "a code point of class ALONE has no meaning behind Metaspace");
        if ((rc = wp_codepoint_image(cp, img))) return rc;
    }
    if ((rc = bind_device(ctx))) return rc;

    // ---- entries: every ASCII piece (kind 0) and every piece that is R + ASCII bytes (kind 1).  R alone is no entry: its edge is
    // fixed (T.r_*).  ASCII form: every other piece with a byte >= 0x80 cannot match an ASCII line, but counts for the longest-piece
    // bound.  UTF-8 form: those pieces enter too.
    const uint32_t rlen = p->replacement_len;
    const uint64_t r_state = tok_hash_bytes(p->replacement, rlen);
    std::vector<TokEntry> ents;
    ents.reserve(p->n_pieces);
    uint32_t max_piece = 0;
    bool r_known = false;
    uint32_t r_id = 0;
    double r_score = 0.0;
    for (uint64_t i = 0; i < p->n_pieces; ++i) {
        const uint32_t off = p->piece_off[i], len = p->piece_off[i + 1] - off;
        max_piece = std::max(max_piece, len);
        if (len == 0) continue;
        const bool with_r = len >= rlen && memcmp(p->pool + off, p->replacement, rlen) == 0;
        bool ascii = true;
        for (uint32_t j = with_r ? rlen : 0; j < len && ascii; ++j) ascii = (uint8_t)p->pool[off + j] < 0x80;
        if (!ascii && !cp) continue;
        if (with_r && len == rlen) { r_known = true; r_id = p->piece_id[i]; r_score = p->scores[i]; continue; }   // (repeated: the later one wins)
        ents.push_back({off, len, p->piece_id[i], with_r ? 1u : 0u, tok_hash_bytes(p->pool + off, len), i});
    }
    TokTable table;
    tok_build_table(p->pool, ents, table);
    std::vector<double> scores(table.ents.size());
    for (size_t j = 0; j < scores.size(); ++j) scores[j] = p->scores[table.winner[j]];
    std::unique_ptr<smt_unigram> tok(new smt_unigram(ctx));
    UgTable &T = tok->T;
    if ((rc = tok_added_first(p, T.added))) return rc;
    const uint8_t *at[10];
    std::vector<std::pair<const void *, size_t>> parts = {{table.slots.data(), table.slots.size() * 8},
                                                          {table.ents.data(), table.ents.size() * sizeof(uint4)},
                                                          {scores.data(), scores.size() * 8},
                                                          {p->pool, p->n_pieces ? p->piece_off[p->n_pieces] : 0},
                                                          {p->byte_map, 128},
                                                          {p->added_pool, p->n_added ? p->added_off[p->n_added] : 0},
                                                          {p->added_off, p->n_added ? ((size_t)p->n_added + 1) * 4 : 0}};
    if (cp) {
        parts.push_back({img.page.data(), img.page.size() * 2});
        parts.push_back({img.ent.data(), img.ent.size() * 4});
        parts.push_back({img.out.data(), img.out.size()});
    }
    if ((rc = tok_upload_table("unigram", parts, &tok->d_table, at))) return rc;
    tok->table_bytes = 0;
    for (size_t i = 0; i < 7; ++i) tok->table_bytes += parts[i].second;
    if (cp) {
        tok->utf8 = true;
        tok->codepoint_bytes = img.page.size() * 2 + img.ent.size() * 4 + img.out.size();
        tok->table_bytes += tok->codepoint_bytes;
        tok->U.page = reinterpret_cast<const uint16_t *>(at[7]);
        tok->U.ent = reinterpret_cast<const uint32_t *>(at[8]);
        tok->U.out = at[9];
        tok->U.n_pages = (uint32_t)(img.ent.size() / 256);
        tok->U.out_bytes = (uint32_t)img.out.size();
    }
    T.slots = reinterpret_cast<const unsigned long long *>(at[0]);
    T.ent = reinterpret_cast<const uint4 *>(at[1]);
    T.score = reinterpret_cast<const double *>(at[2]);
    T.pool = at[3];
    T.map = at[4];
    T.added.pool = at[5];
    T.added.off = reinterpret_cast<const uint32_t *>(at[6]);
    T.mask = table.mask;
    T.max_piece = max_piece;
    T.unk = p->unk_id < 0 ? TOK_NONE : (uint32_t)p->unk_id;
    T.rlen = rlen;
    T.prepend = p->prepend;
    T.r_unk = r_known ? 0u : 1u;
    T.r_id = r_known ? r_id : (p->unk_id < 0 ? 0u : (uint32_t)p->unk_id);
    T.r_score = r_known ? r_score : p->unk_score;
    T.unk_score = p->unk_score;
    T.r_state = r_state;
    *out = tok.release();
    return SMT_OK;
}

extern "C" {

int smt_unigram_create(smt_ctx *ctx, const smt_unigram_params *p, smt_unigram **out)
try {
    if (!ctx) return tok_null_handle("smt_unigram_create");
    return ug_create(ctx, p, nullptr, out);
} catch (...) { return smt::api_catch(); }

int smt_unigram_create_utf8(smt_ctx *ctx, const smt_unigram_params *p, const smt_wordpiece_codepoints *cp, smt_unigram **out)
try {
    if (!ctx) return tok_null_handle("smt_unigram_create_utf8");
    SMT_REQUIRE(cp != nullptr, "null argument");
    return ug_create(ctx, p, cp, out);
} catch (...) { return smt::api_catch(); }

int smt_unigram_info(const smt_unigram *tok, uint64_t *table_bytes, uint64_t *codepoint_bytes, int *utf8)
try {
    if (!tok) return tok_null_handle("smt_unigram_info");
    if (table_bytes) *table_bytes = tok->table_bytes;
    if (codepoint_bytes) *codepoint_bytes = tok->codepoint_bytes;
    if (utf8) *utf8 = tok->utf8 ? 1 : 0;
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

void smt_unigram_destroy(smt_unigram *tok) { tok_destroy(tok); }

int smt_unigram_scan_device(smt_unigram *tok, const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev,
                            const uint32_t *line_len_dev, uint64_t n_lines, uint32_t keep_bytes, uint32_t max_tokens, int drop_unk,
                            uint32_t *counts_dev, uint8_t *flags_dev, uint32_t *n_flagged_dev)
try {
    if (!tok) return tok_null_handle("smt_unigram_scan_device");
    return tok_scan_device(tok, text_dev, text_bytes, line_begin_dev, line_len_dev, n_lines, keep_bytes, max_tokens, drop_unk, counts_dev, flags_dev,
                           n_flagged_dev);
} catch (...) { return smt::api_catch(); }

int smt_unigram_emit_device(smt_unigram *tok, uint64_t n_lines, const uint64_t *patch_line_dev, const uint64_t *patch_off_dev,
                            const uint32_t *patch_ids_dev, uint64_t n_patch, uint64_t n_patch_ids, uint32_t *ids_out_dev, uint64_t ids_cap,
                            uint64_t *offsets_out_dev)
try {
    if (!tok) return tok_null_handle("smt_unigram_emit_device");
    return tok_emit_device(tok, n_lines, patch_line_dev, patch_off_dev, patch_ids_dev, n_patch, n_patch_ids, ids_out_dev, ids_cap, offsets_out_dev);
} catch (...) { return smt::api_catch(); }

int smt_unigram_tokenize(smt_unigram *tok, const char *text, const uint64_t *line_begin, const uint32_t *line_len, uint64_t n_lines,
                         uint32_t keep_bytes, uint32_t max_tokens, int drop_unk, uint32_t *ids_out, uint64_t ids_cap, uint64_t *offsets_out,
                         uint8_t *flags_out)
try {
    if (!tok) return tok_null_handle("smt_unigram_tokenize");
    return tok_tokenize(tok, text, line_begin, line_len, n_lines, keep_bytes, max_tokens, drop_unk, ids_out, ids_cap, offsets_out, flags_out);
} catch (...) { return smt::api_catch(); }

}  // extern "C"
