// wordpiece_kernels.hip -- WordPiece over pure-ASCII lines on the device: the byte rules of hf_tokenizer.cpp's
// encode_ascii (wordpiece_bytes.h states them as a table), the same ids, as the CSR K1 reads.
//
// The work is dealt by TEXT POSITION, not by line (line lengths are heavy-tailed).  Pass 1, one lane per byte: the lane classifies
// its byte, finds its line (a binary search over the line starts, narrowed per block to the lines the block touches), flags the
// line for a byte >= 0x80 or an added token standing there, and decides whether a word STARTS at its byte -- a punctuation byte
// always, an ordinary byte when the nearest earlier byte of its line that clean_text does not drop is no ordinary byte.  The lane
// at a word start matches the whole word: greedy longest match in ONE forward walk per piece (the hash is carried byte by byte and
// the LAST hit while the end walks forward is the longest matching prefix), against an open-addressing table built on the host
// (load <= 0.5, a 32-bit hash tag per 8-byte slot: a miss is one read).  A word's tokens go to ids_tmp[word start + j]: a token is
// at least one byte, so the slots of a word lie inside the word's own bytes, no two words share one, and TOKEN ORDER == SLOT
// ORDER.  Pass 2 (tokenize_frame.h) is then a prefix sum over the slots: rank of a slot among the used slots minus the rank at its
// line's start is the token's place in its line; lines are laid out by a prefix sum of their (capped, or patched) counts.
//
// Every loop is bounded: probes by the table's capacity, a word's pieces by max_input_chars_per_word, a walk by the line's end.
//
// Also here: the create of both forms of the handle.  The UTF-8 form's pass 1 is wordpiece_utf8_kernels.hip; the table and the handle
// the two share are in wordpiece_table.h.
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "common.h"
#include "tokenize_frame.h"
#include "wordpiece_bytes.h"
#include "wordpiece_table.h"

namespace {

constexpr uint32_t WP_NONE = smt::TOK_NONE;   // an ids_tmp slot that holds no token
constexpr unsigned SCAN_THREADS = 256;        // pass 1: one position per thread

using smt::WpTable;   // (wordpiece_table.h: shared with the UTF-8 form)

// the candidate: clen characters from raw position s (dropped bytes skipped), hash h, as a whole word (kind 0) or a continuing piece
__device__ __forceinline__ uint32_t wp_probe(const WpTable &T, const uint8_t *__restrict__ text, const uint8_t *cls, const uint8_t *nrm,
                                             unsigned long long h, uint32_t kind, uint64_t s, uint32_t clen)
{
    uint32_t idx = (uint32_t)h & T.mask;
    const uint32_t tag = (uint32_t)(h >> 32);
    for (uint32_t probe = 0; probe <= T.mask; ++probe) {
        const unsigned long long slot = T.slots[idx];
        if (slot == 0) return WP_NONE;
        if ((uint32_t)(slot >> 32) == tag) {
            const uint4 e = T.ent[(uint32_t)slot - 1];
            const uint32_t skip = kind ? T.prefix_len : 0;
            if (e.w == kind && e.y - skip == clen) {
                const uint8_t *piece = T.pool + e.x + skip;
                uint64_t q = s;
                uint32_t j = 0;
                bool same = true;
                while (j < clen) {   // (the candidate was walked once already: it has clen characters before the word's end)
                    const uint8_t c = text[q++];
                    if (cls[c] == smt::WP_DROPPED) continue;
                    if (nrm[c] != piece[j]) { same = false; break; }
                    ++j;
                }
                if (same) return e.z;
            }
        }
        idx = (idx + 1) & T.mask;
    }
    return WP_NONE;
}

__global__ void __launch_bounds__(SCAN_THREADS) wp_scan_kernel(WpTable T, const uint8_t *__restrict__ text, uint64_t text_bytes,
                                                               const uint64_t *__restrict__ line_begin, const uint32_t *__restrict__ line_len,
                                                               uint64_t n_lines, uint32_t keep_bytes, int drop_unk, uint32_t *__restrict__ ids_tmp,
                                                               uint32_t *__restrict__ raw_count, uint8_t *__restrict__ flags)
{
    __shared__ uint8_t s_bytes[256];
    __shared__ uint64_t s_win[2];
    s_bytes[threadIdx.x] = T.bytes[threadIdx.x];
    uint64_t line, lb, le;
    uint8_t c;
    if (!smt::tok_scan_lane(T.added, SCAN_THREADS, s_win, text, text_bytes, line_begin, line_len, n_lines, keep_bytes, flags, line, lb, le, c)) return;
    const uint8_t *cls = s_bytes, *nrm = s_bytes + 128;
    const uint64_t p = (uint64_t)blockIdx.x * SCAN_THREADS + threadIdx.x;
    const uint8_t k = cls[c];
    if (k == smt::WP_SPACE || k == smt::WP_DROPPED) return;
    uint64_t we = p + 1;      // the raw end of the word
    uint32_t n_chars = 1;
    if (k == smt::WP_ORDINARY) {
        // a word starts here unless the nearest earlier byte that is not dropped is a word's byte too
        for (uint64_t q = p; q > lb;) {
            const uint8_t b = text[--q];
            if (b >= 0x80) return;               // (the line is flagged by that byte's lane: nothing of it is used)
            const uint8_t kb = cls[b];
            if (kb == smt::WP_DROPPED) continue;
            if (kb == smt::WP_ORDINARY) return;
            break;
        }
        // ... and runs to the next white space, punctuation byte or the line's end; only max_chars + 1 characters matter
        for (; we < le; ++we) {
            const uint8_t b = text[we];
            if (b >= 0x80) return;
            const uint8_t kb = cls[b];
            if (kb == smt::WP_DROPPED) continue;
            if (kb != smt::WP_ORDINARY) break;
            if (++n_chars > T.max_chars) break;
        }
    }
    uint32_t n_tok = 0;
    bool bad = n_chars > T.max_chars;
    uint64_t s = p;
    for (uint32_t piece = 0; !bad && piece < n_chars; ++piece) {
        while (s < we && cls[text[s]] == smt::WP_DROPPED) ++s;
        if (s >= we) break;
        const uint32_t kind = n_tok ? 1u : 0u;
        unsigned long long h = kind ? T.prefix_state : smt::TOK_HASH_SEED;
        const uint32_t longest = kind ? T.max_piece - T.prefix_len : T.max_piece;
        uint32_t hit = WP_NONE, clen = 0;
        uint64_t hit_end = s;
        for (uint64_t q = s; q < we && clen < longest;) {
            const uint8_t b = text[q++];
            if (cls[b] == smt::WP_DROPPED) continue;
            h = (h ^ nrm[b]) * smt::TOK_HASH_MUL;
            ++clen;
            const uint32_t id = wp_probe(T, text, cls, nrm, h, kind, s, clen);
            if (id != WP_NONE) { hit = id; hit_end = q; }
        }
        if (hit == WP_NONE) { bad = true; break; }
        ids_tmp[p + n_tok++] = hit;              // n_tok < n_chars <= we - p: inside the word's own bytes
        s = hit_end;
    }
    if (bad) {   // too long, or an unmatched tail: the pieces found are taken back, the word is ONE unk
        for (uint32_t j = 0; j < n_tok; ++j) ids_tmp[p + j] = WP_NONE;
        n_tok = 0;
        if (!drop_unk && T.unk != WP_NONE) { ids_tmp[p] = T.unk; n_tok = 1; }
    } else if (drop_unk && T.unk != WP_NONE) {   // a vocabulary may hold the unk token's text as a piece: dropped like any unk id
        uint32_t kept = 0;
        for (uint32_t j = 0; j < n_tok; ++j) {
            const uint32_t id = ids_tmp[p + j];
            ids_tmp[p + j] = WP_NONE;
            if (id != T.unk) ids_tmp[p + kept++] = id;
        }
        n_tok = kept;
    }
    if (n_tok) atomicAdd(&raw_count[line], n_tok);
}

constexpr smt::TokWords WP_WORDS = {"no scan to emit (smt_wordpiece_scan_device comes first)",
                                    "ids_cap is below the looked-at bytes of all lines + the patch ids",
                                    "ids_cap is below the looked-at bytes of all lines (ids_cap >= looked)"};

}  // namespace

int smt_wordpiece::pass1(const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev, const uint32_t *line_len_dev, uint64_t n_lines,
                         uint32_t keep_bytes, int drop_unk, uint8_t *flags_dev)
{
    if (!n_lines || !text_bytes) return SMT_OK;
    if (utf8) return smt::wp_scan_utf8_launch(this, text_dev, text_bytes, line_begin_dev, line_len_dev, n_lines, keep_bytes, drop_unk, flags_dev);
    hipLaunchKernelGGL(wp_scan_kernel, dim3((unsigned)((text_bytes + SCAN_THREADS - 1) / SCAN_THREADS)), dim3(SCAN_THREADS), 0, ctx->stream, T,
                       text_dev, text_bytes, line_begin_dev, line_len_dev, n_lines, keep_bytes, drop_unk, S.d_ids_tmp, S.raw_count(), flags_dev);
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

using namespace smt;

TokHandle *smt::tok_handle(smt_wordpiece *tok) { return tok; }

// the body of both creates.  cp == nullptr: the ASCII form (a byte >= 0x80 flags its line, pieces with such a byte cannot match and
// are left out); otherwise the UTF-8 form: all pieces enter, the code points come from *cp
static int wp_create(smt_ctx *ctx, const smt_wordpiece_params *p, const smt_wordpiece_codepoints *cp, smt_wordpiece **out)
{
    SMT_REQUIRE(p != nullptr && out != nullptr, "null argument");
    *out = nullptr;
    SMT_REQUIRE(p->n_pieces == 0 || (p->pool && p->piece_off && p->piece_id), "vocabulary arrays");
    SMT_REQUIRE(p->n_pieces < 0x7FFFFFFFull, "too many pieces");
    SMT_REQUIRE(p->prefix_len == 0 || p->prefix != nullptr, "prefix");
    SMT_REQUIRE(p->unk_id >= -1 && p->unk_id < 0xFFFFFFFFll, "unk_id");
    SMT_REQUIRE(p->n_added == 0 || (p->added_pool && p->added_off), "added tokens");
    SMT_REQUIRE((p->flags & ~(SMT_WP_NORMALIZER | SMT_WP_CLEAN_TEXT | SMT_WP_LOWERCASE)) == 0, "unknown flag");
    for (uint64_t i = 0; i < p->n_pieces; ++i) SMT_REQUIRE(p->piece_off[i] <= p->piece_off[i + 1], "piece_off must be non-decreasing");
    for (uint32_t i = 0; i < p->n_added; ++i) SMT_REQUIRE(p->added_off[i] <= p->added_off[i + 1], "added_off must be non-decreasing");
    for (uint32_t i = 0; i < p->prefix_len; ++i) SMT_REQUIRE((uint8_t)p->prefix[i] < 0x80, "the continuing prefix must be ASCII");
    WpCodepointImage img;
    int rc = cp ? wp_codepoint_image(cp, img) : SMT_OK;   // (validated before anything is uploaded)
    if (rc) return rc;
    if ((rc = bind_device(ctx))) return rc;

    // ---- entries: every piece (the ASCII form: every ASCII piece) as a whole word; one that starts with the prefix and goes on, as a
    // continuing piece too
    std::vector<TokEntry> ents;
    ents.reserve(p->n_pieces * 2);
    uint32_t max_piece = 0;
    for (uint64_t i = 0; i < p->n_pieces; ++i) {
        const uint32_t off = p->piece_off[i], len = p->piece_off[i + 1] - off;
        if (len == 0) continue;
        bool ascii = true;
        for (uint32_t j = 0; j < len && ascii; ++j) ascii = (uint8_t)p->pool[off + j] < 0x80;
        if (!ascii && !cp) continue;
        const uint64_t h = tok_hash_bytes(p->pool + off, len);
        max_piece = std::max(max_piece, len);
        ents.push_back({off, len, p->piece_id[i], 0, h, i});
        if (len > p->prefix_len && memcmp(p->pool + off, p->prefix, p->prefix_len) == 0) ents.push_back({off, len, p->piece_id[i], 1, h, i});
    }
    TokTable table;
    tok_build_table(p->pool, ents, table);
    uint8_t bytes[256];
    wordpiece_byte_table(p->flags, bytes, bytes + 128);
    std::unique_ptr<smt_wordpiece> tok(new smt_wordpiece(ctx, WP_WORDS));
    WpTable &T = tok->T;
    if ((rc = tok_added_first(p, T.added))) return rc;
    const uint8_t *at[9];
    if ((rc = tok_upload_table("wordpiece",
                               {{table.slots.data(), table.slots.size() * 8},
                                {table.ents.data(), table.ents.size() * sizeof(uint4)},
                                {p->pool, p->n_pieces ? p->piece_off[p->n_pieces] : 0},
                                {bytes, 256},
                                {p->added_pool, p->n_added ? p->added_off[p->n_added] : 0},
                                {p->added_off, p->n_added ? ((size_t)p->n_added + 1) * 4 : 0},
                                {img.page.data(), img.page.size() * 2},
                                {img.ent.data(), img.ent.size() * 4},
                                {img.out.data(), img.out.size()}},
                               &tok->d_table, at)))
        return rc;
    T.slots = reinterpret_cast<const unsigned long long *>(at[0]);
    T.ent = reinterpret_cast<const uint4 *>(at[1]);
    T.pool = at[2];
    T.bytes = at[3];
    T.added.pool = at[4];
    T.added.off = reinterpret_cast<const uint32_t *>(at[5]);
    T.mask = table.mask;
    T.prefix_len = p->prefix_len;
    T.max_piece = std::max(max_piece, p->prefix_len);   // (max_piece - prefix_len must not wrap)
    T.max_chars = p->max_input_chars_per_word;
    T.unk = p->unk_id < 0 ? WP_NONE : (uint32_t)p->unk_id;
    T.prefix_state = tok_hash_bytes(p->prefix, p->prefix_len);
    tok->table_bytes = table.slots.size() * 8 + table.ents.size() * sizeof(uint4) + (p->n_pieces ? p->piece_off[p->n_pieces] : 0) + 256 +
                       (p->n_added ? p->added_off[p->n_added] + ((size_t)p->n_added + 1) * 4 : 0);
    if (cp) {
        tok->utf8 = true;
        tok->codepoint_bytes = img.page.size() * 2 + img.ent.size() * 4 + img.out.size();
        tok->table_bytes += tok->codepoint_bytes;
        tok->U.page = reinterpret_cast<const uint16_t *>(at[6]);
        tok->U.ent = reinterpret_cast<const uint32_t *>(at[7]);
        tok->U.out = at[8];
        tok->U.n_pages = (uint32_t)(img.ent.size() / 256);
        tok->U.out_bytes = (uint32_t)img.out.size();
    }
    *out = tok.release();
    return SMT_OK;
}

extern "C" {

int smt_wordpiece_create(smt_ctx *ctx, const smt_wordpiece_params *p, smt_wordpiece **out)
try {
    if (!ctx) return tok_null_handle("smt_wordpiece_create");
    return wp_create(ctx, p, nullptr, out);
} catch (...) { return smt::api_catch(); }

int smt_wordpiece_create_utf8(smt_ctx *ctx, const smt_wordpiece_params *p, const smt_wordpiece_codepoints *cp, smt_wordpiece **out)
try {
    if (!ctx) return tok_null_handle("smt_wordpiece_create_utf8");
    SMT_REQUIRE(cp != nullptr, "null argument");
    return wp_create(ctx, p, cp, out);
} catch (...) { return smt::api_catch(); }

int smt_wordpiece_info(const smt_wordpiece *tok, uint64_t *table_bytes, uint64_t *codepoint_bytes, int *utf8)
try {
    if (!tok) return tok_null_handle("smt_wordpiece_info");
    if (table_bytes) *table_bytes = tok->table_bytes;
    if (codepoint_bytes) *codepoint_bytes = tok->codepoint_bytes;
    if (utf8) *utf8 = tok->utf8 ? 1 : 0;
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

void smt_wordpiece_destroy(smt_wordpiece *tok) { tok_destroy(tok); }

int smt_wordpiece_scan_device(smt_wordpiece *tok, const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev,
                              const uint32_t *line_len_dev, uint64_t n_lines, uint32_t keep_bytes, uint32_t max_tokens, int drop_unk,
                              uint32_t *counts_dev, uint8_t *flags_dev, uint32_t *n_flagged_dev)
try {
    if (!tok) return tok_null_handle("smt_wordpiece_scan_device");
    return tok_scan_device(tok, text_dev, text_bytes, line_begin_dev, line_len_dev, n_lines, keep_bytes, max_tokens, drop_unk, counts_dev, flags_dev,
                           n_flagged_dev);
} catch (...) { return smt::api_catch(); }

int smt_wordpiece_emit_device(smt_wordpiece *tok, uint64_t n_lines, const uint64_t *patch_line_dev, const uint64_t *patch_off_dev,
                              const uint32_t *patch_ids_dev, uint64_t n_patch, uint64_t n_patch_ids, uint32_t *ids_out_dev, uint64_t ids_cap,
                              uint64_t *offsets_out_dev)
try {
    if (!tok) return tok_null_handle("smt_wordpiece_emit_device");
    return tok_emit_device(tok, n_lines, patch_line_dev, patch_off_dev, patch_ids_dev, n_patch, n_patch_ids, ids_out_dev, ids_cap, offsets_out_dev);
} catch (...) { return smt::api_catch(); }

int smt_wordpiece_tokenize(smt_wordpiece *tok, const char *text, const uint64_t *line_begin, const uint32_t *line_len, uint64_t n_lines,
                           uint32_t keep_bytes, uint32_t max_tokens, int drop_unk, uint32_t *ids_out, uint64_t ids_cap,
                           uint64_t *offsets_out, uint8_t *flags_out)
try {
    if (!tok) return tok_null_handle("smt_wordpiece_tokenize");
    return tok_tokenize(tok, text, line_begin, line_len, n_lines, keep_bytes, max_tokens, drop_unk, ids_out, ids_cap, offsets_out, flags_out);
} catch (...) { return smt::api_catch(); }

}  // extern "C"
