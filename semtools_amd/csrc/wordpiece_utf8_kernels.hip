// wordpiece_utf8_kernels.hip -- WordPiece over UTF-8 lines on the device (DESIGN.md 4.9 "WordPiece over UTF-8 lines"): pass 1 of the
// handle smt_wordpiece_create_utf8 makes.  The decomposition of wordpiece_kernels.hip -- one lane per text BYTE, the line by the
// block-narrowed binary search, one barrier, a word's tokens in ids_tmp[word's first byte + j] -- with the rules stated on CHARACTERS:
//
//   * a lane at a continuation byte only checks that a lead byte in front of it covers it, and leaves;
//   * a lane at a lead byte decodes its character STRICTLY (a sequence cut by the line's end, an overlong form, a surrogate, a value
//     above U+10FFFF, a byte that can lead nothing: the line is flagged) and looks it up: ASCII in the 128-entry tables in LDS, the rest
//     in the two-level table of wordpiece_table.h -- class, and what the character becomes (nothing, itself, or up to 16 bytes of a pool);
//   * a word starts at an ALONE character, and at an ORDINARY one whose nearest earlier not-dropped character is not ORDINARY;
//   * the normalised bytes of a word are read through a cursor (raw position of a character, byte within its output): a character may
//     become several, and a piece may end between them.  Candidates end at character boundaries of the normalised stream only.
//
// The character, the cursor and the lane prologue are utf8_cursor.h's, shared with the Unigram form (unigram_utf8_kernels.hip).
//
// Bounds: every decode is handed the end it may read to and checks it before the read; page and pool indices are checked against the
// table's sizes; a token slot never leaves [p, we) of its word.  Every loop is bounded: probes by the table's capacity, a word's pieces
// by its characters, a walk by the line's end (each step moves at least one byte).
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "tokenize_frame.h"
#include "utf8_cursor.h"
#include "wordpiece_bytes.h"
#include "wordpiece_table.h"

namespace {

constexpr uint32_t WP_NONE = smt::TOK_NONE;
constexpr unsigned SCAN_THREADS = 256;
using smt::WpChar;
using smt::WpCodepoints;
using smt::WpTable;
using smt::wp_byte;
using smt::wp_char_at;
using smt::wp_next_char;
using smt::wp_scan_lane_utf8;

// the candidate: clen normalised bytes from the cursor (s, sk) -- sc is the character at s --, hash h, as a whole word (kind 0) or a
// continuing piece
__device__ __forceinline__ uint32_t wp_probe_utf8(const WpTable &T, const WpCodepoints &U, const uint8_t *__restrict__ text, const uint8_t *cls,
                                                  const uint8_t *nrm, unsigned long long h, uint32_t kind, uint64_t s, uint32_t sk, const WpChar &sc,
                                                  uint64_t we, uint32_t clen)
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
                uint32_t k = sk, j = 0;
                WpChar qc = sc;
                bool same = true;
                while (j < clen) {   // (the candidate was walked once already: it has clen bytes before the word's end)
                    if (q >= we || wp_byte(U, text, q, qc, k) != piece[j]) { same = false; break; }
                    ++j;
                    if (++k >= qc.n) { q += qc.src; k = 0; wp_next_char(U, cls, nrm, text, q, we, qc); }
                }
                if (same) return e.z;
            }
        }
        idx = (idx + 1) & T.mask;
    }
    return WP_NONE;
}

__global__ void __launch_bounds__(SCAN_THREADS) wp_scan_utf8_kernel(WpTable T, WpCodepoints U, const uint8_t *__restrict__ text, uint64_t text_bytes,
                                                                    const uint64_t *__restrict__ line_begin, const uint32_t *__restrict__ line_len,
                                                                    uint64_t n_lines, uint32_t keep_bytes, int drop_unk, uint32_t *__restrict__ ids_tmp,
                                                                    uint32_t *__restrict__ raw_count, uint8_t *__restrict__ flags)
{
    __shared__ uint8_t s_bytes[256];
    __shared__ uint64_t s_win[2];
    s_bytes[threadIdx.x] = T.bytes[threadIdx.x];
    uint64_t line, lb, le;
    uint8_t c;
    if (!wp_scan_lane_utf8(T.added, SCAN_THREADS, s_win, text, text_bytes, line_begin, line_len, n_lines, keep_bytes, flags, line, lb, le, c)) return;
    const uint8_t *cls = s_bytes, *nrm = s_bytes + 128;
    const uint64_t p = (uint64_t)blockIdx.x * SCAN_THREADS + threadIdx.x;
    WpChar me;
    wp_char_at(U, cls, nrm, text, p, le, me);
    if (me.cls == smt::WP_FLAG) { flags[line] = 1; return; }   // a FLAG code point, or malformed UTF-8
    if (me.cls == smt::WP_SPACE || me.cls == smt::WP_DROPPED) return;
    uint64_t we = p + me.src;        // the raw end of the word
    uint32_t n_chars = me.chars;     // its normalised characters
    if (me.cls == smt::WP_ORDINARY) {
        // a word starts here unless the nearest earlier character that is not dropped is a word's character too
        for (uint64_t q = p; q > lb;) {
            uint64_t r = q - 1;
            for (uint32_t back = 0; back < 3 && r > lb && (text[r] & 0xC0) == 0x80; ++back) --r;   // the start of the character that ends at q
            WpChar pc;
            wp_char_at(U, cls, nrm, text, r, q, pc);
            if (pc.cls == smt::WP_FLAG || r + pc.src != q) return;   // (flagged by the lanes that stand there: nothing of the line is used)
            q = r;
            if (pc.cls == smt::WP_DROPPED) continue;
            if (pc.cls == smt::WP_ORDINARY) return;
            break;
        }
        // ... and runs to the next white space, ALONE character or the line's end; only max_chars + 1 characters matter
        while (we < le) {
            WpChar nc;
            wp_char_at(U, cls, nrm, text, we, le, nc);
            if (nc.cls == smt::WP_FLAG) return;
            if (nc.cls == smt::WP_DROPPED) { we += nc.src; continue; }
            if (nc.cls != smt::WP_ORDINARY) break;
            we += nc.src;
            n_chars += nc.chars;
            if (n_chars > T.max_chars) break;
        }
    }
    uint32_t n_tok = 0;
    bool bad = n_chars > T.max_chars;
    uint64_t s = p;          // the cursor: byte sk of what the character at s (sc) becomes
    uint32_t sk = 0;
    WpChar sc = me;
    for (uint32_t piece = 0; !bad && piece < n_chars; ++piece) {
        if (s >= we) break;
        const uint32_t kind = n_tok ? 1u : 0u;
        unsigned long long h = kind ? T.prefix_state : smt::TOK_HASH_SEED;
        const uint32_t longest = kind ? T.max_piece - T.prefix_len : T.max_piece;
        uint32_t hit = WP_NONE, clen = 0, hit_k = sk, k = sk;
        uint64_t hit_end = s, q = s;
        WpChar qc = sc;
        while (q < we) {
            const uint32_t b = wp_byte(U, text, q, qc, k);
            if (clen && (b & 0xC0u) != 0x80u) {   // a character boundary of the normalised stream: a candidate ends here
                const uint32_t id = wp_probe_utf8(T, U, text, cls, nrm, h, kind, s, sk, sc, we, clen);
                if (id != WP_NONE) { hit = id; hit_end = q; hit_k = k; }
            }
            if (clen >= longest) break;
            h = (h ^ b) * smt::TOK_HASH_MUL;
            ++clen;
            if (++k >= qc.n) { q += qc.src; k = 0; wp_next_char(U, cls, nrm, text, q, we, qc); }
        }
        if (q >= we && clen) {   // ... and at the word's end
            const uint32_t id = wp_probe_utf8(T, U, text, cls, nrm, h, kind, s, sk, sc, we, clen);
            if (id != WP_NONE) { hit = id; hit_end = we; hit_k = 0; }
        }
        if (hit == WP_NONE || p + n_tok >= we) { bad = true; break; }
        ids_tmp[p + n_tok++] = hit;              // n_tok < n_chars <= we - p (an output has no more characters than its source has bytes)
        s = hit_end;
        sk = hit_k;
        if (s < we) wp_char_at(U, cls, nrm, text, s, we, sc);
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

// strict UTF-8 of [b, b + n): the number of characters, or -1
int utf8_chars(const uint8_t *b, uint32_t n)
{
    int chars = 0;
    for (uint32_t i = 0; i < n;) {
        const uint32_t b0 = b[i];
        uint32_t len, cp;
        if (b0 < 0x80) { len = 1; cp = b0; }
        else if (b0 >= 0xC2 && b0 <= 0xDF) { len = 2; cp = b0 & 0x1Fu; }
        else if ((b0 & 0xF0u) == 0xE0u) { len = 3; cp = b0 & 0x0Fu; }
        else if (b0 >= 0xF0 && b0 <= 0xF4) { len = 4; cp = b0 & 0x07u; }
        else return -1;
        if (i + len > n) return -1;
        for (uint32_t k = 1; k < len; ++k) {
            if ((b[i + k] & 0xC0u) != 0x80u) return -1;
            cp = (cp << 6) | (b[i + k] & 0x3Fu);
        }
        if (len == 3 && (cp < 0x800u || (cp >= 0xD800u && cp <= 0xDFFFu))) return -1;
        if (len == 4 && (cp < 0x10000u || cp > 0x10FFFFu)) return -1;
        i += len;
        ++chars;
    }
    return chars;
}

}  // namespace

namespace smt {

int wp_codepoint_image(const smt_wordpiece_codepoints *cp, WpCodepointImage &img)
{
    SMT_REQUIRE(cp->n < 0x110000ull, "too many code point ranges");
    SMT_REQUIRE(cp->n == 0 || (cp->first && cp->last && cp->cls && cp->out_off), "code point arrays");
    SMT_REQUIRE(cp->n == 0 || cp->out_off[cp->n] == 0 || cp->out_pool != nullptr, "out_pool");
    SMT_REQUIRE(cp->n == 0 || cp->out_off[cp->n] <= WP_CP_MAX_POOL, "the outputs hold more than 2 MiB");
    // the offsets as a whole first: no byte of out_pool is read before every output is known to lie inside [0, out_off[n])
    for (uint64_t i = 0; i < cp->n; ++i) SMT_REQUIRE(cp->out_off[i] <= cp->out_off[i + 1], "out_off must be non-decreasing");
    std::vector<uint32_t> flat(0x110000u, (uint32_t)WP_FLAG);
    for (uint64_t i = 0; i < cp->n; ++i) {
        const uint32_t a = cp->first[i], b = cp->last[i], k = cp->cls[i];
        SMT_REQUIRE(a >= 0x80u && a <= b && b <= 0x10FFFFu, "a code point range must lie in U+0080 .. U+10FFFF, first <= last");
        SMT_REQUIRE(i == 0 || a > cp->last[i - 1], "the code point ranges must be sorted and disjoint");
        SMT_REQUIRE(k <= SMT_WP_CP_FLAG, "unknown code point class");
        const uint32_t off = cp->out_off[i], len = cp->out_off[i + 1] - off;
        uint32_t e = k;
        if (len) {
            SMT_REQUIRE(k != SMT_WP_CP_DROPPED && k != SMT_WP_CP_FLAG, "a DROPPED or FLAG range has no output");
            SMT_REQUIRE(a == b, "a range with an explicit output is a single code point");
            SMT_REQUIRE(len <= WP_CP_MAX_OUT, "an output is longer than 16 bytes");
            const int chars = utf8_chars(reinterpret_cast<const uint8_t *>(cp->out_pool) + off, len);
            SMT_REQUIRE(chars > 0, "an output is not valid UTF-8");
            const uint32_t src = a < 0x800u ? 2u : a < 0x10000u ? 3u : 4u;
            SMT_REQUIRE((uint32_t)chars <= src, "an output holds more characters than its code point has bytes");
            SMT_REQUIRE(chars == 1 || k == SMT_WP_CP_ORDINARY, "a SPACE or ALONE output is one character");
            e |= (uint32_t)chars << 3 | len << 6 | off << 11;
        }
        for (uint32_t c = a; c <= b; ++c) flat[c] = e;
    }
    img.page.assign(WP_CP_PAGES, 0);
    img.ent.clear();
    std::unordered_map<std::string, uint16_t> seen;   // pages of equal content are stored once
    for (uint32_t pg = 0; pg < WP_CP_PAGES; ++pg) {
        const std::string key(reinterpret_cast<const char *>(flat.data() + (size_t)pg * 256), 1024);
        auto it = seen.find(key);
        if (it == seen.end()) {
            it = seen.emplace(key, (uint16_t)(img.ent.size() / 256)).first;
            img.ent.insert(img.ent.end(), flat.begin() + (size_t)pg * 256, flat.begin() + (size_t)(pg + 1) * 256);
        }
        img.page[pg] = it->second;
    }
    img.out.clear();
    if (cp->n && cp->out_off[cp->n]) img.out.assign(cp->out_pool, cp->out_pool + cp->out_off[cp->n]);
    return SMT_OK;
}

int wp_scan_utf8_launch(smt_wordpiece *tok, const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev,
                        const uint32_t *line_len_dev, uint64_t n_lines, uint32_t keep_bytes, int drop_unk, uint8_t *flags_dev)
{
    hipLaunchKernelGGL(wp_scan_utf8_kernel, dim3((unsigned)((text_bytes + SCAN_THREADS - 1) / SCAN_THREADS)), dim3(SCAN_THREADS), 0, tok->ctx->stream,
                       tok->T, tok->U, text_dev, text_bytes, line_begin_dev, line_len_dev, n_lines, keep_bytes, drop_unk, tok->S.d_ids_tmp,
                       tok->S.raw_count(), flags_dev);
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

}  // namespace smt
