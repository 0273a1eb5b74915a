// precompiled.h -- the `Precompiled` normalizer of tokenizer.json files converted from sentencepiece models (XLM-R and its
// descendants: the `nmt_nfkc` rules), restated from what the `tokenizers` crate does with it (its spm_precompiled dependency):
//
//   * the blob (base64 in the file): a u32 LE trie size in bytes, that many bytes of u32 LE darts-clone double-array units, then a
//     pool of NUL-terminated normalised strings; a leaf's value is an offset into the pool;
//   * the text is cut into extended grapheme clusters (UAX #29, the tables of grapheme_break.h); a cluster SHORTER THAN 6 BYTES is
//     looked up whole by a common-prefix search and the FIRST (shortest) hit replaces the whole cluster; otherwise, or on a miss,
//     each of its characters is looked up on its own the same way, and a miss keeps the character.
//
// The blob is untrusted: every size and offset read from it is checked before use, and a malformed one is an Error -- at load (the
// header, the pool's last NUL) or at the lookup that meets it (a node outside the trie, a value outside the pool).
// Header-only, so that a stand-alone program can feed it bytes (tools/sanitize/precompiled_main.cpp, for a sanitizer build on the CPU).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "grapheme_break.h"
#include "host.h"

namespace semtools {

inline std::string base64_decode(const std::string &in)
{
    std::string out;
    out.reserve(in.size() / 4 * 3);
    uint32_t acc = 0, bits = 0;
    for (const char ch : in) {
        uint32_t v;
        if (ch >= 'A' && ch <= 'Z') v = (uint32_t)(ch - 'A');
        else if (ch >= 'a' && ch <= 'z') v = (uint32_t)(ch - 'a') + 26;
        else if (ch >= '0' && ch <= '9') v = (uint32_t)(ch - '0') + 52;
        else if (ch == '+' || ch == '-') v = 62;
        else if (ch == '/' || ch == '_') v = 63;
        else if (ch == '=' || ch == '\n' || ch == '\r') continue;
        else throw Error("tokenizer.json: precompiled_charsmap is not base64");
        acc = (acc << 6) | v;
        bits += 6;
        if (bits >= 8) { bits -= 8; out.push_back((char)((acc >> bits) & 0xFFu)); }
    }
    return out;
}

namespace grapheme {

inline uint32_t run_value(const unicode::BreakRun *r, size_t n, uint32_t cp)
{
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        if (cp > r[mid].last) lo = mid + 1;
        else if (cp < r[mid].first) hi = mid;
        else return r[mid].value;
    }
    return 0;
}
#define SMT_BREAK_VALUE(table, cp) run_value(unicode::table, sizeof(unicode::table) / sizeof(unicode::table[0]), cp)
inline uint32_t gcb(uint32_t cp) { return cp < 0x300 && cp >= 0x20 && cp != 0x7F && cp != 0xAD && !(cp >= 0x80 && cp < 0xA0) ? 0u : SMT_BREAK_VALUE(GCB_RUNS, cp); }
inline bool ext_pict(uint32_t cp) { return cp >= 0xA9 && SMT_BREAK_VALUE(EXT_PICT_RUNS, cp) != 0; }
inline uint32_t incb(uint32_t cp) { return cp < 0x300 ? 0u : SMT_BREAK_VALUE(INCB_RUNS, cp); }
#undef SMT_BREAK_VALUE

// the end of the extended grapheme cluster of `s` that starts at `b` (rules GB3 .. GB13, GB999)
inline size_t cluster_end(const std::u32string &s, size_t b)
{
    using namespace unicode;
    size_t i = b + 1;
    uint32_t prev = gcb(s[b]);
    // what the rules that look further back than one character need: GB11 (an Extended_Pictographic, then Extend*), GB9c (a
    // Consonant, then InCB Extend / Linker with at least one Linker), GB12/13 (the Regional_Indicators in front, counted)
    int pict = ext_pict(s[b]) ? 1 : 0;   // 1: an Extended_Pictographic and Extend* stand in front, 2: and then one ZWJ
    bool conjunct = incb(s[b]) == INCB_CONSONANT, linker = false;
    uint32_t n_ri = prev == GCB_REGIONAL_INDICATOR ? 1 : 0;
    for (; i < s.size(); ++i) {
        const uint32_t cp = s[i], cur = gcb(cp);
        bool join;
        if (prev == GCB_CR) join = cur == GCB_LF;                                                        // GB3, GB4
        else if (prev == GCB_CONTROL || prev == GCB_LF) join = false;                                    // GB4
        else if (cur == GCB_CONTROL || cur == GCB_CR || cur == GCB_LF) join = false;                     // GB5
        else if (prev == GCB_L && (cur == GCB_L || cur == GCB_V || cur == GCB_LV || cur == GCB_LVT)) join = true;   // GB6
        else if ((prev == GCB_LV || prev == GCB_V) && (cur == GCB_V || cur == GCB_T)) join = true;       // GB7
        else if ((prev == GCB_LVT || prev == GCB_T) && cur == GCB_T) join = true;                        // GB8
        else if (cur == GCB_EXTEND || cur == GCB_ZWJ || cur == GCB_SPACINGMARK) join = true;             // GB9, GB9a
        else if (prev == GCB_PREPEND) join = true;                                                       // GB9b
        else if (conjunct && linker && incb(cp) == INCB_CONSONANT) join = true;                          // GB9c
        else if (pict == 2 && ext_pict(cp)) join = true;                                                   // GB11
        else if (prev == GCB_REGIONAL_INDICATOR && cur == GCB_REGIONAL_INDICATOR) join = n_ri % 2 == 1;  // GB12, GB13
        else join = false;                                                                               // GB999
        if (!join) break;
        const uint32_t ic = incb(cp);
        if (ic == INCB_CONSONANT) { conjunct = true; linker = false; }
        else if (ic == INCB_LINKER) linker = conjunct;
        else if (ic != INCB_EXTEND) conjunct = linker = false;
        pict = ext_pict(cp) ? 1 : pict == 1 && cur == GCB_EXTEND ? 1 : pict == 1 && cur == GCB_ZWJ ? 2 : 0;
        n_ri = cur == GCB_REGIONAL_INDICATOR ? n_ri + 1 : 0;
        prev = cur;
    }
    return i;
}

}  // namespace grapheme

class PrecompiledMap {
public:
    PrecompiledMap() = default;
    explicit PrecompiledMap(const std::string &blob)
    {
        if (blob.size() < 4) throw Error("Precompiled normalizer: the character map is shorter than its 4-byte header");
        const uint64_t trie_size = u32_at(blob, 0);
        if (trie_size % 4 != 0) throw Error("Precompiled normalizer: the trie size is not a multiple of 4");
        if (trie_size > blob.size() - 4) throw Error("Precompiled normalizer: the trie size passes the end of the character map");
        units_.resize(trie_size / 4);
        for (size_t i = 0; i < units_.size(); ++i) units_[i] = u32_at(blob, 4 + 4 * i);
        pool_.assign(blob, 4 + trie_size, std::string::npos);
        if (!pool_.empty() && pool_.back() != '\0') throw Error("Precompiled normalizer: the last normalised string has no terminating NUL");
    }
    bool empty() const { return units_.empty(); }

    // the first hit of the common-prefix search over `key`: true and the normalised string's [begin, end) in the pool
    bool lookup(const char *key, size_t n, const char *&begin, const char *&end) const
    {
        if (units_.empty()) return false;
        size_t node = 0;
        uint32_t unit = units_[0];
        node ^= offset(unit);
        for (size_t i = 0; i < n; ++i) {
            const uint8_t c = (uint8_t)key[i];
            if (c == 0) return false;
            node ^= c;
            if (node >= units_.size()) throw Error("Precompiled normalizer: a trie node lies outside the trie");
            unit = units_[node];
            if ((unit & 0x800000FFu) != c) return false;
            node ^= offset(unit);
            if ((unit >> 8) & 1u) {
                if (node >= units_.size()) throw Error("Precompiled normalizer: a trie node lies outside the trie");
                const size_t value = units_[node] & 0x7FFFFFFFu;
                if (value >= pool_.size()) throw Error("Precompiled normalizer: a trie value lies outside the pool of normalised strings");
                begin = pool_.data() + value;
                end = begin;
                while (*end) ++end;   // (inside the pool: it ends with a NUL)
                return true;
            }
        }
        return false;
    }

    void normalize(const std::u32string &in, std::u32string &out) const
    {
        out.clear();
        out.reserve(in.size());
        std::string key;
        const char *b, *e;
        for (size_t at = 0; at < in.size();) {
            const size_t stop = grapheme::cluster_end(in, at);
            if (stop - at > 1) {   // (a cluster of one character: the per-character lookup below is the same lookup)
                key.clear();
                for (size_t i = at; i < stop; ++i) put_utf8(key, in[i]);
                if (key.size() < 6 && lookup(key.data(), key.size(), b, e)) { append_utf8(out, b, e); at = stop; continue; }
            }
            for (; at < stop; ++at) {
                key.clear();
                put_utf8(key, in[at]);
                if (lookup(key.data(), key.size(), b, e)) append_utf8(out, b, e);
                else out.push_back(in[at]);
            }
        }
    }

private:
    static uint32_t u32_at(const std::string &s, size_t i)
    {
        return (uint32_t)(uint8_t)s[i] | (uint32_t)(uint8_t)s[i + 1] << 8 | (uint32_t)(uint8_t)s[i + 2] << 16 | (uint32_t)(uint8_t)s[i + 3] << 24;
    }
    static size_t offset(uint32_t unit) { return (size_t)(unit >> 10) << ((unit & 0x200u) >> 6); }
    static void put_utf8(std::string &o, uint32_t cp)
    {
        if (cp < 0x80) o.push_back((char)cp);
        else if (cp < 0x800) { o.push_back((char)(0xC0 | (cp >> 6))); o.push_back((char)(0x80 | (cp & 0x3F))); }
        else if (cp < 0x10000) { o.push_back((char)(0xE0 | (cp >> 12))); o.push_back((char)(0x80 | ((cp >> 6) & 0x3F))); o.push_back((char)(0x80 | (cp & 0x3F))); }
        else { o.push_back((char)(0xF0 | (cp >> 18))); o.push_back((char)(0x80 | ((cp >> 12) & 0x3F))); o.push_back((char)(0x80 | ((cp >> 6) & 0x3F))); o.push_back((char)(0x80 | (cp & 0x3F))); }
    }
    // a pool string is UTF-8 written by sentencepiece; a malformed byte becomes U+FFFD and never reads past `e`
    static void append_utf8(std::u32string &out, const char *b, const char *e)
    {
        while (b < e) {
            const uint8_t c = (uint8_t)*b;
            const size_t want = c < 0x80 ? 1 : (c >> 5) == 0x6 ? 2 : (c >> 4) == 0xE ? 3 : (c >> 3) == 0x1E ? 4 : 0;
            bool ok = want != 0 && (size_t)(e - b) >= want;
            for (size_t k = 1; ok && k < want; ++k) ok = ((uint8_t)b[k] & 0xC0) == 0x80;
            if (!ok) { out.push_back(0xFFFD); ++b; continue; }
            uint32_t cp = want == 1 ? c : want == 2 ? (c & 0x1Fu) : want == 3 ? (c & 0x0Fu) : (c & 0x07u);
            for (size_t k = 1; k < want; ++k) cp = (cp << 6) | ((uint8_t)b[k] & 0x3Fu);
            out.push_back(cp);
            b += want;
        }
    }

    std::vector<uint32_t> units_;
    std::string pool_;
};

}  // namespace semtools
