// unigram_probe.h -- the vocabulary probes of the Unigram device tokenizer's pass-1 kernels, shared by the kernels without the space
// rules (unigram_kernels.hip, unigram_utf8_kernels.hip) and with them (unigram_rules_kernels.hip): a candidate's hash is looked up in
// the open-addressed table and its bytes are compared with the text it was walked from.  Device code only; internal to the library.
#pragma once

#include "common.h"
#include "tokenize_frame.h"
#include "unigram_table.h"
#include "utf8_cursor.h"

namespace smt {

// the candidate: clen kept bytes from raw position s (dropped bytes skipped), behind R for kind 1, hash h: its entry + 1, or 0
__device__ __forceinline__ uint32_t ug_probe(const UgTable &T, const uint8_t *__restrict__ text, const uint8_t *map, unsigned long long h,
                                             uint32_t kind, uint64_t s, uint32_t clen)
{
    uint32_t idx = (uint32_t)h & T.mask;
    const uint32_t tag = (uint32_t)(h >> 32);
    const uint32_t skip = kind ? T.rlen : 0;
    for (uint32_t probe = 0; probe <= T.mask; ++probe) {
        const unsigned long long slot = T.slots[idx];
        if (slot == 0) return 0;
        if ((uint32_t)(slot >> 32) == tag) {
            const uint4 e = T.ent[(uint32_t)slot - 1];
            if (e.w == kind && e.y == clen + skip) {
                const uint8_t *piece = T.pool + e.x + skip;
                uint64_t q = s;
                uint32_t j = 0;
                bool same = true;
                while (j < clen) {   // (the candidate was walked once already: it has clen kept bytes before the piece's end)
                    const uint8_t m = map[text[q++]];
                    if (m == UG_DROP) continue;
                    if (m != piece[j]) { same = false; break; }
                    ++j;
                }
                if (same) return (uint32_t)slot;
            }
        }
        idx = (idx + 1) & T.mask;
    }
    return 0;
}

// the cursor: output character j of the source character at raw byte q starts at byte k of that character's output (c)
struct UgCursor {
    uint64_t q;
    uint32_t k, j;
    WpChar c;
};

// the candidate: clen normalised bytes from the cursor `s`, behind R for kind 1, hash h: its entry + 1, or 0
__device__ __forceinline__ uint32_t ug_probe_utf8(const UgTable &T, const WpCodepoints &U, const uint8_t *__restrict__ text, const uint8_t *cls,
                                                  const uint8_t *nrm, unsigned long long h, uint32_t kind, const UgCursor &s, uint64_t end,
                                                  uint32_t clen)
{
    uint32_t idx = (uint32_t)h & T.mask;
    const uint32_t tag = (uint32_t)(h >> 32);
    const uint32_t skip = kind ? T.rlen : 0;
    for (uint32_t probe = 0; probe <= T.mask; ++probe) {
        const unsigned long long slot = T.slots[idx];
        if (slot == 0) return 0;
        if ((uint32_t)(slot >> 32) == tag) {
            const uint4 e = T.ent[(uint32_t)slot - 1];
            if (e.w == kind && e.y == clen + skip) {
                const uint8_t *piece = T.pool + e.x + skip;
                uint64_t q = s.q;
                uint32_t k = s.k, j = 0;
                WpChar qc = s.c;
                bool same = true;
                while (j < clen) {   // (the candidate was walked once already: it has clen bytes before the piece's end)
                    if (q >= end || wp_byte(U, text, q, qc, k) != piece[j]) { same = false; break; }
                    ++j;
                    if (++k >= qc.n) { q += qc.src; k = 0; wp_next_char(U, cls, nrm, text, q, end, qc); }
                }
                if (same) return (uint32_t)slot;
            }
        }
        idx = (idx + 1) & T.mask;
    }
    return 0;
}

}  // namespace smt
