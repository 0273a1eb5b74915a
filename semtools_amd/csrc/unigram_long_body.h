// unigram_long_body.h -- the body of the long-piece kernels of the Unigram device tokenizer (DESIGN.md 4.9 "long pieces"), one
// __device__ function ul_body<UTF8, RULES> that two files instantiate as the whole text of their kernels:
//   unigram_long_kernels.hip        ug_long_kernel<UTF8>        RULES = false  behind ug_scan_kernel / ug_scan_utf8_kernel
//   unigram_long_rules_kernels.hip  ug_long_rules_kernel<UTF8>  RULES = true   behind the scan kernels of unigram_rules_kernels.hip
// Every difference is behind `if (RULES ...)` on the template argument: the RULES = false instantiations compile what they compiled
// when this text stood in unigram_long_kernels.hip.  Everything here is local to the including file (an unnamed namespace).
//
// The second pass-1 kernel, on the same stream, run only while smt_unigram_set_long_pieces has the switch on.  The
// scan kernels' owner lane stops at SMT_UG_MAX_WORD raw bytes; with the switch on it leaves a record {owner position, line, bit 0: at
// a SPACE (otherwise at the line's start), bit 1: the line's first piece} in the work list of the handle's scratch (unigram_table.h)
// instead of a flag.  Here ONE WAVE (a block of 64
// lanes) takes the records i, i + grid, .. below the device counter -- the host never learns the count -- and for each piece:
//
//   1. finds the end, 64 raw bytes a step: the first byte (ASCII form) or character (UTF-8 form) that normalises to SPACE, or the
//      line's looked-at end.  A byte >= 0x80 (ASCII form), a FLAG code point, malformed UTF-8 or a continuation byte no lead byte of
//      the piece covers (UTF-8 form) in front of that end flags the line; every decode is handed the line's looked-at end.  The
//      measure is the scan kernels': the raw bytes, the SPACE character or a prepended R counted as one; above max_long: flagged.
//   2. normalises the piece once into LDS, compacted by a wave prefix sum: the bytes (nb) and the byte offset of every character
//      (off); dropped bytes and characters leave nothing.  Character i of the piece is lattice node i -- a node numbering of this
//      kernel's own: only the order of the nodes and the slots reach the output, and those are the scan kernels'.
//   3. matches, dealt by position: 64 starts a step, every lane walks forward from its start up to the longest piece, carries the FNV
//      state byte by byte and probes the table at every character end (ug_probe's logic on the normalised buffer).  A start is a KEY as
//      in the scan kernels: KEY_START (the walk behind R: kind 1 from T.r_state, or kind 0 without R), KEY_R (kind 0 from the first
//      character, behind R's own edge), 2 + i (kind 0 from character i + 1).  A lane keeps its first UL_HITS matches {score, id, end
//      node} in LDS and counts all of them.
//   4. relaxes, key by key in key order: node key - 2 is final when its key's turn comes, since every edge into it starts at a smaller
//      key.  The edges of ONE key end at different nodes, so the lanes relax them side by side; a key with more matches than UL_HITS
//      is walked again by lane 0, which relaxes as it goes.  The sums are score[piece] + best[at], one rounded add per edge; THE TIE
//      RULE is the comparison of keys in relax(): among equal sums for one end the smallest start wins, whatever the order of visits.
//      Maximum and tie rule do not depend on the order, every candidate is one add: the bits are the serial lattice's.
//   5. walks back along the best path (lane 0; consecutive unknowns fuse, the unk id is dropped under drop_unk, an unknown without an
//      unk id flags the line), then all lanes copy the ids to the piece's own slots from `base`, and one atomicAdd goes to raw_count.
//
// Bounds: step 1 runs at most max_long / 64 + 2 rounds, steps 2 - 4 over the piece's bytes and characters, walks by the longest piece,
// probes by the table's capacity, step 5 by the nodes.  LDS: 14 bytes per node, SMT_UG_MAX_LONG nodes, 4 normalised bytes and one
// offset per node, the ids of the path, the matches of 64 starts: under 64 KiB a block.
//
// RULES (a space rule of smt_unigram_set_space_rules is on, and smt_unigram_set_long_rules let the scan kernels hand over) changes:
//   1. under collapse_runs, for a record at a SPACE, the ABSORBED RUN is skipped first: from behind the owner's SPACE character, 64
//      raw bytes a step, to the first character that is neither SPACE nor DROPPED (the same flags as the search for the end; no LDS).
//      The end is searched from that character.  The measure is the scan kernels' under the rules: the owner's SPACE counts one,
//      and every raw byte behind it up to the end counts, absorbed, dropped or kept; both loops leave early on it.
//   2. starts at the first kept character: absorbed spaces and dropped characters leave no node.
//   drop_trailing: a piece without a kept character that ends at the line's looked-at end emits nothing, and flags the line when the
//      record says it is the line's first piece (the chains differ there: the host's).  The witness has counted it: it was measured.
// Steps 3 - 5, the slots, the tie rule and the sums are the same text.
#pragma once

#include "common.h"
#include "tokenize_frame.h"
#include "unigram_table.h"
#include "utf8_cursor.h"

namespace {

using smt::FROM_UNK;
using smt::FROM_UNSET;
using smt::KEY_R;
using smt::KEY_START;
using smt::UG_DROP;
using smt::UgLongList;
using smt::UgTable;
using smt::WpChar;
using smt::WpCodepoints;

constexpr uint32_t UL_LANES = 64;                       // one wave
constexpr uint32_t UL_NODES = SMT_UG_MAX_LONG;          // characters <= raw bytes
constexpr uint32_t UL_BYTES = 4 * UL_NODES;             // a character is at most 4 bytes
constexpr uint32_t UL_HITS = 8;                         // matches a lane keeps per start; more: the start is walked again
constexpr unsigned UL_GRID = 512;                       // two blocks a CU

struct UlLds {
    double score[UL_NODES];
    double h_score[UL_HITS][UL_LANES];
    uint32_t id[UL_NODES];
    uint32_t out[UL_NODES + 1];                         // the path's ids, last first
    uint32_t h_id[UL_HITS][UL_LANES];
    uint32_t misc[2];                                   // the path's tokens; 1 = the line is flagged
    uint16_t from[UL_NODES];
    uint16_t off[UL_NODES + 2];                         // byte of nb at which character i starts; [n_chars] = n_bytes (a walk reads one further)
    uint16_t h_end[UL_HITS][UL_LANES];
    uint16_t h_cnt[UL_LANES];
    uint8_t h_single[UL_LANES];
    uint8_t bytes[256];                                 // the byte map [128], or cls[128] | nrm[128] of the ASCII bytes
    uint8_t nb[UL_BYTES];
};

// the candidate: clen bytes of the normalised buffer from byte bo, behind R for kind 1, hash h: its entry + 1, or 0
__device__ __forceinline__ uint32_t ul_probe(const UgTable &T, const uint8_t *nb, unsigned long long h, uint32_t kind, uint32_t bo, uint32_t clen)
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
                bool same = true;
                for (uint32_t j = 0; j < clen && same; ++j) same = nb[bo + j] == piece[j];
                if (same) return (uint32_t)slot;
            }
        }
        idx = (idx + 1) & T.mask;
    }
    return 0;
}

// one edge into node n: better, or equal with the smaller start
__device__ __forceinline__ void ul_relax(UlLds &S, uint32_t n, double cand, uint32_t id, uint32_t key, uint16_t unk)
{
    const uint16_t f = S.from[n];
    if (f == FROM_UNSET || cand > S.score[n] || (cand == S.score[n] && key < (uint32_t)(f & 0x7FFF))) {
        S.score[n] = cand;
        S.id[n] = id;
        S.from[n] = (uint16_t)(key | unk);
    }
}

// The walk of one start: from character s0 (byte S.off[s0]) forward, at most T.max_piece bytes (R's counted for kind 1), a probe at
// every character end.  DIRECT: every match is relaxed at once with `here` and `key`; otherwise the first UL_HITS matches go to the
// lane's list.  -> the matches found; single: a piece covers exactly the first character.
template <bool DIRECT>
__device__ __forceinline__ uint32_t ul_walk(const UgTable &T, UlLds &S, uint32_t s0, uint32_t n_bytes, uint32_t kind, uint32_t lane, double here,
                                            uint32_t key, bool &single)
{
    unsigned long long h = kind ? T.r_state : smt::TOK_HASH_SEED;
    uint32_t len = kind ? T.rlen : 0, clen = 0, cnt = 0, c = s0;
    const uint32_t bo = S.off[s0];
    uint32_t next = S.off[s0 + 1];
    single = false;
    for (uint32_t b = bo; b < n_bytes; ++b) {
        if (len >= T.max_piece) break;
        h = (h ^ S.nb[b]) * smt::TOK_HASH_MUL;
        ++clen;
        ++len;
        if (b + 1 != next) continue;             // inside a character
        const uint32_t e = ul_probe(T, S.nb, h, kind, bo, clen);
        if (e) {
            if (c == s0) single = true;
            if (DIRECT) ul_relax(S, c, T.score[e - 1] + here, T.ent[e - 1].z, key, 0);
            else if (cnt < UL_HITS) {
                S.h_score[cnt][lane] = T.score[e - 1];
                S.h_id[cnt][lane] = T.ent[e - 1].z;
                S.h_end[cnt][lane] = (uint16_t)c;
            }
            ++cnt;
        }
        ++c;
        next = S.off[c + 1];                     // (c <= n_chars here: b + 1 <= n_bytes = off[n_chars])
    }
    return cnt;
}

__device__ __forceinline__ uint32_t ul_scan_incl(uint32_t v, uint32_t lane)
{
    for (uint32_t d = 1; d < UL_LANES; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, UL_LANES);
        if (lane >= d) v += o;
    }
    return v;
}

// the whole text of a long-piece kernel (S: the block's LDS; rules: the UG_RULE_* bits, read under RULES only)
template <bool UTF8, bool RULES>
__device__ __forceinline__ void ul_body(UlLds &S, const UgTable &T, const WpCodepoints &U, uint32_t rules, const uint8_t *__restrict__ text,
                                        uint64_t text_bytes, const uint64_t *__restrict__ line_begin, const uint32_t *__restrict__ line_len,
                                        uint64_t n_lines, uint32_t keep_bytes, int drop_unk, uint32_t max_long, uint32_t *__restrict__ ids_tmp,
                                        uint32_t *__restrict__ raw_count, uint8_t *__restrict__ flags, const UgLongList &W)
{
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < 256; i += UL_LANES) {
        const uint8_t m = T.map[i & 127];
        if (!UTF8) S.bytes[i] = m;
        else S.bytes[i] = i >= 128 ? m : m == ' ' ? (uint8_t)smt::WP_SPACE : m == UG_DROP ? (uint8_t)smt::WP_DROPPED : (uint8_t)smt::WP_ORDINARY;
    }
    const uint8_t *cls = S.bytes, *nrm = S.bytes + 128;
    const uint32_t handed = *W.head, n_rec = handed < W.cap ? handed : W.cap;
    unsigned long long *stats = reinterpret_cast<unsigned long long *>(W.head) + 1;
    const double r_score = T.r_score + 0.0;
    const bool dropping = drop_unk && T.unk != smt::TOK_NONE;
    // (every branch that leaves a record below depends on the record and on wave-wide votes only: the barriers are met by all lanes)
    for (uint32_t r = blockIdx.x; r < n_rec; r += gridDim.x) {
        __syncthreads();                         // the last record's LDS is done with; S.bytes is filled
        const uint4 rec = W.rec[r];
        const uint64_t p = (uint64_t)rec.x | ((uint64_t)rec.y << 32), line = rec.z;
        const bool at_space = (rec.w & 1u) != 0;
        if (line >= n_lines || p >= text_bytes) continue;
        const uint64_t lb = line_begin[line];
        const uint32_t ll = line_len[line];
        const uint64_t le_line = lb + (keep_bytes && keep_bytes < ll ? keep_bytes : ll);
        const uint64_t le = le_line < text_bytes ? le_line : text_bytes;   // the end of what is looked at
        if (p < lb || p >= le) continue;
        uint32_t space_src = 1;
        if (UTF8 && at_space) {
            WpChar me;
            smt::wp_char_at(U, cls, nrm, text, p, le, me);
            space_src = me.src;
        }
        const bool has_r = at_space || T.prepend != 2;
        const uint64_t run = at_space ? p + space_src : p;
        const uint64_t base = at_space ? p + line + 1 : lb + line;   // the piece's first slot
        // ---- 1. the end
        const uint32_t room = max_long - (has_r ? 1u : 0u);          // the raw bytes the piece may hold
        bool bad = false;
        uint64_t start = run;                    // the piece's first kept character: behind the absorbed run (RULES), or `run` itself
        if (RULES && (rules & smt::UG_RULE_COLLAPSE) && at_space) {
            start = le < run ? run : le;
            for (uint64_t t = run; t < le; t += UL_LANES) {
                if (t - run > room) { bad = true; break; }           // over the limit already: the absorbed bytes count
                const uint64_t q = t + lane;
                bool stop = false, flag = false;
                if (q < le) {
                    const uint32_t b = text[q];
                    if (!UTF8) {
                        flag = b >= 0x80;
                        stop = !flag && S.bytes[b] != ' ' && S.bytes[b] != UG_DROP;
                    } else if ((b & 0xC0u) == 0x80u) {               // a continuation byte: a lead byte of the run covers it, or it is malformed
                        bool covered = false;
                        for (uint32_t d = 1; d <= 3 && q - run >= d; ++d) {
                            const uint32_t l = text[q - d];
                            if ((l & 0xC0u) == 0x80u) continue;
                            const uint32_t len = (l >= 0xC2 && l <= 0xDF) ? 2u : (l & 0xF0u) == 0xE0u ? 3u : (l >= 0xF0 && l <= 0xF4) ? 4u : 0u;
                            covered = len > d;
                            break;
                        }
                        flag = !covered;
                    } else {
                        WpChar ch;
                        smt::wp_char_at(U, cls, nrm, text, q, le, ch);
                        flag = ch.cls == smt::WP_FLAG;
                        stop = !flag && ch.cls != smt::WP_SPACE && ch.cls != smt::WP_DROPPED;
                    }
                }
                const unsigned long long fm = __ballot(flag), m = fm | __ballot(stop);
                if (m) {
                    const uint32_t at = (uint32_t)__ffsll((long long)m) - 1;
                    start = t + at;
                    bad = (fm >> at) & 1;
                    break;
                }
            }
            if (bad) {                           // (a flagging byte's lane of the scan kernel has flagged the line too; over the limit: here)
                if (lane == 0) flags[line] = 1;
                continue;
            }
        }
        uint64_t end = le < start ? start : le;
        for (uint64_t t = start; t < le; t += UL_LANES) {
            if (t - run > room) { end = t; break; }                  // over the limit already
            const uint64_t q = t + lane;
            bool stop = false, flag = false;
            if (q < le) {
                const uint32_t b = text[q];
                if (!UTF8) {
                    flag = b >= 0x80;
                    stop = !flag && S.bytes[b] == ' ';
                } else if ((b & 0xC0u) == 0x80u) {                   // a continuation byte: a lead byte of the piece covers it, or it is malformed
                    bool covered = false;
                    for (uint32_t d = 1; d <= 3 && q - start >= d; ++d) {
                        const uint32_t l = text[q - d];
                        if ((l & 0xC0u) == 0x80u) continue;
                        const uint32_t len = (l >= 0xC2 && l <= 0xDF) ? 2u : (l & 0xF0u) == 0xE0u ? 3u : (l >= 0xF0 && l <= 0xF4) ? 4u : 0u;
                        covered = len > d;
                        break;
                    }
                    flag = !covered;
                } else {
                    WpChar ch;
                    smt::wp_char_at(U, cls, nrm, text, q, le, ch);
                    flag = ch.cls == smt::WP_FLAG;
                    stop = ch.cls == smt::WP_SPACE;
                }
            }
            const unsigned long long fm = __ballot(flag), m = fm | __ballot(stop);
            if (m) {
                const uint32_t at = (uint32_t)__ffsll((long long)m) - 1;
                end = t + at;
                bad = (fm >> at) & 1;
                break;
            }
        }
        if (bad) {                               // (that byte's lane of the scan kernel has flagged the line too)
            if (lane == 0) flags[line] = 1;
            continue;
        }
        const uint64_t measure = (has_r ? 1u : 0u) + (end - run);
        if (measure > max_long) {
            if (lane == 0) flags[line] = 1;
            continue;
        }
        if (lane == 0) {
            atomicAdd(stats, 1ull);
            atomicAdd(stats + 1, (unsigned long long)measure);
        }
        // ---- 2. the normalised piece
        uint32_t n_chars = 0, n_bytes = 0;
        bool over = false;
        for (uint64_t t = start; t < end; t += UL_LANES) {
            const uint64_t q = t + lane;
            uint32_t n = 0, chars = 0;
            WpChar ch;
            ch.where = smt::AT_BYTE;
            ch.at = 0;
            if (q < end) {
                const uint32_t b = text[q];
                if (!UTF8) {
                    ch.at = S.bytes[b & 127];
                    n = chars = ch.at != UG_DROP ? 1u : 0u;
                } else if ((b & 0xC0u) != 0x80u) {
                    smt::wp_char_at(U, cls, nrm, text, q, end, ch);
                    if (ch.cls != smt::WP_FLAG) { n = ch.n; chars = ch.chars; }
                }
            }
            const uint32_t incl = ul_scan_incl(n | (chars << 16), lane);
            const uint32_t total = __shfl(incl, UL_LANES - 1, UL_LANES);
            if (n_bytes + (total & 0xFFFFu) > UL_BYTES || n_chars + (total >> 16) > UL_NODES) { over = true; break; }
            uint32_t at_b = n_bytes + (incl & 0xFFFFu) - n, at_c = n_chars + (incl >> 16) - chars, j = 0;
            for (uint32_t k = 0; k < n; ++k) {
                const uint32_t o = smt::wp_byte(U, text, q, ch, k);
                S.nb[at_b + k] = (uint8_t)o;
                if ((o & 0xC0u) != 0x80u && j < chars) S.off[at_c + j++] = (uint16_t)(at_b + k);
            }
            n_bytes += total & 0xFFFFu;
            n_chars += total >> 16;
        }
        if (over) {                              // (cannot be: a character has at most 4 bytes, an output no more characters than its source bytes)
            if (lane == 0) flags[line] = 1;
            continue;
        }
        if (!at_space && n_chars == 0 && end < le) continue;   // the normalised text starts with R: that character's piece is the first
        if (!has_r && n_chars == 0) continue;                   // nothing is left of the line
        if (RULES && (rules & smt::UG_RULE_DROP_TRAILING) && n_chars == 0 && end == le) {   // R alone at the line's end emits nothing; as
            if ((rec.w & 2u) && lane == 0) flags[line] = 1;                                   // the line's first piece it is the host's
            continue;
        }
        if (lane == 0) S.off[n_chars] = (uint16_t)n_bytes;
        for (uint32_t i = lane; i < n_chars; i += UL_LANES) S.from[i] = FROM_UNSET;
        __syncthreads();
        // ---- 3. and 4. the lattice, 64 keys a step
        for (uint32_t kb = 0; kb <= n_chars && n_chars; kb += UL_LANES) {
            {
                const uint32_t key = kb + lane, s0 = key < 2 ? 0 : key - 1;
                const bool valid = s0 < n_chars && !(key == KEY_R && !has_r);
                bool single = false;
                uint32_t cnt = 0;
                if (valid) cnt = ul_walk<false>(T, S, s0, n_bytes, key == KEY_START && has_r ? 1u : 0u, lane, 0.0, key, single);
                S.h_cnt[lane] = (uint16_t)cnt;
                S.h_single[lane] = single ? 1 : 0;
            }
            __syncthreads();
            for (uint32_t j = 0; j < UL_LANES; ++j) {
                const uint32_t key = kb + j, s0 = key < 2 ? 0 : key - 1;
                if (s0 >= n_chars) break;
                if (key == KEY_R && !has_r) continue;
                const uint32_t kind = key == KEY_START && has_r ? 1u : 0u;
                const double here = key == KEY_START ? 0.0 : key == KEY_R ? r_score : S.score[key - 2];
                const uint32_t cnt = S.h_cnt[j];
                if (cnt > UL_HITS) {
                    bool single;
                    if (lane == 0) ul_walk<true>(T, S, s0, n_bytes, kind, lane, here, key, single);
                } else if (lane < cnt) {
                    ul_relax(S, S.h_end[lane][j], S.h_score[lane][j] + here, S.h_id[lane][j], key, 0);
                }
                // the unknown edge over the first character when no piece covers exactly it (the walk through R offers none)
                if (lane == UL_LANES - 1 && kind == 0 && !S.h_single[j]) ul_relax(S, s0, T.unk_score + here, T.unk == smt::TOK_NONE ? 0u : T.unk, key, FROM_UNK);
                __syncthreads();
            }
        }
        // ---- 5. back along the best path: what stays (consecutive unknowns fuse, the unk id is dropped), last first
        if (lane == 0) {
            uint32_t key = n_chars ? n_chars + 1 : KEY_R, n_tok = 0, flagged = 0;
            for (uint32_t step = 0; step <= UL_NODES && key != KEY_START; ++step) {
                uint32_t id, from;
                bool unk;
                if (key == KEY_R) { id = T.r_id; unk = T.r_unk != 0; from = KEY_START; }
                else {
                    if (key - 2 >= n_chars) { flagged = 1; break; }   // (cannot be: every node has an edge into it, from a smaller key)
                    const uint16_t f = S.from[key - 2];
                    id = S.id[key - 2];
                    unk = (f & FROM_UNK) != 0;
                    from = f & 0x7FFF;
                }
                bool pred_unk = false;
                if (from == KEY_R) pred_unk = T.r_unk != 0;
                else if (from != KEY_START && from - 2 < n_chars) pred_unk = (S.from[from - 2] & FROM_UNK) != 0;
                if (unk && T.unk == smt::TOK_NONE) { flagged = 1; break; }
                if (!(unk && pred_unk) && !(dropping && id == T.unk)) S.out[n_tok++] = id;
                key = from;
            }
            if (n_tok > end + line + 1 - base) flagged = 1;   // (cannot be: tokens <= characters + 1 <= the piece's slots)
            S.misc[0] = n_tok;
            S.misc[1] = flagged;
        }
        __syncthreads();
        const uint32_t n_tok = S.misc[0];
        if (S.misc[1]) {
            if (lane == 0) flags[line] = 1;
            continue;
        }
        for (uint32_t i = lane; i < n_tok; i += UL_LANES) ids_tmp[base + i] = S.out[n_tok - 1 - i];
        if (lane == 0 && n_tok) atomicAdd(&raw_count[line], n_tok);
    }
}

}  // namespace
