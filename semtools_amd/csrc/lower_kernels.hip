// lower_kernels.hip -- lower-casing packed UTF-8 lines on the device (DESIGN.md 4.9 "Lower-casing"): byte for byte what to_lowercase of
// host/host.cpp returns for every line alone -- Rust's str::to_lowercase: ASCII + 32, the runs of host/unicode_lower.h, the
// multi-code-point entry, Final_Sigma inside the line -- for the lines of --ignore-case on their way into the device tokenizers.
//
// The work is dealt by TEXT POSITION in the frame of the tokenizers (tokenize_frame.h): one lane per byte, the block's line window in
// LDS, the lane's line by tok_count_le.  The lane on the first byte of a character owns it; continuation lanes and lanes between two
// lines own nothing.  A line's bytes move both ways (U+0130 2 -> 3, U+212A 3 -> 1), so nothing is written before every position is
// known; and a line with ill-formed UTF-8 is copied as it is, so nothing is counted before every flag is known.  Three launches:
//   lower_flag_kernel          the strict decode of utf8_cursor.h at every byte >= 0x80: flags[line]
//   lower_pass_kernel<false>   what every lane's character becomes, in bytes: a scan within the block, the block's total, and one
//                              atomicAdd per (line, block) into out_len (integer adds: the sums do not depend on their order)
//   -- the frame's one-block prefix sums: block totals -> block bases, out_len -> out_begin --
//   lower_pass_kernel<true>    the same recomputed, and the bytes written at block base + place in the block
// The tables (about 7 KB for the built-in ones) lie in LDS, loaded only by a block that holds a byte >= 0x80 of an unflagged line: a
// pure-ASCII block touches none of them.  The Final_Sigma look is a loop over neighbours that only a lane on U+03A3 runs; every look
// ends at the nearest code point that is not case-ignorable, so it stays inside the line and its total is linear in the text.
//
// Bounds: every read of the text lies in [line begin, min(line end, text_bytes)), every write below out_cap; indices into the LDS
// tables are below the counts smt_lower_tables_check has bounded by the arrays' sizes.
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "common.h"
#include "host/unicode_lower.h"
#include "tokenize_frame.h"

namespace smt {

constexpr unsigned LOWER_THREADS = 256;
// what the LDS image holds (the built-in tables: 175 runs, 1 multi entry, 133 + 402 ranges >= U+0080)
constexpr uint32_t LOWER_MAX_RUNS = 256, LOWER_MAX_MULTI = 8, LOWER_MAX_CASED = 192, LOWER_MAX_IGNORABLE = 512;

// the tables on the device
struct LowerDev {
    const uint4 *runs;        // {first, last, delta, stride}
    const uint32_t *multi;    // [n_multi][5]: cp, n, to[3]
    const uint2 *cased;       // {first, last}
    const uint2 *ignorable;
    uint32_t n_runs, n_multi, n_cased, n_ignorable, final_sigma;
};

}  // namespace smt

struct smt_lower {
    smt_ctx *ctx = nullptr;
    void *d_table = nullptr;
    smt::LowerDev T = {};
    void *d_blocks = nullptr;   // block_base u64 [blocks_cap + 1] | block_total u32 [blocks_cap]
    uint64_t blocks_cap = 0;

    uint64_t *block_base() const { return static_cast<uint64_t *>(d_blocks); }
    uint32_t *block_total() const { return reinterpret_cast<uint32_t *>(block_base() + blocks_cap + 1); }
};

namespace {

using smt::LOWER_THREADS;
using smt::LowerDev;

struct LowerLds {
    uint4 runs[smt::LOWER_MAX_RUNS];
    uint2 cased[smt::LOWER_MAX_CASED];
    uint2 ignorable[smt::LOWER_MAX_IGNORABLE];
    uint32_t multi[smt::LOWER_MAX_MULTI * 5];
};

// where a lane stands: byte p, and -- when `in` -- byte c of `line`, which is [lb, le) of the text
struct LowerLane {
    uint64_t p, line, lb, le;
    bool in;
    uint8_t c;
};

// the block's line window behind a barrier that every lane reaches, then the lane's line
__device__ __forceinline__ void lower_lane(uint64_t *s_win, const uint8_t *__restrict__ text, uint64_t text_bytes,
                                           const uint64_t *__restrict__ line_begin, const uint32_t *__restrict__ line_len, uint64_t n_lines,
                                           LowerLane &L)
{
    const uint64_t first = (uint64_t)blockIdx.x * LOWER_THREADS;
    if (threadIdx.x < 2) {
        const uint64_t last = first + LOWER_THREADS - 1 < text_bytes ? first + LOWER_THREADS - 1 : text_bytes - 1;
        s_win[threadIdx.x] = smt::tok_count_le(line_begin, 0, n_lines, threadIdx.x == 0 ? first : last);
    }
    __syncthreads();
    L.p = first + threadIdx.x;
    L.line = L.lb = L.le = 0;
    L.in = false;
    L.c = 0;
    if (L.p >= text_bytes) return;
    const uint64_t n_le = smt::tok_count_le(line_begin, s_win[0], s_win[1], L.p);
    if (n_le == 0) return;                       // in front of the first line
    L.line = n_le - 1;
    L.lb = line_begin[L.line];
    if (L.p < L.lb) return;                      // (a list out of order)
    const uint64_t le_line = L.lb + line_len[L.line];
    L.le = le_line < text_bytes ? le_line : text_bytes;
    if (L.p >= L.le) return;                     // between two lines
    L.in = true;
    L.c = text[L.p];
}

// the strict decode of utf8_cursor.h: the code point that starts at q and ends at or before `end` (q < end; nothing outside [q, end)
// is read).  False: a continuation byte, 0xC0 / 0xC1, 0xF5 .. 0xFF, a sequence cut by `end`, an overlong form, a surrogate, a value
// above U+10FFFF -- then len is 1.
__device__ __forceinline__ bool lower_decode(const uint8_t *__restrict__ text, uint64_t q, uint64_t end, uint32_t &cp, uint32_t &len)
{
    const uint32_t b0 = text[q];
    len = 1;
    cp = b0;
    if (b0 < 0x80) return true;
    uint32_t n;
    if (b0 >= 0xC2 && b0 <= 0xDF) { n = 2; cp = b0 & 0x1Fu; }
    else if ((b0 & 0xF0u) == 0xE0u) { n = 3; cp = b0 & 0x0Fu; }
    else if (b0 >= 0xF0 && b0 <= 0xF4) { n = 4; cp = b0 & 0x07u; }
    else return false;
    if (q + n > end) return false;
    for (uint32_t k = 1; k < n; ++k) {
        const uint32_t b = text[q + k];
        if ((b & 0xC0u) != 0x80u) return false;
        cp = (cp << 6) | (b & 0x3Fu);
    }
    if (n == 3 && (cp < 0x800u || (cp >= 0xD800u && cp <= 0xDFFFu))) return false;
    if (n == 4 && (cp < 0x10000u || cp > 0x10FFFFu)) return false;
    len = n;
    return true;
}

__global__ void __launch_bounds__(LOWER_THREADS) lower_flag_kernel(const uint8_t *__restrict__ text, uint64_t text_bytes,
                                                                   const uint64_t *__restrict__ line_begin, const uint32_t *__restrict__ line_len,
                                                                   uint64_t n_lines, uint8_t *__restrict__ flags)
{
    __shared__ uint64_t s_win[2];
    LowerLane L;
    lower_lane(s_win, text, text_bytes, line_begin, line_len, n_lines, L);
    if (!L.in || L.c < 0x80) return;
    bool good = false;
    if ((L.c & 0xC0) == 0x80) {
        // a continuation byte: good when a lead byte at most three bytes in front, inside the line, covers it (that lead's lane
        // checks the sequence as a whole)
        for (uint32_t d = 1; d <= 3 && L.p - L.lb >= d; ++d) {
            const uint32_t b = text[L.p - d];
            if ((b & 0xC0u) == 0x80u) continue;
            const uint32_t len = (b >= 0xC2 && b <= 0xDF) ? 2u : (b & 0xF0u) == 0xE0u ? 3u : (b >= 0xF0 && b <= 0xF4) ? 4u : 0u;
            good = len > d;
            break;
        }
    } else {
        uint32_t cp, len;
        good = lower_decode(text, L.p, L.le, cp, len);
    }
    if (!good) flags[L.line] = 1;
}

__device__ __forceinline__ bool lower_in_ranges(const uint2 *r, uint32_t n, uint32_t cp)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        const uint2 e = r[mid];
        if (cp > e.y) lo = mid + 1;
        else if (cp < e.x) hi = mid;
        else return true;
    }
    return false;
}
// ASCII is fixed: the letters are cased, ' . : ^ ` are case-ignorable
__device__ __forceinline__ bool lower_cased(const LowerLds &S, const LowerDev &T, uint32_t cp)
{
    if (cp < 0x80) return (cp >= 'A' && cp <= 'Z') || (cp >= 'a' && cp <= 'z');
    return lower_in_ranges(S.cased, T.n_cased, cp);
}
__device__ __forceinline__ bool lower_ignorable(const LowerLds &S, const LowerDev &T, uint32_t cp)
{
    if (cp < 0x80) return cp == 0x27 || cp == 0x2E || cp == 0x3A || cp == 0x5E || cp == 0x60;
    return lower_in_ranges(S.ignorable, T.n_ignorable, cp);
}

__device__ __forceinline__ uint32_t lower_utf8_bytes(uint32_t cp) { return cp < 0x80 ? 1u : cp < 0x800 ? 2u : cp < 0x10000 ? 3u : 4u; }

// cp as UTF-8 at out[pos ..), nothing at or beyond cap; the position behind it
__device__ __forceinline__ uint64_t lower_put(uint8_t *__restrict__ out, uint64_t pos, uint64_t cap, uint32_t cp)
{
    const uint32_t n = lower_utf8_bytes(cp);
    if (pos + n > cap) return pos + n;
    if (n == 1) out[pos] = (uint8_t)cp;
    else if (n == 2) { out[pos] = (uint8_t)(0xC0 | (cp >> 6)); out[pos + 1] = (uint8_t)(0x80 | (cp & 0x3F)); }
    else if (n == 3) {
        out[pos] = (uint8_t)(0xE0 | (cp >> 12));
        out[pos + 1] = (uint8_t)(0x80 | ((cp >> 6) & 0x3F));
        out[pos + 2] = (uint8_t)(0x80 | (cp & 0x3F));
    } else {
        out[pos] = (uint8_t)(0xF0 | (cp >> 18));
        out[pos + 1] = (uint8_t)(0x80 | ((cp >> 12) & 0x3F));
        out[pos + 2] = (uint8_t)(0x80 | ((cp >> 6) & 0x3F));
        out[pos + 3] = (uint8_t)(0x80 | (cp & 0x3F));
    }
    return pos + n;
}

// Final_Sigma for the U+03A3 of `len` bytes at L.p: preceded by a cased code point and not followed by one, case-ignorable code
// points skipped on both sides, all of it inside [L.lb, L.le).  The line is well formed (it is not flagged).
__device__ __forceinline__ bool lower_final_sigma(const LowerLds &S, const LowerDev &T, const uint8_t *__restrict__ text, const LowerLane &L, uint32_t len)
{
    bool before = false, after = false;
    for (uint64_t k = L.p; k > L.lb;) {
        uint64_t b = k - 1;
        for (int s = 0; s < 3 && b > L.lb && (text[b] & 0xC0) == 0x80; ++s) --b;
        uint32_t q, l2;
        const bool ok = lower_decode(text, b, k, q, l2);
        k = b;
        if (ok && lower_ignorable(S, T, q)) continue;
        before = ok && lower_cased(S, T, q);
        break;
    }
    for (uint64_t k = L.p + len; before && k < L.le;) {
        uint32_t q, l2;
        const bool ok = lower_decode(text, k, L.le, q, l2);
        k += l2;
        if (ok && lower_ignorable(S, T, q)) continue;
        after = ok && lower_cased(S, T, q);
        break;
    }
    return before && !after;
}

// WRITE false: block_total[block] = the bytes the block's lanes yield, out_len[line] += those of the line's lanes here, *n_flagged +=
// the flagged lines that start here.  WRITE true: the bytes, at block_base[block] + the lane's place in the block.
template <bool WRITE>
__global__ void __launch_bounds__(LOWER_THREADS) lower_pass_kernel(LowerDev T, const uint8_t *__restrict__ text, uint64_t text_bytes,
                                                                   const uint64_t *__restrict__ line_begin, const uint32_t *__restrict__ line_len,
                                                                   uint64_t n_lines, const uint8_t *__restrict__ flags, uint32_t *__restrict__ block_total,
                                                                   uint32_t *__restrict__ out_len, uint32_t *__restrict__ n_flagged,
                                                                   const uint64_t *__restrict__ block_base, uint8_t *__restrict__ out, uint64_t out_cap)
{
    __shared__ LowerLds S;
    __shared__ uint64_t s_win[2];
    __shared__ uint32_t s_wsum[LOWER_THREADS / 64];
    __shared__ uint32_t s_ex[WRITE ? 1 : LOWER_THREADS];
    const unsigned t = threadIdx.x, lane = t & 63, w = t >> 6;
    LowerLane L;
    lower_lane(s_win, text, text_bytes, line_begin, line_len, n_lines, L);
    const bool flagged = L.in && flags[L.line] != 0;
    if (__syncthreads_or(L.in && !flagged && L.c >= 0x80)) {
        uint32_t *d = reinterpret_cast<uint32_t *>(S.runs);
        const uint32_t *s = reinterpret_cast<const uint32_t *>(T.runs);
        for (uint32_t i = t; i < T.n_runs * 4; i += LOWER_THREADS) d[i] = s[i];
        d = reinterpret_cast<uint32_t *>(S.cased);
        s = reinterpret_cast<const uint32_t *>(T.cased);
        for (uint32_t i = t; i < T.n_cased * 2; i += LOWER_THREADS) d[i] = s[i];
        d = reinterpret_cast<uint32_t *>(S.ignorable);
        s = reinterpret_cast<const uint32_t *>(T.ignorable);
        for (uint32_t i = t; i < T.n_ignorable * 2; i += LOWER_THREADS) d[i] = s[i];
        for (uint32_t i = t; i < T.n_multi * 5; i += LOWER_THREADS) S.multi[i] = T.multi[i];
        __syncthreads();
    }
    // what the lane yields: `raw`, its own byte; otherwise n_cp code points o0 .. o2.  n: the bytes of it
    bool raw = flagged;
    uint32_t n = 0, n_cp = 0, o0 = 0, o1 = 0, o2 = 0;
    if (L.in) {
        if (flagged) n = 1;
        else if (L.c < 0x80) { o0 = (L.c >= 'A' && L.c <= 'Z') ? L.c + 32u : L.c; n_cp = 1; n = 1; }
        else if ((L.c & 0xC0) != 0x80) {
            uint32_t cp, len;
            if (!lower_decode(text, L.p, L.le, cp, len)) { raw = true; n = 1; }   // (cannot be: the line would be flagged)
            else {
                n_cp = 1;
                o0 = cp;
                if (T.final_sigma && cp == 0x3A3u) o0 = lower_final_sigma(S, T, text, L, len) ? 0x3C2u : 0x3C3u;
                else {
                    bool multi = false;
                    for (uint32_t i = 0; i < T.n_multi && !multi; ++i)
                        if (S.multi[i * 5] == cp) {
                            multi = true;
                            n_cp = S.multi[i * 5 + 1];
                            o0 = S.multi[i * 5 + 2];
                            o1 = S.multi[i * 5 + 3];
                            o2 = S.multi[i * 5 + 4];
                        }
                    uint32_t lo = 0, hi = multi ? 0 : T.n_runs;
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi) / 2;
                        const uint4 r = S.runs[mid];
                        if (cp > r.y) lo = mid + 1;
                        else if (cp < r.x) hi = mid;
                        else {
                            if ((cp - r.x) % r.w == 0) o0 = cp + r.z;   // (the delta as two's complement)
                            break;
                        }
                    }
                }
                n = lower_utf8_bytes(o0) + (n_cp > 1 ? lower_utf8_bytes(o1) : 0u) + (n_cp > 2 ? lower_utf8_bytes(o2) : 0u);
            }
        }
    }
    uint32_t inc = n;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if ((int)lane >= d) inc += o;
    }
    if (lane == 63) s_wsum[w] = inc;
    __syncthreads();
    uint32_t wbase = 0, total = 0;
#pragma unroll
    for (unsigned j = 0; j < LOWER_THREADS / 64; ++j) {
        const uint32_t x = s_wsum[j];
        wbase += j < w ? x : 0;
        total += x;
    }
    const uint32_t ex = wbase + inc - n;         // the bytes of the lanes in front of this one
    if (!WRITE) {
        s_ex[t] = ex;
        __syncthreads();
        if (t == 0) block_total[blockIdx.x] = total;
        if (!L.in) return;
        if (flagged && L.p == L.lb) atomicAdd(n_flagged, 1u);
        if (L.p + 1 == L.le || t == LOWER_THREADS - 1) {   // the line's last lane in this block: the sum from its first one here
            const uint64_t first = (uint64_t)blockIdx.x * LOWER_THREADS;
            const uint32_t from = L.lb > first ? (uint32_t)(L.lb - first) : 0u;
            const uint32_t sum = ex + n - s_ex[from];
            if (sum) atomicAdd(&out_len[L.line], sum);
        }
    } else {
        if (!n) return;
        uint64_t pos = block_base[blockIdx.x] + ex;
        if (raw) {
            if (pos < out_cap) out[pos] = L.c;
            return;
        }
        pos = lower_put(out, pos, out_cap, o0);
        if (n_cp > 1) pos = lower_put(out, pos, out_cap, o1);
        if (n_cp > 2) lower_put(out, pos, out_cap, o2);
    }
}

size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

bool is_surrogate(uint32_t cp) { return cp >= 0xD800u && cp <= 0xDFFFu; }
uint32_t utf8_bytes(uint32_t cp) { return cp < 0x80 ? 1u : cp < 0x800 ? 2u : cp < 0x10000 ? 3u : 4u; }

int check_ranges(const uint32_t *first, const uint32_t *last, uint64_t n, uint32_t cap)
{
    SMT_REQUIRE(n == 0 || (first && last), "range arrays");
    SMT_REQUIRE(n <= cap, "more ranges than the device form holds");
    for (uint64_t i = 0; i < n; ++i) {
        SMT_REQUIRE(first[i] >= 0x80u, "a table entry below U+0080: ASCII is fixed");
        SMT_REQUIRE(last[i] >= first[i], "a range with last < first");
        SMT_REQUIRE(last[i] <= 0x10FFFFu, "a range beyond U+10FFFF");
        SMT_REQUIRE(i == 0 || first[i] > last[i - 1], "ranges must be sorted and disjoint");
    }
    return SMT_OK;
}

int tables_check(const smt_lower_tables *t)
{
    SMT_REQUIRE(t != nullptr, "null argument");
    SMT_REQUIRE(t->n_runs == 0 || (t->run_first && t->run_last && t->run_delta && t->run_stride), "run arrays");
    SMT_REQUIRE(t->n_runs <= smt::LOWER_MAX_RUNS, "more runs than the device form holds");
    for (uint64_t i = 0; i < t->n_runs; ++i) {
        const uint32_t f = t->run_first[i], l = t->run_last[i], stride = t->run_stride[i];
        const int64_t delta = t->run_delta[i];
        SMT_REQUIRE(f >= 0x80u, "a table entry below U+0080: ASCII is fixed");
        SMT_REQUIRE(l >= f, "a run with last < first");
        SMT_REQUIRE(l <= 0x10FFFFu, "a run beyond U+10FFFF");
        SMT_REQUIRE(i == 0 || f > t->run_last[i - 1], "runs must be sorted and disjoint");
        SMT_REQUIRE(stride >= 1, "a run with stride 0");
        const int64_t lo = (int64_t)f + delta, hi = (int64_t)(f + (l - f) / stride * stride) + delta;   // the first and the last target
        SMT_REQUIRE(lo >= 0 && hi <= 0x10FFFF, "a run's delta leaves [0, U+10FFFF]");
        if (hi >= 0xD800 && lo <= 0xDFFF) {
            const int64_t k = lo >= 0xD800 ? 0 : (0xD800 - lo + stride - 1) / stride;   // the first target at or behind U+D800
            SMT_REQUIRE(lo + k * (int64_t)stride > 0xDFFF, "a run's delta lands on a surrogate");
        }
        if (f < 0x800u && delta > 0) {   // a two-byte code point may become three bytes, not four
            const uint32_t l2 = std::min<uint32_t>(l, 0x7FFu);
            SMT_REQUIRE((int64_t)(f + (l2 - f) / stride * stride) + delta < 0x10000, "a run maps two bytes to four (a line grows by half at most)");
        }
    }
    SMT_REQUIRE(t->n_multi == 0 || (t->multi_cp && t->multi_n && t->multi_to), "multi arrays");
    SMT_REQUIRE(t->n_multi <= smt::LOWER_MAX_MULTI, "more multi entries than the device form holds");
    for (uint64_t i = 0; i < t->n_multi; ++i) {
        const uint32_t cp = t->multi_cp[i], n = t->multi_n[i];
        SMT_REQUIRE(cp >= 0x80u, "a table entry below U+0080: ASCII is fixed");
        SMT_REQUIRE(cp <= 0x10FFFFu && !is_surrogate(cp), "a multi code point that is none");
        SMT_REQUIRE(i == 0 || cp > t->multi_cp[i - 1], "multi entries must be sorted and distinct");
        SMT_REQUIRE(n >= 1 && n <= 3, "a multi entry with n outside 1 .. 3");
        uint32_t bytes = 0;
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t to = t->multi_to[i * 3 + k];
            SMT_REQUIRE(to <= 0x10FFFFu && !is_surrogate(to), "a multi entry with an invalid target");
            bytes += utf8_bytes(to);
        }
        SMT_REQUIRE(bytes <= utf8_bytes(cp) + utf8_bytes(cp) / 2, "a multi entry grows its code point by more than half its bytes");
        for (uint64_t r = 0; r < t->n_runs; ++r)
            SMT_REQUIRE(cp < t->run_first[r] || cp > t->run_last[r], "a multi code point that also lies in a run");
    }
    int rc = check_ranges(t->cased_first, t->cased_last, t->n_cased, smt::LOWER_MAX_CASED);
    if (rc) return rc;
    return check_ranges(t->ignorable_first, t->ignorable_last, t->n_ignorable, smt::LOWER_MAX_IGNORABLE);
}

// Rust's str::to_lowercase: the arrays of host/unicode_lower.h without their ASCII entries (ASCII is fixed in the kernels)
struct BuiltinTables {
    std::vector<uint32_t> run_first, run_last, run_stride, multi_cp, multi_n, multi_to, cased_first, cased_last, ign_first, ign_last;
    std::vector<int32_t> run_delta;
    smt_lower_tables t;
    BuiltinTables()
    {
        namespace u = semtools::unicode;
        for (const u::LowerRun &r : u::LOWER_RUNS) {
            run_first.push_back(r.first);
            run_last.push_back(r.last);
            run_delta.push_back(r.delta);
            run_stride.push_back(r.stride);
        }
        for (const u::LowerMulti &m : u::LOWER_MULTI) {
            multi_cp.push_back(m.cp);
            multi_n.push_back(m.n);
            for (int k = 0; k < 3; ++k) multi_to.push_back(m.to[k]);
        }
        for (const u::CpRange &r : u::CASED)
            if (r.first >= 0x80) { cased_first.push_back(r.first); cased_last.push_back(r.last); }
        for (const u::CpRange &r : u::CASE_IGNORABLE)
            if (r.first >= 0x80) { ign_first.push_back(r.first); ign_last.push_back(r.last); }
        t.run_first = run_first.data();
        t.run_last = run_last.data();
        t.run_delta = run_delta.data();
        t.run_stride = run_stride.data();
        t.n_runs = run_first.size();
        t.multi_cp = multi_cp.data();
        t.multi_n = multi_n.data();
        t.multi_to = multi_to.data();
        t.n_multi = multi_cp.size();
        t.cased_first = cased_first.data();
        t.cased_last = cased_last.data();
        t.n_cased = cased_first.size();
        t.ignorable_first = ign_first.data();
        t.ignorable_last = ign_last.data();
        t.n_ignorable = ign_first.size();
        t.final_sigma = 1;
    }
};

int lower_create(smt_ctx *ctx, const smt_lower_tables *t, smt_lower **out)
{
    SMT_REQUIRE(out != nullptr, "null argument");
    *out = nullptr;
    std::unique_ptr<BuiltinTables> own;
    if (!t) {
        own.reset(new BuiltinTables());
        t = &own->t;
    }
    int rc = tables_check(t);   // (validated before anything is uploaded)
    if (rc) return rc;
    if ((rc = smt::bind_device(ctx))) return rc;
    std::vector<uint32_t> runs, multi, cased, ign;
    for (uint64_t i = 0; i < t->n_runs; ++i) {
        runs.push_back(t->run_first[i]);
        runs.push_back(t->run_last[i]);
        runs.push_back((uint32_t)t->run_delta[i]);
        runs.push_back(t->run_stride[i]);
    }
    for (uint64_t i = 0; i < t->n_multi; ++i) {
        multi.push_back(t->multi_cp[i]);
        multi.push_back(t->multi_n[i]);
        for (uint32_t k = 0; k < 3; ++k) multi.push_back(k < t->multi_n[i] ? t->multi_to[i * 3 + k] : 0u);
    }
    for (uint64_t i = 0; i < t->n_cased; ++i) { cased.push_back(t->cased_first[i]); cased.push_back(t->cased_last[i]); }
    for (uint64_t i = 0; i < t->n_ignorable; ++i) { ign.push_back(t->ignorable_first[i]); ign.push_back(t->ignorable_last[i]); }
    std::unique_ptr<smt_lower> h(new smt_lower());
    h->ctx = ctx;
    const uint8_t *at[4];
    if ((rc = smt::tok_upload_table("lower-casing",
                                    {{runs.data(), runs.size() * 4}, {multi.data(), multi.size() * 4}, {cased.data(), cased.size() * 4},
                                     {ign.data(), ign.size() * 4}},
                                    &h->d_table, at)))
        return rc;
    h->T.runs = reinterpret_cast<const uint4 *>(at[0]);
    h->T.multi = reinterpret_cast<const uint32_t *>(at[1]);
    h->T.cased = reinterpret_cast<const uint2 *>(at[2]);
    h->T.ignorable = reinterpret_cast<const uint2 *>(at[3]);
    h->T.n_runs = (uint32_t)t->n_runs;
    h->T.n_multi = (uint32_t)t->n_multi;
    h->T.n_cased = (uint32_t)t->n_cased;
    h->T.n_ignorable = (uint32_t)t->n_ignorable;
    h->T.final_sigma = t->final_sigma;
    *out = h.release();
    return SMT_OK;
}

int lower_device(smt_lower *h, const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev, const uint32_t *line_len_dev,
                 uint64_t n_lines, uint8_t *out_text_dev, uint64_t out_cap, uint64_t *out_begin_dev, uint32_t *out_len_dev, uint8_t *flags_dev,
                 uint32_t *n_flagged_dev)
{
    SMT_REQUIRE(n_flagged_dev != nullptr && out_begin_dev != nullptr, "null argument");
    SMT_REQUIRE(n_lines == 0 || (line_begin_dev && line_len_dev && out_len_dev && flags_dev), "null argument");
    SMT_REQUIRE(text_bytes == 0 || text_dev != nullptr, "text_dev");
    SMT_REQUIRE(text_bytes <= (1ull << 32), "at most 4 GiB of text per call");
    SMT_REQUIRE(n_lines <= (1ull << 32), "at most 2^32 lines per call");
    SMT_REQUIRE(out_cap >= text_bytes + text_bytes / 2, "out_cap is below text_bytes + text_bytes / 2");
    SMT_REQUIRE(out_cap == 0 || out_text_dev != nullptr, "out_text_dev");
    smt_ctx *ctx = h->ctx;
    int rc = smt::bind_device(ctx);
    if (rc) return rc;
    const uint64_t blocks = n_lines ? (text_bytes + LOWER_THREADS - 1) / LOWER_THREADS : 0;
    if (blocks > h->blocks_cap) {
        SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // earlier kernels may still read the old buffer
        if (h->d_blocks) SMT_HIP_CHECK(hipFree(h->d_blocks));
        h->d_blocks = nullptr;
        h->blocks_cap = 0;
        const size_t bytes = ((size_t)blocks + 1) * 8 + (size_t)blocks * 4;
        const hipError_t e = hipMalloc(&h->d_blocks, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            h->d_blocks = nullptr;
            smt::set_error("hipMalloc(%zu) for lower-casing block sums: %s", bytes, hipGetErrorString(e));
            return SMT_E_NOMEM;
        }
        h->blocks_cap = blocks;
    }
    hipStream_t st = ctx->stream;
    SMT_HIP_CHECK(hipMemsetAsync(n_flagged_dev, 0, sizeof(uint32_t), st));
    if (n_lines) {
        SMT_HIP_CHECK(hipMemsetAsync(flags_dev, 0, n_lines, st));
        SMT_HIP_CHECK(hipMemsetAsync(out_len_dev, 0, (size_t)n_lines * 4, st));
    }
    const auto launches = [&]() -> int {
        if (blocks) {
            const dim3 grid((unsigned)blocks), block(LOWER_THREADS);
            hipLaunchKernelGGL(lower_flag_kernel, grid, block, 0, st, text_dev, text_bytes, line_begin_dev, line_len_dev, n_lines, flags_dev);
            hipLaunchKernelGGL(lower_pass_kernel<false>, grid, block, 0, st, h->T, text_dev, text_bytes, line_begin_dev, line_len_dev, n_lines, flags_dev,
                               h->block_total(), out_len_dev, n_flagged_dev, nullptr, nullptr, 0);
            SMT_HIP_CHECK(hipGetLastError());
            if ((rc = smt::tok_exscan(ctx, h->block_total(), blocks, h->block_base()))) return rc;
        }
        if ((rc = smt::tok_exscan(ctx, out_len_dev, n_lines, out_begin_dev))) return rc;
        if (blocks) {
            hipLaunchKernelGGL(lower_pass_kernel<true>, dim3((unsigned)blocks), dim3(LOWER_THREADS), 0, st, h->T, text_dev, text_bytes, line_begin_dev,
                               line_len_dev, n_lines, flags_dev, nullptr, nullptr, nullptr, h->block_base(), out_text_dev, out_cap);
            SMT_HIP_CHECK(hipGetLastError());
        }
        return SMT_OK;
    };
    smt::prof_begin(ctx, "lower");
    rc = launches();
    smt::prof_end(ctx, "lower");   // (on every path: an event pair left open would be read as a running one)
    return rc;
}

int lower_host(smt_lower *h, const char *text, const uint64_t *line_begin, const uint32_t *line_len, uint64_t n_lines, char *out_text, uint64_t out_cap,
               uint64_t *out_begin, uint32_t *out_len, uint8_t *flags_out)
{
    SMT_REQUIRE(out_begin != nullptr, "out_begin");
    SMT_REQUIRE(n_lines == 0 || (line_begin && line_len && out_len), "null argument");
    uint64_t text_bytes = 0;
    for (uint64_t i = 0; i < n_lines; ++i) {
        SMT_REQUIRE(line_begin[i] >= text_bytes, "lines must lie in line order and must not overlap");
        text_bytes = line_begin[i] + line_len[i];
    }
    SMT_REQUIRE(text_bytes == 0 || text != nullptr, "text");
    SMT_REQUIRE(out_cap >= text_bytes + text_bytes / 2, "out_cap is below text_bytes + text_bytes / 2");
    SMT_REQUIRE(out_cap == 0 || out_text != nullptr, "out_text");
    smt_ctx *ctx = h->ctx;
    int rc = smt::bind_device(ctx);
    if (rc) return rc;
    const size_t o_begin = 0, o_obegin = o_begin + up16((size_t)n_lines * 8 + 8), o_len = o_obegin + up16(((size_t)n_lines + 1) * 8),
                 o_olen = o_len + up16((size_t)n_lines * 4 + 4), o_nflag = o_olen + up16((size_t)n_lines * 4 + 4), o_flags = o_nflag + 16,
                 o_text = o_flags + up16((size_t)n_lines + 1), o_out = o_text + up16((size_t)text_bytes + 1),
                 total = o_out + up16((size_t)out_cap + 1);
    struct Temp { void *p = nullptr; ~Temp() { if (p) (void)hipFree(p); } } tmp;
    {
        const hipError_t e = hipMalloc(&tmp.p, total);
        if (e != hipSuccess) { (void)hipGetLastError(); smt::set_error("hipMalloc(%zu) for lower-casing staging: %s", total, hipGetErrorString(e)); return SMT_E_NOMEM; }
    }
    char *d = static_cast<char *>(tmp.p);
    hipStream_t st = ctx->stream;
    if (n_lines) {
        SMT_HIP_CHECK(hipMemcpyAsync(d + o_begin, line_begin, (size_t)n_lines * 8, hipMemcpyHostToDevice, st));
        SMT_HIP_CHECK(hipMemcpyAsync(d + o_len, line_len, (size_t)n_lines * 4, hipMemcpyHostToDevice, st));
    }
    if (text_bytes) SMT_HIP_CHECK(hipMemcpyAsync(d + o_text, text, (size_t)text_bytes, hipMemcpyHostToDevice, st));
    if ((rc = lower_device(h, reinterpret_cast<const uint8_t *>(d + o_text), text_bytes, reinterpret_cast<const uint64_t *>(d + o_begin),
                           reinterpret_cast<const uint32_t *>(d + o_len), n_lines, reinterpret_cast<uint8_t *>(d + o_out), out_cap,
                           reinterpret_cast<uint64_t *>(d + o_obegin), reinterpret_cast<uint32_t *>(d + o_olen),
                           reinterpret_cast<uint8_t *>(d + o_flags), reinterpret_cast<uint32_t *>(d + o_nflag)))) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    SMT_HIP_CHECK(hipMemcpyAsync(out_begin, d + o_obegin, ((size_t)n_lines + 1) * 8, hipMemcpyDeviceToHost, st));
    if (n_lines) SMT_HIP_CHECK(hipMemcpyAsync(out_len, d + o_olen, (size_t)n_lines * 4, hipMemcpyDeviceToHost, st));
    if (flags_out && n_lines) SMT_HIP_CHECK(hipMemcpyAsync(flags_out, d + o_flags, (size_t)n_lines, hipMemcpyDeviceToHost, st));
    SMT_HIP_CHECK(hipStreamSynchronize(st));
    const uint64_t n_out = out_begin[n_lines];
    if (n_out > out_cap) { smt::set_error("lower-casing produced more bytes than out_cap"); return SMT_E_HIP; }
    if (n_out) SMT_HIP_CHECK(hipMemcpy(out_text, d + o_out, (size_t)n_out, hipMemcpyDeviceToHost));
    return SMT_OK;
}

}  // namespace

extern "C" {

int smt_lower_tables_check(const smt_lower_tables *t)
try {
    if (!t) {
        const BuiltinTables own;
        return tables_check(&own.t);
    }
    return tables_check(t);
} catch (...) { return smt::api_catch(); }

int smt_lower_create(smt_ctx *ctx, const smt_lower_tables *t, smt_lower **out)
try {
    if (!ctx) return smt::tok_null_handle("smt_lower_create");
    return lower_create(ctx, t, out);
} catch (...) { return smt::api_catch(); }

void smt_lower_destroy(smt_lower *h)
{
    if (!h) return;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    if (h->d_table) (void)hipFree(h->d_table);
    if (h->d_blocks) (void)hipFree(h->d_blocks);
    delete h;
}

int smt_lower_device(smt_lower *h, const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev, const uint32_t *line_len_dev,
                     uint64_t n_lines, uint8_t *out_text_dev, uint64_t out_cap, uint64_t *out_begin_dev, uint32_t *out_len_dev, uint8_t *flags_dev,
                     uint32_t *n_flagged_dev)
try {
    if (!h) return smt::tok_null_handle("smt_lower_device");
    return lower_device(h, text_dev, text_bytes, line_begin_dev, line_len_dev, n_lines, out_text_dev, out_cap, out_begin_dev, out_len_dev, flags_dev,
                        n_flagged_dev);
} catch (...) { return smt::api_catch(); }

int smt_lower_lines(smt_lower *h, const char *text, const uint64_t *line_begin, const uint32_t *line_len, uint64_t n_lines, char *out_text,
              uint64_t out_cap, uint64_t *out_begin, uint32_t *out_len, uint8_t *flags_out)
try {
    if (!h) return smt::tok_null_handle("smt_lower_lines");
    return lower_host(h, text, line_begin, line_len, n_lines, out_text, out_cap, out_begin, out_len, flags_out);
} catch (...) { return smt::api_catch(); }

}  // extern "C"
