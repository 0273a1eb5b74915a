// tokenize_kernels.hip -- WordPiece over pure-ASCII lines on the device: the byte rules of hf_tokenizer.cpp's
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
// ORDER.  Pass 2 is then a prefix sum over the slots: rank of a slot among the used slots minus the rank at its line's start is
// the token's place in its line; lines are laid out by a prefix sum of their (capped, or patched) counts.
//
// Every loop is bounded: probes by the table's capacity, a word's pieces by max_input_chars_per_word, a walk by the line's end.
#include <algorithm>
#include <string>
#include <vector>

#include "common.h"
#include "tokenize_pass2.h"
#include "wordpiece_bytes.h"

namespace {

constexpr uint32_t WP_NONE = smt::TOK_NONE;   // an ids_tmp slot that holds no token
constexpr unsigned SCAN_THREADS = 256;        // pass 1: one position per thread
constexpr unsigned EMIT_THREADS = smt::TOK_EMIT_THREADS;   // pass 2: four slots per thread
constexpr unsigned EMIT_CHUNK = smt::TOK_EMIT_CHUNK;

struct WpTable {
    const unsigned long long *slots;   // (tag << 32) | entry + 1; 0 = empty
    const uint4 *ent;                  // {pool offset of the piece, its length, its id, 1 = continuing piece}
    const uint8_t *pool;
    const uint8_t *bytes;              // cls[128] | nrm[128]
    const uint8_t *added_pool;
    const uint32_t *added_off;
    uint32_t mask;                     // capacity - 1
    uint32_t prefix_len;
    uint32_t max_piece;                // longest piece, in bytes: no match can be longer
    uint32_t max_chars;
    uint32_t n_added;
    uint32_t unk;                      // WP_NONE: none
    unsigned long long prefix_state;   // the hash after the continuing prefix
    unsigned long long added_first[2]; // bit c: an added token starts with byte c
};

// the number of i in [0, hi) with begin[i] <= p, given that every i < lo has
__device__ __forceinline__ uint64_t count_le(const uint64_t *__restrict__ begin, uint64_t lo, uint64_t hi, uint64_t p)
{
    for (int step = 0; step < 64 && lo < hi; ++step) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (begin[mid] <= p) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

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
    const uint64_t first = (uint64_t)blockIdx.x * SCAN_THREADS;
    if (threadIdx.x < 2) {
        const uint64_t last = first + SCAN_THREADS - 1 < text_bytes ? first + SCAN_THREADS - 1 : text_bytes - 1;
        const uint64_t at = threadIdx.x == 0 ? first : last;
        s_win[threadIdx.x] = count_le(line_begin, 0, n_lines, at);
    }
    __syncthreads();
    const uint8_t *cls = s_bytes, *nrm = s_bytes + 128;
    const uint64_t p = first + threadIdx.x;
    if (p >= text_bytes) return;
    const uint64_t n_le = count_le(line_begin, s_win[0], s_win[1], p);
    if (n_le == 0) return;                       // in front of the first line
    const uint64_t line = n_le - 1;
    const uint64_t lb = line_begin[line];
    const uint32_t ll = line_len[line];
    const uint64_t le_line = lb + (keep_bytes && keep_bytes < ll ? keep_bytes : ll);
    const uint64_t le = le_line < text_bytes ? le_line : text_bytes;   // the end of what is looked at
    if (p < lb || p >= le) return;               // behind the cut, or between two lines
    const uint8_t c = text[p];
    if (c >= 0x80) { flags[line] = 1; return; }
    if (((c < 64 ? T.added_first[0] : T.added_first[1]) >> (c & 63)) & 1) {
        for (uint32_t t = 0; t < T.n_added; ++t) {
            const uint32_t a = T.added_off[t], tl = T.added_off[t + 1] - a;
            if (tl == 0 || p + tl > le) continue;
            bool same = true;
            for (uint32_t j = 0; j < tl && same; ++j) same = text[p + j] == T.added_pool[a + j];
            if (same) { flags[line] = 1; break; }
        }
    }
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
        unsigned long long h = kind ? T.prefix_state : smt::WP_HASH_SEED;
        const uint32_t longest = kind ? T.max_piece - T.prefix_len : T.max_piece;
        uint32_t hit = WP_NONE, clen = 0;
        uint64_t hit_end = s;
        for (uint64_t q = s; q < we && clen < longest;) {
            const uint8_t b = text[q++];
            if (cls[b] == smt::WP_DROPPED) continue;
            h = (h ^ nrm[b]) * smt::WP_HASH_MUL;
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

__global__ void __launch_bounds__(256) wp_lines_kernel(uint64_t n_lines, const uint32_t *__restrict__ raw_count, const uint8_t *__restrict__ flags,
                                                       uint32_t max_tokens, uint32_t *__restrict__ counts, uint32_t *__restrict__ n_flagged)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_lines) return;
    const bool f = flags[i] != 0;
    const uint32_t r = raw_count[i];
    counts[i] = f ? 0 : (max_tokens && r > max_tokens ? max_tokens : r);
    if (f) atomicAdd(n_flagged, 1u);
}

__global__ void __launch_bounds__(256) wp_patch_counts_kernel(uint64_t n_patch, uint64_t n_lines, const uint64_t *__restrict__ patch_line,
                                                              const uint64_t *__restrict__ patch_off, const uint8_t *__restrict__ flags,
                                                              uint32_t *__restrict__ final_count)
{
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_patch) return;
    const uint64_t line = patch_line[j];
    if (line < n_lines && flags[line] && patch_off[j + 1] >= patch_off[j]) final_count[line] = (uint32_t)(patch_off[j + 1] - patch_off[j]);
}

// out[i] = in[0] + ... + in[i - 1] for i in [0, n]: one block, 4096 entries a round
__global__ void __launch_bounds__(1024) wp_exscan_kernel(const uint32_t *__restrict__ in, uint64_t n, uint64_t *__restrict__ out)
{
    __shared__ unsigned long long wsum[16];
    const unsigned t = threadIdx.x, lane = t & 63, w = t >> 6;
    unsigned long long carry = 0;
    for (uint64_t base = 0; base < n; base += 4096) {
        const uint64_t i0 = base + (uint64_t)t * 4;
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = i0 + k < n ? in[i0 + k] : 0;
        const unsigned long long sum = (unsigned long long)v[0] + v[1] + v[2] + v[3];
        unsigned long long inc = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long o = __shfl_up(inc, d);
            if ((int)lane >= d) inc += o;
        }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        unsigned long long wbase = 0, total = 0;
#pragma unroll
        for (unsigned j = 0; j < 16; ++j) {
            const unsigned long long x = wsum[j];
            if (j < w) wbase += x;
            total += x;
        }
        unsigned long long ex = carry + wbase + inc - sum;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + k < n) { out[i0 + k] = ex; ex += v[k]; }
        carry += total;
        __syncthreads();
    }
    if (t == 0) out[n] = carry;
}

__device__ __forceinline__ uint32_t used4(const uint4 v) { return (v.x != WP_NONE) + (v.y != WP_NONE) + (v.z != WP_NONE) + (v.w != WP_NONE); }

// used slots per chunk of EMIT_CHUNK positions (ids_tmp is padded to whole chunks with empty slots)
__global__ void __launch_bounds__(EMIT_THREADS) wp_chunk_count_kernel(const uint4 *__restrict__ ids_tmp4, uint32_t *__restrict__ chunk_count)
{
    __shared__ uint32_t wsum[EMIT_THREADS / 64];
    uint32_t c = used4(ids_tmp4[(uint64_t)blockIdx.x * EMIT_THREADS + threadIdx.x]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) chunk_count[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ void __launch_bounds__(EMIT_THREADS) wp_emit_kernel(const uint4 *__restrict__ ids_tmp4, uint64_t text_bytes,
                                                               const uint64_t *__restrict__ chunk_base, const uint64_t *__restrict__ line_begin,
                                                               uint64_t n_lines, const uint64_t *__restrict__ raw_base,
                                                               const uint8_t *__restrict__ flags, const uint32_t *__restrict__ final_count,
                                                               const uint64_t *__restrict__ offsets, uint32_t *__restrict__ ids_out, uint64_t ids_cap)
{
    __shared__ uint32_t wsum[EMIT_THREADS / 64];
    __shared__ uint64_t s_win[2];
    const unsigned t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint64_t first = (uint64_t)blockIdx.x * EMIT_CHUNK;
    if (t < 2) s_win[t] = count_le(line_begin, 0, n_lines, t == 0 ? first : (first + EMIT_CHUNK - 1 < text_bytes ? first + EMIT_CHUNK - 1 : text_bytes - 1));
    const uint4 v = ids_tmp4[(uint64_t)blockIdx.x * EMIT_THREADS + t];
    const uint32_t c = used4(v);
    uint32_t inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if ((int)lane >= d) inc += o;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    if (c == 0) return;
    uint32_t wbase = 0;
#pragma unroll
    for (unsigned j = 0; j < EMIT_THREADS / 64; ++j) wbase += j < w ? wsum[j] : 0;
    uint64_t g = chunk_base[blockIdx.x] + wbase + inc - c;   // used slots in front of this thread's first one
    const uint32_t id[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (id[k] == WP_NONE) continue;
        const uint64_t n_le = count_le(line_begin, s_win[0], s_win[1], first + t * 4 + k);
        if (n_le) {
            const uint64_t line = n_le - 1;
            const uint64_t r = g - raw_base[line];           // the token's place in its line
            const uint64_t at = offsets[line] + r;
            if (!flags[line] && r < final_count[line] && at < ids_cap) ids_out[at] = id[k];
        }
        ++g;
    }
}

// one block per patched line (grid-stride): its ids to their place
__global__ void __launch_bounds__(256) wp_patch_copy_kernel(uint64_t n_patch, uint64_t n_lines, const uint64_t *__restrict__ patch_line,
                                                            const uint64_t *__restrict__ patch_off, const uint32_t *__restrict__ patch_ids,
                                                            uint64_t n_patch_ids, const uint8_t *__restrict__ flags, const uint64_t *__restrict__ offsets,
                                                            uint32_t *__restrict__ ids_out, uint64_t ids_cap)
{
    for (uint64_t j = blockIdx.x; j < n_patch; j += gridDim.x) {
        const uint64_t line = patch_line[j];
        if (line >= n_lines || !flags[line]) continue;
        const uint64_t b = patch_off[j], e = patch_off[j + 1];
        if (e < b || e > n_patch_ids) continue;
        const uint64_t at = offsets[line];
        for (uint64_t i = threadIdx.x; i < e - b; i += 256)
            if (at + i < ids_cap) ids_out[at + i] = patch_ids[b + i];
    }
}

}  // namespace

struct smt_wordpiece {
    smt_ctx *ctx = nullptr;
    void *d_table = nullptr;          // slots | entries | pool | byte tables | added pool | added offsets
    WpTable T{};
    // the state of the last scan
    smt::TokScratch S;
    bool scanned = false;
    uint64_t text_bytes = 0, n_lines = 0, ids_bound = 0;
    const uint64_t *line_begin = nullptr;
    const uint32_t *counts = nullptr;
    const uint8_t *flags = nullptr;
};

namespace smt {

// a compute entry point handed a null handle: on a machine without a device that is what every caller ends up with
int tok_null_handle(const char *what)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        set_error("%s: no HIP device visible: libsemtools_hip has no CPU fallback", what);
        return SMT_E_HIP;
    }
    set_error("invalid argument: %s (null handle)", what);
    return SMT_E_INVALID;
}

static int null_handle(const char *what) { return tok_null_handle(what); }

static int grow(smt_ctx *ctx, void **p, size_t bytes, const char *what)
{
    SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // earlier kernels may still read the old buffer
    if (*p) SMT_HIP_CHECK(hipFree(*p));
    *p = nullptr;
    const hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); *p = nullptr; set_error("hipMalloc(%zu) for %s: %s", bytes, what, hipGetErrorString(e)); return SMT_E_NOMEM; }
    return SMT_OK;
}

static uint64_t hash_bytes(const char *b, size_t n, uint64_t h = WP_HASH_SEED)
{
    for (size_t i = 0; i < n; ++i) h = (h ^ (uint8_t)b[i]) * WP_HASH_MUL;
    return h;
}

void tok_build_table(const char *pool, const std::vector<TokEntry> &in, TokTable &out)
{
    uint32_t cap = 16;
    while ((uint64_t)cap < 2 * (uint64_t)in.size()) cap <<= 1;
    const uint32_t mask = cap - 1;
    out.mask = mask;
    out.slots.assign(cap, 0);
    out.ents.clear();
    out.winner.clear();
    out.ents.reserve(in.size());
    out.winner.reserve(in.size());
    for (const TokEntry &e : in) {
        uint32_t idx = (uint32_t)e.h & mask;
        const uint32_t tag = (uint32_t)(e.h >> 32);
        for (;;) {
            const unsigned long long s = out.slots[idx];
            if (s == 0) {
                out.ents.push_back(make_uint4(e.off, e.len, e.id, e.kind));
                out.winner.push_back(e.src);
                out.slots[idx] = ((unsigned long long)tag << 32) | (unsigned long long)out.ents.size();
                break;
            }
            uint4 &o = out.ents[(uint32_t)s - 1];
            if ((uint32_t)(s >> 32) == tag && o.w == e.kind && o.y == e.len && memcmp(pool + o.x, pool + e.off, e.len) == 0) {
                o.z = e.id;   // a repeated piece: the later entry wins
                out.winner[(uint32_t)s - 1] = e.src;
                break;
            }
            idx = (idx + 1) & mask;   // (load <= 0.5: an empty slot exists)
        }
    }
}

int tok_scratch_reserve(smt_ctx *ctx, TokScratch &s, uint64_t n_slots, uint64_t n_lines)
{
    int rc;
    const uint64_t chunks = TokScratch::chunks_of(n_slots);
    if (chunks * EMIT_CHUNK > s.slots_cap) {
        s.slots_cap = 0;
        if ((rc = grow(ctx, reinterpret_cast<void **>(&s.d_ids_tmp), (size_t)chunks * EMIT_CHUNK * 4, "tokenizer id slots"))) return rc;
        s.slots_cap = chunks * EMIT_CHUNK;
    }
    if (chunks > s.chunks_cap) {
        s.chunks_cap = 0;
        if ((rc = grow(ctx, &s.d_chunks, (size_t)chunks * 4 + ((size_t)chunks + 1) * 8 + 8, "tokenizer chunk sums"))) return rc;
        s.chunks_cap = chunks + (chunks & 1);   // (keeps the u64 part 8-byte aligned)
    }
    if (n_lines > s.lines_cap) {
        s.lines_cap = 0;
        if ((rc = grow(ctx, &s.d_lines, (size_t)n_lines * 8 + ((size_t)n_lines + 1) * 8 + (size_t)n_lines * 8, "tokenizer line sums"))) return rc;
        s.lines_cap = n_lines;
    }
    return SMT_OK;
}

int tok_scratch_clear(smt_ctx *ctx, TokScratch &s, uint64_t n_slots, uint64_t n_lines)
{
    const uint64_t chunks = TokScratch::chunks_of(n_slots);
    if (n_lines) SMT_HIP_CHECK(hipMemsetAsync(s.raw_count(), 0, (size_t)n_lines * 4, ctx->stream));
    if (chunks) SMT_HIP_CHECK(hipMemsetAsync(s.d_ids_tmp, 0xFF, (size_t)chunks * EMIT_CHUNK * 4, ctx->stream));
    return SMT_OK;
}

void tok_scratch_free(TokScratch &s)
{
    if (s.d_ids_tmp) (void)hipFree(s.d_ids_tmp);
    if (s.d_lines) (void)hipFree(s.d_lines);
    if (s.d_chunks) (void)hipFree(s.d_chunks);
    s = TokScratch();
}

int tok_line_counts(smt_ctx *ctx, const TokScratch &s, uint64_t n_lines, const uint8_t *flags_dev, uint32_t max_tokens, uint32_t *counts_dev,
                    uint32_t *n_flagged_dev)
{
    if (!n_lines) return SMT_OK;
    hipLaunchKernelGGL(wp_lines_kernel, dim3((unsigned)((n_lines + 255) / 256)), dim3(256), 0, ctx->stream, n_lines, s.raw_count(), flags_dev,
                       max_tokens, counts_dev, n_flagged_dev);
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

int tok_pass2(smt_ctx *ctx, const TokScratch &s, uint64_t n_slots, const uint64_t *slot_begin_dev, uint64_t n_lines, const uint32_t *counts_dev,
              const uint8_t *flags_dev, const uint64_t *patch_line_dev, const uint64_t *patch_off_dev, const uint32_t *patch_ids_dev,
              uint64_t n_patch, uint64_t n_patch_ids, uint32_t *ids_out_dev, uint64_t ids_cap, uint64_t *offsets_out_dev)
{
    hipStream_t st = ctx->stream;
    if (n_lines) SMT_HIP_CHECK(hipMemcpyAsync(s.final_count(), counts_dev, (size_t)n_lines * 4, hipMemcpyDeviceToDevice, st));
    if (n_patch) {
        hipLaunchKernelGGL(wp_patch_counts_kernel, dim3((unsigned)((n_patch + 255) / 256)), dim3(256), 0, st, n_patch, n_lines, patch_line_dev,
                           patch_off_dev, flags_dev, s.final_count());
        SMT_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(wp_exscan_kernel, dim3(1), dim3(1024), 0, st, s.final_count(), n_lines, offsets_out_dev);
    SMT_HIP_CHECK(hipGetLastError());
    const uint64_t chunks = TokScratch::chunks_of(n_slots);
    if (n_lines && chunks) {
        hipLaunchKernelGGL(wp_exscan_kernel, dim3(1), dim3(1024), 0, st, s.raw_count(), n_lines, s.raw_base());
        hipLaunchKernelGGL(wp_chunk_count_kernel, dim3((unsigned)chunks), dim3(EMIT_THREADS), 0, st, reinterpret_cast<const uint4 *>(s.d_ids_tmp),
                           s.chunk_count());
        hipLaunchKernelGGL(wp_exscan_kernel, dim3(1), dim3(1024), 0, st, s.chunk_count(), chunks, s.chunk_base());
        hipLaunchKernelGGL(wp_emit_kernel, dim3((unsigned)chunks), dim3(EMIT_THREADS), 0, st, reinterpret_cast<const uint4 *>(s.d_ids_tmp), n_slots,
                           s.chunk_base(), slot_begin_dev, n_lines, s.raw_base(), flags_dev, s.final_count(), offsets_out_dev, ids_out_dev, ids_cap);
        SMT_HIP_CHECK(hipGetLastError());
    }
    if (n_patch) {
        hipLaunchKernelGGL(wp_patch_copy_kernel, dim3((unsigned)std::min<uint64_t>(n_patch, 65536)), dim3(256), 0, st, n_patch, n_lines,
                           patch_line_dev, patch_off_dev, patch_ids_dev, n_patch_ids, flags_dev, offsets_out_dev, ids_out_dev, ids_cap);
        SMT_HIP_CHECK(hipGetLastError());
    }
    return SMT_OK;
}

}  // namespace smt

using namespace smt;

extern "C" {

int smt_wordpiece_create(smt_ctx *ctx, const smt_wordpiece_params *p, smt_wordpiece **out)
try {
    if (!ctx) return null_handle("smt_wordpiece_create");
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
    int rc = bind_device(ctx);
    if (rc) return rc;

    // ---- entries: every ASCII piece as a whole word; one that starts with the prefix and goes on, as a continuing piece too
    std::vector<TokEntry> ents;
    ents.reserve(p->n_pieces * 2);
    uint32_t max_piece = 0;
    const uint64_t prefix_state = hash_bytes(p->prefix, p->prefix_len);
    for (uint64_t i = 0; i < p->n_pieces; ++i) {
        const uint32_t off = p->piece_off[i], len = p->piece_off[i + 1] - off;
        if (len == 0) continue;
        bool ascii = true;
        for (uint32_t j = 0; j < len && ascii; ++j) ascii = (uint8_t)p->pool[off + j] < 0x80;
        if (!ascii) continue;
        const uint64_t h = hash_bytes(p->pool + off, len);
        max_piece = std::max(max_piece, len);
        ents.push_back({off, len, p->piece_id[i], 0, h, i});
        if (len > p->prefix_len && memcmp(p->pool + off, p->prefix, p->prefix_len) == 0) ents.push_back({off, len, p->piece_id[i], 1, h, i});
    }
    TokTable table;
    tok_build_table(p->pool, ents, table);
    const uint32_t cap = (uint32_t)table.slots.size(), mask = table.mask;
    const std::vector<unsigned long long> &slots = table.slots;
    const std::vector<uint4> &dev_ents = table.ents;
    const size_t pool_bytes = p->n_pieces ? p->piece_off[p->n_pieces] : 0;
    const size_t added_bytes = p->n_added ? p->added_off[p->n_added] : 0;
    uint8_t bytes[256];
    wordpiece_byte_table(p->flags, bytes, bytes + 128);
    unsigned long long added_first[2] = {0, 0};
    for (uint32_t t = 0; t < p->n_added; ++t) {
        const uint32_t a = p->added_off[t], tl = p->added_off[t + 1] - a;
        for (uint32_t j = 0; j < tl; ++j) SMT_REQUIRE((uint8_t)p->added_pool[a + j] < 0x80, "added tokens must be ASCII");
        if (tl) added_first[(uint8_t)p->added_pool[a] >> 6] |= 1ull << ((uint8_t)p->added_pool[a] & 63);
    }
    // ---- one blob, every part 16-byte aligned
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t o_slots = 0, o_ent = o_slots + up16((size_t)cap * 8), o_pool = o_ent + up16(dev_ents.size() * sizeof(uint4) + 16),
                 o_bytes = o_pool + up16(pool_bytes + 16), o_apool = o_bytes + 256, o_aoff = o_apool + up16(added_bytes + 16),
                 total = o_aoff + up16(((size_t)p->n_added + 1) * 4);
    std::vector<uint8_t> blob(total, 0);
    memcpy(blob.data() + o_slots, slots.data(), (size_t)cap * 8);
    if (!dev_ents.empty()) memcpy(blob.data() + o_ent, dev_ents.data(), dev_ents.size() * sizeof(uint4));
    if (pool_bytes) memcpy(blob.data() + o_pool, p->pool, pool_bytes);
    memcpy(blob.data() + o_bytes, bytes, 256);
    if (added_bytes) memcpy(blob.data() + o_apool, p->added_pool, added_bytes);
    if (p->n_added) memcpy(blob.data() + o_aoff, p->added_off, ((size_t)p->n_added + 1) * 4);

    smt_wordpiece *tok = new smt_wordpiece();
    tok->ctx = ctx;
    hipError_t e = hipMalloc(&tok->d_table, total);
    if (e == hipSuccess) e = hipMemcpy(tok->d_table, blob.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (tok->d_table) (void)hipFree(tok->d_table);
        delete tok;
        set_error("wordpiece table upload (%zu bytes): %s", total, hipGetErrorString(e));
        return SMT_E_NOMEM;
    }
    const uint8_t *base = static_cast<const uint8_t *>(tok->d_table);
    WpTable &T = tok->T;
    T.slots = reinterpret_cast<const unsigned long long *>(base + o_slots);
    T.ent = reinterpret_cast<const uint4 *>(base + o_ent);
    T.pool = base + o_pool;
    T.bytes = base + o_bytes;
    T.added_pool = base + o_apool;
    T.added_off = reinterpret_cast<const uint32_t *>(base + o_aoff);
    T.mask = mask;
    T.prefix_len = p->prefix_len;
    T.max_piece = std::max(max_piece, p->prefix_len);   // (max_piece - prefix_len must not wrap)
    T.max_chars = p->max_input_chars_per_word;
    T.n_added = p->n_added;
    T.unk = p->unk_id < 0 ? WP_NONE : (uint32_t)p->unk_id;
    T.prefix_state = prefix_state;
    T.added_first[0] = added_first[0];
    T.added_first[1] = added_first[1];
    *out = tok;
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

void smt_wordpiece_destroy(smt_wordpiece *tok)
{
    if (!tok) return;
    (void)hipSetDevice(tok->ctx->device);
    (void)hipStreamSynchronize(tok->ctx->stream);
    if (tok->d_table) (void)hipFree(tok->d_table);
    tok_scratch_free(tok->S);
    delete tok;
}

int smt_wordpiece_scan_device(smt_wordpiece *tok, const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev,
                              const uint32_t *line_len_dev, uint64_t n_lines, uint32_t keep_bytes, uint32_t max_tokens, int drop_unk,
                              uint32_t *counts_dev, uint8_t *flags_dev, uint32_t *n_flagged_dev)
try {
    if (!tok) return null_handle("smt_wordpiece_scan_device");
    SMT_REQUIRE(n_flagged_dev != nullptr, "n_flagged_dev");
    SMT_REQUIRE(n_lines == 0 || (line_begin_dev && line_len_dev && counts_dev && flags_dev), "null argument");
    SMT_REQUIRE(text_bytes == 0 || text_dev != nullptr, "text_dev");
    SMT_REQUIRE(text_bytes <= (1ull << 32), "at most 4 GiB of text per scan");
    SMT_REQUIRE(n_lines <= (1ull << 32), "at most 2^32 lines per scan");
    smt_ctx *ctx = tok->ctx;
    int rc = bind_device(ctx);
    if (rc) return rc;
    tok->scanned = false;
    if ((rc = tok_scratch_reserve(ctx, tok->S, text_bytes, n_lines))) return rc;
    hipStream_t st = ctx->stream;
    SMT_HIP_CHECK(hipMemsetAsync(n_flagged_dev, 0, sizeof(uint32_t), st));
    if (n_lines) SMT_HIP_CHECK(hipMemsetAsync(flags_dev, 0, n_lines, st));
    if ((rc = tok_scratch_clear(ctx, tok->S, text_bytes, n_lines))) return rc;
    prof_begin(ctx, "tokenize");
    if (n_lines && text_bytes) {
        hipLaunchKernelGGL(wp_scan_kernel, dim3((unsigned)((text_bytes + SCAN_THREADS - 1) / SCAN_THREADS)), dim3(SCAN_THREADS), 0, st, tok->T,
                           text_dev, text_bytes, line_begin_dev, line_len_dev, n_lines, keep_bytes, drop_unk, tok->S.d_ids_tmp, tok->S.raw_count(),
                           flags_dev);
        SMT_HIP_CHECK(hipGetLastError());
    }
    if ((rc = tok_line_counts(ctx, tok->S, n_lines, flags_dev, max_tokens, counts_dev, n_flagged_dev))) return rc;
    prof_end(ctx, "tokenize");
    tok->scanned = true;
    tok->text_bytes = text_bytes;
    tok->n_lines = n_lines;
    tok->ids_bound = keep_bytes ? std::min<uint64_t>(text_bytes, n_lines * (uint64_t)keep_bytes) : text_bytes;
    tok->line_begin = line_begin_dev;
    tok->counts = counts_dev;
    tok->flags = flags_dev;
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

int smt_wordpiece_emit_device(smt_wordpiece *tok, uint64_t n_lines, const uint64_t *patch_line_dev, const uint64_t *patch_off_dev,
                              const uint32_t *patch_ids_dev, uint64_t n_patch, uint64_t n_patch_ids, uint32_t *ids_out_dev, uint64_t ids_cap,
                              uint64_t *offsets_out_dev)
try {
    if (!tok) return null_handle("smt_wordpiece_emit_device");
    SMT_REQUIRE(tok->scanned, "no scan to emit (smt_wordpiece_scan_device comes first)");
    SMT_REQUIRE(n_lines == tok->n_lines, "n_lines differs from the scan's");
    SMT_REQUIRE(offsets_out_dev != nullptr, "offsets_out_dev");
    SMT_REQUIRE(n_patch == 0 || (patch_line_dev && patch_off_dev), "patch arrays");
    SMT_REQUIRE(n_patch <= n_lines, "more patched lines than lines");
    SMT_REQUIRE(n_patch_ids == 0 || (n_patch && patch_ids_dev), "patch ids");
    SMT_REQUIRE(n_patch_ids <= (1ull << 40), "patch ids");
    SMT_REQUIRE(ids_cap >= tok->ids_bound + n_patch_ids, "ids_cap is below the looked-at bytes of all lines + the patch ids");
    SMT_REQUIRE(ids_cap == 0 || ids_out_dev != nullptr, "ids_out_dev");
    smt_ctx *ctx = tok->ctx;
    int rc = bind_device(ctx);
    if (rc) return rc;
    prof_begin(ctx, "tokenize_emit");
    if ((rc = tok_pass2(ctx, tok->S, tok->text_bytes, tok->line_begin, n_lines, tok->counts, tok->flags, patch_line_dev, patch_off_dev, patch_ids_dev,
                        n_patch, n_patch_ids, ids_out_dev, ids_cap, offsets_out_dev)))
        return rc;
    prof_end(ctx, "tokenize_emit");
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

int smt_wordpiece_tokenize(smt_wordpiece *tok, const char *text, const uint64_t *line_begin, const uint32_t *line_len, uint64_t n_lines,
                           uint32_t keep_bytes, uint32_t max_tokens, int drop_unk, uint32_t *ids_out, uint64_t ids_cap,
                           uint64_t *offsets_out, uint8_t *flags_out)
try {
    if (!tok) return null_handle("smt_wordpiece_tokenize");
    SMT_REQUIRE(offsets_out != nullptr, "offsets_out");
    SMT_REQUIRE(n_lines == 0 || (line_begin && line_len), "null argument");
    uint64_t text_bytes = 0, looked = 0;
    for (uint64_t i = 0; i < n_lines; ++i) {
        SMT_REQUIRE(line_begin[i] >= text_bytes, "lines must lie in line order and must not overlap");
        text_bytes = line_begin[i] + line_len[i];
        looked += keep_bytes && keep_bytes < line_len[i] ? keep_bytes : line_len[i];
    }
    SMT_REQUIRE(text_bytes == 0 || text != nullptr, "text");
    SMT_REQUIRE(ids_cap >= looked, "ids_cap is below the looked-at bytes of all lines");
    SMT_REQUIRE(ids_cap == 0 || ids_out != nullptr, "ids_out");
    smt_ctx *ctx = tok->ctx;
    int rc = bind_device(ctx);
    if (rc) return rc;
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const uint64_t dev_cap = std::max<uint64_t>(ids_cap, text_bytes);   // (the device form's bound is the text's size)
    const size_t o_begin = 0, o_off = o_begin + up16((size_t)n_lines * 8 + 8), o_ids = o_off + up16(((size_t)n_lines + 1) * 8),
                 o_len = o_ids + up16((size_t)dev_cap * 4 + 4), o_counts = o_len + up16((size_t)n_lines * 4 + 4),
                 o_nflag = o_counts + up16((size_t)n_lines * 4 + 4), o_flags = o_nflag + 16, o_text = o_flags + up16((size_t)n_lines + 1),
                 total = o_text + up16((size_t)text_bytes + 1);
    struct Temp { void *p = nullptr; ~Temp() { if (p) (void)hipFree(p); } } tmp;
    {
        const hipError_t e = hipMalloc(&tmp.p, total);
        if (e != hipSuccess) { (void)hipGetLastError(); set_error("hipMalloc(%zu) for tokenizer staging: %s", total, hipGetErrorString(e)); return SMT_E_NOMEM; }
    }
    char *d = static_cast<char *>(tmp.p);
    hipStream_t st = ctx->stream;
    if (n_lines) {
        SMT_HIP_CHECK(hipMemcpyAsync(d + o_begin, line_begin, (size_t)n_lines * 8, hipMemcpyHostToDevice, st));
        SMT_HIP_CHECK(hipMemcpyAsync(d + o_len, line_len, (size_t)n_lines * 4, hipMemcpyHostToDevice, st));
    }
    if (text_bytes) SMT_HIP_CHECK(hipMemcpyAsync(d + o_text, text, (size_t)text_bytes, hipMemcpyHostToDevice, st));
    uint8_t *d_flags = reinterpret_cast<uint8_t *>(d + o_flags);
    if ((rc = smt_wordpiece_scan_device(tok, reinterpret_cast<const uint8_t *>(d + o_text), text_bytes, reinterpret_cast<const uint64_t *>(d + o_begin),
                                        reinterpret_cast<const uint32_t *>(d + o_len), n_lines, keep_bytes, max_tokens, drop_unk,
                                        reinterpret_cast<uint32_t *>(d + o_counts), d_flags, reinterpret_cast<uint32_t *>(d + o_nflag)))) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    if ((rc = smt_wordpiece_emit_device(tok, n_lines, nullptr, nullptr, nullptr, 0, 0, reinterpret_cast<uint32_t *>(d + o_ids), dev_cap,
                                        reinterpret_cast<uint64_t *>(d + o_off)))) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    SMT_HIP_CHECK(hipMemcpyAsync(offsets_out, d + o_off, ((size_t)n_lines + 1) * 8, hipMemcpyDeviceToHost, st));
    if (flags_out && n_lines) SMT_HIP_CHECK(hipMemcpyAsync(flags_out, d_flags, (size_t)n_lines, hipMemcpyDeviceToHost, st));
    SMT_HIP_CHECK(hipStreamSynchronize(st));
    const uint64_t n_ids = offsets_out[n_lines];
    if (n_ids > ids_cap) { set_error("tokenizer produced more ids than looked-at bytes"); return SMT_E_HIP; }
    if (n_ids) SMT_HIP_CHECK(hipMemcpy(ids_out, d + o_ids, (size_t)n_ids * 4, hipMemcpyDeviceToHost));
    tok->scanned = false;   // (the staged line arrays go away with this call)
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

}  // extern "C"
