// tokenize_kernels.hip -- what the device tokenizers share (tokenize_frame.h): the table builder and its upload, the
// scratch between the passes, pass 2 with its kernels, and scan / emit / tokenize written once on the handle base.
//
// Pass 1 is a family's own (wordpiece_kernels.hip, unigram_kernels.hip): it leaves token ids in slots, a line's slots in token order.
// Pass 2 is a prefix sum over the slots: rank of a slot among the used slots minus the rank at its line's start is the token's
// place in its line; lines are laid out by a prefix sum of their (capped, or patched) counts.
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"
#include "tokenize_frame.h"

namespace {

constexpr uint32_t WP_NONE = smt::TOK_NONE;   // an ids_tmp slot that holds no token
constexpr unsigned EMIT_THREADS = smt::TOK_EMIT_THREADS;   // pass 2: four slots per thread
constexpr unsigned EMIT_CHUNK = smt::TOK_EMIT_CHUNK;

// pre (nullptr: none): flags an earlier step raised; such a line is flagged here too, whatever pass 1 looked at
__global__ void __launch_bounds__(256) wp_lines_kernel(uint64_t n_lines, const uint32_t *__restrict__ raw_count, uint8_t *__restrict__ flags,
                                                       const uint8_t *__restrict__ pre, uint32_t max_tokens, uint32_t *__restrict__ counts,
                                                       uint32_t *__restrict__ n_flagged)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_lines) return;
    bool f = flags[i] != 0;
    if (!f && pre && pre[i]) { f = true; flags[i] = 1; }
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
    if (t < 2) s_win[t] = smt::tok_count_le(line_begin, 0, n_lines, t == 0 ? first : (first + EMIT_CHUNK - 1 < text_bytes ? first + EMIT_CHUNK - 1 : text_bytes - 1));
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
        const uint64_t n_le = smt::tok_count_le(line_begin, s_win[0], s_win[1], first + t * 4 + k);
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

size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

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

static int grow(smt_ctx *ctx, void **p, size_t bytes, const char *what)
{
    SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // earlier kernels may still read the old buffer
    if (*p) SMT_HIP_CHECK(hipFree(*p));
    *p = nullptr;
    const hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); *p = nullptr; set_error("hipMalloc(%zu) for %s: %s", bytes, what, hipGetErrorString(e)); return SMT_E_NOMEM; }
    return SMT_OK;
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

int tok_upload_table(const char *family, const std::vector<std::pair<const void *, size_t>> &parts, void **d_table, const uint8_t **at)
{
    std::vector<size_t> off;
    size_t total = 0;
    for (const auto &part : parts) { off.push_back(total); total += up16(part.second) + 16; }
    std::vector<uint8_t> blob(total, 0);
    for (size_t i = 0; i < parts.size(); ++i)
        if (parts[i].second) memcpy(blob.data() + off[i], parts[i].first, parts[i].second);
    *d_table = nullptr;
    hipError_t e = hipMalloc(d_table, total);
    if (e == hipSuccess) e = hipMemcpy(*d_table, blob.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (*d_table) (void)hipFree(*d_table);
        *d_table = nullptr;
        set_error("%s table upload (%zu bytes): %s", family, total, hipGetErrorString(e));
        return SMT_E_NOMEM;
    }
    for (size_t i = 0; i < parts.size(); ++i) at[i] = static_cast<const uint8_t *>(*d_table) + off[i];
    return SMT_OK;
}

int tok_scratch_reserve(smt_ctx *ctx, TokScratch &s, uint64_t n_slots, uint64_t n_lines, uint64_t n_long)
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
    if (n_long > s.long_cap) {
        s.long_cap = 0;
        if ((rc = grow(ctx, &s.d_long, 32 + (size_t)n_long * 16, "tokenizer work list"))) return rc;
        s.long_cap = n_long;
    }
    return SMT_OK;
}

int tok_scratch_clear(smt_ctx *ctx, TokScratch &s, uint64_t n_slots, uint64_t n_lines)
{
    const uint64_t chunks = TokScratch::chunks_of(n_slots);
    if (n_lines) SMT_HIP_CHECK(hipMemsetAsync(s.raw_count(), 0, (size_t)n_lines * 4, ctx->stream));
    if (chunks) SMT_HIP_CHECK(hipMemsetAsync(s.d_ids_tmp, 0xFF, (size_t)chunks * EMIT_CHUNK * 4, ctx->stream));
    if (s.d_long) SMT_HIP_CHECK(hipMemsetAsync(s.d_long, 0, 32, ctx->stream));
    return SMT_OK;
}

void tok_scratch_free(TokScratch &s)
{
    if (s.d_ids_tmp) (void)hipFree(s.d_ids_tmp);
    if (s.d_lines) (void)hipFree(s.d_lines);
    if (s.d_chunks) (void)hipFree(s.d_chunks);
    if (s.d_long) (void)hipFree(s.d_long);
    s = TokScratch();
}

int tok_exscan(smt_ctx *ctx, const uint32_t *in_dev, uint64_t n, uint64_t *out_dev)
{
    hipLaunchKernelGGL(wp_exscan_kernel, dim3(1), dim3(1024), 0, ctx->stream, in_dev, n, out_dev);
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

int tok_line_counts(smt_ctx *ctx, const TokScratch &s, uint64_t n_lines, uint8_t *flags_dev, uint32_t max_tokens, uint32_t *counts_dev,
                    uint32_t *n_flagged_dev, const uint8_t *pre_flags_dev)
{
    if (!n_lines) return SMT_OK;
    hipLaunchKernelGGL(wp_lines_kernel, dim3((unsigned)((n_lines + 255) / 256)), dim3(256), 0, ctx->stream, n_lines, s.raw_count(), flags_dev,
                       pre_flags_dev, max_tokens, counts_dev, n_flagged_dev);
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

void tok_destroy(TokHandle *tok)
{
    if (!tok) return;
    (void)hipSetDevice(tok->ctx->device);
    (void)hipStreamSynchronize(tok->ctx->stream);
    if (tok->d_table) (void)hipFree(tok->d_table);
    tok_scratch_free(tok->S);
    delete tok;
}

int tok_scan_device(TokHandle *tok, const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev, const uint32_t *line_len_dev,
                    uint64_t n_lines, uint32_t keep_bytes, uint32_t max_tokens, int drop_unk, uint32_t *counts_dev, uint8_t *flags_dev,
                    uint32_t *n_flagged_dev, const uint8_t *pre_flags_dev)
{
    SMT_REQUIRE(n_flagged_dev != nullptr, "n_flagged_dev");
    SMT_REQUIRE(n_lines == 0 || (line_begin_dev && line_len_dev && counts_dev && flags_dev), "null argument");
    SMT_REQUIRE(text_bytes == 0 || text_dev != nullptr, "text_dev");
    SMT_REQUIRE(text_bytes <= (1ull << 32), "at most 4 GiB of text per scan");
    SMT_REQUIRE(n_lines <= (1ull << 32), "at most 2^32 lines per scan");
    smt_ctx *ctx = tok->ctx;
    int rc = bind_device(ctx);
    if (rc) return rc;
    tok->scanned = false;
    const uint64_t n_slots = tok->slots_of(text_bytes, n_lines);
    if ((rc = tok_scratch_reserve(ctx, tok->S, n_slots, n_lines, tok->long_records(text_bytes)))) return rc;
    hipStream_t st = ctx->stream;
    SMT_HIP_CHECK(hipMemsetAsync(n_flagged_dev, 0, sizeof(uint32_t), st));
    if (n_lines) SMT_HIP_CHECK(hipMemsetAsync(flags_dev, 0, n_lines, st));
    if ((rc = tok_scratch_clear(ctx, tok->S, n_slots, n_lines))) return rc;
    const auto launches = [&]() -> int {
        int r = tok->pass1(text_dev, text_bytes, line_begin_dev, line_len_dev, n_lines, keep_bytes, drop_unk, flags_dev);
        if (r) return r;
        return tok_line_counts(ctx, tok->S, n_lines, flags_dev, max_tokens, counts_dev, n_flagged_dev, pre_flags_dev);
    };
    prof_begin(ctx, "tokenize");
    rc = launches();
    prof_end(ctx, "tokenize");   // (on every path: an event pair left open would be read as a running one)
    if (rc) return rc;
    tok->scanned = true;
    tok->text_bytes = text_bytes;
    tok->n_lines = n_lines;
    tok->ids_bound = tok->slots_of(keep_bytes ? std::min<uint64_t>(text_bytes, n_lines * (uint64_t)keep_bytes) : text_bytes, n_lines);
    tok->slot_begin = tok->extra_slot ? tok->S.slot_begin() : line_begin_dev;
    tok->counts = counts_dev;
    tok->flags = flags_dev;
    return SMT_OK;
}

int tok_emit_device(TokHandle *tok, uint64_t n_lines, const uint64_t *patch_line_dev, const uint64_t *patch_off_dev, const uint32_t *patch_ids_dev,
                    uint64_t n_patch, uint64_t n_patch_ids, uint32_t *ids_out_dev, uint64_t ids_cap, uint64_t *offsets_out_dev)
{
    SMT_REQUIRE(tok->scanned, tok->words.no_scan);
    SMT_REQUIRE(n_lines == tok->n_lines, "n_lines differs from the scan's");
    SMT_REQUIRE(offsets_out_dev != nullptr, "offsets_out_dev");
    SMT_REQUIRE(n_patch == 0 || (patch_line_dev && patch_off_dev), "patch arrays");
    SMT_REQUIRE(n_patch <= n_lines, "more patched lines than lines");
    SMT_REQUIRE(n_patch_ids == 0 || (n_patch && patch_ids_dev), "patch ids");
    SMT_REQUIRE(n_patch_ids <= (1ull << 40), "patch ids");
    SMT_REQUIRE(ids_cap >= tok->ids_bound + n_patch_ids, tok->words.emit_cap);
    SMT_REQUIRE(ids_cap == 0 || ids_out_dev != nullptr, "ids_out_dev");
    smt_ctx *ctx = tok->ctx;
    int rc = bind_device(ctx);
    if (rc) return rc;
    prof_begin(ctx, "tokenize_emit");
    if ((rc = tok_pass2(ctx, tok->S, tok->slots_of(tok->text_bytes, n_lines), tok->slot_begin, n_lines, tok->counts, tok->flags, patch_line_dev,
                        patch_off_dev, patch_ids_dev, n_patch, n_patch_ids, ids_out_dev, ids_cap, offsets_out_dev)))
        return rc;
    prof_end(ctx, "tokenize_emit");
    return SMT_OK;
}

int tok_tokenize(TokHandle *tok, const char *text, const uint64_t *line_begin, const uint32_t *line_len, uint64_t n_lines, uint32_t keep_bytes,
                 uint32_t max_tokens, int drop_unk, uint32_t *ids_out, uint64_t ids_cap, uint64_t *offsets_out, uint8_t *flags_out)
{
    SMT_REQUIRE(offsets_out != nullptr, "offsets_out");
    SMT_REQUIRE(n_lines == 0 || (line_begin && line_len), "null argument");
    uint64_t text_bytes = 0, looked = 0;
    for (uint64_t i = 0; i < n_lines; ++i) {
        SMT_REQUIRE(line_begin[i] >= text_bytes, "lines must lie in line order and must not overlap");
        text_bytes = line_begin[i] + line_len[i];
        looked += keep_bytes && keep_bytes < line_len[i] ? keep_bytes : line_len[i];
    }
    SMT_REQUIRE(text_bytes == 0 || text != nullptr, "text");
    if (ids_cap < tok->slots_of(looked, n_lines)) {   // (SMT_REQUIRE, with the family's wording of message and condition)
        set_error("invalid argument: %s", tok->words.tokenize_cap);
        return SMT_E_INVALID;
    }
    SMT_REQUIRE(ids_cap == 0 || ids_out != nullptr, "ids_out");
    smt_ctx *ctx = tok->ctx;
    int rc = bind_device(ctx);
    if (rc) return rc;
    const uint64_t dev_cap = std::max<uint64_t>(ids_cap, tok->slots_of(text_bytes, n_lines));   // (the device form's bound)
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
    if ((rc = tok_scan_device(tok, reinterpret_cast<const uint8_t *>(d + o_text), text_bytes, reinterpret_cast<const uint64_t *>(d + o_begin),
                              reinterpret_cast<const uint32_t *>(d + o_len), n_lines, keep_bytes, max_tokens, drop_unk,
                              reinterpret_cast<uint32_t *>(d + o_counts), d_flags, reinterpret_cast<uint32_t *>(d + o_nflag))) ||
        (rc = tok_emit_device(tok, n_lines, nullptr, nullptr, nullptr, 0, 0, reinterpret_cast<uint32_t *>(d + o_ids), dev_cap,
                              reinterpret_cast<uint64_t *>(d + o_off)))) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    SMT_HIP_CHECK(hipMemcpyAsync(offsets_out, d + o_off, ((size_t)n_lines + 1) * 8, hipMemcpyDeviceToHost, st));
    if (flags_out && n_lines) SMT_HIP_CHECK(hipMemcpyAsync(flags_out, d_flags, (size_t)n_lines, hipMemcpyDeviceToHost, st));
    SMT_HIP_CHECK(hipStreamSynchronize(st));
    const uint64_t n_ids = offsets_out[n_lines];
    if (n_ids > ids_cap) { set_error("tokenizer produced more ids than ids_cap"); return SMT_E_HIP; }
    if (n_ids) SMT_HIP_CHECK(hipMemcpy(ids_out, d + o_ids, (size_t)n_ids * 4, hipMemcpyDeviceToHost));
    tok->scanned = false;   // (the staged line arrays go away with this call)
    return SMT_OK;
}

}  // namespace smt
