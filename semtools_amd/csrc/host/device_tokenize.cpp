// device_tokenize.cpp -- the host layer's device route for a batch of lines: pack the line bytes back to back into a
// pinned buffer, upload, tokenize on the device (tok_scan_device of tokenize_frame.h, whichever family the handle is), tokenize the lines
// the kernel flags with the host tokenizer, splice them in (tok_emit_device) and pool the device CSR with K1 -- the token ids never visit the host
// unless a caller wants them (the workspace's cached ids).  One-rank groups only; StaticModel decides when the route applies.
// A batch of --ignore-case is packed as it is and lowered on the device between the upload and pass 1 (smt_lower_device, DESIGN.md 4.9
// "Lower-casing"): pass 1 then reads the lowered lines and their line list in place of the uploaded ones.
#include <chrono>

#include "../common.h"
#include "../group.h"
#include "../tokenize_frame.h"
#include "host.h"
#include "host_internal.h"

namespace semtools {
namespace search {

struct DeviceTokenRoute {
    smt_group *group = nullptr;
    smt_ctx *ctx = nullptr;
    smt::TokHandle *tok = nullptr;   // an smt_wordpiece or an smt_unigram
    smt_lower *lower = nullptr;      // the library's own tables (to_lowercase's), made by the first call that lowers (device_route_can_lower)
    bool lower_tried = false;
    struct Slot {   // one batch packed for upload: line_begin u64 [n] | line_len u32 [n] | text
        char *pin = nullptr;
        size_t pin_bytes = 0;
        uint64_t n = 0, text_bytes = 0;
        size_t o_len = 0, o_text = 0, up_bytes = 0;
    } slot[2];
    void *d_main = nullptr, *d_ids = nullptr, *d_patch = nullptr, *d_rows = nullptr;
    size_t main_bytes = 0, ids_bytes = 0, patch_bytes = 0, rows_bytes = 0;
    uint64_t lines_done = 0, lines_lowered = 0;
};

namespace {

size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

void hip_ok(hipError_t e, const char *what)
{
    if (e != hipSuccess) { (void)hipGetLastError(); throw Error(std::string("device tokenizer route: ") + what + ": " + hipGetErrorString(e)); }
}

void api_ok(int rc, const char *what)
{
    if (rc != SMT_OK) throw Error(std::string("device tokenizer route: ") + what + ": " + smt_last_error());
}

void grow_device(DeviceTokenRoute *r, void **p, size_t *have, size_t want, const char *what)
{
    if (want <= *have) return;
    hip_ok(hipStreamSynchronize(r->ctx->stream), "stream sync");   // earlier kernels may still read the old buffer
    if (*p) hip_ok(hipFree(*p), "hipFree");
    *p = nullptr;
    *have = 0;
    want += want / 4;
    hip_ok(hipMalloc(p, want), what);
    *have = want;
}

double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

DeviceTokenRoute *device_route_create(smt_group *group, const Tokenizer &tok, bool utf8, bool long_pieces)
{
    int n_ranks = 0;
    if (smt_group_info(group, &n_ranks, nullptr, nullptr, nullptr, nullptr) != SMT_OK || n_ranks != 1) return nullptr;
    smt_ctx *ctx = smt_group_ctx(group, 0);
    if (!ctx) return nullptr;
    smt::TokHandle *h = nullptr;
    WordpieceExport x;
    UnigramExport u;
    WordpieceUtf8Export x8;
    UnigramUtf8Export u8;
    if (utf8 && tok.export_wordpiece_utf8(x8)) {
        const smt_wordpiece_params p = x8.base.params();
        const smt_wordpiece_codepoints cp = x8.codepoints();
        smt_wordpiece *wp = nullptr;
        api_ok(smt_wordpiece_create_utf8(ctx, &p, &cp, &wp), "smt_wordpiece_create_utf8");
        h = smt::tok_handle(wp);
    } else if (utf8 && tok.export_unigram_utf8(u8)) {
        const smt_unigram_params p = u8.base.params();
        const smt_wordpiece_codepoints cp = u8.codepoints();
        smt_unigram *ug = nullptr;
        api_ok(smt_unigram_create_utf8(ctx, &p, &cp, &ug), "smt_unigram_create_utf8");
        api_ok(smt_unigram_set_space_rules(ug, (int)u8.base.collapse_runs, (int)u8.base.drop_trailing), "smt_unigram_set_space_rules");
        if (long_pieces) {
            api_ok(smt_unigram_set_long_pieces(ug, SMT_UG_MAX_LONG), "smt_unigram_set_long_pieces");
            api_ok(smt_unigram_set_long_rules(ug, 1), "smt_unigram_set_long_rules");   // (a Precompiled chain has its space rules on)
        }
        h = smt::tok_handle(ug);
    } else if (tok.export_wordpiece(x)) {
        const smt_wordpiece_params p = x.params();
        smt_wordpiece *wp = nullptr;
        api_ok(smt_wordpiece_create(ctx, &p, &wp), "smt_wordpiece_create");
        h = smt::tok_handle(wp);
    } else if (tok.export_unigram(u)) {
        const smt_unigram_params p = u.params();
        smt_unigram *ug = nullptr;
        api_ok(smt_unigram_create(ctx, &p, &ug), "smt_unigram_create");
        api_ok(smt_unigram_set_space_rules(ug, (int)u.collapse_runs, (int)u.drop_trailing), "smt_unigram_set_space_rules");
        if (long_pieces) {
            api_ok(smt_unigram_set_long_pieces(ug, SMT_UG_MAX_LONG), "smt_unigram_set_long_pieces");
            api_ok(smt_unigram_set_long_rules(ug, 1), "smt_unigram_set_long_rules");
        }
        h = smt::tok_handle(ug);
    } else {
        return nullptr;
    }
    auto *r = new DeviceTokenRoute();
    r->group = group;
    r->ctx = ctx;
    r->tok = h;
    return r;
}

void device_route_destroy(DeviceTokenRoute *r)
{
    if (!r) return;
    smt::tok_destroy(r->tok);   // (waits for the stream)
    smt_lower_destroy(r->lower);
    (void)hipSetDevice(r->ctx->device);
    for (auto &s : r->slot) if (s.pin) (void)hipHostFree(s.pin);
    for (void *p : {r->d_main, r->d_ids, r->d_patch, r->d_rows}) if (p) (void)hipFree(p);
    delete r;
}

uint64_t device_route_lines(const DeviceTokenRoute *r) { return r ? r->lines_done : 0; }
uint64_t device_route_lowered(const DeviceTokenRoute *r) { return r ? r->lines_lowered : 0; }

bool device_route_can_lower(DeviceTokenRoute *r)
{
    if (!r) return false;
    if (!r->lower_tried) {
        r->lower_tried = true;
        if (smt_lower_create(r->ctx, nullptr, &r->lower) != SMT_OK) r->lower = nullptr;   // (the caller lowers on the host)
    }
    return r->lower != nullptr;
}

bool device_route_pack(DeviceTokenRoute *r, int which, const std::string_view *sentences, size_t n, bool lower)
{
    const auto t0 = std::chrono::steady_clock::now();
    DeviceTokenRoute::Slot &s = r->slot[which];
    uint64_t total = 0;
    for (size_t i = 0; i < n; ++i) {
        if (sentences[i].size() > 0xFFFFFFFFull) return false;
        total += sentences[i].size();
    }
    // (the scan's limits: such a batch keeps the host path.  lower: the scan is handed the lowered text's bound, half as much again)
    if (total + (lower ? total / 2 : 0) > (1ull << 32) || n > (1ull << 32)) return false;
    s.n = n;
    s.text_bytes = total;
    s.o_len = up16(n * 8);
    s.o_text = s.o_len + up16(n * 4);
    s.up_bytes = s.o_text + up16((size_t)total);
    if (s.up_bytes + 16 > s.pin_bytes) {
        hip_ok(hipSetDevice(r->ctx->device), "hipSetDevice");
        if (s.pin) hip_ok(hipHostFree(s.pin), "hipHostFree");
        s.pin = nullptr;
        s.pin_bytes = 0;
        const size_t want = s.up_bytes + s.up_bytes / 4 + 16;
        hip_ok(hipHostMalloc(reinterpret_cast<void **>(&s.pin), want, hipHostMallocDefault), "pinned staging buffer");
        s.pin_bytes = want;
    }
    uint64_t *begin = reinterpret_cast<uint64_t *>(s.pin);
    uint32_t *len = reinterpret_cast<uint32_t *>(s.pin + s.o_len);
    uint64_t at = 0;
    for (size_t i = 0; i < n; ++i) { begin[i] = at; len[i] = (uint32_t)sentences[i].size(); at += sentences[i].size(); }
    char *text = s.pin + s.o_text;
    parallel_slices(n, 8192, [&](size_t b, size_t e) {   // (at most 8 threads)
        for (size_t i = b; i < e; ++i)
            if (!sentences[i].empty()) memcpy(text + begin[i], sentences[i].data(), sentences[i].size());
    });
    PhaseTimer::add("within_embed:device_pack", ms_since(t0));
    return true;
}

uint64_t device_route_run(DeviceTokenRoute *r, int which, smt_sharded_model *model, uint32_t keep_bytes, uint32_t max_tokens, bool drop_unk,
                          const DeviceFlaggedFn &tokenize_flagged, float *out_host, smt_sharded_corpus *corpus, TokenCsr *sink, bool lower)
{
    const DeviceTokenRoute::Slot &s = r->slot[which];
    const uint64_t n = s.n;
    if (n == 0) return 0;
    smt_ctx *ctx = r->ctx;
    hip_ok(hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t st = ctx->stream;
    auto t0 = std::chrono::steady_clock::now();
    if (lower && !r->lower) throw Error("device tokenizer route: a batch to lower without device_route_can_lower");
    // ---- device block: [the uploaded block] | counts u32 [n] | flags u8 [n] | n_flagged, lines the lower-casing flagged | offsets u64 [n + 1]
    // lower: | out_begin u64 [n + 1] | out_len u32 [n] | lower-casing flags u8 [n] | the lowered text, low_cap bytes
    const uint64_t low_cap = lower ? s.text_bytes + s.text_bytes / 2 : 0;
    const size_t o_counts = up16(s.up_bytes), o_flags = o_counts + up16(n * 4), o_nflag = o_flags + up16(n), o_off = o_nflag + 16,
                 o_lbegin = o_off + up16((n + 1) * 8), o_llen = o_lbegin + (lower ? up16((n + 1) * 8) : 0), o_lflags = o_llen + (lower ? up16(n * 4) : 0),
                 o_ltext = o_lflags + (lower ? up16(n) : 0), main_total = o_ltext + (lower ? up16((size_t)low_cap + 1) : 0);
    grow_device(r, &r->d_main, &r->main_bytes, main_total, "line arrays");
    char *d = static_cast<char *>(r->d_main);
    hip_ok(hipMemcpyAsync(d, s.pin, s.up_bytes, hipMemcpyHostToDevice, st), "upload of the packed lines");
    uint8_t *d_flags = reinterpret_cast<uint8_t *>(d + o_flags);
    {
        const uint8_t *text = reinterpret_cast<const uint8_t *>(d + s.o_text);
        const uint64_t *begin = reinterpret_cast<const uint64_t *>(d);
        const uint32_t *len = reinterpret_cast<const uint32_t *>(d + s.o_len);
        uint32_t *counts = reinterpret_cast<uint32_t *>(d + o_counts), *nflag = reinterpret_cast<uint32_t *>(d + o_nflag);
        uint64_t text_bytes = s.text_bytes;
        const uint8_t *lower_flags = nullptr;
        if (lower) {
            // the lowered lines stand back to back in [0, out_begin[n]) of the region; pass 1 is handed the region's size as its
            // text_bytes -- the total is known on the device only, and the bytes behind it belong to no line
            uint8_t *ltext = reinterpret_cast<uint8_t *>(d + o_ltext);
            uint64_t *lbegin = reinterpret_cast<uint64_t *>(d + o_lbegin);
            uint32_t *llen = reinterpret_cast<uint32_t *>(d + o_llen);
            api_ok(smt_lower_device(r->lower, text, s.text_bytes, begin, len, n, ltext, low_cap, lbegin, llen, reinterpret_cast<uint8_t *>(d + o_lflags),
                                    nflag + 1),
                   "lower-casing");
            text = ltext;
            begin = lbegin;
            len = llen;
            text_bytes = low_cap;   // (pass 1's grid and slots grow by half with it, most of them owning no line: intended)
            // a line the lower-casing left as it was is flagged for pass 1 too, wherever its ill-formed byte stands: behind the cut of
            // keep_bytes pass 1 would not see it, and would tokenize the line's un-lowered head
            lower_flags = reinterpret_cast<const uint8_t *>(d + o_lflags);
        }
        api_ok(smt::tok_scan_device(r->tok, text, text_bytes, begin, len, n, keep_bytes, max_tokens, drop_unk ? 1 : 0, counts, d_flags, nflag, lower_flags),
               "pass 1");
    }
    uint32_t n_flagged_both[2] = {0, 0};   // pass 1's, the lower-casing's
    hip_ok(hipMemcpyAsync(n_flagged_both, d + o_nflag, lower ? 8 : 4, hipMemcpyDeviceToHost, st), "n_flagged");
    hip_ok(hipStreamSynchronize(st), "pass 1");
    const uint32_t n_flagged = n_flagged_both[0];
    PhaseTimer::add("within_embed:device_upload_and_pass1", ms_since(t0));
    // ---- the lines the kernel does not cover go through the host tokenizer: same truncate, unk-drop and cap steps
    std::vector<uint64_t> patch_line, patch_off(1, 0);
    std::vector<uint32_t> patch_ids;
    if (n_flagged) {
        t0 = std::chrono::steady_clock::now();
        std::vector<uint8_t> flags(n);
        hip_ok(hipMemcpy(flags.data(), d_flags, n, hipMemcpyDeviceToHost), "flags");
        patch_line.reserve(n_flagged);
        for (uint64_t i = 0; i < n; ++i) if (flags[i]) patch_line.push_back(i);
        tokenize_flagged(patch_line, patch_ids, patch_off);
        if (patch_off.size() != patch_line.size() + 1) throw Error("device tokenizer route: the flagged lines came back malformed");
        PhaseTimer::add("within_embed:device_flagged_on_host", ms_since(t0));
    }
    t0 = std::chrono::steady_clock::now();
    const uint64_t n_patch = patch_line.size(), n_patch_ids = patch_ids.size();
    const uint64_t ids_cap = r->tok->ids_bound + n_patch_ids;   // (the scan's bound on its own ids)
    grow_device(r, &r->d_ids, &r->ids_bytes, (size_t)ids_cap * 4 + 16, "token ids");
    const size_t p_off = up16(n_patch * 8), p_ids = p_off + up16((n_patch + 1) * 8);
    char *dp = nullptr;
    if (n_patch) {
        grow_device(r, &r->d_patch, &r->patch_bytes, p_ids + up16(n_patch_ids * 4 + 4), "patch");
        dp = static_cast<char *>(r->d_patch);
        hip_ok(hipMemcpyAsync(dp, patch_line.data(), n_patch * 8, hipMemcpyHostToDevice, st), "patch lines");
        hip_ok(hipMemcpyAsync(dp + p_off, patch_off.data(), (n_patch + 1) * 8, hipMemcpyHostToDevice, st), "patch offsets");
        if (n_patch_ids) hip_ok(hipMemcpyAsync(dp + p_ids, patch_ids.data(), n_patch_ids * 4, hipMemcpyHostToDevice, st), "patch ids");
    }
    uint32_t *d_ids = static_cast<uint32_t *>(r->d_ids);
    uint64_t *d_off = reinterpret_cast<uint64_t *>(d + o_off);
    {
        const uint64_t *pl = reinterpret_cast<const uint64_t *>(dp), *po = dp ? reinterpret_cast<const uint64_t *>(dp + p_off) : nullptr;
        const uint32_t *pi = dp ? reinterpret_cast<const uint32_t *>(dp + p_ids) : nullptr;
        api_ok(smt::tok_emit_device(r->tok, n, pl, po, pi, n_patch, n_patch_ids, d_ids, ids_cap, d_off), "pass 2");
    }
    // ---- K1 on the device CSR (the lines are already truncated: no cap here, as on the host path)
    smt_model *m = model->model.at(0);
    if (corpus) api_ok(smt::sharded_embed_device_append(model, d_ids, d_off, n, corpus), "K1 into the corpus");   // (waits for the stream)
    if (out_host) {
        grow_device(r, &r->d_rows, &r->rows_bytes, (size_t)n * m->D * sizeof(float), "output rows");
        api_ok(smt_embed_device(m, d_ids, d_off, n, 0, static_cast<float *>(r->d_rows)), "K1");
        hip_ok(hipMemcpyAsync(out_host, r->d_rows, (size_t)n * m->D * sizeof(float), hipMemcpyDeviceToHost, st), "rows");
        hip_ok(hipStreamSynchronize(st), "pass 2 + K1");
    }
    if (!corpus && !out_host) hip_ok(hipStreamSynchronize(st), "pass 2");
    PhaseTimer::add("within_embed:device_pass2_and_K1", ms_since(t0));
    if (sink) {   // the ids that were pooled, as the host path stores them
        std::vector<uint64_t> off(n + 1);
        hip_ok(hipMemcpy(off.data(), d_off, (n + 1) * 8, hipMemcpyDeviceToHost), "offsets");
        const size_t old = sink->ids.size();
        sink->ids.resize(old + off[n]);
        if (off[n]) hip_ok(hipMemcpy(sink->ids.data() + old, d_ids, off[n] * 4, hipMemcpyDeviceToHost), "ids");
        for (uint64_t i = 0; i < n; ++i) sink->lens.push_back((uint32_t)(off[i + 1] - off[i]));
    }
    r->lines_done += n - n_flagged;
    if (lower) r->lines_lowered += n - n_flagged_both[1];
    return n_flagged;
}

}  // namespace search
}  // namespace semtools
