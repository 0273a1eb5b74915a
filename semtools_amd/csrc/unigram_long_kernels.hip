// unigram_long_kernels.hip -- the long pieces of the Unigram device tokenizer (DESIGN.md 4.9 "long pieces"): the second pass-1 kernel,
// behind ug_scan_kernel / ug_scan_utf8_kernel on the same stream, run only while smt_unigram_set_long_pieces has the switch on.  The
// kernel's text -- the five steps, the bounds, the LDS -- is ul_body<UTF8, false> of unigram_long_body.h; the instantiation with the
// space rules is unigram_long_rules_kernels.hip's.  Also here: the switch and the witness of both.
#include "unigram_long_body.h"

namespace {

template <bool UTF8>
__global__ void __launch_bounds__(UL_LANES) ug_long_kernel(UgTable T, WpCodepoints U, const uint8_t *__restrict__ text, uint64_t text_bytes,
                                                          const uint64_t *__restrict__ line_begin, const uint32_t *__restrict__ line_len,
                                                          uint64_t n_lines, uint32_t keep_bytes, int drop_unk, uint32_t max_long,
                                                          uint32_t *__restrict__ ids_tmp, uint32_t *__restrict__ raw_count,
                                                          uint8_t *__restrict__ flags, UgLongList W)
{
    __shared__ UlLds S;
    ul_body<UTF8, false>(S, T, U, 0u, text, text_bytes, line_begin, line_len, n_lines, keep_bytes, drop_unk, max_long, ids_tmp, raw_count, flags, W);
}

}  // namespace

namespace smt {

int ug_long_launch(smt_unigram *tok, const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev, const uint32_t *line_len_dev,
                   uint64_t n_lines, uint32_t keep_bytes, int drop_unk, uint8_t *flags_dev)
{
    const UgLongList W = tok->long_list();
    SMT_REQUIRE(W.head != nullptr, "the long pieces' work list is not reserved");
    prof_begin(tok->ctx, "tokenize_long");
    if (tok->utf8)
        hipLaunchKernelGGL(ug_long_kernel<true>, dim3(UL_GRID), dim3(UL_LANES), 0, tok->ctx->stream, tok->T, tok->U, text_dev, text_bytes, line_begin_dev,
                           line_len_dev, n_lines, keep_bytes, drop_unk, tok->max_long, tok->S.d_ids_tmp, tok->S.raw_count(), flags_dev, W);
    else
        hipLaunchKernelGGL(ug_long_kernel<false>, dim3(UL_GRID), dim3(UL_LANES), 0, tok->ctx->stream, tok->T, tok->U, text_dev, text_bytes, line_begin_dev,
                           line_len_dev, n_lines, keep_bytes, drop_unk, tok->max_long, tok->S.d_ids_tmp, tok->S.raw_count(), flags_dev, W);
    SMT_HIP_CHECK(hipGetLastError());
    prof_end(tok->ctx, "tokenize_long");
    return SMT_OK;
}

}  // namespace smt

extern "C" {

int smt_unigram_set_long_pieces(smt_unigram *tok, uint32_t max_raw_bytes)
try {
    if (!tok) return smt::tok_null_handle("smt_unigram_set_long_pieces");
    SMT_REQUIRE(max_raw_bytes == 0 || (max_raw_bytes > SMT_UG_MAX_WORD && max_raw_bytes <= SMT_UG_MAX_LONG),
                "max_raw_bytes is 0, or above SMT_UG_MAX_WORD and at most SMT_UG_MAX_LONG");
    tok->max_long = max_raw_bytes;
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

int smt_unigram_long_stats(smt_unigram *tok, uint64_t *pieces, uint64_t *raw_bytes)
try {
    if (!tok) return smt::tok_null_handle("smt_unigram_long_stats");
    uint64_t head[smt::UG_LONG_HEADER / 8] = {};
    if (tok->long_scanned && tok->S.d_long) {
        int rc = smt::bind_device(tok->ctx);
        if (rc) return rc;
        SMT_HIP_CHECK(hipMemcpyAsync(head, tok->S.d_long, sizeof(head), hipMemcpyDeviceToHost, tok->ctx->stream));
        SMT_HIP_CHECK(hipStreamSynchronize(tok->ctx->stream));
    }
    if (pieces) *pieces = head[1];
    if (raw_bytes) *raw_bytes = head[2];
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

}  // extern "C"
