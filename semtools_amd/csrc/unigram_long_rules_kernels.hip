// unigram_long_rules_kernels.hip -- the long pieces of the Unigram device tokenizer while a space rule of smt_unigram_set_space_rules
// is on (DESIGN.md 4.9 "long pieces under the space rules"): the second pass-1 kernel behind ug_scan_rules_kernel /
// ug_scan_utf8_rules_kernel, run only while smt_unigram_set_long_pieces set a limit AND smt_unigram_set_long_rules has its switch on.
// The kernel's text is ul_body<UTF8, true> of unigram_long_body.h: ug_long_kernel's, with the absorbed run skipped in front of the
// piece, the measure of the scan kernels under the rules, and drop_trailing.  Also here: that switch.
#include "unigram_long_body.h"

namespace {

template <bool UTF8>
__global__ void __launch_bounds__(UL_LANES) ug_long_rules_kernel(UgTable T, WpCodepoints U, uint32_t rules, const uint8_t *__restrict__ text,
                                                                uint64_t text_bytes, const uint64_t *__restrict__ line_begin,
                                                                const uint32_t *__restrict__ line_len, uint64_t n_lines, uint32_t keep_bytes,
                                                                int drop_unk, uint32_t max_long, uint32_t *__restrict__ ids_tmp,
                                                                uint32_t *__restrict__ raw_count, uint8_t *__restrict__ flags, UgLongList W)
{
    __shared__ UlLds S;
    ul_body<UTF8, true>(S, T, U, rules, text, text_bytes, line_begin, line_len, n_lines, keep_bytes, drop_unk, max_long, ids_tmp, raw_count, flags, W);
}

}  // namespace

namespace smt {

int ug_long_rules_launch(smt_unigram *tok, const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev,
                         const uint32_t *line_len_dev, uint64_t n_lines, uint32_t keep_bytes, int drop_unk, uint8_t *flags_dev)
{
    const UgLongList W = tok->long_list();
    SMT_REQUIRE(W.head != nullptr, "the long pieces' work list is not reserved");
    prof_begin(tok->ctx, "tokenize_long");
    if (tok->utf8)
        hipLaunchKernelGGL(ug_long_rules_kernel<true>, dim3(UL_GRID), dim3(UL_LANES), 0, tok->ctx->stream, tok->T, tok->U, tok->rules, text_dev, text_bytes,
                           line_begin_dev, line_len_dev, n_lines, keep_bytes, drop_unk, tok->max_long, tok->S.d_ids_tmp, tok->S.raw_count(), flags_dev, W);
    else
        hipLaunchKernelGGL(ug_long_rules_kernel<false>, dim3(UL_GRID), dim3(UL_LANES), 0, tok->ctx->stream, tok->T, tok->U, tok->rules, text_dev, text_bytes,
                           line_begin_dev, line_len_dev, n_lines, keep_bytes, drop_unk, tok->max_long, tok->S.d_ids_tmp, tok->S.raw_count(), flags_dev, W);
    SMT_HIP_CHECK(hipGetLastError());
    prof_end(tok->ctx, "tokenize_long");
    return SMT_OK;
}

}  // namespace smt

extern "C" {

int smt_unigram_set_long_rules(smt_unigram *tok, int on)
try {
    if (!tok) return smt::tok_null_handle("smt_unigram_set_long_rules");
    SMT_REQUIRE(on == 0 || on == 1, "on is 0 or 1");
    tok->long_rules = on != 0;
    return SMT_OK;
} catch (...) { return smt::api_catch(); }

}  // extern "C"
