/*
 * semtools_hip.h -- C ABI of libsemtools_hip.so, the MI355X (gfx950) core for
 * the `semtools search` / `semtools workspace` hot path:
 *
 *     embed (token-id gather + mean-pool + L2-normalise)
 *       -> cosine scan of query vector(s) over the row-major f32 corpus
 *       -> top-k / max-distance selection
 *
 * The reference (run-llama/semtools v3.0.0, /root/reference) has NO FFI seam
 * for this path: the arithmetic sits behind three Rust crates (model2vec-rs,
 * simsimd, qdrant-edge) called from ordinary Rust functions.  Each entry point
 * below names the reference interface (file:line, relative to /root/reference)
 * it replaces; INTEGRATION.md shows the Rust `extern "C"` stub a maintainer
 * would add at those call sites.
 *
 * Conventions
 *   - Plain C: opaque handles, raw pointers, sizes.  No torch/C++ types.
 *   - Every function returning `int` returns SMT_OK (0) or a negative SMT_E_*;
 *     smt_last_error() returns a thread-local message for the last failure.
 *     Nothing unwinds or aborts across the ABI.
 *   - Host buffers are owned by the caller; device memory lives behind handles.
 *   - Handles are not thread-safe: serialise calls per handle (the reference
 *     calls this path synchronously from one task, src/bin/semtools.rs:134).
 *   - One smt_ctx == one GPU + one HIP stream.  Multi-GPU lives behind smt_group /
 *     smt_sharded_corpus (bottom of this file): the library owns one context per GPU and
 *     the RCCL communicator; a single host thread drives the whole node, or one rank
 *     per process joins the same communicator (smt_group_create_rank).
 *   - "_device" entry points take/return DEVICE pointers and enqueue on the
 *     context's stream without synchronising (bench / multi-GPU pipelines).
 *   - There is no CPU fallback: every compute entry point fails with
 *     SMT_E_HIP when no gfx950 device is usable.
 *
 * Domain (semtools_amd/csrc/domain.hip)
 *   A row or query vector is IN DOMAIN iff every component is finite and its largest magnitude is 0 or lies in
 *   [2^-40, 2^40].  Inside it the returned distance is simsimd's cosine in its f64 "accurate" form, bit for bit, and
 *   scaling a vector by a power of two changes no answer.  Outside it the reference itself has no single answer --
 *   cos_finish turns a NaN into distance 0.0 (the BEST score: src/search/mod.rs:86-89 pushes it, :107-111 sorts it
 *   first) and the f32 accumulators of simsimd's serial / SIMD backends overflow beyond |x| ~ 1.8e19 and underflow
 *   below ~1e-19 in an order-dependent way -- and the f32 / fp16 nominating kernels and their error bounds do not
 *   cover it.  Such vectors are REFUSED at the boundary instead of being answered for:
 *     - rows, where they enter a corpus (smt_corpus_append_host, smt_corpus_write_rows, smt_corpus_from_device,
 *       smt_embed with append_to, the sharded forms of these): SMT_E_INVALID, the corpus unchanged, the message
 *       names the first offending row; the file loaders return SMT_E_IO (a damaged file);
 *     - queries of the host-form searches: SMT_E_INVALID before anything is launched;
 *     - queries of the *_device entry points: SMT_STATUS_INVALID_QUERY in the _ex form's status word (and the
 *       context's uncertain counter); that query's list means nothing.
 *   model2vec's pool step with `normalize` emits unit or zero rows: nothing the reference's own path produces is
 *   ever refused.  A corpus adopted with smt_corpus_from_device is checked once, as it is at that call.
 */
#ifndef SEMTOOLS_HIP_H
#define SEMTOOLS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMT_OK 0
#define SMT_E_INVALID (-1)     /* bad argument                                   */
#define SMT_E_HIP (-2)         /* HIP runtime / device error, or no GPU          */
#define SMT_E_NOMEM (-3)       /* host or device allocation failed / capacity    */
#define SMT_E_TRUNCATED (-4)   /* more hits than out_cap; counts hold true sizes */
#define SMT_E_IO (-5)          /* file error in save/load                        */
#define SMT_E_UNSUPPORTED (-6) /* e.g. embedding dim other than 256              */

#define SMT_DIM 256u /* LINE_EMBEDDING_SIZE, src/workspace/store.rs:37 */

/* selection semantics of smt_search */
#define SMT_MODE_DOCUMENTS 0 /* search_documents, src/search/mod.rs:77-120            */
#define SMT_MODE_WORKSPACE 1 /* Store::search_line_embeddings, store.rs:481-546        */

typedef struct smt_ctx smt_ctx;
typedef struct smt_model smt_model;
typedef struct smt_corpus smt_corpus;

/* half-open range of corpus rows [begin, end) */
typedef struct smt_range {
    uint64_t begin;
    uint64_t end;
} smt_range;

/* ------------------------------------------------------------------ context */

/* Bind to GPU `device` and create a private (non-blocking) HIP stream.  Everything the library enqueues is ordered on THAT stream
 * only: device memory handed in (smt_corpus_from_device, the *_device entry points) must be complete before the call -- synchronise
 * the stream that produced it, or create the context on that stream (below). */
int smt_ctx_create(int device, smt_ctx **out);
/* Same, but enqueue on an existing hipStream_t owned by the caller (e.g. the
 * host framework's current stream).  NULL here means THE NULL STREAM. */
int smt_ctx_create_on_stream(int device, void *stream, smt_ctx **out);
void smt_ctx_destroy(smt_ctx *ctx);
int smt_ctx_synchronize(smt_ctx *ctx);
const char *smt_last_error(void);
const char *smt_version(void);
/* number of visible HIP devices, or SMT_E_HIP */
int smt_device_count(void);

/* Per-kernel timing with HIP events recorded on the context's stream around
 * each launch of the named kernel family ("scan", "gemm", "embed", "select").
 * Reading synchronises the stream. */
int smt_prof_enable(smt_ctx *ctx, int on);
int smt_prof_reset(smt_ctx *ctx);
int smt_prof_read(smt_ctx *ctx, const char *kernel, uint64_t *launches, double *total_ms);

/* -------------------------------------------------------------------- model
 * Replaces the device half of StaticModel::from_pretrained (call sites
 * src/cmds/search.rs:123-128, src/cmds/ask.rs:128-133): the f32 `embeddings`
 * table [V x D] is uploaded once and stays resident.  `normalize` is the
 * model's config flag (true for potion-multilingual-128M). */
int smt_model_create(smt_ctx *ctx, const float *table_host, uint64_t V, uint32_t D,
                     int normalize, smt_model **out);
/* Stream an f32 table [V x D] that sits at `byte_offset` of a file (the `embeddings` tensor of model.safetensors)
 * straight into HBM through two pinned buffers: the file read of chunk j+1 overlaps the PCIe copy of chunk j, and no
 * pageable staging copy of the whole table (512 MB for potion-multilingual-128M) is ever made. */
int smt_model_create_from_file(smt_ctx *ctx, const char *path, uint64_t byte_offset, uint64_t V, uint32_t D,
                               int normalize, smt_model **out);
/* adopt a table already in device memory (not copied, not freed) */
int smt_model_create_from_device(smt_ctx *ctx, const float *table_dev, uint64_t V, uint32_t D,
                                 int normalize, smt_model **out);
void smt_model_destroy(smt_model *model);

/* Typed tables.  StaticModel::from_pretrained accepts an `embeddings` tensor of dtype F32, F16 or I8; the three creators below
 * take the table AS STORED -- nothing is widened on the host or in HBM, a half table occupies V x 512 bytes and an int8 table
 * V x 256 -- and K1 widens the rows in registers (half -> f32 and i8 as f32 are exact, I8 has no scale, as in model2vec-rs), so
 * every output row is bit-identical to that of an f32 model built from the widened table.  The three creators above are the
 * SMT_TABLE_F32 case of these.  An unknown dtype is SMT_E_INVALID; table_dev must be 16-byte aligned, else SMT_E_INVALID.
 * smt_embed / smt_embed_device are unchanged: the model carries its type. */
#define SMT_TABLE_F32 0 /* float, 1024-byte rows           */
#define SMT_TABLE_F16 1 /* IEEE binary16, 512-byte rows    */
#define SMT_TABLE_I8 2  /* signed 8-bit, 256-byte rows     */
int smt_model_create_typed(smt_ctx *ctx, const void *table_host, int table_dtype, uint64_t V, uint32_t D,
                           int normalize, smt_model **out);
int smt_model_create_from_file_typed(smt_ctx *ctx, const char *path, uint64_t byte_offset, int table_dtype, uint64_t V,
                                     uint32_t D, int normalize, smt_model **out);
int smt_model_create_from_device_typed(smt_ctx *ctx, const void *table_dev, int table_dtype, uint64_t V, uint32_t D,
                                       int normalize, smt_model **out);
/* what the model holds: its SMT_TABLE_* kind, row count and the bytes of the table in device memory; any out may be NULL */
int smt_model_info(const smt_model *model, int *table_dtype, uint64_t *V, uint64_t *table_bytes);

/* Indexed tables (vocabulary-quantised model2vec models: `embeddings` [n_rows x 256] shared by many tokens, `mapping` [n_tokens]
 * token id -> row, `weights` [n_tokens] one scalar per token).  A line's sum is, in token order,
 *     acc_d = acc_d + fl32(weights[t] * widen(table[mapping[t]][d]))        for every id t < n_tokens
 * (product rounded to f32, then added, no FMA), divided by max(count, 1) where the count includes ids >= n_tokens, then the usual norm
 * step: bit-identical to a plain SMT_TABLE_F32 model over the expanded table E'[t] = fl32(weights[t] * widen(table[mapping[t]])).
 * These semantics are this project's restatement of newer model2vec versions; they are not pinned against a crate.
 * mapping (u32) and weights (f32) have n_tokens entries; either may be NULL (identity / 1).  With mapping NULL, n_tokens must equal
 * n_rows.  Both NULL == smt_model_create*_typed.  The library keeps its own packed copy (8 B per token): the arrays may be
 * freed after the call.  SMT_E_INVALID, with nothing left allocated and *out untouched: unknown dtype, unaligned table_dev, n_tokens == 0
 * with an array given, mapping NULL and n_tokens != n_rows, a mapping entry >= n_rows, a weight that is not finite (the message names
 * the first such token).  smt_embed / smt_embed_device are unchanged: the model carries its form. */
int smt_model_create_indexed(smt_ctx *ctx, const void *table_host, int table_dtype, uint64_t n_rows, uint32_t D,
                             const uint32_t *mapping_host, const float *weights_host, uint64_t n_tokens, int normalize, smt_model **out);
int smt_model_create_from_file_indexed(smt_ctx *ctx, const char *path, uint64_t byte_offset, int table_dtype, uint64_t n_rows, uint32_t D,
                                       const uint32_t *mapping_host, const float *weights_host, uint64_t n_tokens, int normalize,
                                       smt_model **out);
int smt_model_create_from_device_indexed(smt_ctx *ctx, const void *table_dev, int table_dtype, uint64_t n_rows, uint32_t D,
                                         const uint32_t *mapping_dev, const float *weights_dev, uint64_t n_tokens, int normalize,
                                         smt_model **out);
/* the token side of a model (smt_model_info keeps reporting table rows and table bytes): the number of token ids it knows (a plain
 * model: its rows), whether it was given a mapping / weights, and the bytes of its token array (0 for a plain model); any out may be NULL */
int smt_model_token_info(const smt_model *model, uint64_t *n_tokens, int *has_mapping, int *has_weights, uint64_t *token_bytes);

/* Replaces the pool step of StaticModel::encode_with_args / encode_single
 * (call sites src/search/mod.rs:69,138,153; src/cmds/search.rs:136,154).
 * Tokenisation happens before this call -- on the host, or for pure-ASCII lines of a WordPiece tokenizer on the
 * device (section "tokenizer" below, smt_wordpiece_*): `ids` are the unk-filtered token ids of all
 * lines back to back, `offsets[n_lines+1]` the CSR boundaries.  Each line is
 * truncated to `max_tokens` ids (2048 for lines, 512 for queries; 0 = no cap),
 * rows are summed in token order in f32, divided by the count, and (if the
 * model normalises) divided by max(||v||, 1e-12).  An empty line gives the
 * zero vector.  Output goes to `out_host` [n_lines x D] and/or is appended to
 * `append_to` (first new row index in *first_row). Either may be NULL. */
int smt_embed(smt_model *model, const uint32_t *ids, const uint64_t *offsets, uint64_t n_lines,
              uint32_t max_tokens, float *out_host, smt_corpus *append_to, uint64_t *first_row);
/* everything resident: ids/offsets/out are device pointers; async on the stream */
int smt_embed_device(smt_model *model, const uint32_t *ids_dev, const uint64_t *offsets_dev,
                     uint64_t n_lines, uint32_t max_tokens, float *out_dev);

/* ---------------------------------------------------------------- tokenizer
 * Pure-ASCII lines through BertNormalizer -> BertPreTokenizer -> WordPiece on the device (wordpiece_kernels.hip): the
 * byte rules of the host tokenizer's ASCII path, the same ids.  A line the kernel does not cover -- a byte >= 0x80, or an added
 * token standing in it -- is FLAGGED and left to the caller, who may splice its ids in as a patch.
 *
 * The vocabulary as tokenizer.json has it: `pool` holds all pieces back to back (continuing pieces WITH their prefix), piece i is
 * [piece_off[i], piece_off[i + 1]) with id piece_id[i]; of a repeated piece the later entry wins.  A piece with a byte >= 0x80 can
 * never match and is left out.  unk_id -1: a word without a match yields nothing.  Everything is copied: the arrays may be freed
 * after smt_wordpiece_create. */
#define SMT_WP_NORMALIZER 1u /* a BertNormalizer is present (without it the two flags below mean nothing) */
#define SMT_WP_CLEAN_TEXT 2u /* \t \n \r become ' ', NUL / controls / DEL are dropped and JOIN their neighbours */
#define SMT_WP_LOWERCASE 4u  /* A-Z are lowered */
typedef struct smt_wordpiece smt_wordpiece;
typedef struct smt_wordpiece_params {
    const char *pool;
    const uint32_t *piece_off; /* [n_pieces + 1] */
    const uint32_t *piece_id;  /* [n_pieces] */
    uint64_t n_pieces;
    const char *prefix; /* continuing_subword_prefix ("##") */
    uint32_t prefix_len;
    int64_t unk_id;
    uint32_t max_input_chars_per_word;
    uint32_t flags;            /* SMT_WP_* */
    const char *added_pool;    /* pure-ASCII added tokens matched on the raw text: a line in which one stands is FLAGGED */
    const uint32_t *added_off; /* [n_added + 1] */
    uint32_t n_added;
} smt_wordpiece_params;
int smt_wordpiece_create(smt_ctx *ctx, const smt_wordpiece_params *p, smt_wordpiece **out);
void smt_wordpiece_destroy(smt_wordpiece *tok);

/* The UTF-8 form of the same tokenizer (wordpiece_utf8_kernels.hip, DESIGN 4.9 "WordPiece over UTF-8 lines"): the handle and the
 * calls below are shared, only pass 1 differs.  BertNormalizer and BertPreTokenizer act on one code point without context, so the
 * caller states what every code point >= U+0080 becomes: n sorted, disjoint ranges first[i] .. last[i] (>= U+0080, <= U+10FFFF),
 * each with a class and an output, out_pool[out_off[i], out_off[i + 1]), valid UTF-8.  An empty output on a class other than DROPPED
 * and FLAG means "itself" (one character); a range with an explicit output is a single code point.  A code point in no range is
 * FLAG.  ASCII keeps coming from p->flags.
 *   ORDINARY  every output character is a character of a word (there may be several: a Hangul syllable becomes its jamo)
 *   SPACE     white space: ends a word, yields nothing (an explicit output is not used)
 *   ALONE     the output is ONE character that is a word by itself: punctuation, a CJK character (given WITHOUT the two spaces)
 *   DROPPED   no output; the neighbours join
 *   FLAG      the line is left to the caller
 * An output may not hold more characters than the UTF-8 form of `first` has bytes: a word's tokens then fit into the word's own
 * bytes, as in the ASCII form.  All pieces enter the table, those with bytes >= 0x80 too; max_input_chars_per_word counts
 * normalised CHARACTERS; the continuing prefix and the added tokens stay pure ASCII.
 * A line is FLAGGED for an added token standing in it, a FLAG code point, malformed UTF-8 (a lone continuation byte, a sequence cut
 * by the line's end, an overlong form, a surrogate, a value above U+10FFFF), or ANY byte >= 0x80 within the looked-at bytes of a line
 * that is longer than keep_bytes: the host layer cuts such a line by characters, the kernel by bytes, and the two agree only while
 * the looked-at part is ASCII.  Malformed input ends in a flag, never in an access outside the text.
 * SMT_E_INVALID, before anything is uploaded, for ranges out of order or overlapping, offsets that decrease, an unknown class, an
 * output that is not UTF-8 or too long, an explicit output on a range of several code points or on DROPPED / FLAG, an ALONE output
 * of more than one character, a non-ASCII added token.  Everything is copied. */
#define SMT_WP_CP_ORDINARY 0u
#define SMT_WP_CP_SPACE 1u
#define SMT_WP_CP_ALONE 2u
#define SMT_WP_CP_DROPPED 3u
#define SMT_WP_CP_FLAG 4u
typedef struct smt_wordpiece_codepoints {
    const uint32_t *first;   /* [n] */
    const uint32_t *last;    /* [n] */
    const uint8_t *cls;      /* [n] SMT_WP_CP_* */
    const char *out_pool;
    const uint32_t *out_off; /* [n + 1] */
    uint64_t n;
} smt_wordpiece_codepoints;
int smt_wordpiece_create_utf8(smt_ctx *ctx, const smt_wordpiece_params *p, const smt_wordpiece_codepoints *cp, smt_wordpiece **out);
/* what the handle holds on the device: all of its table in bytes, the code-point part of it (page index + distinct pages + outputs;
 * 0 for the ASCII form), and which form it is.  Any out may be NULL. */
int smt_wordpiece_info(const smt_wordpiece *tok, uint64_t *table_bytes, uint64_t *codepoint_bytes, int *utf8);

/* Pass 1: tokenize.  text_dev: text_bytes bytes; line i is [line_begin[i], line_begin[i] + line_len[i]) of them.  The lines lie in
 * line order and do not overlap (line_begin[i] + line_len[i] <= line_begin[i + 1]; gaps and no separators are both fine) and end
 * inside the text: the work is dealt by text position, so the host form checks this, and the device form trusts it -- a list that
 * breaks the rule gives unspecified ids, but no access outside the text.  Only the first min(line_len[i], keep_bytes) bytes of a
 * line are looked at (keep_bytes = max_tokens * median token length, the truncation of the host layer; 0 = no cut).
 * counts_dev[i] = ids the line yields after the unk drop (drop_unk != 0) and the max_tokens cap (0 = none); flags_dev[i] != 0: not
 * covered (a byte >= 0x80 within the looked-at bytes, or an added token standing there), count 0.  *n_flagged_dev = flagged lines.
 * Enqueued on the context's stream; does not wait.  The ids stay inside `tok` for pass 2; the four per-line arrays must stay
 * valid and unchanged until pass 2 has run.  One scan at a time per tokenizer: a second scan forgets the first. */
int smt_wordpiece_scan_device(smt_wordpiece *tok, const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev,
                              const uint32_t *line_len_dev, uint64_t n_lines, uint32_t keep_bytes, uint32_t max_tokens,
                              int drop_unk, uint32_t *counts_dev, uint8_t *flags_dev, uint32_t *n_flagged_dev);
/* Pass 2: lay the ids of the last scan out as the CSR smt_embed_device reads.  Optional patch: the ids of n_patch lines (sorted
 * line numbers, each flagged by pass 1; a patch for a line that is not flagged is ignored) tokenized elsewhere, n_patch_ids in
 * all, spliced in at their place.  ids_cap >= min(text_bytes, n_lines * keep_bytes) + n_patch_ids always suffices (a token is at
 * least one byte); less is SMT_E_INVALID before anything is enqueued.  Enqueued on the context's stream; does not wait. */
int smt_wordpiece_emit_device(smt_wordpiece *tok, uint64_t n_lines, const uint64_t *patch_line_dev,
                              const uint64_t *patch_off_dev /* [n_patch + 1] */, const uint32_t *patch_ids_dev, uint64_t n_patch,
                              uint64_t n_patch_ids, uint32_t *ids_out_dev, uint64_t ids_cap, uint64_t *offsets_out_dev /* [n_lines + 1] */);
/* Host convenience (tests, small callers): upload, both passes without a patch, download.  ids_cap >= the looked-at bytes of all
 * lines, else SMT_E_INVALID; a line list out of order, overlapping or outside the text (its end is taken as the largest line
 * end) likewise.  flags_out may be NULL. */
int smt_wordpiece_tokenize(smt_wordpiece *tok, const char *text, const uint64_t *line_begin, const uint32_t *line_len,
                           uint64_t n_lines, uint32_t keep_bytes, uint32_t max_tokens, int drop_unk, uint32_t *ids_out,
                           uint64_t ids_cap, uint64_t *offsets_out, uint8_t *flags_out);

/* Pure-ASCII lines through a per-byte normalizer -> Metaspace -> Unigram on the device (unigram_kernels.hip): the ids of
 * the host tokenizer's Viterbi (f64 sums, one add per edge; among equal sums for one end the smallest start wins; consecutive
 * unknowns of a piece fuse).  byte_map[c] is what byte c < 0x80 becomes: an ASCII byte (' ' = a space, which Metaspace turns into
 * the replacement character and which starts a piece), or 0xFF = dropped.  The vocabulary as tokenizer.json has it: piece i is
 * [piece_off[i], piece_off[i + 1]) of `pool` with id piece_id[i] and score scores[i]; of a repeated piece the later entry wins.  A
 * piece with a byte >= 0x80 other than a leading replacement cannot match and is left out of the table (it still counts for the
 * longest piece).  unk_score: what an unknown character costs (the vocabulary's lowest score - 10); unk_id -1: none.  A line is
 * FLAGGED for a byte >= 0x80, an added token standing in it, an unknown character on its best path while unk_id is -1, or a piece
 * whose raw bytes (its space, dropped bytes and a prepended replacement counted) exceed SMT_UG_MAX_WORD -- or, after
 * smt_unigram_set_long_pieces, the limit set there.  Everything is copied. */
#define SMT_UG_MAX_WORD 64
#define SMT_UG_MAX_LONG 2048
typedef struct smt_unigram smt_unigram;
typedef struct smt_unigram_params {
    const char *pool;
    const uint32_t *piece_off; /* [n_pieces + 1] */
    const uint32_t *piece_id;  /* [n_pieces] */
    uint64_t n_pieces;
    const double *scores; /* [n_pieces] */
    double unk_score;
    int64_t unk_id;
    const char *replacement; /* Metaspace's replacement character as UTF-8: one character >= U+0080 */
    uint32_t replacement_len;
    uint32_t prepend;          /* 0 always, 1 first, 2 never */
    const uint8_t *byte_map;   /* [128] */
    const char *added_pool;    /* pure-ASCII added tokens matched on the raw text: a line in which one stands is FLAGGED */
    const uint32_t *added_off; /* [n_added + 1] */
    uint32_t n_added;
} smt_unigram_params;
int smt_unigram_create(smt_ctx *ctx, const smt_unigram_params *p, smt_unigram **out);
/* The UTF-8 form of the same tokenizer (unigram_utf8_kernels.hip, DESIGN 4.9 "Unigram over UTF-8 lines"): the handle and the calls
 * below are shared, only pass 1 differs.  The normalizers this form serves act on one code point without context, so the caller
 * states what every code point >= U+0080 becomes, with the struct and the rules of smt_wordpiece_create_utf8.  Behind Metaspace the
 * classes mean:
 *   ORDINARY  every output character is a character of a piece (there may be several: a Hangul syllable becomes its jamo, and a
 *             piece may end between them)
 *   SPACE     the code point becomes exactly U+0020: Metaspace turns it into the replacement, and it starts a piece.  The
 *             replacement's own code point is stated as SPACE when the normalizer leaves it alone: Metaspace splits at it too
 *   DROPPED   no output
 *   FLAG      the line is left to the caller (a code point in no range is FLAG)
 *   ALONE     has no meaning here: SMT_E_INVALID
 * ASCII keeps coming from p->byte_map.  An output may not hold more characters than the UTF-8 form of `first` has bytes: a piece's
 * tokens <= its normalised characters <= its raw bytes, so the slot rule of the ASCII form holds.  All pieces enter the table, those
 * with bytes >= 0x80 too; SMT_UG_MAX_WORD (and the limit of smt_unigram_set_long_pieces) stays in raw bytes, with a SPACE character
 * of any length counted as one; the added tokens stay pure ASCII.
 * A line is FLAGGED for what flags it in the ASCII form other than a byte >= 0x80, and for a FLAG code point, malformed UTF-8 (a lone
 * continuation byte, a sequence cut by the line's looked-at end, an overlong form, a surrogate, a value above U+10FFFF, a byte that
 * leads nothing), or ANY byte >= 0x80 within the looked-at bytes of a line longer than keep_bytes (the host layer cuts such a line by
 * characters).  Malformed input ends in a flag, never in an access outside the text.
 * SMT_E_INVALID, before anything is uploaded, for what smt_wordpiece_create_utf8 refuses in the ranges, for a range of class ALONE,
 * and for a non-ASCII added token.  Everything is copied. */
int smt_unigram_create_utf8(smt_ctx *ctx, const smt_unigram_params *p, const smt_wordpiece_codepoints *cp, smt_unigram **out);
/* what the handle holds on the device: all of its table in bytes, the code-point part of it (0 for the ASCII form), and which form
 * it is.  Any out may be NULL. */
int smt_unigram_info(const smt_unigram *tok, uint64_t *table_bytes, uint64_t *codepoint_bytes, int *utf8);
void smt_unigram_destroy(smt_unigram *tok);
/* 0 (the default) = today's behaviour: a piece over SMT_UG_MAX_WORD raw bytes flags its line.
 * Otherwise SMT_UG_MAX_WORD < max_raw_bytes <= SMT_UG_MAX_LONG: pieces up to that measure are tokenized on the device by
 * ug_long_kernel, same ids as the host tokenizer; pieces over it flag the line.  Any other value: SMT_E_INVALID.  Takes effect
 * from the next scan; both forms of the handle. */
int smt_unigram_set_long_pieces(smt_unigram *tok, uint32_t max_raw_bytes);
/* The space rules an XLM-R-style chain puts around Metaspace (unigram_rules_kernels.hip, DESIGN 4.9 "Behind a Precompiled normalizer").
 * 0, 0 (the default) = today's behaviour, bit for bit, by today's kernels.
 * collapse_runs 1: a SPACE character whose nearest earlier not-dropped character of the line is a SPACE too is absorbed -- it starts
 *   no piece and ends none, and counts toward the measure of the piece in front like a dropped byte: "a  b" is R+a, R+b.
 * drop_trailing 1: a piece that is the replacement alone and ends at the line's looked-at end emits nothing: "a " is R+a.  A line
 *   whose ONLY piece is such a one (spaces and dropped characters, nothing else) is FLAGGED.
 * LONG PIECES: while a rule is on, a piece over SMT_UG_MAX_WORD raw bytes flags its line whatever smt_unigram_set_long_pieces set,
 *   and smt_unigram_long_stats answers 0, 0 -- unless smt_unigram_set_long_rules (below) switched the long pieces on under the rules
 *   too.  A SPACE character with more than SMT_UG_MAX_WORD raw bytes of dropped characters directly in front of it flags its line
 *   either way (the look-back bound of the device form).  Other values: SMT_E_INVALID.  Takes effect from the next scan; both forms. */
int smt_unigram_set_space_rules(smt_unigram *tok, int collapse_runs, int drop_trailing);
/* Long pieces under the space rules (unigram_long_rules_kernels.hip, DESIGN 4.9 "long pieces under the space rules").  0 (the
 * default) = today's behaviour.  1: while a space rule is on AND smt_unigram_set_long_pieces set a limit, a piece over
 * SMT_UG_MAX_WORD raw bytes and within that limit is tokenized on the device by ug_long_rules_kernel instead of flagging its line,
 * same ids as the host tokenizer, and smt_unigram_long_stats reports what that kernel measured.  The measure is the one of the
 * rules: the owner's SPACE character counts one, every raw byte behind it up to the piece's end counts too, absorbed space, dropped
 * or kept.  Under drop_trailing a long piece without a kept character at the line's looked-at end emits nothing, and FLAGS the line
 * when it is the line's first piece.  With rules 0, 0, or without a limit, the switch is inert: the same kernels, the same bytes.
 * Any other value: SMT_E_INVALID.  Takes effect from the next scan; both forms of the handle. */
int smt_unigram_set_long_rules(smt_unigram *tok, int on);
/* witness for tests and profiles: long pieces the last scan handed to ug_long_kernel and their raw bytes; waits for the stream.
 * Counted are the pieces the kernel measured to their end within the limit (a piece that runs into a byte or character that flags
 * its line, or over the limit, is not), each with its measure: its raw bytes, the SPACE character or a prepended replacement counted
 * as one.  Under the space rules (smt_unigram_set_long_rules) the measure is theirs, absorbed spaces counted, and a piece that
 * drop_trailing then leaves without a token -- no kept character, at the line's looked-at end -- is counted too: it was measured to
 * its end within the limit.  Both 0 after a scan with the switch off.  Either out may be NULL. */
int smt_unigram_long_stats(smt_unigram *tok, uint64_t *pieces, uint64_t *raw_bytes);
/* The two passes and the host convenience: the contracts of smt_wordpiece_scan_device / _emit_device / _tokenize, with one
 * difference: a line can hold one token more than looked-at bytes (the prepended replacement), so
 * ids_cap >= min(text_bytes, n_lines * keep_bytes) + n_lines + n_patch_ids for the device form, and the looked-at bytes of all
 * lines + n_lines for smt_unigram_tokenize; less is SMT_E_INVALID before anything is enqueued. */
int smt_unigram_scan_device(smt_unigram *tok, const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev,
                            const uint32_t *line_len_dev, uint64_t n_lines, uint32_t keep_bytes, uint32_t max_tokens, int drop_unk,
                            uint32_t *counts_dev, uint8_t *flags_dev, uint32_t *n_flagged_dev);
int smt_unigram_emit_device(smt_unigram *tok, uint64_t n_lines, const uint64_t *patch_line_dev,
                            const uint64_t *patch_off_dev /* [n_patch + 1] */, const uint32_t *patch_ids_dev, uint64_t n_patch,
                            uint64_t n_patch_ids, uint32_t *ids_out_dev, uint64_t ids_cap, uint64_t *offsets_out_dev /* [n_lines + 1] */);
int smt_unigram_tokenize(smt_unigram *tok, const char *text, const uint64_t *line_begin, const uint32_t *line_len, uint64_t n_lines,
                         uint32_t keep_bytes, uint32_t max_tokens, int drop_unk, uint32_t *ids_out, uint64_t ids_cap,
                         uint64_t *offsets_out, uint8_t *flags_out);

/* -------------------------------------------------------------- lower-casing
 * The lines of --ignore-case (reference src/search/mod.rs:63-67: every line through str::to_lowercase before it is embedded) lowered
 * on the device (lower_kernels.hip, DESIGN 4.9 "Lower-casing"), so that they can go on into a device tokenizer without a host pass.
 * Line i of the output is byte for byte what the host layer's to_lowercase (smt_host_to_lowercase) returns for line i ALONE:
 *   ASCII A-Z get + 32; every other ASCII byte, NUL included, stays.  ASCII is fixed: the tables state code points >= U+0080 only,
 *     the ASCII letters count as cased, and ' . : ^ ` as case-ignorable.
 *   A code point cp inside a run [run_first, run_last] becomes cp + run_delta when (cp - run_first) % run_stride == 0, else itself.
 *   A multi entry (multi_cp -> multi_n code points multi_to[3 * i ..]) is expanded; it goes before the runs.
 *   final_sigma != 0: U+03A3 becomes U+03C2 when it is preceded by a cased code point and not followed by one, case-ignorable code
 *     points skipped on both sides (a code point in both sets is skipped), and U+03C3 otherwise.  The look never leaves the line: the
 *     previous line's last letter is no context, even with no separator between the lines.  final_sigma == 0: U+03A3 is a code point
 *     like any other.
 *   A code point in no table stays.
 * Byte lengths change both ways (U+0130 2 -> 3, U+023A 2 -> 3, U+212A 3 -> 1, U+212B, U+2126, U+1E9E 3 -> 2); a line of n bytes yields
 * at most n + n / 2, which smt_lower_tables_check holds every table to.
 * smt_lower_tables_check (host only, needs no device) returns SMT_E_INVALID for: ranges or runs out of order or overlapping; last <
 * first; stride 0; a delta that leaves [0, U+10FFFF] or lands on a surrogate; a multi entry with n outside 1 .. 3, with an invalid
 * target (above U+10FFFF, a surrogate), or out of order; a multi code point that also lies in a run; any entry below U+0080; a mapping
 * that grows a code point by more than half its bytes (two bytes to four, a multi entry likewise); more entries than the device form
 * holds in LDS (256 runs, 8 multi entries, 192 cased and 512 case-ignorable ranges).  All arrays sorted by `first`; everything is
 * copied by smt_lower_create. */
typedef struct smt_lower smt_lower;
typedef struct smt_lower_tables {
    const uint32_t *run_first; /* [n_runs] */
    const uint32_t *run_last;
    const int32_t *run_delta;
    const uint32_t *run_stride;
    uint64_t n_runs;
    const uint32_t *multi_cp; /* [n_multi] */
    const uint32_t *multi_n;
    const uint32_t *multi_to; /* [n_multi * 3] */
    uint64_t n_multi;
    const uint32_t *cased_first; /* [n_cased] */
    const uint32_t *cased_last;
    uint64_t n_cased;
    const uint32_t *ignorable_first; /* [n_ignorable] */
    const uint32_t *ignorable_last;
    uint64_t n_ignorable;
    uint32_t final_sigma; /* != 0: U+03A3 follows the Final_Sigma rule */
} smt_lower_tables;
int smt_lower_tables_check(const smt_lower_tables *t /* NULL: the library's own tables, those of smt_lower_create(ctx, NULL, ..) */);
/* t == NULL: Rust's str::to_lowercase, from the arrays the host layer's to_lowercase reads (Unicode 13), final_sigma on.  Otherwise
 * the caller's tables, refused with SMT_E_INVALID before anything is uploaded when smt_lower_tables_check refuses them. */
int smt_lower_create(smt_ctx *ctx, const smt_lower_tables *t, smt_lower **out);
void smt_lower_destroy(smt_lower *h);
/* Lower n_lines lines of text_dev.  The line list follows the rule of smt_wordpiece_scan_device: line i is [line_begin[i],
 * line_begin[i] + line_len[i]), the lines lie in line order and do not overlap, gaps are fine; the device form trusts the list -- one
 * that breaks the rule gives unspecified bytes, but no access outside [0, text_bytes) or [0, out_cap).
 * The lowered lines stand back to back in out_text_dev: out_begin[0] = 0, out_begin[i + 1] = out_begin[i] + out_len[i], and
 * out_begin[n_lines] is the total.  Bytes in gaps are neither read as context nor written; nothing at or beyond out_begin[n_lines] is
 * written.  out_cap >= text_bytes + text_bytes / 2 always suffices; less is SMT_E_INVALID before anything is enqueued.
 * The decode is the strict one of the UTF-8 tokenizers.  A line that holds ill-formed UTF-8 -- a lone continuation byte, a sequence cut
 * by the line's end, an overlong form, a surrogate, a value above U+10FFFF, 0xC0, 0xC1, 0xF5 .. 0xFF -- is FLAGGED: flags_dev[i] != 0,
 * out_len[i] = line_len[i], its bytes copied unchanged, for the caller to lower elsewhere (to_lowercase of the host layer passes such
 * bytes through one by one, which the device does not imitate).  *n_flagged_dev = flagged lines.  Ill-formed input ends in a flag,
 * never in a read outside the line.
 * The output depends on the input alone.  Enqueued on the context's stream; does not wait (but for the stream when an internal
 * buffer has to grow). */
int smt_lower_device(smt_lower *h, const uint8_t *text_dev, uint64_t text_bytes, const uint64_t *line_begin_dev,
                     const uint32_t *line_len_dev, uint64_t n_lines, uint8_t *out_text_dev, uint64_t out_cap,
                     uint64_t *out_begin_dev /* [n_lines + 1] */, uint32_t *out_len_dev, uint8_t *flags_dev, uint32_t *n_flagged_dev);
/* Host convenience (tests, small callers): upload, lower, download.  The text's end is taken as the largest line end; a line list
 * out of order or overlapping is SMT_E_INVALID, and so is out_cap below text_bytes + text_bytes / 2.  flags_out may be NULL. */
int smt_lower_lines(smt_lower *h, const char *text, const uint64_t *line_begin, const uint32_t *line_len, uint64_t n_lines, char *out_text,
              uint64_t out_cap, uint64_t *out_begin /* [n_lines + 1] */, uint32_t *out_len, uint8_t *flags_out);

/* ------------------------------------------------------------------- corpus
 * Replaces `Document::embeddings: Vec<Vec<f32>>` (src/search/mod.rs:18-22)
 * and the vector half of the workspace store (line_embeddings.qdrant,
 * src/workspace/store.rs:152-166, upsert :402-434): one row-major f32 matrix
 * [rows x D] resident in HBM; row index == insertion order. */
int smt_corpus_create(smt_ctx *ctx, uint32_t D, uint64_t capacity_rows, smt_corpus **out);
/* adopt rows already in device memory (not copied, not freed, not growable) */
int smt_corpus_from_device(smt_ctx *ctx, const float *rows_dev, uint64_t n_rows, uint32_t D,
                           smt_corpus **out);
void smt_corpus_destroy(smt_corpus *corpus);
int smt_corpus_append_host(smt_corpus *corpus, const float *rows, uint64_t n_rows,
                           uint64_t *first_row);
/* overwrite existing rows [first_row, first_row+n_rows) (upsert of a changed doc) */
int smt_corpus_write_rows(smt_corpus *corpus, uint64_t first_row, const float *rows,
                          uint64_t n_rows);
int smt_corpus_read_rows(smt_corpus *corpus, uint64_t first_row, uint64_t n_rows, float *out_host);
/* Forget the rows from n_rows on.  A host-side count: nothing is enqueued and the one-query pipeline is NOT drained -- calls
 * queued earlier keep the row count they were made with, a call made behind a truncation that dropped rows has another count and so
 * is not taken along by one of them (n_rows equal to the count drops nothing and changes nothing), and whatever writes the freed
 * rows next (append, embed, write_rows) drains first.  Every other call that changes what a
 * corpus holds drains the pipeline before it touches a row (append, write_rows, compact unless it keeps everything, prepack,
 * embed into the corpus, destroy). */
int smt_corpus_truncate(smt_corpus *corpus, uint64_t n_rows);
/* Keep exactly the rows inside `keep` (sorted, disjoint, inside [0, rows)), in order, and close the gaps IN PLACE:
 * afterwards the corpus holds sum(len) rows and old row keep[i].begin + j is row prefix[i] + j.  n_keep == 0 empties it.
 * What qdrant's optimiser does behind the reference's store when it vacuums deleted points (src/workspace/store.rs:152-166
 * opens the collection it maintains); here the rows move HBM to HBM (compact.hip), never through the host, and no second
 * corpus exists meanwhile.  Rows in front of the first dropped row are not touched; *rows_moved (may be NULL) = the kept rows
 * behind it.  A list that drops nothing is a no-op: no kernel is enqueued and 0 rows move -- so the row count never stays
 * the same while rows change places.
 *   - A list that is unsorted, overlapping or out of range: SMT_E_INVALID, the corpus untouched.
 *   - A corpus adopted with smt_corpus_from_device: SMT_E_UNSUPPORTED (its memory is the caller's to rearrange).
 *   - Ordering: the move runs after everything already enqueued on the context (its stream and the scan streams of the
 *     one-query pipeline, tuning keys async_select / scan_overlap) and before anything enqueued later; the call does not wait
 *     for the move itself.
 *   - The fp16 operand image is derived data: the tiles from the first moved row on are packed again by the next batch that
 *     wants them; the allocation and the prepack mode stay.  Kept range sets depend on ranges only and stay.
 *   - An smt_ivfpq built on the corpus names rows BY POSITION.  smt_ivfpq_compact (below, with the index) is this call AND the
 *     index following it: use it instead of this one.  An index that was not carried refuses to search after a compaction that
 *     dropped rows ("the corpus shrank ... rebuild"): destroy and rebuild it.
 * Steps whose gap is shorter than the bounce buffer go through it (tuning key compact_bounce_rows). */
int smt_corpus_compact(smt_corpus *corpus, const smt_range *keep, uint32_t n_keep, uint64_t *rows_moved /* may be NULL */);
/* smt_corpus_compact calls that succeeded on this context (no-ops included) and the rows they moved; any pointer may be NULL;
 * reset != 0 clears both. */
int smt_ctx_compact_stats(smt_ctx *ctx, uint64_t *calls, uint64_t *rows_moved, int reset);
/* The fp16 OPERAND IMAGE of a corpus: what the batched nomination modes multiply with (unit rows x 2^10 as fp16 in MFMA operand
 * order, 512 B per row beside the 1 KiB of f32), so that a batch of >= 8 queries reads half the bytes per row and converts
 * nothing.  Derived data only: nominations come from it, every returned distance is re-scored from the f32 rows, results are
 * identical with and without it.  A corpus whose memory the library owns builds and maintains it by itself (first batch of
 * >= 8 queries over >= 64 Ki rows, or the fourth smaller search of a shard of >= 4 M rows, which then answers single queries
 * from it as well; appends, writes and truncation are tracked; tuning key corpus_image = 0 turns that off).
 * smt_corpus_prepack(corpus, 1) builds it NOW from the rows as they are -- the way to have one for a corpus adopted with
 * smt_corpus_from_device, whose caller then answers for calling it again after changing rows; (corpus, 0) drops it and keeps the
 * corpus without one.  The shards of an smt_sharded_corpus are corpora like any other (smt_sharded_corpus_shard hands them out):
 * shards the library filled keep their images by themselves, adopted shards get one per shard through this call.
 * No reference counterpart (the reference scores Vec<Vec<f32>> rows one by one, src/search/mod.rs:84-119). */
int smt_corpus_prepack(smt_corpus *corpus, int enable);
uint64_t smt_corpus_image_bytes(const smt_corpus *corpus);
uint64_t smt_corpus_rows(const smt_corpus *corpus);
uint32_t smt_corpus_dim(const smt_corpus *corpus);
/* flat little-endian file: 32-byte header + rows*D f32 */
int smt_corpus_save(smt_corpus *corpus, const char *path);
int smt_corpus_load(smt_ctx *ctx, const char *path, smt_corpus **out);
/* Incremental flush: `path` must already hold exactly the first `rows_on_disk` rows of this corpus;
 * rows [rows_on_disk, rows) are appended and the header is updated (O(new rows), not O(corpus)). */
int smt_corpus_append_to_file(smt_corpus *corpus, const char *path, uint64_t rows_on_disk);

/* ------------------------------------------------------------------- search
 * Replaces f32::cosine + the selection in search_documents
 * (src/search/mod.rs:84-119) and Store::search_line_embeddings
 * (src/workspace/store.rs:481-546).
 *
 *   queries     host, [nq x D] f32
 *   max_distance NaN = "None".
 *   mode SMT_MODE_DOCUMENTS: max_distance None -> the top_k rows by
 *        (distance asc, row asc) [= the reference's stable sort + take(top_k)];
 *        max_distance given -> ALL rows with distance < max_distance (strict),
 *        same order, top_k ignored.
 *   mode SMT_MODE_WORKSPACE: rows with score > 1 - max_distance (f32, if given),
 *        then ALWAYS the top_k of them; top_k == 0 -> nothing.
 *   ranges      optional filter: only rows inside these sorted, disjoint
 *        ranges are scanned (workspace path subset; a document's lines are
 *        contiguous rows).  NULL/0 = whole corpus.
 *   row_base    added to every returned row (global index of this shard's row 0).
 *   out_rows/out_dist  [nq x out_cap]; out_counts[nq] = hits for each query
 *        (the TRUE count even when > out_cap, in which case the call returns
 *        SMT_E_TRUNCATED after filling the first out_cap of each).
 *
 * Distances are f64: the f32 scan only nominates candidates; every returned
 * distance is recomputed on the GPU with f64 accumulation in index order --
 * simsimd's "accurate" formula -- so results do not depend on reduction order.
 */
int smt_search(smt_corpus *corpus, const float *queries, uint32_t nq, uint32_t top_k,
               double max_distance, int mode, const smt_range *ranges, uint32_t n_ranges,
               uint64_t row_base, uint64_t *out_rows, double *out_dist, uint64_t *out_counts,
               uint64_t out_cap);

/* Resident top-k (mode DOCUMENTS, no threshold, no ranges): queries_dev
 * [nq x D] and outputs [nq x top_k] are device pointers; unused slots are
 * (row = UINT64_MAX, dist = +inf).  Enqueues on the stream, no sync.  1 <= top_k <= 1024 (57 .. 1024: the
 * sampled-threshold route, tuning key largek_sampled; with largek_sampled = 0, 1 <= top_k <= 56). */
int smt_search_topk_device(smt_corpus *corpus, const float *queries_dev, uint32_t nq,
                           uint32_t top_k, uint64_t row_base, uint64_t *out_rows_dev,
                           double *out_dist_dev);
/* The same with a verdict PER QUERY: search_documents returns a definite list (src/search/mod.rs:107-119), so a caller that
 * pipelines device calls must be able to tell which answer of which call is the proved exact top-k and which is not.
 * out_status_dev [nq] (device-addressable: HBM or pinned host; NULL = smt_search_topk_device) receives, in stream order with
 * the lists:
 *   SMT_STATUS_PROVED     the list IS the exact top-k (the select's exactness certificate held: "Exactness bookkeeping" below)
 *   SMT_STATUS_UNCERTAIN  more near-ties around the k-th place than the guard band holds: every returned (row, distance) pair is
 *                         exact, but a row outside the list may belong to it -- re-ask this query through smt_search
 *   SMT_STATUS_OVERFLOW   batched path only: a candidate buffer overflowed (adversarial row order) and rows were dropped on the
 *                         way; same remedy
 *   SMT_STATUS_INVALID_QUERY  the query is outside the library's domain ("Domain" at the top of this file: a non-finite
 *                         component or an absurd magnitude); the list means nothing.  smt_search refuses such a query instead
 * Queries with a non-zero status are also counted by smt_ctx_uncertain_count.  smt_search / smt_sharded_search never return such
 * a list: they re-answer the query exhaustively themselves. */
#define SMT_STATUS_PROVED 0
#define SMT_STATUS_UNCERTAIN 1
#define SMT_STATUS_OVERFLOW 2
#define SMT_STATUS_INVALID_QUERY 3
int smt_search_topk_device_ex(smt_corpus *corpus, const float *queries_dev, uint32_t nq,
                              uint32_t top_k, uint64_t row_base, uint64_t *out_rows_dev,
                              double *out_dist_dev, uint32_t *out_status_dev);

/* Merge `n_lists` sorted (dist asc, row asc) lists of length k_in each (padded
 * with UINT64_MAX/+inf) per query into the best k_out.  Inputs are laid out
 * [n_lists][nq][k_in] -- exactly what an all-gather of per-rank
 * smt_search_topk_device outputs produces.  The output is ordered (dist asc, row asc) and padded the same way.
 * Preconditions, of the host and of every device form:
 *   - rows are DISTINCT within a query across all lists (shards own disjoint rows).  Every candidate takes the output slot of its
 *     rank among the others; two equal (distance, row) pairs would take the same slot and leave a padding entry in the middle
 *     of the list (device forms; the host form would return the pair twice)
 *   - n_lists x k_in <= 8192 on the device forms; more is SMT_E_INVALID and nothing is written
 *   - padding is recognised by the ROW alone (UINT64_MAX); the distance stored beside it is never read
 * n_lists == 0 writes k_out padding entries per query, also with the output buffers given as the (unread) inputs.
 * Host version: */
int smt_merge_topk(const uint64_t *rows, const double *dist, uint32_t n_lists, uint32_t nq,
                   uint32_t k_in, uint32_t k_out, uint64_t *out_rows, double *out_dist,
                   uint64_t *out_counts);
/* device version (all pointers device, async on the stream) */
int smt_merge_topk_device(smt_ctx *ctx, const uint64_t *rows_dev, const double *dist_dev,
                          uint32_t n_lists, uint32_t nq, uint32_t k_in, uint32_t k_out,
                          uint64_t *out_rows_dev, double *out_dist_dev);

/* Packed variant: one buffer per rank [nq][2][k] of 8-byte words -- row ids, then the f64
 * distance bits -- so that ONE all-gather moves both.  packed_dev is the gathered
 * [n_lists][nq][2][k_in]; out_packed_dev receives [nq][2][k_out].  Device pointers, async. */
int smt_merge_topk_packed_device(smt_ctx *ctx, const uint64_t *packed_dev, uint32_t n_lists, uint32_t nq,
                                 uint32_t k_in, uint32_t k_out, uint64_t *out_packed_dev);

/* ----------------------------------------------------------------- IVF-PQ
 * Approximate index over a resident corpus (BASELINE config 5).  There is NO reference
 * counterpart: the reference's workspace store scans exactly (README's "IVF_PQ" is a stale
 * label); the contract is recall against smt_search on the same corpus.  Every returned
 * (row, distance) is exact -- candidates from the ADC scan are re-ranked with the exact f64
 * distance -- only top-k membership is approximate.  The index keeps a pointer to `corpus`,
 * which must stay alive and unchanged.  It is built for what model2vec emits -- UNIT rows (zero
 * rows are fine): its quantisers work on the rows as they are, not on their directions, so
 * smt_ivfpq_build / smt_ivfpq_append refuse a corpus holding rows of other lengths
 * (| |x|^2 - 1 | > 1e-3) with SMT_E_UNSUPPORTED; the exact searches have no such condition. */
typedef struct smt_ivfpq smt_ivfpq;
typedef struct smt_ivfpq_params {
    uint32_t nlist;        /* coarse lists: multiple of 32 in [32, 4096]                  */
    uint32_t m;            /* PQ sub-quantisers: 32 (dsub = 8)                            */
    uint32_t nbits;        /* 8                                                           */
    uint32_t train_iters;  /* k-means iterations for both quantisers (0 = 10)            */
    uint64_t train_sample; /* training rows, evenly spaced (0 = 64 * nlist)              */
    uint32_t reserved;     /* must be 0 (was `refine`: an int8 refinement stage, measured +6 % for a 7x larger index, removed) */
    uint32_t local_pca;    /* 0 = one global residual codebook set (8 dims x 256 codes per sub-quantiser);    */
                           /* 1 = per-list PCA: every list gets its own orthonormal basis of its 32 principal */
                           /* residual directions and one 8-bit scalar quantiser per direction (still 32 B    */
                           /* per row; + 32 KiB per list).  Ranks the rows inside a list far better on        */
                           /* clustered data -- the workspace store builds its index this way                 */
} smt_ivfpq_params;
int smt_ivfpq_build(smt_corpus *corpus, const smt_ivfpq_params *params, smt_ivfpq **out);
void smt_ivfpq_destroy(smt_ivfpq *index);
/* nprobe lists scanned per query; in every probed list UP TO `rerank` ADC candidates
 * (0 = 512; range [4, 512]) are re-scored against the full-precision rows inside the scan
 * kernel, and the best top_k + 8 of all lists get the exact f64 distance.  top_k <= 56
 * (smt_ivfpq_search_wide below takes up to 1024).
 * `rerank` is a budget, not a count: the codes of a list (of each 8192-code segment of a long
 * list) are dealt to the 4 or 8 waves of a block in groups of 64 (8 waves above a budget of 256;
 * when nprobe leaves a long list fewer segments than it wants, the budget per segment grows by the
 * same factor first), each wave keeps its own ceil(budget / waves) best, and it compares the top
 * 16 bits of the f32 ADC distance (a relative step of 2^-7).  A list of 64 rows lies in one wave: rerank = 64 re-scores 16 of
 * its rows, not all 64.  What IS guaranteed: a row is re-scored whenever fewer than
 * ceil(rerank / 8) rows of its list have an ADC distance <= its own * (1 + 2^-7); and a list of
 * at most 512 rows is re-scored entirely at rerank = 512 (tests/test_gpu_ivf_search_contract.py).
 * Outputs as in smt_search. */
int smt_ivfpq_search(smt_ivfpq *index, const float *queries, uint32_t nq, uint32_t top_k, uint32_t nprobe,
                     uint32_t rerank, uint64_t row_base, uint64_t *out_rows, double *out_dist,
                     uint64_t *out_counts, uint64_t out_cap);
/* Device-resident form: queries [nq x 256] f32 and the outputs [nq x top_k] (rows u64, padded with
 * UINT64_MAX; exact f64 distances, padded with +inf) live in device (or pinned host) memory; enqueued on
 * the context's stream, complete after smt_ctx_synchronize. */
int smt_ivfpq_search_device(smt_ivfpq *index, const float *queries_dev, uint32_t nq, uint32_t top_k, uint32_t nprobe,
                            uint32_t rerank, uint64_t row_base, uint64_t *out_rows_dev, double *out_dist_dev);
/* The same search INSIDE ROW RANGES (the path subset of a workspace search): only rows of `ranges` are candidates.  Ranges are
 * corpus-local row positions (before row_base is added), sorted and disjoint, begin <= end <= corpus rows, empty ones allowed, as in
 * smt_search; a violation, or ranges == NULL with n_ranges > 0, is SMT_E_INVALID, found before anything is enqueued.  n_ranges == 0
 * IS the unfiltered search: the same code path and the same bytes as smt_ivfpq_search.  Rows at or beyond the row count the index
 * covers (appended to the corpus, not yet taken in by smt_ivfpq_append) are not in the index and are never returned.  A query gets
 * fewer than top_k hits when its probed lists hold fewer rows of the ranges; counts and padding as in smt_ivfpq_search.
 * How: every call turns the ranges into a bitmap over the index's list positions (one pass over the 4 B row ids, nothing kept
 * between calls); the scan skips the positions whose bit is clear -- no code bytes are read for them -- and is otherwise the scan of
 * smt_ivfpq_search.  Its guarantee therefore carries over with "rows" read as "in-range rows": a row is re-scored whenever fewer
 * than ceil(rerank / 8) IN-RANGE rows of its list segment have an ADC distance <= its own * (1 + 2^-7); and a list with at most 512
 * in-range rows per segment is re-scored entirely at rerank = 512 (tests/test_gpu_ivf_ranges.py). */
int smt_ivfpq_search_ranges(smt_ivfpq *index, const float *queries, uint32_t nq, uint32_t top_k, uint32_t nprobe,
                            uint32_t rerank, const smt_range *ranges, uint32_t n_ranges, uint64_t row_base,
                            uint64_t *out_rows, double *out_dist, uint64_t *out_counts, uint64_t out_cap);
/* Device-resident form of the search inside ranges; `ranges` is a HOST array, copied into a pinned buffer of the context before the
 * call returns.  Enqueued like smt_ivfpq_search_device: the call does not wait for the stream (only, when ranged calls follow each
 * other, for the previous call's few-KiB range upload to have left that buffer). */
int smt_ivfpq_search_ranges_device(smt_ivfpq *index, const float *queries_dev, uint32_t nq, uint32_t top_k, uint32_t nprobe,
                                   uint32_t rerank, const smt_range *ranges, uint32_t n_ranges, uint64_t row_base,
                                   uint64_t *out_rows_dev, double *out_dist_dev);
/* WIDE searches: 1 <= top_k <= 1024 (the host form also takes 0), with or without ranges in one entry point.  ranges == NULL is the
 * unfiltered search; a non-NULL `ranges` is a filter even with n_ranges == 0 (an empty filter: every answer is empty); the rules for
 * the ranges themselves are those of smt_ivfpq_search_ranges.  top_k <= 56 is forwarded to the narrow route above and returns the
 * same bytes.  For 57 <= top_k <= 1024 the answer is DEFINED as follows.  Let C(q) be the rows that the scan re-scores in f32 for
 * query q: the same set the narrow route draws from, for the same nprobe, rerank and list segments (every guarantee stated for
 * smt_ivfpq_search / _ranges about which rows are re-scored holds unchanged).  Let S be the kg = min(|C|, top_k + max(64, top_k / 16))
 * rows of C with the smallest (f32 re-scored distance, row) keys.  The answer is the top_k best rows of S by (exact f64 distance,
 * row), with their exact distances; when C holds fewer than top_k rows the answer is shorter.  Counts and padding as in
 * smt_ivfpq_search.  In particular, where every list segment is re-scored entirely (lists of at most 512 rows at rerank = 512) the
 * answer is the exact top_k over the rows of the probed lists (tests/test_gpu_ivf_wide.py).
 * How: the scan writes every re-scored row of a query into a candidate pool in the context's scratch -- nprobe x segments x 256 or
 * 512 keys, at most 2 MiB per query -- and one block per query selects S from it (radix select on the 64-bit keys: deterministic,
 * ties by row) and finishes exactly.  A batch whose pool would pass 256 MiB runs in rounds of queries.
 * The host form waits for its answer.  The device form is enqueued on the context's stream and does not wait, except when the
 * context's scratch has to grow (and, inside ranges, as smt_ivfpq_search_ranges_device does). */
int smt_ivfpq_search_wide(smt_ivfpq *index, const float *queries, uint32_t nq, uint32_t top_k, uint32_t nprobe,
                          uint32_t rerank, const smt_range *ranges, uint32_t n_ranges, uint64_t row_base,
                          uint64_t *out_rows, double *out_dist, uint64_t *out_counts, uint64_t out_cap);
int smt_ivfpq_search_wide_device(smt_ivfpq *index, const float *queries_dev, uint32_t nq, uint32_t top_k, uint32_t nprobe,
                                 uint32_t rerank, const smt_range *ranges, uint32_t n_ranges, uint64_t row_base,
                                 uint64_t *out_rows_dev, double *out_dist_dev);
/* build_ms4 = {coarse k-means, assign all rows, PQ training, sort + encode} */
int smt_ivfpq_info(const smt_ivfpq *index, uint64_t *n_rows, uint32_t *nlist, uint64_t *index_bytes,
                   double *build_ms4);
int smt_ivfpq_list_sizes(const smt_ivfpq *index, uint64_t *sizes_host /* [nlist] */);
/* Persist / restore the index (centroids, quantisers, list table, ids, codes: ~36 B per row).  The file
 * refers to corpus rows by position: load fails with SMT_E_INVALID unless `corpus` holds AT LEAST the
 * row count the index covers (then smt_ivfpq_append if the corpus only grew; smt_ivfpq_compact carries a loaded index through a
 * compaction; else rebuild -- 0.5 s per 10 M rows). */
int smt_ivfpq_save(smt_ivfpq *index, const char *path);
int smt_ivfpq_load(smt_corpus *corpus, const char *path, smt_ivfpq **out);
/* Incremental insert: rows appended to the corpus since the index was built (or last extended) are assigned to
 * their nearest list and encoded with that list's EXISTING quantiser (no retraining), then merged into the
 * inverted lists -- O(new rows) arithmetic plus one 36 B/row re-layout.  *n_added = rows taken in (may be NULL).
 * The quantisers drift away from the data as it grows: rebuild when the corpus has roughly doubled. */
int smt_ivfpq_append(smt_ivfpq *index, uint64_t *n_added);
/* Compact the corpus AND carry the index along, instead of a rebuild.  The call compacts index->corpus exactly as smt_corpus_compact
 * would -- the same validation, ordering rules, *rows_moved, effect on the image and on kept range sets -- and the index then describes
 * the compacted corpus.  One call on purpose: the index update needs the keep list in the row numbering from BEFORE the compaction.
 * With P the list's prefix map (old row keep[i].begin + j -> prefix[i] + j) and n_old the rows the index covered:
 *   ids      P(id) of every kept entry and nothing else, in their old relative order: every list stays ascending by row
 *   codes    the kept entries' 32 bytes, unchanged
 *   offsets  offsets[l] = kept entries in front of list l; offsets[nlist] = the new covered row count = the kept rows below n_old
 *   rows at or past n_old stay uncovered, as before the call: a later smt_ivfpq_append takes them in
 *   centroids, |c|^2 / 2, codebooks, per-list bases and scales: the same allocations, the same bytes
 *   *entries_dropped (may be NULL) = n_old - the new covered row count
 * One stable stream compaction over the 36-byte entries and an id remap (ivfpq_compact.hip), out of place into fresh arrays sized for
 * the kept count; no k-means, no quantiser fit, no encode, no sort.  The quantisers stay fitted to the rows of the build, as with
 * smt_ivfpq_append.
 *   - A list that drops nothing is a no-op for the index too: no kernel, no allocation, *entries_dropped = 0.
 *   - Refused with the corpus AND the index untouched: an invalid list (SMT_E_INVALID), a corpus adopted with
 *     smt_corpus_from_device (SMT_E_UNSUPPORTED), a list that keeps no row the index covers (SMT_E_UNSUPPORTED -- compact the
 *     corpus alone and rebuild: this call never leaves an empty index).
 *   - If the rows moved and the index then could not follow (memory, a HIP error), the index is marked stale: every later search,
 *     append, save or compact on it returns SMT_E_INVALID ("... rebuild").  It is never left half updated.
 *   - The call drains the one-query pipeline first and waits for the context's stream before it frees the old arrays: device
 *     searches enqueued earlier complete with the answers of the corpus as it was.
 *   - Only THIS index is carried.  A second smt_ivfpq on the same corpus is not: it is what an index is after smt_corpus_compact --
 *     destroy and rebuild it. */
int smt_ivfpq_compact(smt_ivfpq *index, const smt_range *keep, uint32_t n_keep, uint64_t *rows_moved /* may be NULL */,
                      uint64_t *entries_dropped /* may be NULL */);

/* ------------------------------------------------------- groups of GPUs (RCCL)
 * The reference runs the whole search synchronously from ONE task of ONE process (src/bin/semtools.rs:134-135,
 * src/cmds/search.rs:197-206); these entry points let that one caller use every GPU of the node.  There is no
 * reference counterpart for the sharding itself; the contract is: sharded result == single-shard result.
 *
 *   smt_init(devices, n)            process-wide default group; NULL / 0 = every visible GPU;
 *                                   idempotent for the same list.  smt_shutdown() releases it.
 *   smt_group_create(devices, n)    single process: one context + stream per device, ncclCommInitAll.
 *   smt_group_unique_id / smt_group_create_rank
 *                                   one rank per process (torchrun / MPI): rank 0 makes the 128-byte id, the host
 *                                   broadcasts it by any means, every process joins with its device and rank
 *                                   (ncclCommInitRank).  Calls on the group are then SPMD: every process makes
 *                                   the same calls with the same host arguments.
 * RCCL (librccl.so.1) is loaded when the first group is created, not when the library is. */
typedef struct smt_group smt_group;
typedef struct smt_sharded_corpus smt_sharded_corpus;
#define SMT_UNIQUE_ID_BYTES 128
int smt_init(const int *devices, int n_dev);
int smt_shutdown(void);
smt_group *smt_default_group(void);
int smt_group_create(const int *devices, int n_dev, smt_group **out);
/* n_shards logical ranks on ONE device, exchanging through device copies instead of RCCL (RCCL refuses two
 * ranks on one GPU): lets a single-GPU box run the whole sharded path -- the GPU tests do -- and splits a
 * corpus into independently growable shards.  smt_group_info reports rccl_ranks = 0 for such a group. */
int smt_group_create_logical(int device, int n_shards, smt_group **out);
/* A ONE-rank group around an existing context (which the caller keeps and destroys after the group): every smt_sharded_*
 * entry point then forwards to its single-GPU counterpart on that context -- no RCCL is loaded, nothing is exchanged.
 * It lets a host layer written against the sharded API serve the default single-GPU case at single-GPU cost. */
int smt_group_from_ctx(smt_ctx *ctx, smt_group **out);
int smt_group_unique_id(void *id_out /* SMT_UNIQUE_ID_BYTES */);
int smt_group_create_rank(int device, int rank, int n_ranks, const void *unique_id, smt_group **out);
void smt_group_destroy(smt_group *group);
/* n_ranks: size of the group; n_local: GPUs driven by this process (ranks first_rank .. first_rank+n_local-1);
 * rccl_ranks: what ncclCommCount reports for the communicator; rccl_version: ncclGetVersion.  Any may be NULL. */
int smt_group_info(const smt_group *group, int *n_ranks, int *n_local, int *first_rank, int *rccl_ranks, int *rccl_version);
/* the context of local device i (tuning keys, profiling, smt_model_create / smt_embed on that GPU); NULL if out of range */
smt_ctx *smt_group_ctx(smt_group *group, int local_index);
int smt_group_synchronize(smt_group *group); /* every local stream, async pipelines drained */
int smt_group_barrier(smt_group *group);     /* + an all-gather across the ranks */
/* How the per-shard k-lists of a sharded top-k search meet ("all-gather of the per-shard top-k"):
 *   SMT_TRANSPORT_RCCL  one ncclAllGather of the packed lists, then merge_topk_kernel.  The only choice when the ranks are
 *                       separate processes (smt_group_create_rank); available to smt_group_create groups.
 *   SMT_TRANSPORT_COPY  logical groups: the same all-gather made of event-ordered device copies.
 *   SMT_TRANSPORT_PEER  one-process groups (smt_group_create when every device can read every other's memory -- peer access is
 *                       enabled at creation --, smt_group_create_logical): nothing is gathered; the merge kernel of the device
 *                       that needs the answer reads the ranks' lists where they lie, ordered by one stream event per rank.
 *                       DEFAULT wherever it is possible: an answer costs n - 1 stream waits (enqueued by the ranks' issuing threads)
 *                       and one launch instead of RCCL's per-call host cost for a 960-byte payload.
 * $SEMTOOLS_GROUP_TRANSPORT = rccl | copy | peer overrides the default at creation (ignored where impossible).
 * smt_group_set_transport synchronises the group first; SMT_E_INVALID if the group cannot use that transport.
 * Threshold mode / large k (host-list exchange), barriers and the shared-centroid all-reduce always use RCCL (or copies). */
#define SMT_TRANSPORT_RCCL 0
#define SMT_TRANSPORT_COPY 1
#define SMT_TRANSPORT_PEER 2
int smt_group_set_transport(smt_group *group, int transport);
int smt_group_transport(const smt_group *group); /* SMT_TRANSPORT_*; negative = error */

/* A corpus row-sharded over the group.  Global row = position in the whole corpus = INSERTION ORDER (the reference's tie
 * order: document, then line -- src/search/mod.rs:84-85,107-111).  A corpus made in one go is cut into contiguous ranges,
 * rows_per_rank = ceil(N / n_ranks) (a document's lines and the path-subset ranges stay ranges).  A corpus
 * that GROWS (the workspace store: src/workspace/store.rs:402-434 appends, never rewrites) deals every append over the
 * ranks -- the emptier shards are filled first, a handful of rows goes to one shard -- so that all GPUs keep equal shares;
 * the numbering is then a list of pieces (smt_sharded_corpus_layout).  Inside a shard local order == global order.
 *   create       empty corpus (rows arrive through smt_sharded_embed / append_host)
 *   from_host    `rows` is the WHOLE matrix [total_rows x D]; every process uploads the slices of its local ranks.
 *   from_device  adopt one resident buffer per LOCAL device (not copied, not freed); the ranks' sizes are
 *                exchanged with one all-gather.
 *   load / save / append_to_file   the smt_corpus_save file format (rows in global order -- a file written by N GPUs
 *                loads on one, and back); every rank streams its own pieces.  load cuts the file into ceil(N / n_ranks)
 *                ranges; load_layout restores a recorded piece list (piece k = piece_rows[k] consecutive global rows on
 *                rank piece_rank[k]), e.g. so that per-shard index files stay valid.  A failing rank reports through the
 *                collective: every process returns the error.
 *   layout       the piece list in global order; returns the piece count (call with cap 0 to size the arrays).
 *   append_host  n_rows new global rows, dealt to the ranks as described above; every process passes the same rows.
 *   read_rows / write_rows   rows by global position <-> host (single-process groups: the one caller sees the matrix).
 *   shard        the smt_corpus behind local device i and its row count; row_base (may be NULL) is only defined -- and
 *                only accepted -- while the corpus is one range per rank.  Do not append to a shard directly. */
int smt_sharded_corpus_create(smt_group *group, uint32_t D, smt_sharded_corpus **out);
int smt_sharded_corpus_from_host(smt_group *group, const float *rows, uint64_t total_rows, uint32_t D, smt_sharded_corpus **out);
int smt_sharded_corpus_from_device(smt_group *group, const float *const *shard_rows_dev, const uint64_t *shard_rows,
                                   uint32_t D, smt_sharded_corpus **out);
int smt_sharded_corpus_load(smt_group *group, const char *path, smt_sharded_corpus **out);
int smt_sharded_corpus_load_layout(smt_group *group, const char *path, const uint64_t *piece_rows, const uint32_t *piece_rank,
                                   uint64_t n_pieces, smt_sharded_corpus **out);
uint64_t smt_sharded_corpus_layout(const smt_sharded_corpus *corpus, uint64_t *piece_rows, uint32_t *piece_rank, uint64_t cap);
int smt_sharded_corpus_save(smt_sharded_corpus *corpus, const char *path);
int smt_sharded_corpus_append_to_file(smt_sharded_corpus *corpus, const char *path, uint64_t rows_on_disk);
/* The same in two steps, so that persisting overlaps embedding (src/workspace/store.rs:402-434 flushes every 1000-point chunk while
 * it goes; a 1 M-line workspace is 1 GB of rows whose fsync takes as long as tokenising + pooling them):
 *   SMT_APPEND_WRITE_AHEAD  rows [rows_written, rows) go to their places in the file and the kernel is asked to start writing them
 *                           out (sync_file_range), but nothing is durable and the header still names rows_on_disk rows -- a crash
 *                           leaves the old, consistent prefix.  Call it after every embedded batch; one-shard corpora only
 *                           (SMT_E_UNSUPPORTED otherwise: keep the rows for the commit).
 *   SMT_APPEND_CREATE       rows_on_disk == 0 and no file yet: start one (empty header).
 *   flags 0                 the commit: rows [rows_written, rows) written, fsync, header last.  rows_on_disk <= rows_written: what
 *                           earlier WRITE_AHEAD calls put there.  smt_sharded_corpus_append_to_file(c, p, r) == _ex(c, p, r, r, 0). */
#define SMT_APPEND_WRITE_AHEAD 1
#define SMT_APPEND_CREATE 2
int smt_sharded_corpus_append_to_file_ex(smt_sharded_corpus *corpus, const char *path, uint64_t rows_on_disk, uint64_t rows_written,
                                         int flags);
void smt_sharded_corpus_destroy(smt_sharded_corpus *corpus);
uint64_t smt_sharded_corpus_rows(const smt_sharded_corpus *corpus);
int smt_sharded_corpus_rank_rows(const smt_sharded_corpus *corpus, uint64_t *rows_per_rank /* [n_ranks] */);
int smt_sharded_corpus_shard(smt_sharded_corpus *corpus, int local_index, smt_corpus **shard, uint64_t *row_base, uint64_t *rows);
int smt_sharded_corpus_append_host(smt_sharded_corpus *corpus, const float *rows, uint64_t n_rows, uint64_t *first_row);
int smt_sharded_corpus_read_rows(smt_sharded_corpus *corpus, uint64_t first_row, uint64_t n_rows, float *out_host);
int smt_sharded_corpus_write_rows(smt_sharded_corpus *corpus, uint64_t first_row, const float *rows, uint64_t n_rows);
/* smt_corpus_compact over the sharded corpus: `keep_global` names GLOBAL rows.  Every shard keeps its part of the list and closes
 * its own gaps in place (no row changes rank); the piece list shrinks with it -- empty pieces go, neighbours of one rank that
 * became contiguous merge -- so global order, and with it the tie order of every search, is unchanged.  *rows_moved (may be NULL)
 * = the rows moved on all shards.  One-process groups only (physical or logical): SMT_E_UNSUPPORTED for a one-rank-per-process
 * group, and for a corpus made of adopted device buffers.  A refused call leaves the corpus untouched. */
int smt_sharded_corpus_compact(smt_sharded_corpus *corpus, const smt_range *keep_global, uint32_t n_keep, uint64_t *rows_moved);

/* The embedding table replicated on every device of the group, and K1 sharded by line ("K1 shards by
 * line with a replicated table", no collective): the device half of StaticModel::from_pretrained / encode_with_args
 * (call sites src/search/mod.rs:69,138,153; src/cmds/search.rs:123-128,136,154) for a caller that owns N GPUs.
 * smt_sharded_embed = smt_embed's arguments and results: the lines are dealt to the ranks in contiguous blocks, block r is
 * pooled on rank r from its copy of the table (one host thread per device) and, with `append_to`, appended to rank r's
 * shard; the blocks in rank order become the new global rows, so global row == line order and *first_row = the first of
 * them.  Every row is bit-identical to smt_embed's (same kernel, same table).  out_host receives [n_lines x D] (in a
 * multi-process group: the blocks of the local ranks only).  If any rank fails, no shard keeps rows of the call. */
typedef struct smt_sharded_model smt_sharded_model;
int smt_sharded_model_create(smt_group *group, const float *table_host, uint64_t V, uint32_t D, int normalize, smt_sharded_model **out);
int smt_sharded_model_create_from_file(smt_group *group, const char *path, uint64_t byte_offset, uint64_t V, uint32_t D,
                                       int normalize, smt_sharded_model **out);
/* the same over a table of SMT_TABLE_F32 / F16 / I8 as stored (smt_model_create_typed): one typed replica per local device */
int smt_sharded_model_create_typed(smt_group *group, const void *table_host, int table_dtype, uint64_t V, uint32_t D, int normalize,
                                   smt_sharded_model **out);
int smt_sharded_model_create_from_file_typed(smt_group *group, const char *path, uint64_t byte_offset, int table_dtype, uint64_t V,
                                             uint32_t D, int normalize, smt_sharded_model **out);
/* the indexed form (smt_model_create_indexed): one replica of table and token array per local device */
int smt_sharded_model_create_indexed(smt_group *group, const void *table_host, int table_dtype, uint64_t n_rows, uint32_t D,
                                     const uint32_t *mapping_host, const float *weights_host, uint64_t n_tokens, int normalize,
                                     smt_sharded_model **out);
int smt_sharded_model_create_from_file_indexed(smt_group *group, const char *path, uint64_t byte_offset, int table_dtype, uint64_t n_rows,
                                               uint32_t D, const uint32_t *mapping_host, const float *weights_host, uint64_t n_tokens,
                                               int normalize, smt_sharded_model **out);
int smt_sharded_model_token_info(const smt_sharded_model *model, uint64_t *n_tokens, int *has_mapping, int *has_weights,
                                 uint64_t *token_bytes);
/* smt_model_info of the replicas (they are alike): table_bytes is what ONE replica holds in device memory */
int smt_sharded_model_info(const smt_sharded_model *model, int *table_dtype, uint64_t *V, uint64_t *table_bytes);
void smt_sharded_model_destroy(smt_sharded_model *model);
int smt_sharded_embed(smt_sharded_model *model, const uint32_t *ids, const uint64_t *offsets, uint64_t n_lines, uint32_t max_tokens,
                      float *out_host, smt_sharded_corpus *append_to, uint64_t *first_row);

/* smt_search over the sharded corpus: same arguments and semantics (ranges and returned rows are GLOBAL), same
 * result as smt_search on the unsharded matrix.  top_k <= 56 without "all under threshold": per-device scan +
 * select -> ONE ncclAllGather of the packed [nq][2][k] lists -> merge_topk_kernel.  Threshold mode and larger k:
 * all-gather of the hit counts, one all-gather of a max-count-padded buffer, host merge. */
int smt_sharded_search(smt_sharded_corpus *corpus, const float *queries, uint32_t nq, uint32_t top_k, double max_distance,
                       int mode, const smt_range *ranges, uint32_t n_ranges, uint64_t *out_rows, double *out_dist,
                       uint64_t *out_counts, uint64_t out_cap);
/* Device-resident top-k (mode DOCUMENTS, no threshold, no ranges), nothing synchronises: queries_dev[i] is a
 * pointer ON LOCAL DEVICE i to the nq queries; out_packed[i] (NULL = this device does not need the answer) is
 * device-addressable memory of local device i -- HBM or pinned host -- receiving [nq][2][top_k] 8-byte words:
 * global rows (padding UINT64_MAX), then the f64 distance bit patterns (padding +inf).  With tuning key
 * async_select set on the contexts and nq == 1, the select, the all-gather and the merge of call i run on the
 * contexts' aux streams while the scan of call i+1 streams.  1 <= top_k <= 1024 with n_ranks * top_k <= 8192 (57 .. 1024: the
 * sampled-threshold route on every shard, tuning key largek_sampled; with largek_sampled = 0, top_k <= 56). */
int smt_sharded_search_topk_device(smt_sharded_corpus *corpus, const float *const *queries_dev, uint32_t nq, uint32_t top_k,
                                   uint64_t *const *out_packed);
/* ... with the per-query verdict of smt_search_topk_device_ex: out_status (NULL = none) holds one pointer per LOCAL device,
 * out_status[i] (NULL = not wanted there; needs out_packed[i]) receiving [nq] SMT_STATUS_* codes -- the WORST status any shard
 * of the group reported for that query (every rank's status words travel with its k-lists: same all-gather, or read in place by
 * the peer transport). */
int smt_sharded_search_topk_device_ex(smt_sharded_corpus *corpus, const float *const *queries_dev, uint32_t nq, uint32_t top_k,
                                      uint64_t *const *out_packed, uint32_t *const *out_status);

/* IVF index over a sharded corpus: every rank indexes ITS rows.  shared_centroids != 0 makes the build data-parallel
 * (SURVEY.md 8(e)): the coarse k-means runs on every rank's sample of its own rows and the fixed-point centroid
 * sums + counts are summed over the ranks after every accumulation (ncclAllReduce on the ranks' streams), so all
 * ranks end with the SAME nlist centroids -- "nlist lists over the whole corpus", each list spread over the shards --
 * while quantisers and codes are fitted locally.  shared_centroids == 0: independent per-shard indexes (own centroids,
 * no collective in the build).  Search: per-shard smt_ivfpq_search with global rows -> the same all-gather + merge as
 * smt_sharded_search.  Exact distances, approximate membership; top_k <= 56 (smt_sharded_ivfpq_search_wide: up to 1024). */
typedef struct smt_sharded_ivfpq smt_sharded_ivfpq;
int smt_sharded_ivfpq_build(smt_sharded_corpus *corpus, const smt_ivfpq_params *params, int shared_centroids,
                            smt_sharded_ivfpq **out);
void smt_sharded_ivfpq_destroy(smt_sharded_ivfpq *index);
smt_ivfpq *smt_sharded_ivfpq_shard(smt_sharded_ivfpq *index, int local_index); /* smt_ivfpq_info etc.; NULL if out of range */
int smt_sharded_ivfpq_search(smt_sharded_ivfpq *index, const float *queries, uint32_t nq, uint32_t top_k, uint32_t nprobe,
                             uint32_t rerank, uint64_t *out_rows, double *out_dist, uint64_t *out_counts, uint64_t out_cap);
/* Inside GLOBAL row ranges (rules as in smt_sharded_search; n_ranges == 0 is smt_sharded_ivfpq_search): every rank searches its
 * index inside its part of the ranges (smt_ivfpq_search_ranges), a rank they leave nothing contributes nothing. */
int smt_sharded_ivfpq_search_ranges(smt_sharded_ivfpq *index, const float *queries, uint32_t nq, uint32_t top_k, uint32_t nprobe,
                                    uint32_t rerank, const smt_range *ranges, uint32_t n_ranges, uint64_t *out_rows,
                                    double *out_dist, uint64_t *out_counts, uint64_t out_cap);
/* The wide form over a sharded corpus: 1 <= top_k <= 1024 and n_ranks x top_k <= 8192, GLOBAL ranges or NULL, with the meaning of
 * NULL / n_ranges == 0 of smt_ivfpq_search_wide.  Every rank answers as smt_ivfpq_search_wide defines it for its own rows (for
 * top_k <= 56: the narrow route), and the ranks' lists of top_k are merged by (exact distance, global row) through the exchange of
 * smt_sharded_search_topk_device_ex, on either transport.  Every argument is checked before anything is enqueued. */
int smt_sharded_ivfpq_search_wide(smt_sharded_ivfpq *index, const float *queries, uint32_t nq, uint32_t top_k, uint32_t nprobe,
                                  uint32_t rerank, const smt_range *ranges, uint32_t n_ranges, uint64_t *out_rows,
                                  double *out_dist, uint64_t *out_counts, uint64_t out_cap);
/* Life cycle, shard by shard (smt_ivfpq_save / _load / _append / _info on every local rank).  A one-rank group uses `path`
 * itself; otherwise rank r's part is `<path>.r<r>of<n_ranks>` -- the files name LOCAL rows by position, so they are valid
 * for the layout they were built on (persist it with smt_sharded_corpus_layout, restore it with _load_layout).
 * info: rows covered and index bytes summed over the local ranks, the largest nlist. */
int smt_sharded_ivfpq_save(smt_sharded_ivfpq *index, const char *path);
int smt_sharded_ivfpq_load(smt_sharded_corpus *corpus, const char *path, smt_sharded_ivfpq **out);
int smt_sharded_ivfpq_append(smt_sharded_ivfpq *index, uint64_t *n_added);
int smt_sharded_ivfpq_info(const smt_sharded_ivfpq *index, uint64_t *rows_covered, uint32_t *nlist, uint64_t *index_bytes);
/* smt_sharded_corpus_compact over index->corpus (GLOBAL rows, the same rules and refusals) with every shard's index following its
 * shard's rows as in smt_ivfpq_compact: each rank's part of the list is cut out against the piece layout as it is before the call,
 * then the piece list shrinks.  Every shard is checked before one row moves: SMT_E_UNSUPPORTED if the list leaves some shard's index
 * without a covered row.  *rows_moved / *entries_dropped (may be NULL): summed over the shards.  If a shard's rows moved and its
 * index could not follow, the compaction is completed on every shard, every shard's index is marked stale and the error is returned. */
int smt_sharded_ivfpq_compact(smt_sharded_ivfpq *index, const smt_range *keep_global, uint32_t n_keep, uint64_t *rows_moved,
                              uint64_t *entries_dropped);

/* Exactness bookkeeping.  The f32 scan nominates top_k + 8 rows per list and the select stage PROVES per query
 * that no other row can belong to the exact answer (the k-th exact distance lies more than the f32 error bound
 * below the worst nominated f32 distance).  When the proof fails -- more than 8 near-ties around the k-th place --
 * smt_search / smt_sharded_search re-answer that query exhaustively; the *_device entry points cannot (nothing
 * synchronises): they count such queries here and, in their _ex form, say WHICH query of the call it was
 * (SMT_STATUS_*).  A batched query whose candidate buffer overflowed is reported the same way (the device entry points
 * deliver its list as it is; the host entry points re-answer it).  reset != 0 clears the counter.
 * (smt_ivfpq_search_device has no _ex form: an IVF answer carries no certificate -- exact distances, approximate
 * membership by contract -- so there is no per-query verdict to report.) */
int smt_ctx_uncertain_count(smt_ctx *ctx, uint64_t *count, int reset);

/* Test hook for the kept range sets: a range list (the path subset of a workspace search) that a corpus sees for the second time
 * is kept on the device with its tile / chunk tables -- up to 4 lists per corpus, least recently used first out -- so that a session
 * searching the same file set again uploads only its queries.  kept: sets alive; hits: searches answered from one; builds: sets made. */
int smt_debug_range_sets(const smt_corpus *corpus, uint64_t *kept, uint64_t *hits, uint64_t *builds);

/* Test hook for the fp16 operand image: brings the image up to date, as a batched search would, and copies the 16 KiB of 32-row
 * tile `tile` (and the tile's zero-row mask, bit r = tile row r packed as a zero row) to the host.  Rows at or past the row count are
 * packed as zero rows, whatever lies there: tests/test_gpu_image_tile.py compares the tile that straddles the row count between
 * corpora whose memory behind the rows differs, and every tile's content with a float64 reference.  SMT_E_INVALID when the corpus
 * has no image or the tile holds no row. */
int smt_debug_image_tile(smt_corpus *corpus, uint64_t tile, void *out_tile_host, uint32_t *out_zero_mask);

/* Test hook for delivered answers (tuning key direct_delivery): how many host-form searches on this context got their answer written
 * into pinned host memory by the select kernel and waited on its completion word, instead of a D2H copy + hipStreamSynchronize. */
int smt_debug_deliveries(smt_ctx *ctx, uint64_t *count);

/* Test hook for paired scans (tuning key scan_pair): after a synchronise, how many one-query scans of this context's scan_overlap
 * pipeline took the query of the call two steps later along (paired), ran with their own query only (alone), or found their rows
 * already scanned by the call two steps earlier and ended at once (absorbed; equal to paired once the pipeline is empty).
 * Counted on the device since the context was created.  With scan_pair > 1 a scan may take up to three later calls along: `paired`
 * counts the scans that took at least one, `absorbed` every scan that ended at once (paired <= absorbed <= 3 x paired). */
int smt_debug_scan_pairs(smt_ctx *ctx, uint64_t *paired, uint64_t *alone, uint64_t *absorbed);

/* The same launches by the number of calls their corpus pass served: by_size[n - 1] = scans that served n calls, their own and
 * n - 1 taken along (n = 1..4).  by_size[0] is `alone` above, by_size[1] + by_size[2] + by_size[3] is `paired`, and the sum of
 * n x by_size[n - 1] is the number of calls once the pipeline is empty.  Synchronises. */
int smt_debug_scan_groups(smt_ctx *ctx, uint64_t *by_size /* [4] */);

/* The same with the passes of more than four calls (tuning key scan_take): by_size[n - 1] = scans that served n calls, n = 1..8.  The
 * first four entries are those of smt_debug_scan_groups; the sum of n x by_size[n - 1] is the number of calls once the pipeline is
 * empty, whichever kernel served them.  With scan_take > 3, absorbed <= 7 x paired.  Synchronises. */
int smt_debug_scan_groups_wide(smt_ctx *ctx, uint64_t *by_size /* [8] */);

/* The launches of the sixteen-call kernel alone (tuning key scan_deep above 7): by_size[n - 1] = scans of scan_deep_kernel that
 * served n calls, n = 1..16.  The eight entries above do not count these launches beyond by_size[0], which counts every scan that
 * ran alone; smt_debug_scan_pairs counts them like any other.  All zero while scan_deep_kernel does not run.  Synchronises. */
int smt_debug_scan_groups_deep(smt_ctx *ctx, uint64_t *by_size /* [16] */);

/* One select launch per pass (tuning key select_group, default 1): a launch of the sixteen-call kernel is followed by ONE select
 * launch that serves every call of its pass, in place of one select launch per call.  by_size[n] = those select launches that served
 * n calls, n = 0..16; 0 means the call was absorbed and its answer came from its leader's launch.  The sum of n x by_size[n] is the
 * number of calls served that way; all zero with select_group = 0 or while the sixteen-call kernel does not run.  Synchronises. */
int smt_debug_select_groups(smt_ctx *ctx, uint64_t *by_size /* [17] */);

/* Pipeline calls (scan_overlap) that recorded an event on the caller's stream and made their internal stream wait for it.  With the
 * tuning key ov_skip_ready (default 1) a call made while the caller's stream is empty records none.  Does not synchronise. */
int smt_debug_ov_ready(smt_ctx *ctx, uint64_t *records);

/* Host time of the pipeline calls since the tuning key host_timing was set to 1 (setting it clears the sums): ns[0] stream queries,
 * ns[1] the ready event's record and wait, ns[2] the scan launch, ns[3] the select launch, ns[4] the aux-stream event, ns[5] the whole
 * call below the entry point, ns[6..7] unused; *calls = pipeline calls timed.  Does not synchronise. */
int smt_debug_host_timing(smt_ctx *ctx, uint64_t *ns /* [8] */, uint64_t *calls);

/* Test hook for the SPMD error paths of multi-process groups: arms ONE injected failure with status `code` (an SMT_E_* value) on
 * THIS process's ranks; it fires at the next step of kind `where` and disarms.  The tests arm it on one rank of an n-rank group and
 * check that every rank returns `code` from the same call and that none is left waiting inside a collective.
 *   SMT_DEBUG_FAIL_STAGE  the local scan + select stage of the next smt_sharded_search that exchanges packed k-lists
 *   SMT_DEBUG_FAIL_AGREE  the next status agreement (threshold / large-k searches, sharded save / append / embed / index life cycle)
 *   SMT_DEBUG_FAIL_BUILD  the set-up of the next shared-centroid smt_sharded_ivfpq_build (before its first all-reduce)
 * where == 0 disarms. */
#define SMT_DEBUG_FAIL_STAGE 1
#define SMT_DEBUG_FAIL_AGREE 2
#define SMT_DEBUG_FAIL_BUILD 3
int smt_debug_group_fail_next(smt_group *group, int where, int code);

/* Test hook for the certificate's error bound: the f32 distances the batched kernels NOMINATE candidates with
 * (f32 MFMA, or bf16 x 3 split products when tuning key gemm_bf16x3 is set -- the default), for nq <= 32 host
 * queries against rows [first_row, first_row + n_rows) of the corpus; out is a host buffer [n_rows][32].
 * These values never reach an answer: results carry exact (f64) distances. */
int smt_debug_batched_scores(smt_corpus *corpus, const float *queries, uint32_t nq, uint64_t first_row, uint32_t n_rows,
                             float *out);

/* Test hook for what the batched PRODUCTION kernels nominate (smt_debug_batched_scores above runs a 64-thread restatement of one
 * of them).  Builds the launch arguments of a real batched top_k call of nq <= 64 host queries over the corpus -- optional row ranges
 * as smt_search takes them, the operand image when the corpus has one -- and runs the kernel family the current tuning picks for that
 * call (row-register, LDS-row or level kernel; bf16 x 3, f16 x 2, f16 x 1 or f32 MFMA) with the production query preparation, as ONE
 * level over all tiles: for a filtered call the entries of its tile resp. chunk table.  tau [nq]: the distance threshold of each query
 * (+inf admits every row); buffered != 0: row-register nominations go through the wave's LDS buffer.  At most 2048 rows may be scanned
 * (the capacity of a candidate list): SMT_E_INVALID beyond that and beyond 64 queries.
 *   out_dist   [rows of the corpus][nq] f32, preset to NaN: the distance bits of a nominated key, at the slot of the key's row
 *   out_hits   [rows of the corpus][nq] how many keys named that (row, query) pair: a pair written twice shows here
 *   out_counts [ceil(nq / 32) * 32] the raw nomination count per query, the padding queries of the last query tile included
 *   out_route  family (0 row-register, 1 LDS-row, 2 level) | arithmetic << 4 (0 bf16 x 3, 1 f16 x 2, 2 f16 x 1, 3 f32 MFMA)
 *              | 0x100 operands from the image | 0x200 range-filtered
 * A key that names a row outside the corpus, or a counted slot that was never written, is SMT_E_INVALID. */
int smt_debug_nominations(smt_corpus *corpus, const float *queries, uint32_t nq, uint32_t top_k, const smt_range *ranges, uint32_t n_ranges,
                          const float *tau, int buffered, float *out_dist, uint32_t *out_hits, uint32_t *out_counts, uint32_t *out_route);

/* Test hooks for the K3 LEVEL STAGE: everything between "one level nominates" (smt_debug_nominations) and "the select ranks"
 * (smt_debug_select_lists).  tests/test_level_plan_cpu.py and tests/test_gpu_level_stage.py hold them against tests/level_ref.py.
 *
 * smt_debug_gemm_plan   the LEVEL PLAN of a batched call: the ordered launches launch_gemm_topk makes (it walks the very list this
 *     returns).  A pure host function: no context, no GPU.  plan_tiles: tiles of the call (32-row tiles, entries of the tile table, or
 *     groups of 8 chunk-table entries; 1 .. 2^27 - 1); kp: k' (1..64); family: 0 row-register, 1 LDS-row, 2 level kernel; blocks: tuning
 *     key gemm_blocks or the CU count; then the tuning keys of those names.  out [out_cap][SMT_GEMM_PLAN_WORDS] receives per launch
 *       [0] kind: 0 bootstrap (tile minima, bootstrap_tau_kernel behind it), 1 appended (level_select_kernel behind it)
 *       [1] stride  [2] skip (0, 4, 16, 64)  [3] tile_begin  [4] tile_end: level tile indices [tile_begin, tile_end); level tile i is
 *           tile stride x i (skip 0) resp. stride x the (i + 1)-th positive integer that is no multiple of skip
 *       [5] qsplit  [6] blocks of the launch  [7] bootstrap slots  [8] 1: a select pass follows
 *       [9] bit 0: runs under thresholds an earlier select published; bit 1: its nominations fit the waves' LDS buffers
 *     *out_n: the launches of the plan, also when they exceed out_cap (SMT_E_INVALID then).
 * smt_debug_level_nominations   smt_debug_nominations for an arbitrary level: the launch visits level tiles [tile_begin, tile_end) of
 *     (stride, skip) instead of every tile.  At most 2048 rows may be visited; the last tile must exist; tile_begin != 0 only with the
 *     row-register kernel (the others always start at 0); anything else is SMT_E_INVALID.
 * smt_debug_bootstrap_minima    the BOOTSTRAP launch of the batched call over the corpus (1..64 host queries, optional ranges), exactly
 *     as launch_gemm_topk makes it: the head launch with the +inf fill, then gemm_rowreg_kernel with tile_min, grid and query split as
 *     planned.  out_tile_min [*out_slots][ceil(nq / 32) * 32] (host, room for 1024 slots): slot s = the minimum over the level tiles
 *     with index = s mod 1024 of the tile's best nominating distance.  No candidates are written, so any number of rows may be scanned.
 *     SMT_E_INVALID when the call's plan has no bootstrap level.  out_stride: the bootstrap stride; out_route as smt_debug_nominations.
 * smt_debug_bootstrap_tau       bootstrap_tau_kernel on device buffers: tile_min_dev [n_slots <= 1024][nq_pad], nq <= nq_pad (a multiple
 *     of 32), kp 1..64; tau_dev [nq_pad]; qconst_dev [nq_pad][2], word 2q + 1 = 1/|q| as the head launch left it, word 2q receives the
 *     score threshold of the new tau.  Asynchronous on the context's stream.
 * smt_debug_level_select        level_select_kernel on device buffers, in place: cand_dev [nq][2048] keys (f32 distance bits << 32 | row),
 *     counts_dev [nq] (any value: above 2048 the query overflowed), overflow_dev [nq] (sticky), tau_dev [nq], qconst_dev [nq][2] or NULL.
 *     PRECONDITION: the first min(count, 2048) keys of a query are DISTINCT -- the kernel ranks with a strict <, two equal keys would
 *     share a rank and leave a hole.  Production keeps it because every tile belongs to exactly one appended launch (the plan, P1 of
 *     tests/test_level_plan_cpu.py).  Asynchronous on the context's stream.
 * smt_debug_gemm_trace          sets (buf_dev != NULL, cap_words 32-bit words) or clears the TRACE BUFFER of the context and returns what
 *     was recorded since it was last set: *out_selects select passes, *out_words words.  While set, every batched top_k call appends,
 *     with device-to-device copies on its stream, per select pass (bootstrap_tau_kernel, the select between the two parts of a level,
 *     the select at a level's end) nq count words as the pass finds them and nq tau words as it leaves them, and at its end nq overflow
 *     words and [nq][k'] keys from the head of the candidate buffers.  Nothing else changes, and nothing at all while no buffer is
 *     set.  SMT_E_INVALID when the buffer was too small.  Synchronise before reading the buffer. */
#define SMT_GEMM_PLAN_WORDS 10
int smt_debug_gemm_plan(uint64_t plan_tiles, uint32_t nq, uint32_t kp, int family, int f16x1, uint32_t blocks, int gemm_bootstrap,
                        int gemm_boot_fine, int gemm_split_last, int gemm_qsplit, uint64_t *out, uint32_t out_cap, uint32_t *out_n);
int smt_debug_level_nominations(smt_corpus *corpus, const float *queries, uint32_t nq, uint32_t top_k, const smt_range *ranges,
                                uint32_t n_ranges, const float *tau, int buffered, uint64_t stride, uint32_t skip, uint64_t tile_begin,
                                uint64_t tile_end, float *out_dist, uint32_t *out_hits, uint32_t *out_counts, uint32_t *out_route);
int smt_debug_bootstrap_minima(smt_corpus *corpus, const float *queries, uint32_t nq, uint32_t top_k, const smt_range *ranges,
                               uint32_t n_ranges, float *out_tile_min, uint32_t *out_slots, uint64_t *out_stride, uint32_t *out_route);
int smt_debug_bootstrap_tau(smt_ctx *ctx, const float *tile_min_dev, uint32_t n_slots, uint32_t nq, uint32_t nq_pad, uint32_t kp,
                            float *tau_dev, float *qconst_dev);
int smt_debug_level_select(smt_ctx *ctx, uint64_t *cand_dev, uint32_t *counts_dev, uint32_t *overflow_dev, float *tau_dev, float *qconst_dev,
                           uint32_t nq, uint32_t kp);
int smt_debug_gemm_trace(smt_ctx *ctx, uint32_t *buf_dev, uint64_t cap_words, uint32_t *out_selects, uint64_t *out_words);

/* Test hooks for the cross-shard merge (csrc/merge.hip): the kernels behind every sharded answer, run on lists a test constructs
 * instead of lists a group's shards produced.  tests/test_gpu_merge.py compares them bit for bit with a NumPy merge
 * (tests/merge_ref.py).  The preconditions of smt_merge_topk hold here too.  Device pointers unless said otherwise; asynchronous on the
 * context's stream; nq == 0 or k_out == 0 returns SMT_OK and enqueues nothing.
 *   smt_debug_merge_sources         the merge of lists that are NOT gathered, as the peer transport runs it: lists_dev is a HOST array of
 *                                   n_lists (1..64) device pointers, each a packed [nq][2][k_in] list in a buffer of its own;
 *                                   out_packed_dev receives [nq][2][k_out]
 *   smt_debug_merge_packed_strided  smt_merge_topk_packed_device as the copy and RCCL transports run it: list l starts
 *                                   l x list_stride_words words behind packed_dev (0 = dense, nq x 2 x k_in), so that a rank's status
 *                                   words may lie between the lists
 *   smt_debug_combine_status        out_status_dev[q] = the largest of the n sources' q-th 64-bit status word.  Exactly one of words_dev
 *                                   (a HOST array of n <= 64 device pointers, nq words each) and base_dev (n blocks of nq words,
 *                                   stride_words >= nq apart) is given; both or neither is SMT_E_INVALID */
int smt_debug_merge_sources(smt_ctx *ctx, const uint64_t *const *lists_dev, uint32_t n_lists, uint32_t nq, uint32_t k_in, uint32_t k_out,
                            uint64_t *out_packed_dev);
int smt_debug_merge_packed_strided(smt_ctx *ctx, const uint64_t *packed_dev, uint64_t list_stride_words, uint32_t n_lists, uint32_t nq,
                                   uint32_t k_in, uint32_t k_out, uint64_t *out_packed_dev);
int smt_debug_combine_status(smt_ctx *ctx, const uint64_t *const *words_dev, const uint64_t *base_dev, uint64_t stride_words, uint32_t n,
                             uint32_t nq, uint32_t *out_status_dev);

/* Test hook for the select stage (csrc/select.hip): the kernel behind every top_k <= 56 answer, run on block lists a test constructs
 * instead of lists a scan produced.  tests/test_gpu_select.py compares it bit for bit with a NumPy select (tests/select_ref.py).
 * Device pointers; asynchronous on the stream of the corpus's context; nq == 0 returns SMT_OK and enqueues nothing.  The corpus gives
 * the context, the f32 rows behind the keys and nothing else: nothing is scanned.
 *   queries_dev        [nq][256] f32
 *   lists_dev          query q's lists start q x list_stride keys behind it (0 = dense, n_lists x kp): n_lists (1..512) lists of kp keys,
 *                      a key = f32 distance bits << 32 | row, each list ascending, distinct rows within a query, UINT64_MAX padding
 *                      at the tail of a list
 *   kp, k_out          1 <= k_out <= kp <= 72; anything else, and a list count outside 1..512, is SMT_E_INVALID
 *   ws_threshold, ws_thr_score   != 0: only rows with 1 - distance > ws_thr_score are kept
 *   f32_err            > 0: the exactness certificate with this bound on |f32 distance - exact distance|; 0: none
 *   overflow_dev       [nq] or NULL; given, a non-zero word makes the query's verdict SMT_STATUS_OVERFLOW
 *   out_stride         words between two queries' output lists (0 = k_out); the words between the lists are not written
 *   out_rows_dev, out_dist_dev   [nq][out_stride]: row_base + row and the exact distance, best first, UINT64_MAX / +inf behind them
 *   out_counts_dev, out_uncertain_dev ([nq] 64-bit), out_status_dev ([nq] 32-bit)   each may be NULL
 * THE CALLER'S CONTRACT: every row a key names lies below the corpus's row count -- the kernel reads that row and checks nothing. */
int smt_debug_select_lists(smt_corpus *corpus, const float *queries_dev, uint32_t nq, const uint64_t *lists_dev, uint64_t list_stride,
                           uint32_t n_lists, uint32_t kp, uint32_t k_out, int ws_threshold, float ws_thr_score, uint64_t row_base,
                           double f32_err, const uint32_t *overflow_dev, uint64_t out_stride, uint64_t *out_rows_dev, double *out_dist_dev,
                           uint64_t *out_counts_dev, uint64_t *out_uncertain_dev, uint32_t *out_status_dev);

/* Test hooks for the scan stage (K2: csrc/scan_launch.hip and the units that hold its kernels): the block lists a scan WRITES, which
 * answers show only through the select's guard band and f64 re-score.  tests/test_gpu_scan_lists.py checks them against a NumPy
 * restatement of the deal and float64 distances (tests/scan_ref.py).
 *   smt_debug_scan_lists   the synchronous path of a top_k call (1 <= top_k <= 56) of nq (1..8) HOST queries over the corpus, optional
 *       row ranges as smt_search takes them, up to the select and no further: the plan, the pipeline step, the chunk table of a filtered
 *       call, the STEAL set-up and one launch per pass -- the very functions a search runs, under the current tuning.  In front of the
 *       first pass (nq + 1) x blocks x k' keys of the list area are preset to the byte 0x5A; behind the last all of them are copied to
 *       out_keys (host), layout [nq + 1][blocks][k'].  A key = f32 distance bits << 32 | row, a list ascending with UINT64_MAX padding.
 *       The extra set is a guard that no pass may touch: a pass of 3 queries rides in 4 slots, and slot 3 must write nothing.
 *       out_blocks, out_kp  the grid and k' = min(64, top_k + guard_band); set before the capacity is checked, so a refused call says
 *                           how many keys it needs
 *       out_route           scan_unroll as planned (filtered: 4) | 0x10 non-temporal row loads | 0x20 range-filtered | 0x40 a pass ran
 *                           the STEAL kernel | block size << 8 | query slots (1, 2, 4) of pass i << (20 + 4 i).  A pass of two or four
 *                           slots planned at 2 rows per chunk runs the kernel built for 8.
 *       SMT_E_INVALID for top_k outside 1..56, nq outside 1..8, nothing to scan, and out_cap_keys < (nq + 1) x blocks x k'.
 *   smt_debug_scan_ring    waits for the one-query pipeline (async_select with scan_overlap), then copies the first n_keys keys
 *       (<= 512 x 64) of the list set of the pipeline call made calls_back (< 32) calls ago to out_keys (host): set
 *       (step - calls_back) & 31 of the ring, at the ring's fixed stride of 512 x 64 keys; a call's lists are [blocks][k'] at its head.
 *       SMT_E_INVALID when the context has made no such call, or when its latest scan was not a call of that pipeline -- any other
 *       scan carves the scratch buffer up its own way, smt_debug_scan_lists included: read the ring first. */
int smt_debug_scan_lists(smt_corpus *corpus, const float *queries, uint32_t nq, uint32_t top_k, const smt_range *ranges, uint32_t n_ranges,
                         uint64_t *out_keys, uint64_t out_cap_keys, uint32_t *out_blocks, uint32_t *out_kp, uint32_t *out_route);
int smt_debug_scan_ring(smt_ctx *ctx, uint32_t calls_back, uint64_t n_keys, uint64_t *out_keys);

/* The context's second stream (hipStream_t), created on first use: async selects run on it, or, with tuning key
 * scan_overlap, it waits for them (every select of an overlapped call enqueued before the work).  A host that
 * chains more work behind an async select (an RCCL all-gather of its output, the merge of the gathered
 * lists with tuning key merge_on_aux) enqueues it here so that the main stream carries nothing but scans.
 * The aux stream is ordered behind async selects ONLY.  Every other device call -- several queries, a filtered call, top_k > 56
 * (the sampled-threshold route) -- runs on the context's stream, and work that depends on its output goes on that stream, or on
 * the aux stream after it has been made to wait for the context's stream (an event, hipStreamWaitEvent). */
int smt_ctx_aux_stream(smt_ctx *ctx, void **stream_out);

/* Tuning knobs; for benchmarking sweeps and throughput pipelines.  Keys:
 *   scan_blocks, scan_threads, scan_unroll (2/4/8), scan_nontemporal   K2 launch shape
 *   scan_steal (0/1/2/4/8/16), scan_steal_pct (1..50)   K2, unfiltered: the last scan_steal_pct per cent of the rows are dealt to the
 *                        blocks WHILE the kernel runs, in groups of scan_steal rounds (0, the default: the static deal).  Evens the
 *                        blocks' finish times out and gains nothing: the launch is bound by the aggregate read rate (A/B only)
 *   gemm_blocks, gemm_qsplit, gemm_ldsrow, gemm_dma_nt                     K3 (f32 kernels / range-filtered batches)
 *   gemm_bootstrap (1)                                                     K3 row-register kernel: first thresholds from a bootstrap level of
 *                                                                          tile minima (0: the appended-levels plan of rounds 1-3; A/B only)
 *   fallback_batch_min_rows   two or more uncertain queries of one call on a shard of at least this many rows (100 000)
 *                        are re-answered by ONE batched threshold pass instead of one exhaustive scan each
 *   guard_band (8..56)   the scans nominate min(64, top_k + guard_band) rows per list; the exactness proof tolerates that
 *                        many near-ties around the k-th place before a query has to be re-answered exhaustively
 *   gemm_min_nq, gemm_min_rows_small   from this many queries (default 3; 8+ always) on shards of this many rows (1 M)
 *                        a call takes the batched path K3 instead of K2 passes of <= 4 queries (2 queries: 4 x the rows)
 *   gemm_rowreg (1/0)    unfiltered batches run gemm_rowreg_kernel (coalesced row loads + LDS transpose)
 *   gemm_nominate (0/1/2/3) how the row-register kernel nominates: 1 bf16 x 3 (band 7e-5), 2 f16 x 2 (a third fewer MFMAs,
 *                        band 5.2e-4, guard band >= 16), 3 f16 x 1 (a third of the MFMAs, band 1.0e-3, guard band >= 24);
 *                        0 = on shards <= 32 M rows f16 x 1 from 129 queries, f16 x 2 at 128, bf16 x 3 below; with the corpus'
 *                        operand image: f16 x 1 from 128 queries, f16 x 2 below, shards up to 2^28 rows
 *   corpus_image (1/0)   corpora the library owns build and keep their fp16 operand image (smt_corpus_prepack)
 *   gemm_image (1/0)     batched searches read the image when the corpus has one
 *   image_scan_min_rows  shards of at least this many rows (1 500 000; 0 = never) answer ONE query from their image as well
 *                        (3..7 queries from two thirds of that), and build it at their fourth small search if they have none
 *   image_use_min_rows   a shard that already HAS its image answers one query from it from this many rows (400 000), two from
 *                        1/5 of it, three and more from 1/60 (unfiltered calls; 0 = only the rule above)
 *   gemm_boot_fine (1/0) corpora of 2 Ki .. 32 Ki tiles take their first thresholds from every 2nd / 4th / 8th tile (0: every 16th)
 *   gemm_buffered (1/0)  A/B switch of the LDS nomination buffer
 *   gemm_split_last (0/1/2)  levels run in two parts with a select pass in between: 0 none, 1 a ratio-16 last level, 2 (default)
 *                        also the first level after the bootstrap
 *   embed_batched (bit mask, default 3)  K1: bit 0 batched id loads, bit 1 the id-prefetch kernel, bit 2 a test hook (64-token
 *                        spans), bit 3 runs of equal line counts instead of equal work (A/B); 0 = the round-2 kernel.  NOTE: 1 no
 *                        longer means "everything on" -- pass 3
 *   gemm_resident        accepted and ignored (its kernel left in round 2)
 *   gemm_bf16x3 (1/0)    K3 nominates with bf16 x 3 split products on the bf16 MFMA pipe (default) or with f32 MFMAs;
 *                        answers are identical either way (exact re-scoring + the exactness certificate)
 *   direct_delivery (1/0)  smt_search top-k calls with a small answer (<= 32 queries, <= 8 KiB of rows and distances) get it DELIVERED
 *                        by the select kernel: its last block writes the answer into pinned host memory and a completion word behind
 *                        it, which the host waits on -- no D2H copy command, no hipStreamSynchronize (~10 us of a small call); 0: A/B
 *   prof_select (0/1), prof_every (N: HIP events on one launch in N)       profiling cost control
 *   scan_debug_ptr, select_debug_ptr                                       device pointers for phase stamps
 *   async_select (0/1)   smt_search_topk_device with ONE query: calls pipeline -- call i's select runs while call i+1
 *                        scans.  By default (scan_overlap = 1, one unfiltered query) call i enqueues its scan AND its select
 *                        on internal stream i & 1, behind an event on the context's stream (inputs written on that stream
 *                        before the call are seen), so scan i + 1 also overlaps the end of scan i; the aux stream
 *                        (smt_ctx_aux_stream) waits for each such select.  With scan_overlap = 0, and on the group path, the
 *                        scans stay on the context's stream and the select runs on the aux stream, the two kernels meeting
 *                        through device-scope flags.  Outputs are complete after smt_ctx_synchronize (or any other call on
 *                        the context, which drains the pipeline first; both wait for every internal stream).  Throughput mode
 *                        for back-to-back single queries; off by default.
 *   scan_overlap (1/0)   see async_select (default 1; 0 = the aux-stream / flag pipeline).  A launch bracketed by profiling
 *                        events (prof_every) waits for its predecessor and the next launch waits for it, so the events
 *                        time the kernel alone, not the gate or a shared HBM.
 *   scan_gate_pct (-1..100)  scan_overlap: a scan's blocks start loading rows once this per cent of the previous call's blocks have
 *                        finished theirs, or after a bound of at most 0.5 ms (0 = at once).  The gate counts calls served: a
 *                        scan that serves n calls in one pass (scan_pair) counts n for each of its blocks, so the point lies at
 *                        (m - 1 + pct / 100) / n of that pass when the previous call is the m-th it serves.  Default -1: 50, and
 *                        no gate with scan_pair >= 2.  Changes timing only, never an answer
 *   scan_pair (0..3)     scan_overlap: the number of later calls a scan may take along.  A scan that queues up behind a predecessor on
 *                        its internal stream looks, on the device when it starts, for the calls two, four and six steps later (the
 *                        next ones on that stream); the longest run of them that is queued in front of the same corpus with the same
 *                        list size and grid, with no work pending on the context's stream when each was made, has its queries
 *                        taken along in the same corpus pass, and those calls' own scans end at once.  The run is a prefix: a call
 *                        that cannot be taken ends it.  Each call's select, outputs and status word stay its own, so no answer
 *                        changes.  A launch bracketed by profiling events and its successor neither take nor are taken, and a
 *                        call made while the GPU keeps up runs the plain kernel.  1 = pairs only.  Switching it drains the
 *                        pipeline.  The key sets the limit that scan_take sets, within the range of the four-call kernel
 *   scan_take (0..7)     the same limit with the range of the eight-call kernel: above 3, a launch whose lists hold at
 *                        most 32 candidates (top_k <= 24 at the default guard_band) in blocks of at most 512 threads runs
 *                        scan_wide_kernel and looks for the calls two, four, ... fourteen steps later; any other launch runs as
 *                        with scan_pair = 3.  Switching it drains the pipeline
 *   scan_deep (0..15)    the same limit with the range of the sixteen-call kernel: above 7, a launch that scan_take would give to
 *                        scan_wide_kernel runs scan_deep_kernel and looks for the calls two, four, ... thirty steps later; up to 7
 *                        the key is scan_take.  The default limit is 15.  Switching it drains the pipeline
 *   select_group (0/1)   1 (default): a launch of scan_deep_kernel is followed by ONE select launch that serves every call of its
 *                        pass -- the calls it took along get their answers from it, earlier in stream order than from a select of
 *                        their own, which is safe because a call is only taken when the context's stream was empty at the call --
 *                        and the select launches of those calls return at once.  Rows, distances, status words and the uncertain
 *                        count are bit for bit those of 0, where every call runs its own select.  Switching it drains the pipeline
 *   ov_skip_ready (0/1)  1 (default): a scan_overlap call made while the context's stream is empty records no event on that stream
 *                        and puts no wait in front of its scan; 0: every call does (smt_debug_ov_ready counts them)
 *   host_timing (0/1)    1: clock_gettime around the runtime calls of a scan_overlap call, read with smt_debug_host_timing; setting
 *                        the key clears the sums (default 0)
 *   scan_pair_ring (64..4096, a power of two)  scan_pair: slots of the descriptor ring in use.  A call can be taken along while the
 *                        host is fewer calls ahead of the GPU than this; a call further ahead simply scans for itself.  Switching
 *                        it drains the pipeline (default 4096; tests use 64 to see slots reused)
 *   scan_pair_wait_us (0..5000)  tests only: every call counts as queued behind a predecessor, and the block that decides waits this
 *                        long for the later call's descriptor, which makes pairing deterministic on corpora that scan in a few
 *                        microseconds (default 0)
 *   merge_on_aux (0/1)   smt_merge_topk_packed_device is enqueued on the aux stream (see smt_ctx_aux_stream)
 *   compact_bounce_rows (64 .. 2^20, default 65536 = 64 MiB)  smt_corpus_compact: a step whose rows move down by fewer rows than this
 *                        goes through a bounce buffer of this many rows in the context's scratch (a launch must not overwrite its own
 *                        sources); a step with a longer gap is one direct launch.  At most 2 x ceil(rows / this) enqueues per call
 *   thr_hit_cap (>= 1, default 2^20)  K4 (every row under max_distance): slots of the hit buffer of the first pass, at most the rows
 *                        scanned.  A pass that counts more hits than slots is run again with a buffer of exactly that many; the
 *                        answer does not depend on the key (tests lower it to reach the second pass on small corpora)
 * The keys and the one-query pipeline.  The keys that say so above drain it.  scan_blocks, scan_threads, scan_unroll and
 * guard_band are stored without a drain, while the list sets of earlier calls are still in flight: they shape the NEXT launch
 * only.  direct_delivery is stored without one too and concerns the host form alone (smt_search, smt_ivfpq_search), which drains
 * the pipeline itself before it scans; a queued device call never reads the key.  A queued leader takes a later call when corpus address, scanned rows, list size and grid all agree, so a call
 * made behind a changed guard_band or scan_blocks starts a group of its own; scan_threads is not part of that test and need not
 * be -- a leader scans with its own block size and writes one list per block whatever the taken call's would have been; with
 * scan_unroll other than 4 a call runs the plain kernel.  tests/test_gpu_pipeline_life.py switches every key named here between
 * queued calls, away from its default and back, and compares every answer with the oracle. */
int smt_set_tuning(smt_ctx *ctx, const char *key, int64_t value);

/* ------------------------------------------------------------------ host ids
 * FNV-1a 64 and the point ids of the workspace store
 * (src/workspace/store.rs:651-661, :82-89, :75-80) -- pure host helpers. */
uint64_t smt_fnv1a_hash(const uint8_t *bytes, uint64_t n);
uint64_t smt_line_embedding_id(const char *path, int32_t line_number);
uint64_t smt_doc_meta_id(const char *path);

#ifdef __cplusplus
}
#endif
#endif /* SEMTOOLS_HIP_H */
