/*
 * semtools_host.h -- C ABI of the HOST layer of libsemtools_hip.so: the reference's
 * search module and workspace store re-implemented over the kernel-level ABI
 * (semtools_hip.h).  These entry points exist so that non-C++ callers (tests, the
 * CLI replica) can drive the same functions the reference exposes:
 *
 *   smt_host_model_*          model2vec_rs::StaticModel (from_pretrained / encode*)
 *   smt_host_search_files     search_files + print_search_results      (src/search/mod.rs:122-143,
 *                                                                        src/cmds/search.rs:35-63,245-257)
 *   smt_host_search_content   the stdin branch of search_cmd            (src/cmds/search.rs:145-176)
 *   smt_host_search_workspace search_with_workspace + workspace printing (src/search/mod.rs:146-216,
 *                                                                        src/cmds/search.rs:66-110,197-244)
 *   smt_host_workspace_*      workspace use / status / prune            (src/cmds/workspace.rs)
 *
 * Text comes back as a malloc'd, NUL-terminated UTF-8 string (*out_text) that the caller
 * releases with smt_host_free; it is byte-for-byte what the reference prints to stdout.
 * Progress lines go to stderr exactly where the reference prints them.
 */
#ifndef SEMTOOLS_HOST_H
#define SEMTOOLS_HOST_H

#include "semtools_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct smt_host_model smt_host_model;

#define SMT_TOK_HASH 0     /* whitespace words hashed (FNV-1a) into [0, V): synthetic tests      */
#define SMT_TOK_VOCAB 1    /* whitespace words looked up in vocab_path (one token per line)      */
#define SMT_TOK_CALLBACK 2 /* caller-provided tokenizer (e.g. the real HF tokenizers binding)    */

/* Writes up to `cap` ids of `text` to `ids`, the total count to *n; returns 0 on success. */
typedef int (*smt_tokenize_cb)(void *user, const char *text, uint64_t len, uint32_t *ids, uint64_t cap,
                               uint64_t *n);

/* StaticModel::from_pretrained: `table` = the f32 `embeddings` tensor [V x 256] (host);
 * unk_id = UINT32_MAX when the tokenizer has no unk token; median_len = median vocabulary
 * token length in characters (used only for callback tokenizers). */
int smt_host_model_create(smt_ctx *ctx, const float *table, uint64_t V, int normalize, int tok_kind,
                          const char *vocab_path, const char *unk_token, smt_tokenize_cb cb, void *user,
                          uint32_t unk_id, uint32_t median_len, smt_host_model **out);
/* directory with model.safetensors ("embeddings", F32 or F16), vocab.txt, optional config.json */
int smt_host_model_from_dir(smt_ctx *ctx, const char *dir, smt_host_model **out);
/* The model's embedding table as the device holds it: its SMT_TABLE_* kind (F16 and I8 tables of a model directory stay as stored),
 * rows, and bytes per replica.  *resident = 0 while a directory-backed model has not uploaded the whole table yet (it serves small
 * calls from compact tables of the rows they touch); the figures then describe the table in the file.  Any out may be NULL. */
int smt_host_model_table_info(const smt_host_model *model, int *table_dtype, uint64_t *V, uint64_t *table_bytes, int *resident);
/* The token side of the model (smt_model_token_info).  A directory whose model.safetensors also carries `mapping` (I32 / I64) and / or
 * `weights` (F64 / F32 / F16) is a vocabulary-quantised model: n_tokens is those tensors' length (the tokenizer's vocabulary is checked
 * against it, not against the table's rows), token_bytes the 8 B per token of the device array per replica.  A plain model reports its
 * rows, 0, 0, 0.  Any out may be NULL. */
int smt_host_model_token_info(const smt_host_model *model, uint64_t *n_tokens, int *has_mapping, int *has_weights, uint64_t *token_bytes);
void smt_host_model_destroy(smt_host_model *model);

/* encode_with_args(texts, Some(max_length) / None when 0, batch 16384) -> out [n x 256] */
int smt_host_encode(smt_host_model *model, const char *const *texts, uint64_t n, uint32_t max_length,
                    float *out);
/* the rows of smt_host_to_lowercase(texts[i]): what an ignore_case search embeds for a line (src/search/mod.rs:63-67).  The texts
 * are lowered inside the call -- on the device where smt_host_model_set_device_lower applies, else on the host; same rows */
int smt_host_encode_lowered(smt_host_model *model, const char *const *texts, uint64_t n, uint32_t max_length,
                            float *out);

/* max_distance: NaN = None.  json != 0: SearchOutput JSON (to_string_pretty) instead of text. */
int smt_host_search_files(smt_host_model *model, const char *query, const char *const *files, uint64_t n_files,
                          uint64_t n_lines, uint64_t top_k, double max_distance, int ignore_case, int json,
                          int is_tty, char **out_text);
int smt_host_search_content(smt_host_model *model, const char *query, const char *filename, const char *content,
                            uint64_t n_lines, uint64_t top_k, double max_distance, int ignore_case, int json,
                            int is_tty, char **out_text);
int smt_host_search_workspace(smt_host_model *model, const char *query, const char *const *files,
                              uint64_t n_files, uint64_t n_lines, uint64_t top_k, double max_distance,
                              int ignore_case, const char *workspace_name, int json, int is_tty,
                              char **out_text);

/* Resident session (no reference counterpart -- the reference reloads the model and
 * re-embeds the files for every query): the files are embedded ONCE, then any number of query batches are
 * answered against the resident corpus.  out_texts[i] (malloc'd, release each with smt_host_free) is
 * byte-for-byte what `semtools search <queries[i]> <files...>` prints. */
typedef struct smt_host_session smt_host_session;
int smt_host_session_open(smt_host_model *model, const char *const *files, uint64_t n_files, int ignore_case,
                          smt_host_session **out);
int smt_host_session_search(smt_host_session *session, const char *const *queries, uint64_t n_queries,
                            uint64_t n_lines, uint64_t top_k, double max_distance, int json, int is_tty,
                            char **out_texts);
uint64_t smt_host_session_lines(const smt_host_session *session);
void smt_host_session_close(smt_host_session *session);

/* workspace use / status / prune: same stdout text / JSON as src/cmds/workspace.rs */
int smt_host_workspace_use(smt_ctx *ctx, const char *name, int json, char **out_text);
int smt_host_workspace_status(smt_ctx *ctx, const char *name_or_null, int json, char **out_text);
int smt_host_workspace_prune(smt_ctx *ctx, const char *name_or_null, int json, char **out_text);
/* No reference counterpart.  The workspace keeps the token ids it pooled for every stored line
 * (line_tokens.log, written by the workspace search; SEMTOOLS_TOKEN_CACHE=0 disables it).  This call re-creates every
 * stored vector from those ids with `model` -- a new embedding table behind the same tokenizer -- on the GPU, without
 * reading or tokenising the source files; document metadata is untouched.  Documents without cached tokens are listed
 * and nothing is changed.  A model with a different tokenizer is refused. */
int smt_host_workspace_reembed(smt_host_model *model, const char *name_or_null, int json, char **out_text);

void smt_host_free(char *text);

/* ---- the host layer on SEVERAL GPUs.  The caller is one process (src/bin/semtools.rs:134-135 runs the search from one
 * task); it hands the layer an smt_group instead of a context and everything above runs sharded: the embedding table is
 * replicated per GPU (smt_sharded_model), lines are pooled by all GPUs at once (smt_sharded_embed), the Documents' /
 * workspace store's matrix is an smt_sharded_corpus whose rows are dealt over the GPUs as they arrive, searches end in
 * ONE all-gather of per-shard top-k lists, the optional index is built with shared centroids.  Output bytes are the same
 * as on one GPU (the global row order is insertion order either way).  The `smt_ctx *` forms above are these with a
 * one-rank group (smt_group_from_ctx).  The group must outlive the model / calls.
 *   smt_host_group_from_spec   "0,1,2,3" = those GPUs (RCCL), "all" = every visible GPU, "<d>:<n>" = n logical shards on
 *                              GPU d (one-GPU test rigs), "<d>" = GPU d alone.  The CLI reads $SEMTOOLS_DEVICES with it.
 * The workspace store records how its rows were dealt over the GPUs (line_rows.json "shards"); the vector file itself
 * holds the rows in global order, so a store written by N GPUs opens on one, and back. */
int smt_host_group_from_spec(const char *spec, smt_group **out);
int smt_host_model_create_group(smt_group *group, const float *table, uint64_t V, int normalize, int tok_kind,
                                const char *vocab_path, const char *unk_token, smt_tokenize_cb cb, void *user,
                                uint32_t unk_id, uint32_t median_len, smt_host_model **out);
int smt_host_model_from_dir_group(smt_group *group, const char *dir, smt_host_model **out);
int smt_host_workspace_use_group(smt_group *group, const char *name, int json, char **out_text);
int smt_host_workspace_status_group(smt_group *group, const char *name_or_null, int json, char **out_text);
int smt_host_workspace_prune_group(smt_group *group, const char *name_or_null, int json, char **out_text);

/* A Hugging Face `tokenizer.json`, read natively (no Python): what model2vec-rs loads through the `tokenizers` crate
 * (call sites src/cmds/search.rs:123-128; encode_batch_fast(.., add_special_tokens = false) inside encode_with_args).
 * Supported components: BertNormalizer / Lowercase / NFD / StripAccents / Strip / Replace(String) / Sequence;
 * BertPreTokenizer / Whitespace / WhitespaceSplit / Punctuation / Metaspace / Sequence; WordPiece, Unigram; added (special) tokens.
 * Anything else fails at load time with a message naming the component.  smt_host_model_from_dir uses it when the model
 * directory holds a tokenizer.json.  encode: ids of `text` (no special tokens added); SMT_E_TRUNCATED with the true
 * count in *n_ids when cap is too small. */
typedef struct smt_host_tokenizer smt_host_tokenizer;
int smt_host_tokenizer_load(const char *tokenizer_json_path, smt_host_tokenizer **out);
void smt_host_tokenizer_free(smt_host_tokenizer *tok);
int smt_host_tokenizer_encode(smt_host_tokenizer *tok, const char *text, uint32_t *ids, uint64_t cap, uint64_t *n_ids);
int smt_host_tokenizer_info(smt_host_tokenizer *tok, uint64_t *vocab_size, int64_t *unk_id, uint64_t *median_token_bytes);
/* The device form of the tokenizer (include/semtools_hip.h, section "tokenizer"): its vocabulary, byte rules and added tokens as an
 * smt_wordpiece on `ctx`, to be freed with smt_wordpiece_destroy.  SMT_E_UNSUPPORTED for a tokenizer whose pure-ASCII lines are not
 * BertNormalizer (or none) -> BertPreTokenizer -> WordPiece: Unigram models, other pre-tokenizers. */
int smt_host_tokenizer_to_device(smt_host_tokenizer *tok, smt_ctx *ctx, smt_wordpiece **out);
/* ... and its UTF-8 form (smt_wordpiece_create_utf8): the same vocabulary, and what every code point U+0080 .. U+10FFFF becomes under the
 * tokenizer's own normalizer and pre-tokenizer, as ranges.  A code point is FLAG when its output mixes classes, keeps a character of
 * non-zero canonical combining class (NFD's reordering would depend on the neighbours), or holds more characters than the code
 * point has bytes.  SMT_E_UNSUPPORTED on the terms of smt_host_tokenizer_to_device, and when an added token matched on the raw text
 * holds a non-ASCII byte. */
int smt_host_tokenizer_to_device_utf8(smt_host_tokenizer *tok, smt_ctx *ctx, smt_wordpiece **out);
/* ... and of a Unigram tokenizer: an smt_unigram on `ctx`, to be freed with smt_unigram_destroy.  SMT_E_UNSUPPORTED unless the model
 * is Unigram behind exactly one Metaspace (split, a replacement character >= U+0080) and its normalizer, if any, is built only of
 * Lowercase / NFD / StripAccents / BertNormalizer (each acts on an ASCII character without context). */
int smt_host_tokenizer_to_device_unigram(smt_host_tokenizer *tok, smt_ctx *ctx, smt_unigram **out);
/* An XLM-R-style file has the form too, in both shapes in circulation: a Precompiled normalizer (the table states what the character
 * map makes of each character on its own), then Strip(right) and / or Replace(Regex " {2,}") by a space or by the replacement, in front of
 * Metaspace(always) with or without a WhitespaceSplit.  What those add is given to the handle as its space rules
 * (smt_unigram_set_space_rules), which this call reads off the file without a device: the Replace and WhitespaceSplit collapse runs,
 * WhitespaceSplit and Strip drop the trailing replacement; 0, 0 for every other tokenizer with the form.  A line with CR LF is
 * flagged behind a Precompiled normalizer.  SMT_E_UNSUPPORTED as above.  Either out may be NULL. */
int smt_host_tokenizer_unigram_space_rules(smt_host_tokenizer *tok, int *collapse_runs, int *drop_trailing);
/* ... and its UTF-8 form (smt_unigram_create_utf8): the same vocabulary, and what every code point U+0080 .. U+10FFFF becomes under the
 * tokenizer's own normalizer, as ranges: SPACE when it becomes exactly ' ' (or is the replacement character, left alone), DROPPED
 * when nothing is left, ORDINARY when no output is ' ' or the replacement.  A code point is FLAG when ' ' or the replacement stands
 * beside other output (a Chinese character under handle_chinese_chars), when the chain holds NFD and an output keeps a character of
 * non-zero canonical combining class, or when the output holds more characters than the code point has bytes.  SMT_E_UNSUPPORTED on
 * the terms of smt_host_tokenizer_to_device_unigram, and when an added token matched on the raw text holds a non-ASCII byte.
 * Behind a Precompiled normalizer, which looks up whole grapheme clusters, FLAG is also every code point that can join a neighbour
 * into one cluster (Extend, ZWJ, SpacingMark, Prepend, conjoining jamo, Regional_Indicator) and every code point of category C* the
 * map leaves alone; under a space rule also the replacement's own code point, and under drop_trailing white space that does not end as ' '. */
int smt_host_tokenizer_to_device_unigram_utf8(smt_host_tokenizer *tok, smt_ctx *ctx, smt_unigram **out);
/* The device tokenizer route of a model.  OFF by default; the environment variable SEMTOOLS_DEVICE_TOKENIZER=1 turns
 * it on when the model is created.  With it on, a batch of lines is packed, uploaded and tokenized on the GPU when the model's
 * tokenizer has a device form (smt_host_tokenizer_to_device), the group has one rank and the full table is resident (or about to be:
 * calls of more than 32768 lines); lines the kernel flags are tokenized by the host tokenizer and spliced in; everything else keeps
 * the host path.  Rows, search output and the workspace's cached ids are bit-identical with the switch on and off.
 * on = 2 (SEMTOOLS_DEVICE_TOKENIZER=2) chooses the UTF-8 form of a WordPiece tokenizer (smt_host_tokenizer_to_device_utf8) or of a
 * Unigram tokenizer (smt_host_tokenizer_to_device_unigram_utf8) where it has one: lines with valid UTF-8 of covered code points stay
 * on the device.  Otherwise 2 chooses what 1 chooses.
 * smt_host_model_set_device_tokenizer_long (SEMTOOLS_DEVICE_TOKENIZER_LONG=1 at creation): a separate switch, off by default.  With it
 * on, the route's Unigram handle tokenizes pieces of more than SMT_UG_MAX_WORD and up to SMT_UG_MAX_LONG raw bytes on the device
 * (smt_unigram_set_long_pieces) instead of flagging their lines: a URL, a hash, text written without spaces.  A handle with space
 * rules -- an XLM-R-style file behind a Precompiled normalizer -- is covered too (smt_unigram_set_long_rules).  Same rows and ids;
 * ignored for WordPiece and while the route is off.
 * smt_host_debug_device_tokenized (test hook): lines of this model tokenized on the device so far.
 * smt_host_model_set_device_lower (SEMTOOLS_DEVICE_LOWER=0 at creation turns it off): ON by default.  It only matters while the
 * device tokenizer route is on and a call lowers (ignore_case): the batch's original lines are then packed and lowered on the GPU
 * between the upload and the tokenizer (smt_lower_device: the bytes of to_lowercase), and the few lines the route flags are lowered
 * by the host.  With it off, each batch is lowered on the host, on up to eight threads, by the thread that packs it while the previous
 * batch runs on the GPU.  Without the route every batch is lowered on the tokenizer's threads.  Rows, search output and the
 * workspace's cached ids are the same in all three cases; queries are always lowered on the host.
 * smt_host_debug_device_lowered (test hook): lines of this model lowered on the device so far. */
int smt_host_model_set_device_tokenizer(smt_host_model *model, int on);
int smt_host_model_set_device_tokenizer_long(smt_host_model *model, int on);
int smt_host_debug_device_tokenized(smt_host_model *model, uint64_t *lines);
int smt_host_model_set_device_lower(smt_host_model *model, int on);
int smt_host_debug_device_lowered(smt_host_model *model, uint64_t *lines);
/* Wall-clock phases of this process so far as one JSON object (malloc'd): model_load, read_tokenize_embed_files,
 * embed_query, store_open_corpus_load, change_detection, embed_and_persist_changed_files, scan_select, ... -- what the
 * CLI prints to stderr under SEMTOOLS_TIMING=1. */
char *smt_host_timing_json(void);

/* Formatting primitives of the output layer, exported for tests: mode 0 = Rust `{}` of an f64,
 * 1 = Rust `{}` of an f32 (value is narrowed first), 2 = serde_json f64.  Returns malloc'd text. */
char *smt_host_format_float(double value, int mode);
/* Rust str::lines() / str::to_lowercase() as the host layer implements them: returned as "<count>\x1f<line>\x1f<line>...". */
char *smt_host_split_lines(const char *content);
char *smt_host_to_lowercase(const char *text);

#ifdef __cplusplus
}
#endif
#endif
