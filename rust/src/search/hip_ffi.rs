//! FFI declarations for libsemtools_hip.so -- GENERATED from include/semtools_hip.h by tools/gen_rust_ffi.py,
//! do not edit by hand (tests/test_rust_ffi.py compares this file with the header: names, arity, scalar types).
//!
//! Uncompiled in this repository: the build container has no Rust toolchain.  A semtools maintainer adds this
//! file as `src/search/hip_ffi.rs`, the wrappers next to it (`hip.rs`, `../workspace/hip_store.rs`) and
//! `build.rs`; see INTEGRATION.md.
#![allow(non_camel_case_types, dead_code)]
use std::os::raw::{c_char, c_int, c_void};

macro_rules! opaque { ($($name:ident),*) => { $( #[repr(C)] pub struct $name { _private: [u8; 0] } )* } }
opaque!(SmtCtx, SmtModel, SmtCorpus, SmtIvfpq, SmtGroup, SmtShardedCorpus, SmtShardedIvfpq, SmtShardedModel, SmtWordpiece, SmtUnigram, SmtLower);

/// half-open range of corpus rows [begin, end)
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct SmtRange {
    pub begin: u64,
    pub end: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SmtIvfpqParams {
    pub nlist: u32,
    pub m: u32,
    pub nbits: u32,
    pub train_iters: u32,
    pub train_sample: u64,
    pub reserved: u32,
    pub local_pca: u32,
}

/// a WordPiece vocabulary and its byte rules for the device tokenizer (smt_wordpiece_create copies everything)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct SmtWordpieceParams {
    pub pool: *const c_char,
    pub piece_off: *const u32,
    pub piece_id: *const u32,
    pub n_pieces: u64,
    pub prefix: *const c_char,
    pub prefix_len: u32,
    pub unk_id: i64,
    pub max_input_chars_per_word: u32,
    pub flags: u32,
    pub added_pool: *const c_char,
    pub added_off: *const u32,
    pub n_added: u32,
}

/// what every code point >= U+0080 becomes, for the UTF-8 form of the device tokenizer (smt_wordpiece_create_utf8 copies everything)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct SmtWordpieceCodepoints {
    pub first: *const u32,
    pub last: *const u32,
    pub cls: *const u8,
    pub out_pool: *const c_char,
    pub out_off: *const u32,
    pub n: u64,
}

/// a Unigram vocabulary, Metaspace's settings and the byte table for the device tokenizer (smt_unigram_create copies everything)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct SmtUnigramParams {
    pub pool: *const c_char,
    pub piece_off: *const u32,
    pub piece_id: *const u32,
    pub n_pieces: u64,
    pub scores: *const f64,
    pub unk_score: f64,
    pub unk_id: i64,
    pub replacement: *const c_char,
    pub replacement_len: u32,
    pub prepend: u32,
    pub byte_map: *const u8,
    pub added_pool: *const c_char,
    pub added_off: *const u32,
    pub n_added: u32,
}

/// the lower-casing tables for the device (smt_lower_create copies everything; a null pointer there means Rust's str::to_lowercase)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct SmtLowerTables {
    pub run_first: *const u32,
    pub run_last: *const u32,
    pub run_delta: *const i32,
    pub run_stride: *const u32,
    pub n_runs: u64,
    pub multi_cp: *const u32,
    pub multi_n: *const u32,
    pub multi_to: *const u32,
    pub n_multi: u64,
    pub cased_first: *const u32,
    pub cased_last: *const u32,
    pub n_cased: u64,
    pub ignorable_first: *const u32,
    pub ignorable_last: *const u32,
    pub n_ignorable: u64,
    pub final_sigma: u32,
}

pub const SMT_OK: c_int = 0;
pub const SMT_E_INVALID: c_int = -1;
pub const SMT_E_HIP: c_int = -2;
pub const SMT_E_NOMEM: c_int = -3;
pub const SMT_E_TRUNCATED: c_int = -4;
pub const SMT_E_IO: c_int = -5;
pub const SMT_E_UNSUPPORTED: c_int = -6;
pub const SMT_DIM: u32 = 256;
pub const SMT_MODE_DOCUMENTS: c_int = 0;
pub const SMT_MODE_WORKSPACE: c_int = 1;
pub const SMT_TABLE_F32: c_int = 0;
pub const SMT_TABLE_F16: c_int = 1;
pub const SMT_TABLE_I8: c_int = 2;
pub const SMT_WP_NORMALIZER: c_int = 1;
pub const SMT_WP_CLEAN_TEXT: c_int = 2;
pub const SMT_WP_LOWERCASE: c_int = 4;
pub const SMT_WP_CP_ORDINARY: c_int = 0;
pub const SMT_WP_CP_SPACE: c_int = 1;
pub const SMT_WP_CP_ALONE: c_int = 2;
pub const SMT_WP_CP_DROPPED: c_int = 3;
pub const SMT_WP_CP_FLAG: c_int = 4;
pub const SMT_UG_MAX_WORD: c_int = 64;
pub const SMT_UG_MAX_LONG: c_int = 2048;
pub const SMT_STATUS_PROVED: c_int = 0;
pub const SMT_STATUS_UNCERTAIN: c_int = 1;
pub const SMT_STATUS_OVERFLOW: c_int = 2;
pub const SMT_STATUS_INVALID_QUERY: c_int = 3;
pub const SMT_UNIQUE_ID_BYTES: usize = 128;
pub const SMT_TRANSPORT_RCCL: c_int = 0;
pub const SMT_TRANSPORT_COPY: c_int = 1;
pub const SMT_TRANSPORT_PEER: c_int = 2;
pub const SMT_APPEND_WRITE_AHEAD: c_int = 1;
pub const SMT_APPEND_CREATE: c_int = 2;
pub const SMT_DEBUG_FAIL_STAGE: c_int = 1;
pub const SMT_DEBUG_FAIL_AGREE: c_int = 2;
pub const SMT_DEBUG_FAIL_BUILD: c_int = 3;
pub const SMT_GEMM_PLAN_WORDS: c_int = 10;

extern "C" {
    pub fn smt_ctx_create(device: c_int, out: *mut *mut SmtCtx) -> c_int;
    pub fn smt_ctx_create_on_stream(device: c_int, stream: *mut c_void, out: *mut *mut SmtCtx) -> c_int;
    pub fn smt_ctx_destroy(ctx: *mut SmtCtx);
    pub fn smt_ctx_synchronize(ctx: *mut SmtCtx) -> c_int;
    pub fn smt_last_error() -> *const c_char;
    pub fn smt_version() -> *const c_char;
    pub fn smt_device_count() -> c_int;
    pub fn smt_prof_enable(ctx: *mut SmtCtx, on: c_int) -> c_int;
    pub fn smt_prof_reset(ctx: *mut SmtCtx) -> c_int;
    pub fn smt_prof_read(ctx: *mut SmtCtx, kernel: *const c_char, launches: *mut u64, total_ms: *mut f64) -> c_int;
    pub fn smt_model_create(
        ctx: *mut SmtCtx,
        table_host: *const f32,
        V: u64,
        D: u32,
        normalize: c_int,
        out: *mut *mut SmtModel,
    ) -> c_int;
    pub fn smt_model_create_from_file(
        ctx: *mut SmtCtx,
        path: *const c_char,
        byte_offset: u64,
        V: u64,
        D: u32,
        normalize: c_int,
        out: *mut *mut SmtModel,
    ) -> c_int;
    pub fn smt_model_create_from_device(
        ctx: *mut SmtCtx,
        table_dev: *const f32,
        V: u64,
        D: u32,
        normalize: c_int,
        out: *mut *mut SmtModel,
    ) -> c_int;
    pub fn smt_model_destroy(model: *mut SmtModel);
    pub fn smt_model_create_typed(
        ctx: *mut SmtCtx,
        table_host: *const c_void,
        table_dtype: c_int,
        V: u64,
        D: u32,
        normalize: c_int,
        out: *mut *mut SmtModel,
    ) -> c_int;
    pub fn smt_model_create_from_file_typed(
        ctx: *mut SmtCtx,
        path: *const c_char,
        byte_offset: u64,
        table_dtype: c_int,
        V: u64,
        D: u32,
        normalize: c_int,
        out: *mut *mut SmtModel,
    ) -> c_int;
    pub fn smt_model_create_from_device_typed(
        ctx: *mut SmtCtx,
        table_dev: *const c_void,
        table_dtype: c_int,
        V: u64,
        D: u32,
        normalize: c_int,
        out: *mut *mut SmtModel,
    ) -> c_int;
    pub fn smt_model_info(
        model: *const SmtModel,
        table_dtype: *mut c_int,
        V: *mut u64,
        table_bytes: *mut u64,
    ) -> c_int;
    pub fn smt_model_create_indexed(
        ctx: *mut SmtCtx,
        table_host: *const c_void,
        table_dtype: c_int,
        n_rows: u64,
        D: u32,
        mapping_host: *const u32,
        weights_host: *const f32,
        n_tokens: u64,
        normalize: c_int,
        out: *mut *mut SmtModel,
    ) -> c_int;
    pub fn smt_model_create_from_file_indexed(
        ctx: *mut SmtCtx,
        path: *const c_char,
        byte_offset: u64,
        table_dtype: c_int,
        n_rows: u64,
        D: u32,
        mapping_host: *const u32,
        weights_host: *const f32,
        n_tokens: u64,
        normalize: c_int,
        out: *mut *mut SmtModel,
    ) -> c_int;
    pub fn smt_model_create_from_device_indexed(
        ctx: *mut SmtCtx,
        table_dev: *const c_void,
        table_dtype: c_int,
        n_rows: u64,
        D: u32,
        mapping_dev: *const u32,
        weights_dev: *const f32,
        n_tokens: u64,
        normalize: c_int,
        out: *mut *mut SmtModel,
    ) -> c_int;
    pub fn smt_model_token_info(
        model: *const SmtModel,
        n_tokens: *mut u64,
        has_mapping: *mut c_int,
        has_weights: *mut c_int,
        token_bytes: *mut u64,
    ) -> c_int;
    pub fn smt_embed(
        model: *mut SmtModel,
        ids: *const u32,
        offsets: *const u64,
        n_lines: u64,
        max_tokens: u32,
        out_host: *mut f32,
        append_to: *mut SmtCorpus,
        first_row: *mut u64,
    ) -> c_int;
    pub fn smt_embed_device(
        model: *mut SmtModel,
        ids_dev: *const u32,
        offsets_dev: *const u64,
        n_lines: u64,
        max_tokens: u32,
        out_dev: *mut f32,
    ) -> c_int;
    pub fn smt_wordpiece_create(
        ctx: *mut SmtCtx,
        p: *const SmtWordpieceParams,
        out: *mut *mut SmtWordpiece,
    ) -> c_int;
    pub fn smt_wordpiece_destroy(tok: *mut SmtWordpiece);
    pub fn smt_wordpiece_create_utf8(
        ctx: *mut SmtCtx,
        p: *const SmtWordpieceParams,
        cp: *const SmtWordpieceCodepoints,
        out: *mut *mut SmtWordpiece,
    ) -> c_int;
    pub fn smt_wordpiece_info(
        tok: *const SmtWordpiece,
        table_bytes: *mut u64,
        codepoint_bytes: *mut u64,
        utf8: *mut c_int,
    ) -> c_int;
    pub fn smt_wordpiece_scan_device(
        tok: *mut SmtWordpiece,
        text_dev: *const u8,
        text_bytes: u64,
        line_begin_dev: *const u64,
        line_len_dev: *const u32,
        n_lines: u64,
        keep_bytes: u32,
        max_tokens: u32,
        drop_unk: c_int,
        counts_dev: *mut u32,
        flags_dev: *mut u8,
        n_flagged_dev: *mut u32,
    ) -> c_int;
    pub fn smt_wordpiece_emit_device(
        tok: *mut SmtWordpiece,
        n_lines: u64,
        patch_line_dev: *const u64,
        patch_off_dev: *const u64,
        patch_ids_dev: *const u32,
        n_patch: u64,
        n_patch_ids: u64,
        ids_out_dev: *mut u32,
        ids_cap: u64,
        offsets_out_dev: *mut u64,
    ) -> c_int;
    pub fn smt_wordpiece_tokenize(
        tok: *mut SmtWordpiece,
        text: *const c_char,
        line_begin: *const u64,
        line_len: *const u32,
        n_lines: u64,
        keep_bytes: u32,
        max_tokens: u32,
        drop_unk: c_int,
        ids_out: *mut u32,
        ids_cap: u64,
        offsets_out: *mut u64,
        flags_out: *mut u8,
    ) -> c_int;
    pub fn smt_unigram_create(ctx: *mut SmtCtx, p: *const SmtUnigramParams, out: *mut *mut SmtUnigram) -> c_int;
    pub fn smt_unigram_create_utf8(
        ctx: *mut SmtCtx,
        p: *const SmtUnigramParams,
        cp: *const SmtWordpieceCodepoints,
        out: *mut *mut SmtUnigram,
    ) -> c_int;
    pub fn smt_unigram_info(
        tok: *const SmtUnigram,
        table_bytes: *mut u64,
        codepoint_bytes: *mut u64,
        utf8: *mut c_int,
    ) -> c_int;
    pub fn smt_unigram_destroy(tok: *mut SmtUnigram);
    pub fn smt_unigram_set_long_pieces(tok: *mut SmtUnigram, max_raw_bytes: u32) -> c_int;
    pub fn smt_unigram_set_space_rules(tok: *mut SmtUnigram, collapse_runs: c_int, drop_trailing: c_int) -> c_int;
    pub fn smt_unigram_set_long_rules(tok: *mut SmtUnigram, on: c_int) -> c_int;
    pub fn smt_unigram_long_stats(tok: *mut SmtUnigram, pieces: *mut u64, raw_bytes: *mut u64) -> c_int;
    pub fn smt_unigram_scan_device(
        tok: *mut SmtUnigram,
        text_dev: *const u8,
        text_bytes: u64,
        line_begin_dev: *const u64,
        line_len_dev: *const u32,
        n_lines: u64,
        keep_bytes: u32,
        max_tokens: u32,
        drop_unk: c_int,
        counts_dev: *mut u32,
        flags_dev: *mut u8,
        n_flagged_dev: *mut u32,
    ) -> c_int;
    pub fn smt_unigram_emit_device(
        tok: *mut SmtUnigram,
        n_lines: u64,
        patch_line_dev: *const u64,
        patch_off_dev: *const u64,
        patch_ids_dev: *const u32,
        n_patch: u64,
        n_patch_ids: u64,
        ids_out_dev: *mut u32,
        ids_cap: u64,
        offsets_out_dev: *mut u64,
    ) -> c_int;
    pub fn smt_unigram_tokenize(
        tok: *mut SmtUnigram,
        text: *const c_char,
        line_begin: *const u64,
        line_len: *const u32,
        n_lines: u64,
        keep_bytes: u32,
        max_tokens: u32,
        drop_unk: c_int,
        ids_out: *mut u32,
        ids_cap: u64,
        offsets_out: *mut u64,
        flags_out: *mut u8,
    ) -> c_int;
    pub fn smt_lower_tables_check(t: *const SmtLowerTables) -> c_int;
    pub fn smt_lower_create(ctx: *mut SmtCtx, t: *const SmtLowerTables, out: *mut *mut SmtLower) -> c_int;
    pub fn smt_lower_destroy(h: *mut SmtLower);
    pub fn smt_lower_device(
        h: *mut SmtLower,
        text_dev: *const u8,
        text_bytes: u64,
        line_begin_dev: *const u64,
        line_len_dev: *const u32,
        n_lines: u64,
        out_text_dev: *mut u8,
        out_cap: u64,
        out_begin_dev: *mut u64,
        out_len_dev: *mut u32,
        flags_dev: *mut u8,
        n_flagged_dev: *mut u32,
    ) -> c_int;
    pub fn smt_lower_lines(
        h: *mut SmtLower,
        text: *const c_char,
        line_begin: *const u64,
        line_len: *const u32,
        n_lines: u64,
        out_text: *mut c_char,
        out_cap: u64,
        out_begin: *mut u64,
        out_len: *mut u32,
        flags_out: *mut u8,
    ) -> c_int;
    pub fn smt_corpus_create(ctx: *mut SmtCtx, D: u32, capacity_rows: u64, out: *mut *mut SmtCorpus) -> c_int;
    pub fn smt_corpus_from_device(
        ctx: *mut SmtCtx,
        rows_dev: *const f32,
        n_rows: u64,
        D: u32,
        out: *mut *mut SmtCorpus,
    ) -> c_int;
    pub fn smt_corpus_destroy(corpus: *mut SmtCorpus);
    pub fn smt_corpus_append_host(
        corpus: *mut SmtCorpus,
        rows: *const f32,
        n_rows: u64,
        first_row: *mut u64,
    ) -> c_int;
    pub fn smt_corpus_write_rows(corpus: *mut SmtCorpus, first_row: u64, rows: *const f32, n_rows: u64) -> c_int;
    pub fn smt_corpus_read_rows(corpus: *mut SmtCorpus, first_row: u64, n_rows: u64, out_host: *mut f32) -> c_int;
    pub fn smt_corpus_truncate(corpus: *mut SmtCorpus, n_rows: u64) -> c_int;
    pub fn smt_corpus_compact(
        corpus: *mut SmtCorpus,
        keep: *const SmtRange,
        n_keep: u32,
        rows_moved: *mut u64,
    ) -> c_int;
    pub fn smt_ctx_compact_stats(ctx: *mut SmtCtx, calls: *mut u64, rows_moved: *mut u64, reset: c_int) -> c_int;
    pub fn smt_corpus_prepack(corpus: *mut SmtCorpus, enable: c_int) -> c_int;
    pub fn smt_corpus_image_bytes(corpus: *const SmtCorpus) -> u64;
    pub fn smt_corpus_rows(corpus: *const SmtCorpus) -> u64;
    pub fn smt_corpus_dim(corpus: *const SmtCorpus) -> u32;
    pub fn smt_corpus_save(corpus: *mut SmtCorpus, path: *const c_char) -> c_int;
    pub fn smt_corpus_load(ctx: *mut SmtCtx, path: *const c_char, out: *mut *mut SmtCorpus) -> c_int;
    pub fn smt_corpus_append_to_file(corpus: *mut SmtCorpus, path: *const c_char, rows_on_disk: u64) -> c_int;
    pub fn smt_search(
        corpus: *mut SmtCorpus,
        queries: *const f32,
        nq: u32,
        top_k: u32,
        max_distance: f64,
        mode: c_int,
        ranges: *const SmtRange,
        n_ranges: u32,
        row_base: u64,
        out_rows: *mut u64,
        out_dist: *mut f64,
        out_counts: *mut u64,
        out_cap: u64,
    ) -> c_int;
    pub fn smt_search_topk_device(
        corpus: *mut SmtCorpus,
        queries_dev: *const f32,
        nq: u32,
        top_k: u32,
        row_base: u64,
        out_rows_dev: *mut u64,
        out_dist_dev: *mut f64,
    ) -> c_int;
    pub fn smt_search_topk_device_ex(
        corpus: *mut SmtCorpus,
        queries_dev: *const f32,
        nq: u32,
        top_k: u32,
        row_base: u64,
        out_rows_dev: *mut u64,
        out_dist_dev: *mut f64,
        out_status_dev: *mut u32,
    ) -> c_int;
    pub fn smt_merge_topk(
        rows: *const u64,
        dist: *const f64,
        n_lists: u32,
        nq: u32,
        k_in: u32,
        k_out: u32,
        out_rows: *mut u64,
        out_dist: *mut f64,
        out_counts: *mut u64,
    ) -> c_int;
    pub fn smt_merge_topk_device(
        ctx: *mut SmtCtx,
        rows_dev: *const u64,
        dist_dev: *const f64,
        n_lists: u32,
        nq: u32,
        k_in: u32,
        k_out: u32,
        out_rows_dev: *mut u64,
        out_dist_dev: *mut f64,
    ) -> c_int;
    pub fn smt_merge_topk_packed_device(
        ctx: *mut SmtCtx,
        packed_dev: *const u64,
        n_lists: u32,
        nq: u32,
        k_in: u32,
        k_out: u32,
        out_packed_dev: *mut u64,
    ) -> c_int;
    pub fn smt_ivfpq_build(corpus: *mut SmtCorpus, params: *const SmtIvfpqParams, out: *mut *mut SmtIvfpq) -> c_int;
    pub fn smt_ivfpq_destroy(index: *mut SmtIvfpq);
    pub fn smt_ivfpq_search(
        index: *mut SmtIvfpq,
        queries: *const f32,
        nq: u32,
        top_k: u32,
        nprobe: u32,
        rerank: u32,
        row_base: u64,
        out_rows: *mut u64,
        out_dist: *mut f64,
        out_counts: *mut u64,
        out_cap: u64,
    ) -> c_int;
    pub fn smt_ivfpq_search_device(
        index: *mut SmtIvfpq,
        queries_dev: *const f32,
        nq: u32,
        top_k: u32,
        nprobe: u32,
        rerank: u32,
        row_base: u64,
        out_rows_dev: *mut u64,
        out_dist_dev: *mut f64,
    ) -> c_int;
    pub fn smt_ivfpq_search_ranges(
        index: *mut SmtIvfpq,
        queries: *const f32,
        nq: u32,
        top_k: u32,
        nprobe: u32,
        rerank: u32,
        ranges: *const SmtRange,
        n_ranges: u32,
        row_base: u64,
        out_rows: *mut u64,
        out_dist: *mut f64,
        out_counts: *mut u64,
        out_cap: u64,
    ) -> c_int;
    pub fn smt_ivfpq_search_ranges_device(
        index: *mut SmtIvfpq,
        queries_dev: *const f32,
        nq: u32,
        top_k: u32,
        nprobe: u32,
        rerank: u32,
        ranges: *const SmtRange,
        n_ranges: u32,
        row_base: u64,
        out_rows_dev: *mut u64,
        out_dist_dev: *mut f64,
    ) -> c_int;
    pub fn smt_ivfpq_search_wide(
        index: *mut SmtIvfpq,
        queries: *const f32,
        nq: u32,
        top_k: u32,
        nprobe: u32,
        rerank: u32,
        ranges: *const SmtRange,
        n_ranges: u32,
        row_base: u64,
        out_rows: *mut u64,
        out_dist: *mut f64,
        out_counts: *mut u64,
        out_cap: u64,
    ) -> c_int;
    pub fn smt_ivfpq_search_wide_device(
        index: *mut SmtIvfpq,
        queries_dev: *const f32,
        nq: u32,
        top_k: u32,
        nprobe: u32,
        rerank: u32,
        ranges: *const SmtRange,
        n_ranges: u32,
        row_base: u64,
        out_rows_dev: *mut u64,
        out_dist_dev: *mut f64,
    ) -> c_int;
    pub fn smt_ivfpq_info(
        index: *const SmtIvfpq,
        n_rows: *mut u64,
        nlist: *mut u32,
        index_bytes: *mut u64,
        build_ms4: *mut f64,
    ) -> c_int;
    pub fn smt_ivfpq_list_sizes(index: *const SmtIvfpq, sizes_host: *mut u64) -> c_int;
    pub fn smt_ivfpq_save(index: *mut SmtIvfpq, path: *const c_char) -> c_int;
    pub fn smt_ivfpq_load(corpus: *mut SmtCorpus, path: *const c_char, out: *mut *mut SmtIvfpq) -> c_int;
    pub fn smt_ivfpq_append(index: *mut SmtIvfpq, n_added: *mut u64) -> c_int;
    pub fn smt_ivfpq_compact(
        index: *mut SmtIvfpq,
        keep: *const SmtRange,
        n_keep: u32,
        rows_moved: *mut u64,
        entries_dropped: *mut u64,
    ) -> c_int;
    pub fn smt_init(devices: *const c_int, n_dev: c_int) -> c_int;
    pub fn smt_shutdown() -> c_int;
    pub fn smt_default_group() -> *mut SmtGroup;
    pub fn smt_group_create(devices: *const c_int, n_dev: c_int, out: *mut *mut SmtGroup) -> c_int;
    pub fn smt_group_create_logical(device: c_int, n_shards: c_int, out: *mut *mut SmtGroup) -> c_int;
    pub fn smt_group_from_ctx(ctx: *mut SmtCtx, out: *mut *mut SmtGroup) -> c_int;
    pub fn smt_group_unique_id(id_out: *mut c_void) -> c_int;
    pub fn smt_group_create_rank(
        device: c_int,
        rank: c_int,
        n_ranks: c_int,
        unique_id: *const c_void,
        out: *mut *mut SmtGroup,
    ) -> c_int;
    pub fn smt_group_destroy(group: *mut SmtGroup);
    pub fn smt_group_info(
        group: *const SmtGroup,
        n_ranks: *mut c_int,
        n_local: *mut c_int,
        first_rank: *mut c_int,
        rccl_ranks: *mut c_int,
        rccl_version: *mut c_int,
    ) -> c_int;
    pub fn smt_group_ctx(group: *mut SmtGroup, local_index: c_int) -> *mut SmtCtx;
    pub fn smt_group_synchronize(group: *mut SmtGroup) -> c_int;
    pub fn smt_group_barrier(group: *mut SmtGroup) -> c_int;
    pub fn smt_group_set_transport(group: *mut SmtGroup, transport: c_int) -> c_int;
    pub fn smt_group_transport(group: *const SmtGroup) -> c_int;
    pub fn smt_sharded_corpus_create(group: *mut SmtGroup, D: u32, out: *mut *mut SmtShardedCorpus) -> c_int;
    pub fn smt_sharded_corpus_from_host(
        group: *mut SmtGroup,
        rows: *const f32,
        total_rows: u64,
        D: u32,
        out: *mut *mut SmtShardedCorpus,
    ) -> c_int;
    pub fn smt_sharded_corpus_from_device(
        group: *mut SmtGroup,
        shard_rows_dev: *const *const f32,
        shard_rows: *const u64,
        D: u32,
        out: *mut *mut SmtShardedCorpus,
    ) -> c_int;
    pub fn smt_sharded_corpus_load(
        group: *mut SmtGroup,
        path: *const c_char,
        out: *mut *mut SmtShardedCorpus,
    ) -> c_int;
    pub fn smt_sharded_corpus_load_layout(
        group: *mut SmtGroup,
        path: *const c_char,
        piece_rows: *const u64,
        piece_rank: *const u32,
        n_pieces: u64,
        out: *mut *mut SmtShardedCorpus,
    ) -> c_int;
    pub fn smt_sharded_corpus_layout(
        corpus: *const SmtShardedCorpus,
        piece_rows: *mut u64,
        piece_rank: *mut u32,
        cap: u64,
    ) -> u64;
    pub fn smt_sharded_corpus_save(corpus: *mut SmtShardedCorpus, path: *const c_char) -> c_int;
    pub fn smt_sharded_corpus_append_to_file(
        corpus: *mut SmtShardedCorpus,
        path: *const c_char,
        rows_on_disk: u64,
    ) -> c_int;
    pub fn smt_sharded_corpus_append_to_file_ex(
        corpus: *mut SmtShardedCorpus,
        path: *const c_char,
        rows_on_disk: u64,
        rows_written: u64,
        flags: c_int,
    ) -> c_int;
    pub fn smt_sharded_corpus_destroy(corpus: *mut SmtShardedCorpus);
    pub fn smt_sharded_corpus_rows(corpus: *const SmtShardedCorpus) -> u64;
    pub fn smt_sharded_corpus_rank_rows(corpus: *const SmtShardedCorpus, rows_per_rank: *mut u64) -> c_int;
    pub fn smt_sharded_corpus_shard(
        corpus: *mut SmtShardedCorpus,
        local_index: c_int,
        shard: *mut *mut SmtCorpus,
        row_base: *mut u64,
        rows: *mut u64,
    ) -> c_int;
    pub fn smt_sharded_corpus_append_host(
        corpus: *mut SmtShardedCorpus,
        rows: *const f32,
        n_rows: u64,
        first_row: *mut u64,
    ) -> c_int;
    pub fn smt_sharded_corpus_read_rows(
        corpus: *mut SmtShardedCorpus,
        first_row: u64,
        n_rows: u64,
        out_host: *mut f32,
    ) -> c_int;
    pub fn smt_sharded_corpus_write_rows(
        corpus: *mut SmtShardedCorpus,
        first_row: u64,
        rows: *const f32,
        n_rows: u64,
    ) -> c_int;
    pub fn smt_sharded_corpus_compact(
        corpus: *mut SmtShardedCorpus,
        keep_global: *const SmtRange,
        n_keep: u32,
        rows_moved: *mut u64,
    ) -> c_int;
    pub fn smt_sharded_model_create(
        group: *mut SmtGroup,
        table_host: *const f32,
        V: u64,
        D: u32,
        normalize: c_int,
        out: *mut *mut SmtShardedModel,
    ) -> c_int;
    pub fn smt_sharded_model_create_from_file(
        group: *mut SmtGroup,
        path: *const c_char,
        byte_offset: u64,
        V: u64,
        D: u32,
        normalize: c_int,
        out: *mut *mut SmtShardedModel,
    ) -> c_int;
    pub fn smt_sharded_model_create_typed(
        group: *mut SmtGroup,
        table_host: *const c_void,
        table_dtype: c_int,
        V: u64,
        D: u32,
        normalize: c_int,
        out: *mut *mut SmtShardedModel,
    ) -> c_int;
    pub fn smt_sharded_model_create_from_file_typed(
        group: *mut SmtGroup,
        path: *const c_char,
        byte_offset: u64,
        table_dtype: c_int,
        V: u64,
        D: u32,
        normalize: c_int,
        out: *mut *mut SmtShardedModel,
    ) -> c_int;
    pub fn smt_sharded_model_create_indexed(
        group: *mut SmtGroup,
        table_host: *const c_void,
        table_dtype: c_int,
        n_rows: u64,
        D: u32,
        mapping_host: *const u32,
        weights_host: *const f32,
        n_tokens: u64,
        normalize: c_int,
        out: *mut *mut SmtShardedModel,
    ) -> c_int;
    pub fn smt_sharded_model_create_from_file_indexed(
        group: *mut SmtGroup,
        path: *const c_char,
        byte_offset: u64,
        table_dtype: c_int,
        n_rows: u64,
        D: u32,
        mapping_host: *const u32,
        weights_host: *const f32,
        n_tokens: u64,
        normalize: c_int,
        out: *mut *mut SmtShardedModel,
    ) -> c_int;
    pub fn smt_sharded_model_token_info(
        model: *const SmtShardedModel,
        n_tokens: *mut u64,
        has_mapping: *mut c_int,
        has_weights: *mut c_int,
        token_bytes: *mut u64,
    ) -> c_int;
    pub fn smt_sharded_model_info(
        model: *const SmtShardedModel,
        table_dtype: *mut c_int,
        V: *mut u64,
        table_bytes: *mut u64,
    ) -> c_int;
    pub fn smt_sharded_model_destroy(model: *mut SmtShardedModel);
    pub fn smt_sharded_embed(
        model: *mut SmtShardedModel,
        ids: *const u32,
        offsets: *const u64,
        n_lines: u64,
        max_tokens: u32,
        out_host: *mut f32,
        append_to: *mut SmtShardedCorpus,
        first_row: *mut u64,
    ) -> c_int;
    pub fn smt_sharded_search(
        corpus: *mut SmtShardedCorpus,
        queries: *const f32,
        nq: u32,
        top_k: u32,
        max_distance: f64,
        mode: c_int,
        ranges: *const SmtRange,
        n_ranges: u32,
        out_rows: *mut u64,
        out_dist: *mut f64,
        out_counts: *mut u64,
        out_cap: u64,
    ) -> c_int;
    pub fn smt_sharded_search_topk_device(
        corpus: *mut SmtShardedCorpus,
        queries_dev: *const *const f32,
        nq: u32,
        top_k: u32,
        out_packed: *const *mut u64,
    ) -> c_int;
    pub fn smt_sharded_search_topk_device_ex(
        corpus: *mut SmtShardedCorpus,
        queries_dev: *const *const f32,
        nq: u32,
        top_k: u32,
        out_packed: *const *mut u64,
        out_status: *const *mut u32,
    ) -> c_int;
    pub fn smt_sharded_ivfpq_build(
        corpus: *mut SmtShardedCorpus,
        params: *const SmtIvfpqParams,
        shared_centroids: c_int,
        out: *mut *mut SmtShardedIvfpq,
    ) -> c_int;
    pub fn smt_sharded_ivfpq_destroy(index: *mut SmtShardedIvfpq);
    pub fn smt_sharded_ivfpq_shard(index: *mut SmtShardedIvfpq, local_index: c_int) -> *mut SmtIvfpq;
    pub fn smt_sharded_ivfpq_search(
        index: *mut SmtShardedIvfpq,
        queries: *const f32,
        nq: u32,
        top_k: u32,
        nprobe: u32,
        rerank: u32,
        out_rows: *mut u64,
        out_dist: *mut f64,
        out_counts: *mut u64,
        out_cap: u64,
    ) -> c_int;
    pub fn smt_sharded_ivfpq_search_ranges(
        index: *mut SmtShardedIvfpq,
        queries: *const f32,
        nq: u32,
        top_k: u32,
        nprobe: u32,
        rerank: u32,
        ranges: *const SmtRange,
        n_ranges: u32,
        out_rows: *mut u64,
        out_dist: *mut f64,
        out_counts: *mut u64,
        out_cap: u64,
    ) -> c_int;
    pub fn smt_sharded_ivfpq_search_wide(
        index: *mut SmtShardedIvfpq,
        queries: *const f32,
        nq: u32,
        top_k: u32,
        nprobe: u32,
        rerank: u32,
        ranges: *const SmtRange,
        n_ranges: u32,
        out_rows: *mut u64,
        out_dist: *mut f64,
        out_counts: *mut u64,
        out_cap: u64,
    ) -> c_int;
    pub fn smt_sharded_ivfpq_save(index: *mut SmtShardedIvfpq, path: *const c_char) -> c_int;
    pub fn smt_sharded_ivfpq_load(
        corpus: *mut SmtShardedCorpus,
        path: *const c_char,
        out: *mut *mut SmtShardedIvfpq,
    ) -> c_int;
    pub fn smt_sharded_ivfpq_append(index: *mut SmtShardedIvfpq, n_added: *mut u64) -> c_int;
    pub fn smt_sharded_ivfpq_info(
        index: *const SmtShardedIvfpq,
        rows_covered: *mut u64,
        nlist: *mut u32,
        index_bytes: *mut u64,
    ) -> c_int;
    pub fn smt_sharded_ivfpq_compact(
        index: *mut SmtShardedIvfpq,
        keep_global: *const SmtRange,
        n_keep: u32,
        rows_moved: *mut u64,
        entries_dropped: *mut u64,
    ) -> c_int;
    pub fn smt_ctx_uncertain_count(ctx: *mut SmtCtx, count: *mut u64, reset: c_int) -> c_int;
    pub fn smt_debug_range_sets(corpus: *const SmtCorpus, kept: *mut u64, hits: *mut u64, builds: *mut u64) -> c_int;
    pub fn smt_debug_image_tile(
        corpus: *mut SmtCorpus,
        tile: u64,
        out_tile_host: *mut c_void,
        out_zero_mask: *mut u32,
    ) -> c_int;
    pub fn smt_debug_deliveries(ctx: *mut SmtCtx, count: *mut u64) -> c_int;
    pub fn smt_debug_scan_pairs(ctx: *mut SmtCtx, paired: *mut u64, alone: *mut u64, absorbed: *mut u64) -> c_int;
    pub fn smt_debug_scan_groups(ctx: *mut SmtCtx, by_size: *mut u64) -> c_int;
    pub fn smt_debug_scan_groups_wide(ctx: *mut SmtCtx, by_size: *mut u64) -> c_int;
    pub fn smt_debug_scan_groups_deep(ctx: *mut SmtCtx, by_size: *mut u64) -> c_int;
    pub fn smt_debug_select_groups(ctx: *mut SmtCtx, by_size: *mut u64) -> c_int;
    pub fn smt_debug_ov_ready(ctx: *mut SmtCtx, records: *mut u64) -> c_int;
    pub fn smt_debug_host_timing(ctx: *mut SmtCtx, ns: *mut u64, calls: *mut u64) -> c_int;
    pub fn smt_debug_group_fail_next(group: *mut SmtGroup, where_: c_int, code: c_int) -> c_int;
    pub fn smt_debug_batched_scores(
        corpus: *mut SmtCorpus,
        queries: *const f32,
        nq: u32,
        first_row: u64,
        n_rows: u32,
        out: *mut f32,
    ) -> c_int;
    pub fn smt_debug_nominations(
        corpus: *mut SmtCorpus,
        queries: *const f32,
        nq: u32,
        top_k: u32,
        ranges: *const SmtRange,
        n_ranges: u32,
        tau: *const f32,
        buffered: c_int,
        out_dist: *mut f32,
        out_hits: *mut u32,
        out_counts: *mut u32,
        out_route: *mut u32,
    ) -> c_int;
    pub fn smt_debug_gemm_plan(
        plan_tiles: u64,
        nq: u32,
        kp: u32,
        family: c_int,
        f16x1: c_int,
        blocks: u32,
        gemm_bootstrap: c_int,
        gemm_boot_fine: c_int,
        gemm_split_last: c_int,
        gemm_qsplit: c_int,
        out: *mut u64,
        out_cap: u32,
        out_n: *mut u32,
    ) -> c_int;
    pub fn smt_debug_level_nominations(
        corpus: *mut SmtCorpus,
        queries: *const f32,
        nq: u32,
        top_k: u32,
        ranges: *const SmtRange,
        n_ranges: u32,
        tau: *const f32,
        buffered: c_int,
        stride: u64,
        skip: u32,
        tile_begin: u64,
        tile_end: u64,
        out_dist: *mut f32,
        out_hits: *mut u32,
        out_counts: *mut u32,
        out_route: *mut u32,
    ) -> c_int;
    pub fn smt_debug_bootstrap_minima(
        corpus: *mut SmtCorpus,
        queries: *const f32,
        nq: u32,
        top_k: u32,
        ranges: *const SmtRange,
        n_ranges: u32,
        out_tile_min: *mut f32,
        out_slots: *mut u32,
        out_stride: *mut u64,
        out_route: *mut u32,
    ) -> c_int;
    pub fn smt_debug_bootstrap_tau(
        ctx: *mut SmtCtx,
        tile_min_dev: *const f32,
        n_slots: u32,
        nq: u32,
        nq_pad: u32,
        kp: u32,
        tau_dev: *mut f32,
        qconst_dev: *mut f32,
    ) -> c_int;
    pub fn smt_debug_level_select(
        ctx: *mut SmtCtx,
        cand_dev: *mut u64,
        counts_dev: *mut u32,
        overflow_dev: *mut u32,
        tau_dev: *mut f32,
        qconst_dev: *mut f32,
        nq: u32,
        kp: u32,
    ) -> c_int;
    pub fn smt_debug_gemm_trace(
        ctx: *mut SmtCtx,
        buf_dev: *mut u32,
        cap_words: u64,
        out_selects: *mut u32,
        out_words: *mut u64,
    ) -> c_int;
    pub fn smt_debug_merge_sources(
        ctx: *mut SmtCtx,
        lists_dev: *const *const u64,
        n_lists: u32,
        nq: u32,
        k_in: u32,
        k_out: u32,
        out_packed_dev: *mut u64,
    ) -> c_int;
    pub fn smt_debug_merge_packed_strided(
        ctx: *mut SmtCtx,
        packed_dev: *const u64,
        list_stride_words: u64,
        n_lists: u32,
        nq: u32,
        k_in: u32,
        k_out: u32,
        out_packed_dev: *mut u64,
    ) -> c_int;
    pub fn smt_debug_combine_status(
        ctx: *mut SmtCtx,
        words_dev: *const *const u64,
        base_dev: *const u64,
        stride_words: u64,
        n: u32,
        nq: u32,
        out_status_dev: *mut u32,
    ) -> c_int;
    pub fn smt_debug_select_lists(
        corpus: *mut SmtCorpus,
        queries_dev: *const f32,
        nq: u32,
        lists_dev: *const u64,
        list_stride: u64,
        n_lists: u32,
        kp: u32,
        k_out: u32,
        ws_threshold: c_int,
        ws_thr_score: f32,
        row_base: u64,
        f32_err: f64,
        overflow_dev: *const u32,
        out_stride: u64,
        out_rows_dev: *mut u64,
        out_dist_dev: *mut f64,
        out_counts_dev: *mut u64,
        out_uncertain_dev: *mut u64,
        out_status_dev: *mut u32,
    ) -> c_int;
    pub fn smt_debug_scan_lists(
        corpus: *mut SmtCorpus,
        queries: *const f32,
        nq: u32,
        top_k: u32,
        ranges: *const SmtRange,
        n_ranges: u32,
        out_keys: *mut u64,
        out_cap_keys: u64,
        out_blocks: *mut u32,
        out_kp: *mut u32,
        out_route: *mut u32,
    ) -> c_int;
    pub fn smt_debug_scan_ring(ctx: *mut SmtCtx, calls_back: u32, n_keys: u64, out_keys: *mut u64) -> c_int;
    pub fn smt_ctx_aux_stream(ctx: *mut SmtCtx, stream_out: *mut *mut c_void) -> c_int;
    pub fn smt_set_tuning(ctx: *mut SmtCtx, key: *const c_char, value: i64) -> c_int;
    pub fn smt_fnv1a_hash(bytes: *const u8, n: u64) -> u64;
    pub fn smt_line_embedding_id(path: *const c_char, line_number: i32) -> u64;
    pub fn smt_doc_meta_id(path: *const c_char) -> u64;
}

/// `anyhow` error carrying the library's thread-local message (the reference's error type on this path).
pub fn check(rc: c_int) -> anyhow::Result<()> {
    if rc == SMT_OK {
        return Ok(());
    }
    let msg = unsafe { std::ffi::CStr::from_ptr(smt_last_error()) }.to_string_lossy().into_owned();
    anyhow::bail!("semtools_hip error {rc}: {msg}")
}
