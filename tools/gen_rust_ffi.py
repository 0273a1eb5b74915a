#!/usr/bin/env python3
"""Writes rust/src/search/hip_ffi.rs: the complete `extern "C"` block for include/semtools_hip.h (every exported
function, same order, same argument names).  Run after changing the header: python tools/gen_rust_ffi.py"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import cdecl  # noqa: E402

HEADER = os.path.join(ROOT, "include", "semtools_hip.h")
OUT = os.path.join(ROOT, "rust", "src", "search", "hip_ffi.rs")

PRELUDE = '''//! FFI declarations for libsemtools_hip.so -- GENERATED from include/semtools_hip.h by tools/gen_rust_ffi.py,
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

'''

POSTLUDE = '''
/// `anyhow` error carrying the library's thread-local message (the reference's error type on this path).
pub fn check(rc: c_int) -> anyhow::Result<()> {
    if rc == SMT_OK {
        return Ok(());
    }
    let msg = unsafe { std::ffi::CStr::from_ptr(smt_last_error()) }.to_string_lossy().into_owned();
    anyhow::bail!("semtools_hip error {rc}: {msg}")
}
'''

RESERVED = {"type", "ref", "mod", "fn", "in", "box", "move", "match", "loop", "where", "use", "impl", "self"}


def main():
    src = open(HEADER).read()
    consts = re.findall(r"#define\s+(SMT_[A-Z_0-9]+)\s+\(?(-?\d+)u?\)?", src)
    lines = [PRELUDE]
    for name, val in consts:
        ty = "u32" if name in ("SMT_DIM",) else ("usize" if name == "SMT_UNIQUE_ID_BYTES" else "c_int")
        lines.append(f"pub const {name}: {ty} = {val};\n")
    lines.append('\nextern "C" {\n')
    for name, ret, params in cdecl.parse_header(HEADER):
        args = []
        for ctype, pname in params:
            if pname in RESERVED:
                pname += "_"
            args.append(f"{pname}: {cdecl.c_type_to_rust(ctype)}")
        r = "" if ret == "void" else f" -> {cdecl.c_type_to_rust(ret)}"
        one = f"    pub fn {name}({', '.join(args)}){r};\n"
        if len(one) > 118:
            one = f"    pub fn {name}(\n" + "".join(f"        {a},\n" for a in args) + f"    ){r};\n"
        lines.append(one)
    lines.append("}\n")
    lines.append(POSTLUDE)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").write("".join(lines))
    print("wrote", OUT)


if __name__ == "__main__":
    main()
