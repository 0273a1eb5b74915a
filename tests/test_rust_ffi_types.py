"""CPU: the TYPES of the committed Rust bindings (rust/src/search/hip_ffi.rs).  tests/test_rust_ffi.py compares the functions; the
file cannot be compiled here, so this checks what a compiler would say first: every `Smt*` type an extern declaration names is
declared in the file, and every struct include/semtools_hip.h defines with fields has a #[repr(C)] struct of the same field names, in
order, with the mapped types."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import cdecl  # noqa: E402

HEADER = os.path.join(ROOT, "include", "semtools_hip.h")
FFI = os.path.join(ROOT, "rust", "src", "search", "hip_ffi.rs")


def _declared(ffi):
    names = set(re.findall(r"pub struct (\w+)", ffi))
    for group in re.findall(r"opaque!\(([^)]*)\)", ffi):
        names |= {n.strip() for n in group.split(",") if n.strip()}
    return names


def test_every_type_the_extern_block_names_is_declared():
    ffi = open(FFI).read()
    block = ffi[ffi.index('extern "C" {'):]
    used = set(re.findall(r"\b(Smt[A-Z]\w*)\b", block))
    assert len(used) >= 10
    missing = sorted(used - _declared(ffi))
    assert not missing, f"hip_ffi.rs names {missing} without declaring them (the preamble of tools/gen_rust_ffi.py)"


def test_structs_with_fields_match_the_header():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    ffi = open(FFI).read()
    structs = re.findall(r"typedef struct (\w+) \{(.*?)\} \1;", hdr, flags=re.S)
    assert len(structs) >= 5 and "smt_wordpiece_codepoints" in [n for n, _ in structs]
    for name, body in structs:
        fields = []
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if decl:
                m = re.match(r"(.*?)(\w+)$", decl)
                fields.append((m.group(2), cdecl.c_type_to_rust(m.group(1).strip())))
        rust_name = cdecl.c_type_to_rust(name + " *")[len("*mut "):]
        m = re.search(r"#\[repr\(C\)\][^{]*pub struct %s \{(.*?)\n\}" % rust_name, ffi, flags=re.S)
        assert m, f"{name}: no #[repr(C)] pub struct {rust_name}"
        got = re.findall(r"pub (\w+): ([^,]+),", m.group(1))
        assert [(n.rstrip("_"), t.strip()) for n, t in got] == fields, (name, got, fields)
