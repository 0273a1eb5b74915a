"""The wide IVF entry points on paper (no GPU): declared in the header, exported by the library, bound in Python and present in the
generated Rust block; the `wide` keyword of the Python classes defaults to off, so every existing call is what it was."""
import inspect
import os
import re
import subprocess

from semtools_amd import _lib as L
from semtools_amd import core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = ["smt_ivfpq_search_wide", "smt_ivfpq_search_wide_device", "smt_sharded_ivfpq_search_wide"]


def test_declared_exported_and_in_the_rust_block():
    header = open(os.path.join(ROOT, "include", "semtools_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "src", "search", "hip_ffi.rs")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in WIDE:
        assert re.search(rf"\bint {name}\(", header), name
        assert re.search(rf"\bpub fn {name}\(", rust), name
        assert re.search(rf" T {name}$", nm, re.M), name
        assert name in L.EXPORTS


def test_argument_counts_match_the_header():
    header = open(os.path.join(ROOT, "include", "semtools_hip.h")).read()
    lib = L.lib()
    for name in WIDE:
        decl = re.search(rf"\bint {name}\(([^;]*)\);", header).group(1)
        assert len(getattr(lib, name).argtypes) == decl.count(",") + 1, name


def test_the_wide_keyword_defaults_to_off():
    for fn in (core.IvfPq.search, core.IvfPq.search_device, core.ShardedIvfPq.search):
        assert inspect.signature(fn).parameters["wide"].default is False, fn
