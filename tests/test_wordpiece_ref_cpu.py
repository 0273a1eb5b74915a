"""CPU: tests/wordpiece_ref.py -- the Python restatement the device tokenizer's GPU tests compare with -- against the host tokenizer
(hf_tokenizer.cpp through smt_host_tokenizer_encode) on hand-written tokenizer.json files, and against the `tokenizers` wheel where
it is importable: the GPU tests are anchored on two independent host implementations.  Also: which tokenizers have a device form,
and what the new entry points answer on a machine without a device."""
import ctypes as C
import json

import numpy as np
import pytest

from semtools_amd import _lib as L
from tests import wordpiece_ref as W


def _load(path):
    h = C.c_void_p()
    L.check(L.lib().smt_host_tokenizer_load(str(path).encode(), C.byref(h)))
    return h


def _encode(h, raw):
    cap = len(raw) + 16
    ids = np.empty(cap, np.uint32)
    n = C.c_uint64()
    L.check(L.lib().smt_host_tokenizer_encode(h, raw, L.np_ptr(ids), cap, C.byref(n)))
    return ids[: n.value].tolist()


EDGE = [b"", b" ", b"\t\t", b"\x01\x02", b"!", b"ab\x01cd", b"a\x0bb", b"a\x0cb", b"HELLO World", b"w" * 100, b"w" * 101,
        b"w" * 50 + b"\x01\x02" + b"w" * 50, b"w" * 50 + b"\x01" + b"w" * 51, b"abzz", b"embeddings", b"understandings zzz the",
        b"a[b]c", b"[", b"x[PAD]y", b"[UNK]", b"internationalizations", b"don't 0xDEADBEEF e-mail", b"the\x7fthe", b"A\x1fB"]


@pytest.mark.parametrize("name", list(W.FLAG_SETS))
def test_reference_equals_the_host_tokenizer(tmp_path, name):
    flags = W.FLAG_SETS[name]
    ref = W.WordPieceRef(flags)
    h = _load(W.write_tokenizer(tmp_path / "tokenizer.json", flags))
    try:
        n_covered = n_unk = n_multi = 0
        for raw in EDGE + W.ascii_lines(seed=11, n=600):
            want = ref.encode(raw)
            if want is None:
                assert b"[PAD]" in raw or b"[UNK]" in raw, raw    # (pure ASCII: only an added token sends a line away)
                continue
            assert _encode(h, raw) == want, (name, raw)
            n_covered += 1
            n_unk += ref.unk in want
            n_multi += len(want) > len(raw.split())
        assert n_covered > 400 and n_unk > 50 and n_multi > 100   # the inputs do reach unks and multi-piece words
    finally:
        L.lib().smt_host_tokenizer_free(h)


@pytest.mark.parametrize("name", list(W.FLAG_SETS))
def test_reference_equals_the_tokenizers_wheel(tmp_path, name):
    tokenizers = pytest.importorskip("tokenizers")
    flags = W.FLAG_SETS[name]
    ref = W.WordPieceRef(flags)
    tok = tokenizers.Tokenizer.from_file(W.write_tokenizer(tmp_path / "tokenizer.json", flags))
    for raw in EDGE + W.ascii_lines(seed=12, n=400):
        want = ref.encode(raw)
        if want is None or b"\x00" in raw:
            continue
        assert tok.encode(raw.decode(), add_special_tokens=False).ids == want, (name, raw)


def test_the_steps_around_the_tokenizer():
    ref = W.WordPieceRef(7)
    v = ref.vocab
    # zzz is one unk; dropped before the cap, so the cap keeps what lies behind it
    assert ref.line(b"zzz the fox", max_tokens=2, drop_unk=True) == ([v[b"the"], v[b"fox"]], False)
    assert ref.line(b"zzz the fox", max_tokens=2, drop_unk=False) == ([ref.unk, v[b"the"]], False)
    assert ref.line(b"the foxes", keep_bytes=7) == ([v[b"the"], v[b"fox"]], False)       # cut mid-word: tokenized as cut
    assert ref.line(b"the \xc3\xa9", keep_bytes=4) == ([v[b"the"]], False) and ref.line(b"the \xc3\xa9", keep_bytes=5) == ([], True)
    assert ref.line(b"ab\x01cd") == ([v[b"abcd"]], False) and W.WordPieceRef(1).line(b"ab\x01cd")[0] != [v[b"abcd"]]
    assert ref.line(b"a\x0bb") == ([v[b"ab"]], False) and W.WordPieceRef(1).line(b"a\x0bb") == ([v[b"a"], v[b"b"]], False)


def test_only_the_bert_wordpiece_family_has_a_device_form(tmp_path):
    p = tmp_path / "unigram.json"
    p.write_text(json.dumps(W.unigram_json()))
    h = _load(p)
    out = C.c_void_p()
    try:
        assert L.lib().smt_host_tokenizer_to_device(h, None, C.byref(out)) == L.SMT_E_UNSUPPORTED and not out
        assert b"device form" in L.lib().smt_last_error()
    finally:
        L.lib().smt_host_tokenizer_free(h)


@pytest.mark.skipif(L.lib().smt_device_count() > 0, reason="a GPU is present")
def test_without_a_device_the_new_entry_points_fail_loudly(tmp_path):
    lib = L.lib()
    out = C.c_void_p()
    h = _load(W.write_tokenizer(tmp_path / "tokenizer.json", 7))
    try:
        assert lib.smt_host_tokenizer_to_device(h, None, C.byref(out)) == L.SMT_E_HIP and not out
    finally:
        lib.smt_host_tokenizer_free(h)
    prm = L.SmtWordpieceParams()
    assert lib.smt_wordpiece_create(None, C.byref(prm), C.byref(out)) == L.SMT_E_HIP and not out
    assert lib.smt_wordpiece_scan_device(None, None, 0, None, None, 0, 0, 0, 1, None, None, None) == L.SMT_E_HIP
    assert lib.smt_wordpiece_emit_device(None, 0, None, None, None, 0, 0, None, 0, None) == L.SMT_E_HIP
    assert lib.smt_wordpiece_tokenize(None, None, None, None, 0, 0, 0, 1, None, 0, None, None) == L.SMT_E_HIP
    assert b"no HIP device" in lib.smt_last_error()
