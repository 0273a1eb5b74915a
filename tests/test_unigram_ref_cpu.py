"""CPU: tests/unigram_ref.py -- the Python restatement the Unigram device tokenizer's GPU tests compare with -- against the host
tokenizer (hf_tokenizer.cpp through smt_host_tokenizer_encode) on hand-written tokenizer.json files, and against the `tokenizers`
wheel, where it is importable, on a Unigram trained here.  Also: which tokenizers have a Unigram device form, and what the new entry
points answer on a machine without a device."""
import ctypes as C
import json

import numpy as np
import pytest

from semtools_amd import _lib as L
from tests import unigram_ref as U
from tests import wordpiece_ref as W


def _load(path):
    h = C.c_void_p()
    L.check(L.lib().smt_host_tokenizer_load(str(path).encode(), C.byref(h)))
    return h


def _encode(h, raw):
    """ids, or None when the host tokenizer raises"""
    cap = len(raw) + 16
    ids = np.empty(cap, np.uint32)
    n = C.c_uint64()
    if L.lib().smt_host_tokenizer_encode(h, raw, L.np_ptr(ids), cap, C.byref(n)) != L.SMT_OK:
        return None
    return ids[: n.value].tolist()


def _has_device_form(path):
    """export_unigram's answer, without a device: only a tokenizer without the form is SMT_E_UNSUPPORTED (one with it goes on to
    smt_unigram_create, which rejects the null context)"""
    h = _load(path)
    out = C.c_void_p()
    try:
        rc = L.lib().smt_host_tokenizer_to_device_unigram(h, None, C.byref(out))
        assert not out and rc in (L.SMT_E_UNSUPPORTED, L.SMT_E_HIP, L.SMT_E_INVALID)
        if rc == L.SMT_E_UNSUPPORTED:
            assert b"device form" in L.lib().smt_last_error()
        return rc != L.SMT_E_UNSUPPORTED
    finally:
        L.lib().smt_host_tokenizer_free(h)


LINES = list(U.NAMED.values()) + [raw[:keep] for raw, keep in U.CUTS] + U.ascii_lines(seed=21, n=300)


@pytest.mark.parametrize("unk_id", [0, None])
@pytest.mark.parametrize("prepend", U.PREPEND)
@pytest.mark.parametrize("norm", list(U.NORMALIZERS))
def test_reference_equals_the_host_tokenizer(tmp_path, norm, prepend, unk_id):
    tj = U.tokenizer_json(norm=norm, prepend=prepend, unk_id=unk_id)
    ref = U.UnigramRef(tj)
    (tmp_path / "tokenizer.json").write_text(json.dumps(tj))
    h = _load(tmp_path / "tokenizer.json")
    try:
        n_covered = n_unk = n_raise = 0
        for raw in LINES:
            if any(c >= 0x80 for c in raw) or b"<pad>" in raw:
                assert ref.encode(raw) is None, raw
                continue
            got = _encode(h, raw)
            want = ref.encode(raw, check_limit=False)     # (the length limit flags a line for the device only: the host has none)
            if want is None:                                 # an unknown character on the best path and no unk id: the host raises
                assert unk_id is None and got is None, (norm, prepend, raw)
                n_raise += 1
                continue
            assert got == want, (norm, prepend, unk_id, raw)
            n_covered += 1
            n_unk += unk_id is not None and unk_id in want
        # the inputs do reach unknowns: as ids with an unk id, as errors without one (where only lines free of them are compared)
        assert n_covered > 50 and (n_unk > 100 if unk_id is not None else n_raise > 100)
    finally:
        L.lib().smt_host_tokenizer_free(h)


def test_the_named_properties_of_the_vocabulary():
    ref = U.UnigramRef(U.tokenizer_json())
    v = {p: i for i, (p, _) in enumerate(U.build_vocab())}     # (the later index of a repeated piece)
    R = U.R
    assert ref.encode(b"abcd") == [v[R + "ab"], v["cd"]]                    # greedy would take R+abc, d
    assert ref.encode(b"xy") == [v[R], v["xy"]]                             # the tie: -2 + -5 == -3 + -4, the smaller start wins
    assert -2.0 + -5.0 == -3.0 + -4.0
    assert ref.encode(b"the") == [v[R + "the"]] and ref.encode(b"bathe") == [v[R], v["b"], v["a"], v["the"]]
    assert v["the"] != [p for p, _ in U.build_vocab()].index("the")        # the repeated piece resolves to its later id
    assert ref.encode(b"azzqzb") == [v[R + "a"], 0, v["b"]]                 # one fused unk
    assert ref.encode(b" ") == [v[R]] and ref.encode(b"") == [] and ref.encode(b"a") == [v[R + "a"]]
    assert ref.encode(b"z") == [v[R], 0]                                    # two tokens from one byte
    assert ref.encode(b"qu") == [v[R], v["qu"]]                             # q has no single piece, but no unknown is on the path
    never = U.UnigramRef(U.tokenizer_json(prepend="never"))
    assert never.encode(b"the fox") == [v["the"], v[R + "fox"]]
    clean = U.UnigramRef(U.tokenizer_json(norm="bert_clean"))
    assert clean.encode(b"\x01\x02") == [v[R]] and clean.encode(b"the\tfox") == [v[R + "the"], v[R + "fox"]]
    assert ref.encode(b"the\tfox") == [v[R + "the"], v["\t"], v["fox"]]
    assert clean.encode(b"THE") == [v[R + "the"]] and ref.encode(b"THE") == [v[R], v["T"], v["H"], v["E"]]
    # the steps around the tokenizer: the unk drop takes the literal <unk> piece too, the cap comes after it
    assert ref.line(b"z the <unk> fox", max_tokens=2) == ([v[R], v[R + "the"]], False)
    assert ref.line(b"z the", max_tokens=2, drop_unk=False) == ([v[R], 0], False)
    assert ref.line(b"the caf\xc3\xa9", keep_bytes=7)[1] is False and ref.line(b"the caf\xc3\xa9", keep_bytes=8) == ([], True)
    assert ref.line(b"the <pad>", keep_bytes=8)[1] is False and ref.line(b"the <pad>", keep_bytes=9) == ([], True)
    assert ref.line(U.NAMED["exactly_max_word"])[1] is False and ref.line(U.NAMED["max_word_plus_one"]) == ([], True)
    assert U.UnigramRef(U.tokenizer_json(unk_id=None)).line(b"thez") == ([], True)


@pytest.mark.parametrize("prepend", U.PREPEND)
def test_reference_equals_the_tokenizers_wheel(tmp_path, prepend):
    tokenizers = pytest.importorskip("tokenizers")
    from tokenizers import Tokenizer, models, normalizers, pre_tokenizers, trainers
    corpus = ["the quick brown fox jumps over the lazy dog, again and again!", "semantic search over plain text files: embeddings, cosine, top-k.",
              "searching texts and foxes; the fox searches the text 12345 times", "numbers 12345 67.89 1e-5 0xdeadbeef and punct !?.,:;()[]{}"] * 8
    tok = Tokenizer(models.Unigram())
    tok.normalizer = normalizers.Sequence([normalizers.NFD(), normalizers.Lowercase()])
    tok.pre_tokenizer = pre_tokenizers.Metaspace(prepend_scheme=prepend)
    tok.train_from_iterator(corpus, trainers.UnigramTrainer(vocab_size=200, special_tokens=["<unk>", "[PAD]"], unk_token="<unk>", show_progress=False))
    path = tmp_path / "tokenizer.json"
    tok.save(str(path))
    assert _has_device_form(path)
    ref = U.UnigramRef(json.loads(path.read_text()))
    n = 0
    for raw in LINES + [x.encode() for x in corpus[:4]] + [b"the [PAD] fox", b"<unk>"]:
        want = ref.encode(raw, check_limit=False)
        if want is None:
            continue
        assert tok.encode(raw.decode(), add_special_tokens=False).ids == want, (prepend, raw)
        n += 1
    assert n > 300


def test_which_tokenizers_have_a_unigram_device_form(tmp_path):
    def has(name, tj):
        p = tmp_path / (name + ".json")
        p.write_text(json.dumps(tj))
        return _has_device_form(p)

    for norm in U.NORMALIZERS:
        for prepend in U.PREPEND:
            assert has(f"ok_{norm}_{prepend}", U.tokenizer_json(norm=norm, prepend=prepend))
    assert has("ok_seq_pre", U.tokenizer_json(pre_sequence=True)) and has("ok_no_unk", U.tokenizer_json(unk_id=None))
    assert has("ok_other_replacement", U.tokenizer_json(replacement="·"))
    strip = {"type": "Sequence", "normalizers": [{"type": "Strip", "strip_left": True, "strip_right": True}, {"type": "Lowercase"}]}
    replace = {"type": "Replace", "pattern": {"String": "a"}, "content": "b"}
    assert not has("strip", U.tokenizer_json(norm=strip))
    assert not has("replace", U.tokenizer_json(norm=replace))
    assert not has("no_split", U.tokenizer_json(split=False))
    assert not has("ascii_replacement", U.tokenizer_json(replacement="_"))
    two = U.tokenizer_json()
    two["pre_tokenizer"] = {"type": "Sequence", "pretokenizers": [two["pre_tokenizer"], {"type": "Punctuation", "behavior": "Isolated"}]}
    assert not has("two_pretokenizers", two)
    assert not _has_device_form(W.write_tokenizer(tmp_path / "wordpiece.json", 7))
    # ... and a Unigram tokenizer has no WordPiece form, as before
    h = _load(tmp_path / "ok_none_always.json")
    out = C.c_void_p()
    try:
        assert L.lib().smt_host_tokenizer_to_device(h, None, C.byref(out)) == L.SMT_E_UNSUPPORTED and not out
    finally:
        L.lib().smt_host_tokenizer_free(h)


@pytest.mark.skipif(L.lib().smt_device_count() > 0, reason="a GPU is present")
def test_without_a_device_the_new_entry_points_fail_loudly(tmp_path):
    lib = L.lib()
    out = C.c_void_p()
    h = _load(U.write_tokenizer(tmp_path / "tokenizer.json"))
    try:
        assert lib.smt_host_tokenizer_to_device_unigram(h, None, C.byref(out)) == L.SMT_E_HIP and not out
    finally:
        lib.smt_host_tokenizer_free(h)
    prm = L.SmtUnigramParams()
    assert lib.smt_unigram_create(None, C.byref(prm), C.byref(out)) == L.SMT_E_HIP and not out
    assert lib.smt_unigram_scan_device(None, None, 0, None, None, 0, 0, 0, 1, None, None, None) == L.SMT_E_HIP
    assert lib.smt_unigram_emit_device(None, 0, None, None, None, 0, 0, None, 0, None) == L.SMT_E_HIP
    assert lib.smt_unigram_tokenize(None, None, None, None, 0, 0, 0, 1, None, 0, None, None) == L.SMT_E_HIP
    assert b"no HIP device" in lib.smt_last_error()
