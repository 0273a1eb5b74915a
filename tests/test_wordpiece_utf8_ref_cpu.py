"""CPU: tests/wordpiece_utf8_ref.py -- the Python restatement the UTF-8 device tokenizer's GPU tests compare with -- against the host
tokenizer (hf_tokenizer.cpp through smt_host_tokenizer_encode) and, where importable, the `tokenizers` wheel, for the four flag sets,
named lines and 1000 generated lines.  Also: the per-code-point property the device table rests on, asserted on those lines; what is
expected flagged; which tokenizers have a UTF-8 device form; and what the new entry points answer without a device."""
import ctypes as C
import json

import numpy as np
import pytest

from semtools_amd import _lib as L
from tests import wordpiece_ref as W
from tests import wordpiece_utf8_ref as U8

VOCAB = U8.build_vocab()
NAMED = ["café the", "Café CAFÉ café", "naïve über Über", "λόγος Λόγος και",
         "привет мир Мир й", "中文", "the中文fox", "中 x文y", "한글 한", "한글x",
         "“the” fox—again…", "«fox»", "the fox again", "á̀b", "ẃ" * 100, "é" * 100, "é" * 101,
         "ok\U0001f600 \U0001f600\U0001f600", "\U0001d400\U0001d401", "かな か", "x�y", "x​y", "x­y", "ﬁx ǆ İ ß Ω",
         "[PAD] café", "　中　", "한", "ę́ ẛ̣"]
NAMED = [s.encode() for s in NAMED]


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


@pytest.fixture(scope="module")
def lines():
    return NAMED + U8.utf8_lines(seed=21, n=1000)


@pytest.mark.parametrize("name", list(W.FLAG_SETS))
def test_reference_equals_the_host_tokenizer(tmp_path, name, lines):
    flags = W.FLAG_SETS[name]
    ref = U8.WordPieceUtf8Ref(flags, VOCAB, blocks=None)
    h = _load(W.write_tokenizer(tmp_path / "tokenizer.json", flags, vocab=VOCAB))
    try:
        n_covered = n_unk = n_multi = 0
        for raw in lines:
            want = ref.encode(raw)
            if want is None or b"\x00" in raw:    # (the C string ends at a NUL)
                continue
            assert _encode(h, raw) == want, (name, raw)
            n_covered += 1
            n_unk += ref.unk in want
            n_multi += len(want) > len(raw.split())
        print(name, "covered", n_covered, "with unk", n_unk, "multi-piece", n_multi)
        assert n_covered > 500 and n_unk > 100 and n_multi > 100
    finally:
        L.lib().smt_host_tokenizer_free(h)


@pytest.mark.parametrize("name", list(W.FLAG_SETS))
def test_reference_equals_the_tokenizers_wheel(tmp_path, name, lines):
    tokenizers = pytest.importorskip("tokenizers")
    flags = W.FLAG_SETS[name]
    ref = U8.WordPieceUtf8Ref(flags, VOCAB, blocks=None)
    tok = tokenizers.Tokenizer.from_file(W.write_tokenizer(tmp_path / "tokenizer.json", flags, vocab=VOCAB))
    for raw in lines:
        want = ref.encode(raw)
        if want is None or b"\x00" in raw:
            continue
        assert tok.encode(raw.decode(), add_special_tokens=False).ids == want, (name, raw)


@pytest.mark.parametrize("name", list(W.FLAG_SETS))
def test_normalizing_a_covered_line_is_concatenating_the_code_point_answers(name, lines):
    """the property the device table rests on: on a line without a FLAG code point, BertNormalizer over the whole line equals the
    per-code-point outputs back to back (an ALONE CJK character with its two spaces put back)"""
    flags = W.FLAG_SETS[name]
    ref = U8.WordPieceUtf8Ref(flags, VOCAB, blocks=None)
    n = 0
    for raw in lines:
        s = ref.decode(raw)
        if s is None or any(ref.cp_class(ord(ch)) == U8.FLAG for ch in s):
            continue
        parts = []
        for ch in s:
            if ord(ch) < 0x80:
                parts.append(U8.normalize(ch, flags))
                continue
            k, o = U8.classify(ord(ch), flags)
            o = o or ch
            parts.append("" if k == U8.DROPPED else " " if k == U8.SPACE and flags & W.WP_CLEAN_TEXT else ch if k == U8.SPACE else
                         " " + o + " " if k == U8.ALONE and U8.is_chinese_char(ch) and flags & W.WP_NORMALIZER else o)
        assert "".join(parts) == U8.normalize(s, flags), (name, raw)
        for ch in s:
            if ord(ch) >= 0x80:
                k, o = U8.classify(ord(ch), flags)
                assert len(o or ch) <= len(ch.encode()) + (2 if k == U8.ALONE else 0), ch    # an output fits its source's bytes
        n += 1
    assert n > 500


def test_what_is_flagged(lines):
    gen = lines[len(NAMED):]
    non_ascii = [raw for raw in gen if any(c >= 0x80 for c in raw)]
    assert len(non_ascii) > 600
    # uncased: only an added token sends a generated line away
    ref = U8.WordPieceUtf8Ref(W.FLAG_SETS["norm_clean_lower"], VOCAB, blocks=None)
    flagged = [raw for raw in gen if not ref.covered(raw)]
    assert all(b"[PAD]" in raw or b"[UNK]" in raw for raw in flagged), [r for r in flagged if b"[PAD]" not in r and b"[UNK]" not in r][:3]
    assert sum(ref.covered(raw) for raw in non_ascii) >= 0.9 * len(non_ascii)      # a reference that flags everything cannot pass
    # the kernel-level tests' table (U8.BLOCKS) covers them as well
    blk = U8.WordPieceUtf8Ref(W.FLAG_SETS["norm_clean_lower"], VOCAB)
    assert sum(blk.covered(raw) for raw in non_ascii) >= 0.9 * len(non_ascii)
    # without strip_accents a combining mark stays, and its line is flagged
    for name in ("norm_clean", "norm_only", "no_norm"):
        cased = U8.WordPieceUtf8Ref(W.FLAG_SETS[name], VOCAB, blocks=None)
        # (U+034F, the grapheme joiner, is the one mark of the block with combining class 0: no reordering can move it)
        marks = [raw for raw in gen if any(0x300 <= ord(ch) <= 0x36F and ord(ch) != 0x34F for ch in raw.decode())]
        assert len(marks) > 50 and not any(cased.covered(raw) for raw in marks)
        assert cased.covered("café".encode()) and not cased.covered("café".encode())
    # malformed UTF-8, each form
    for bad in (b"a\x80b", b"caf\xc3", b"\xe4\xb8", b"\xc0\xaf", b"\xe0\x80\xaf", b"\xf0\x80\x80\xaf", b"\xed\xa0\x80", b"\xf4\x90\x80\x80",
                b"\xf8\x88\x80\x80\x80", b"\xff", b"\xc3\xa9\xa9"):
        assert not ref.covered(bad) and ref.line(b"the " + bad) == ([], True), bad


FLAG_UNCASED = """1B44 1BAA 1BF2 1BF3 302E 302F A953 A9C0 111C0 11235 1134D 116B6 1193D 16FF0 16FF1 1D15E 1D15F 1D160 1D161 1D162 1D163 1D164
1D165 1D166 1D16D 1D16E 1D16F 1D170 1D171 1D172 1D1BB 1D1BC 1D1BD 1D1BE 1D1BF 1D1C0"""


def test_the_flag_code_points_below_U30000_by_name_and_by_rule():
    """Which code points the table leaves to the host, with the tables of Unicode 13 (this module's unicodedata and the host tokenizer's
    unicode_lower.h alike).  Cased (no strip_accents): exactly the 872 characters of non-zero combining class.  Uncased: 36, the
    characters whose canonical decomposition holds a character of non-zero combining class that is NOT a non-spacing mark (spacing
    viramas and tone marks, the musical symbols that decompose into them) -- strip_accents removes the non-spacing ones.  A count
    taken with the `tokenizers` wheel comes to 154 uncased: its non-spacing-mark table is older and keeps 118 marks of newer scripts
    (U+07FD, U+08D3 .. U+08E1, U+1E000 .. U+1E02A, U+1E944 .. U+1E94A, ...) which the host tokenizer, and so the device, strips."""
    import unicodedata

    below = [cp for cp in range(0x80, 0x30000) if not 0xD800 <= cp <= 0xDFFF]
    cased = [cp for cp in below if U8.classify(cp, W.FLAG_SETS["norm_clean"])[0] == U8.FLAG]
    assert cased == [cp for cp in below if unicodedata.combining(chr(cp))]
    uncased = [cp for cp in below if U8.classify(cp, W.FLAG_SETS["norm_clean_lower"])[0] == U8.FLAG]
    assert uncased == [cp for cp in below if any(unicodedata.combining(c) and unicodedata.category(c) != "Mn"
                                                 for c in unicodedata.normalize("NFD", chr(cp)))]
    if unicodedata.unidata_version == "13.0.0":                     # the version the host tokenizer's tables were generated from
        assert len(cased) == 872 and uncased == [int(x, 16) for x in FLAG_UNCASED.split()]


def test_the_steps_around_the_tokenizer():
    ref = U8.WordPieceUtf8Ref(7, VOCAB)
    v = ref.vocab
    assert ref.line("café the".encode()) == ([v["cafe"], v["the"]], False)
    assert U8.WordPieceUtf8Ref(3, VOCAB).line("café the".encode()) == ([v["café"], v["the"]], False)
    # a line longer than keep_bytes: cut by bytes, flagged for a byte >= 0x80 in front of the cut; a line no longer than the cut has none
    raw = "the café".encode()                                                    # 9 bytes, the two of the accent at 7 and 8
    assert ref.line(raw, keep_bytes=7) == ([v["the"], ref.vocab["c"], v["##a"], v["##f"]], False)
    assert ref.line(raw, keep_bytes=8) == ([], True) and ref.line(raw, keep_bytes=9) == ([v["the"], v["cafe"]], False)
    # the unk of a word is dropped before the cap
    assert ref.line("þþ the fox".encode(), max_tokens=2, drop_unk=True) == ([v["the"], v["fox"]], False)
    assert ref.line("þþ the fox".encode(), max_tokens=2, drop_unk=False) == ([ref.unk, v["the"]], False)
    # a Hangul syllable becomes its jamo under strip_accents, and the pieces split inside it
    assert ref.line("\ud55c".encode()) == ([v[U8.JAMO_HA], v["##" + U8.JAMO_N]], False)
    assert ref.line("\ud55c\uae00".encode()) == ([v[U8.JAMO_HA], v["##" + U8.JAMO_N + U8.JAMO_G], v["##" + U8.JAMO_EUL]], False)
    assert U8.WordPieceUtf8Ref(3, VOCAB).line("\ud55c\uae00".encode()) == ([v["\ud55c"], v["##\uae00"]], False)


def test_only_the_bert_wordpiece_family_has_a_utf8_device_form(tmp_path):
    out = C.c_void_p()
    p = tmp_path / "unigram.json"
    p.write_text(json.dumps(W.unigram_json()))
    h = _load(p)
    try:
        assert L.lib().smt_host_tokenizer_to_device_utf8(h, None, C.byref(out)) == L.SMT_E_UNSUPPORTED and not out
        assert b"device form" in L.lib().smt_last_error()
    finally:
        L.lib().smt_host_tokenizer_free(h)
    # an added token matched on the raw text with a non-ASCII byte: the ASCII form exists (such a token cannot stand in an ASCII line),
    # the UTF-8 form does not
    tj = W.tokenizer_json(7, vocab=dict(VOCAB, **{"[MÄSK]": len(VOCAB)}))
    tj["added_tokens"].append(dict(tj["added_tokens"][0], id=len(VOCAB), content="[MÄSK]"))
    p = tmp_path / "tokenizer.json"
    p.write_text(json.dumps(tj))
    h = _load(p)
    try:
        assert L.lib().smt_host_tokenizer_to_device_utf8(h, None, C.byref(out)) == L.SMT_E_UNSUPPORTED and not out
        assert L.lib().smt_host_tokenizer_to_device(h, None, C.byref(out)) != L.SMT_E_UNSUPPORTED and not out   # (no context: it ends there)
    finally:
        L.lib().smt_host_tokenizer_free(h)


@pytest.mark.skipif(L.lib().smt_device_count() > 0, reason="a GPU is present")
def test_without_a_device_the_new_entry_points_fail_loudly(tmp_path):
    lib = L.lib()
    out = C.c_void_p()
    h = _load(W.write_tokenizer(tmp_path / "tokenizer.json", 7, vocab=VOCAB))
    try:
        assert lib.smt_host_tokenizer_to_device_utf8(h, None, C.byref(out)) == L.SMT_E_HIP and not out
    finally:
        lib.smt_host_tokenizer_free(h)
    prm, cps = L.SmtWordpieceParams(), L.SmtWordpieceCodepoints()
    assert lib.smt_wordpiece_create_utf8(None, C.byref(prm), C.byref(cps), C.byref(out)) == L.SMT_E_HIP and not out
    assert b"no HIP device" in lib.smt_last_error()
