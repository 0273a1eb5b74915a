"""CPU: tests/unigram_utf8_ref.py -- the Python restatement the Unigram device tokenizer's UTF-8 GPU tests compare with -- against the host
tokenizer (hf_tokenizer.cpp through smt_host_tokenizer_encode) and, where it imports, the `tokenizers` wheel, on the named lines and
1000 generated mixed-script lines per configuration (five normalizer chains x three prepend schemes).  Also: the concatenation
property the per-code-point table rests on, the FLAG code points per chain by count and by rule, the cap on what the reference
flags of the generated lines, which tokenizers have the form, and what the new entry points answer without a device.

The host tokenizer is the authority where it and the wheel differ.  The differences met here are named below and asserted by rule."""
import ctypes as C
import json
import unicodedata

import numpy as np
import pytest

from semtools_amd import _lib as L
from tests import unigram_ref as U
from tests import unigram_utf8_ref as G
from tests import wordpiece_ref as W
from tests import wordpiece_utf8_ref as W8

NAMED = list(G.NAMED.values())
DELIBERATE = list(G.MALFORMED.values())      # lines no form covers, counted apart from the generated ones
N_GEN = 1000
V_R = max(i for i, (p, _) in enumerate(G.build_vocab()) if p == G.R)     # (the later id of the repeated piece)
# the 118 non-spacing marks of newer scripts: the host tokenizer strips them, the wheel's older table keeps them
NEWER_MARKS = ["a\u08d4b", "the\u07fd fox", "a\U0001e000b"]


@pytest.fixture(scope="module")
def generated():
    return G.utf8_lines(seed=7, n=N_GEN)


def _load(path):
    h = C.c_void_p()
    L.check(L.lib().smt_host_tokenizer_load(str(path).encode(), C.byref(h)))
    return h


def _encode(h, raw):
    cap = len(raw) + 16
    ids = np.empty(cap, np.uint32)
    n = C.c_uint64()
    if L.lib().smt_host_tokenizer_encode(h, raw, L.np_ptr(ids), cap, C.byref(n)) != L.SMT_OK:
        return None
    return ids[: n.value].tolist()


def _write(tmp_path, tj, name="tokenizer.json"):
    p = tmp_path / name
    p.write_text(json.dumps(tj))
    return p


@pytest.mark.parametrize("prepend", G.PREPEND)
@pytest.mark.parametrize("norm", G.NORMS)
def test_reference_equals_the_host_tokenizer(tmp_path, generated, norm, prepend):
    tj = G.tokenizer_json(norm=norm, prepend=prepend)
    ref = G.UnigramUtf8Ref(tj, blocks=None)
    h = _load(_write(tmp_path, tj))
    try:
        n_covered = n_non_ascii = 0
        for raw in NAMED + generated + [x[:k] for x, k in G.CUTS]:
            want = ref.encode(raw, check_limit=False)      # (the length limit flags a line for the device only: the host has none)
            if want is None:
                continue
            assert _encode(h, raw) == want, (norm, prepend, raw)
            n_covered += 1
            n_non_ascii += any(c >= 0x80 for c in raw)
        assert n_covered > 900 and n_non_ascii > 600
        for raw in DELIBERATE:
            assert ref.encode(raw) is None, raw
    finally:
        L.lib().smt_host_tokenizer_free(h)


def _first_dropped(s, n):
    return s != "" and G.normalize(s[0], n) == ""


def _strips_other_marks(s, n):
    """the chain holds a StripAccents and the text, decomposed, a mark that is not a NON-SPACING mark (Mc, Me)"""
    def has_strip(x):
        return x is not None and (x["type"] == "StripAccents" or (x["type"] == "Sequence" and any(has_strip(c) for c in x["normalizers"])))
    return has_strip(n) and any(unicodedata.category(c) in ("Mc", "Me") for c in unicodedata.normalize("NFD", s))


@pytest.mark.parametrize("prepend", G.PREPEND)
@pytest.mark.parametrize("norm", G.NORMS)
def test_reference_equals_the_tokenizers_wheel(tmp_path, generated, norm, prepend):
    """Equal ids, but for three differences between the host tokenizer and the wheel, each older than the device form and each met by
    the generated lines: EMPTY -- of a line whose normalised text is empty the host tokenizer makes the prepended replacement alone,
    the wheel nothing; FIRST -- under the scheme `first` the wheel prepends only when the first normalised character comes from the
    line's first character, so a dropped character in front suppresses it; MARKS -- the wheel's StripAccents removes every mark
    (Mn, Mc, Me), the host tokenizer's the non-spacing ones (Mn) only.  A capital sigma at a word's end is NOT among them: both
    lower-case it per character, to a medial sigma (asserted below)."""
    tokenizers = pytest.importorskip("tokenizers")
    tj = G.tokenizer_json(norm=norm, prepend=prepend)
    n = G.NORMALIZERS[norm]
    ref = G.UnigramUtf8Ref(tj, blocks=None)
    tok = tokenizers.Tokenizer.from_file(str(_write(tmp_path, tj)))
    seen = {"EMPTY": 0, "FIRST": 0, "MARKS": 0}
    n_same = 0
    for raw in NAMED + generated:
        want = ref.encode(raw, check_limit=False)
        if want is None:
            continue
        s = raw.decode()
        got = tok.encode(s, add_special_tokens=False).ids
        if got == want:
            n_same += 1
            continue
        if G.normalize(s, n) == "" and prepend != "never":
            seen["EMPTY"] += 1
            assert got == [] and want == [V_R], raw
        elif prepend == "first" and _first_dropped(s, n):
            seen["FIRST"] += 1
        elif _strips_other_marks(s, n):
            seen["MARKS"] += 1
        else:
            raise AssertionError((norm, prepend, raw, got, want))
    assert n_same > 850
    drops = norm in ("bert_clean", "bert_noclean", "seq")
    assert (seen["EMPTY"] > 0) == (drops and prepend != "never")
    assert (seen["FIRST"] > 0) == (drops and prepend == "first")
    assert (seen["MARKS"] > 0) == (norm == "seq")
    if norm == "lower":
        sigma = "ΛΟΓΟΣ".encode()
        assert tok.encode(sigma.decode(), add_special_tokens=False).ids == ref.encode(sigma) and G.normalize("Σ", n) == "σ"


@pytest.mark.parametrize("norm", ["bert_clean", "bert_noclean", "seq"])
def test_the_newer_non_spacing_marks_follow_the_host_tokenizer(tmp_path, norm):
    """the named exception of DESIGN 4.9: 118 marks of newer scripts are non-spacing for the host tokenizer and for this reference
    (Unicode 13), and stripped; the wheel's table does not know them"""
    tj = G.tokenizer_json(norm=norm)
    ref = G.UnigramUtf8Ref(tj, blocks=None)
    h = _load(_write(tmp_path, tj))
    try:
        for s in NEWER_MARKS:
            plain = "".join(c for c in s if unicodedata.category(c) != "Mn")
            assert plain != s and _encode(h, s.encode()) == ref.encode(s.encode()) == ref.encode(plain.encode()), s
    finally:
        L.lib().smt_host_tokenizer_free(h)
    tokenizers = pytest.importorskip("tokenizers")
    tok = tokenizers.Tokenizer.from_file(str(tmp_path / "tokenizer.json"))
    differs = [s for s in NEWER_MARKS if tok.encode(s, add_special_tokens=False).ids != ref.encode(s.encode())]
    print("newer marks the wheel keeps:", norm, [s.encode("unicode_escape") for s in differs])
    # BertNormalizer's strip goes by the wheel's older table of non-spacing marks: it keeps all three.  Its StripAccents goes by a
    # newer one, which still lacks U+07FD (Unicode 11)
    assert differs == (NEWER_MARKS if norm.startswith("bert") else NEWER_MARKS[1:2])


@pytest.mark.parametrize("norm", G.NORMS)
def test_normalizing_a_covered_line_is_concatenating_the_code_point_answers(generated, norm):
    """the property the device table rests on: on a line without a FLAG code point, the normalizer over the whole line equals the
    per-code-point outputs back to back"""
    n = G.NORMALIZERS[norm]
    ref = G.UnigramUtf8Ref(G.tokenizer_json(norm=norm), blocks=None)
    n_checked = 0
    for raw in NAMED + generated:
        s = raw.decode()
        if any(ord(ch) >= 0x80 and ref.cp_class(ord(ch))[0] == G.FLAG for ch in s):
            continue
        assert G.normalize(s, n) == "".join(G.normalize(ch, n) for ch in s), raw
        n_checked += 1
    assert n_checked > 900
    if G.has_nfd(n):      # ... and it fails where the table says FLAG: two characters of non-zero combining class that stay (musical
        s = "\U0001d16d\U0001d165"     # symbols of class 226 and 216, spacing marks): NFD swaps them, so the answer depends on the neighbour
        assert G.classify(0x1D16D, norm)[0] == G.classify(0x1D165, norm)[0] == G.FLAG
        assert G.normalize(s, n) != "".join(G.normalize(ch, n) for ch in s)


def test_the_reference_flags_at_most_one_generated_line_in_ten(generated):
    for norm in G.NORMS:
        for prepend in G.PREPEND:
            ref = G.UnigramUtf8Ref(G.tokenizer_json(norm=norm, prepend=prepend), blocks=None)
            flagged = sum(ref.line(raw)[1] for raw in generated)
            deliberate = sum(ref.line(raw)[1] for raw in DELIBERATE + NAMED)
            print(norm, prepend, "flagged of the generated", flagged, "of the deliberate and named", deliberate)
            assert flagged * 10 <= len(generated), (norm, prepend, flagged)
            assert deliberate >= len(DELIBERATE) + 4
    non_ascii = sum(any(c >= 0x80 for c in raw) for raw in generated)
    assert non_ascii > 700                                        # the cap is not met by generating ASCII


FLAG_COUNTS = {"none": 0, "lower": 0, "bert_clean": 81226, "bert_noclean": 81300, "seq": 36}


@pytest.mark.parametrize("norm", G.NORMS)
def test_the_flag_code_points_below_U30000_by_count_and_by_rule(norm):
    """Unicode 13 (this module's unicodedata and the host tokenizer's unicode_lower.h alike).  Without NFD in the chain nothing is
    FLAG.  With it: the 36 characters whose canonical decomposition holds a character of non-zero combining class that is not a
    non-spacing mark, which the strip therefore leaves in.  With handle_chinese_chars: every Chinese character that clean_text does
    not remove (74 unassigned code points of the compatibility block go first)."""
    n = G.NORMALIZERS[norm]
    flag = {cp for cp in range(0x80, 0x30000) if not 0xD800 <= cp <= 0xDFFF and G.classify(cp, norm)[0] == G.FLAG}
    assert len(flag) == FLAG_COUNTS[norm]
    kept = set()
    if G.has_nfd(n):
        kept = {cp for cp in range(0x80, 0x30000) if not 0xD800 <= cp <= 0xDFFF and unicodedata.category(chr(cp))[0] != "C"
                and any(unicodedata.combining(c) and unicodedata.category(c) != "Mn" for c in unicodedata.normalize("NFD", chr(cp)))}
        assert len(kept) == 36
    chinese = set()
    if norm.startswith("bert"):
        clean = n["clean_text"]
        chinese = {cp for a, b in W8.CJK for cp in range(a, min(b, 0x2FFFF) + 1)
                   if not (clean and unicodedata.category(chr(cp)).startswith("C"))}
    assert flag == kept | chinese
    # the replacement's own code point is a SPACE when the normalizer leaves it alone; what clean_text calls white space is one too
    assert G.classify(ord(G.R), norm) == (G.SPACE, "")
    assert (G.classify(0xA0, norm)[0] == G.SPACE) == (norm == "bert_clean") == (G.classify(0x3000, norm)[0] == G.SPACE)


def test_the_steps_around_the_tokenizer():
    ref = G.UnigramUtf8Ref(G.tokenizer_json(norm="seq"))
    V = {p: i for i, (p, _) in enumerate(G.build_vocab())}
    j, R = G.JAMO, G.R
    assert ref.encode(G.HANGUL.encode()) == [V[R], V[j["h"] + j["a"]], V[j["n"] + j["g"]], V[j["eu"]], V[j["l"]]]
    assert ref.line("the café".encode(), keep_bytes=9) == ([V[R + "the"], V[R + "cafe"]], False)
    assert ref.line("the café!".encode(), keep_bytes=9) == ([], True) and ref.line("the café".encode(), keep_bytes=7)[1] is False
    assert ref.line("the ก fox".encode()) == ([], True)         # U+0E01: in no block
    assert G.UnigramUtf8Ref(G.tokenizer_json(norm="seq"), blocks=None).line("the ก fox".encode(), drop_unk=False)[0] == [V[R + "the"], V[R], 0, V[R + "fox"]]
    assert ref.line(G.NAMED["exactly_max_word_multibyte"])[1] is False and ref.line(G.NAMED["max_word_plus_one"]) == ([], True)
    never = G.UnigramUtf8Ref(G.tokenizer_json(prepend="never"))
    assert never.line(G.NAMED["first_word_at_bound_never"])[1] is False and ref.line(G.NAMED["first_word_at_bound_never"])[1] is True
    for bad in G.MALFORMED.values():
        assert ref.line(bad) == ([], True) and ref.line(G.VALID_NEXT)[1] is False
    # pure-ASCII lines: the ASCII reference's answer
    plain = U.UnigramRef(G.tokenizer_json(norm="seq"))
    for raw in list(U.NAMED.values()) + U.ascii_lines(seed=3, n=100):
        if all(c < 0x80 for c in raw):
            assert ref.line(raw) == plain.line(raw), raw


def _form(path):
    """smt_host_tokenizer_to_device_unigram_utf8 without a context: SMT_E_UNSUPPORTED for a tokenizer without the form; one with it
    goes on to smt_unigram_create_utf8, which rejects the null context"""
    h = _load(path)
    out = C.c_void_p()
    try:
        rc = L.lib().smt_host_tokenizer_to_device_unigram_utf8(h, None, C.byref(out))
        assert not out and rc in (L.SMT_E_UNSUPPORTED, L.SMT_E_HIP, L.SMT_E_INVALID)
        if rc == L.SMT_E_UNSUPPORTED:
            assert b"UTF-8 Unigram device form" in L.lib().smt_last_error()
        return rc != L.SMT_E_UNSUPPORTED
    finally:
        L.lib().smt_host_tokenizer_free(h)


def test_which_tokenizers_have_a_utf8_unigram_device_form(tmp_path):
    for norm in G.NORMS:
        for prepend in G.PREPEND:
            assert _form(_write(tmp_path, G.tokenizer_json(norm=norm, prepend=prepend), "ok_%s_%s.json" % (norm, prepend)))
    assert _form(_write(tmp_path, G.tokenizer_json(unk_id=None), "no_unk.json"))
    assert _form(_write(tmp_path, G.tokenizer_json(replacement="·"), "other_replacement.json"))
    vocab = G.build_vocab() + [("<é>", 0.0)]
    assert not _form(_write(tmp_path, G.tokenizer_json(vocab=vocab, added=["<pad>", "<é>"]), "non_ascii_added.json"))
    strip = {"type": "Sequence", "normalizers": [{"type": "Strip", "strip_left": True, "strip_right": True}, {"type": "Lowercase"}]}
    assert not _form(_write(tmp_path, G.tokenizer_json(norm=strip), "strip.json"))
    assert not _form(_write(tmp_path, G.tokenizer_json(split=False), "no_split.json"))
    assert not _form(_write(tmp_path, G.tokenizer_json(replacement="_"), "ascii_replacement.json"))
    assert not _form(W.write_tokenizer(tmp_path / "wordpiece.json", 7))
    out = C.c_void_p()
    assert L.lib().smt_host_tokenizer_to_device_unigram_utf8(None, None, C.byref(out)) == L.SMT_E_INVALID
    h = _load(tmp_path / "no_unk.json")
    try:
        assert L.lib().smt_host_tokenizer_to_device_unigram_utf8(h, None, None) == L.SMT_E_INVALID
    finally:
        L.lib().smt_host_tokenizer_free(h)


@pytest.mark.skipif(L.lib().smt_device_count() > 0, reason="a GPU is present")
def test_without_a_device_the_new_entry_points_fail_loudly(tmp_path):
    lib = L.lib()
    out = C.c_void_p()
    h = _load(_write(tmp_path, G.tokenizer_json()))
    try:
        assert lib.smt_host_tokenizer_to_device_unigram_utf8(h, None, C.byref(out)) == L.SMT_E_HIP and not out
    finally:
        lib.smt_host_tokenizer_free(h)
    prm, cps = L.SmtUnigramParams(), L.SmtWordpieceCodepoints()
    assert lib.smt_unigram_create_utf8(None, C.byref(prm), C.byref(cps), C.byref(out)) == L.SMT_E_HIP and not out
    assert b"no HIP device" in lib.smt_last_error()
    assert lib.smt_unigram_info(None, None, None, None) == L.SMT_E_HIP
