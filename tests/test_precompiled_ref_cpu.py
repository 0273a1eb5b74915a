"""CPU: XLM-R-style tokenizers -- a `Precompiled` sentencepiece normalizer and a regex `Replace` in front of Metaspace and Unigram --
through the host tokenizer (hf_tokenizer.cpp, precompiled.h), against tests/precompiled_ref.py and, where it imports, the `tokenizers`
wheel: the three shapes of tokenizer.json in circulation, the named lines and 1000 generated mixed-script lines per shape.  Also: the
malformed character maps, the regex forms that stay refused, which tokenizers get which device form with which space rules, that the
device view of the reference agrees with the whole chain on every line it covers, the cap on what it flags, and the new entry point
without a device.

The `tokenizers` wheel is the yardstick for the chain (sentencepiece itself differs on the sample line).  The one difference between
the host tokenizer and the wheel that shows here is the EMPTY one of DESIGN 4.9, asserted by rule; `first` and StripAccents cannot
show (the scheme is `always`, the chain has no StripAccents)."""
import ctypes as C
import json
import struct

import numpy as np
import pytest

from semtools_amd import _lib as L
from tests import precompiled_ref as P
from tests import unigram_utf8_ref as G

NAMED = list(P.NAMED.values())
N_GEN = 1000
V_R = max(i for i, (p, _) in enumerate(P.build_vocab()) if p == P.R)


@pytest.fixture(scope="module")
def generated():
    pytest.importorskip("regex")
    return P.lines(seed=7, n=N_GEN)


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


def test_a_shape_A_tokenizer_json_opens_and_tokenizes_the_sample_line(tmp_path):
    """(fails before the Precompiled reader: "normalizer type 'Precompiled' is not supported")"""
    h = _load(_write(tmp_path, P.tokenizer_json("A_ws")))
    try:
        V = {p: i for i, (p, _) in enumerate(P.build_vocab())}
        ids = _encode(h, P.SAMPLE.encode())
        assert ids[0] == V[P.R + "fine"]                                       # the ligature spelled out, the two spaces one
        assert V[P.R + "full"] in ids and V["XII"] in ids and V[P.R + "No"] in ids and V[P.R + "한글"] in ids
        assert _encode(h, b"a  b") == [V[P.R + "a"], V[P.R], V["b"]]          # R+a | R, b: one replacement for the two spaces
    finally:
        L.lib().smt_host_tokenizer_free(h)


def test_the_character_map_normalises_the_sample_line():
    pytest.importorskip("regex")
    assert len(P.blob()) == 240007 and struct.unpack_from("<I", P.blob())[0] == 179200
    n = P.normalizer_json("A")
    assert P.normalize(P.SAMPLE, n) == "fine Straße full x2 カ\u3099 é XII No5 한글"   # (a 6-byte cluster: its two characters one by one, not composed)


@pytest.mark.parametrize("shape", P.SHAPES)
def test_reference_equals_the_host_tokenizer(tmp_path, generated, shape):
    tj = P.tokenizer_json(shape)
    ref = P.PrecompiledRef(tj)
    h = _load(_write(tmp_path, tj))
    try:
        n_covered = n_non_ascii = 0
        for raw in NAMED + generated:
            want = ref.encode_host(raw)
            assert _encode(h, raw) == want, (shape, raw)
            n_non_ascii += any(c >= 0x80 for c in raw)
            # the device view -- the per-character table and the space rules -- where it covers the line
            dev = ref.encode(raw, check_limit=False)
            if dev is not None:
                assert dev == want, (shape, raw)
                n_covered += 1
        assert n_covered > 850 and n_non_ascii > 600
    finally:
        L.lib().smt_host_tokenizer_free(h)


@pytest.mark.parametrize("shape", P.SHAPES)
def test_reference_equals_the_tokenizers_wheel(tmp_path, generated, shape):
    """Equal ids but for EMPTY: of a line whose normalised text is empty the host tokenizer makes the prepended replacement alone, the
    wheel nothing.  It shows under shape B only (Strip leaves nothing of a line of spaces; behind WhitespaceSplit there is no word to
    prepend to, and without either the spaces stay)."""
    tokenizers = pytest.importorskip("tokenizers")
    tj = P.tokenizer_json(shape)
    ref = P.PrecompiledRef(tj)
    tok = tokenizers.Tokenizer.from_file(str(_write(tmp_path, tj)))
    n_empty = 0
    for raw in NAMED + generated:
        want = ref.encode_host(raw)
        s = raw.decode()
        got = tok.encode(s, add_special_tokens=False).ids
        if got == want:
            continue
        assert raw and P.normalize(s, ref.norm) == "" and got == [] and want == [V_R], (shape, raw, got, want)
        n_empty += 1
    assert (n_empty > 0) == (shape == "B")
    assert tok.normalizer.normalize_str(P.SAMPLE) == P.normalize(P.SAMPLE, ref.norm)


def _tiny_trie(value):
    """a 256-unit trie with the one key "a": the root's offset 128 leads to unit 225 (label 'a', has a leaf, offset 1), the leaf unit
    224 holds `value`; the pool is "x" NUL"""
    units = [0] * 256
    units[0] = 128 << 10
    units[128 ^ 97] = 97 | (1 << 8) | (1 << 10)
    units[128 ^ 97 ^ 1] = value
    return struct.pack("<I", 1024) + struct.pack("<256I", *units) + b"x\0"


MALFORMED = {
    "fewer_than_4_bytes": b"\x01\x02",
    "trie_size_no_multiple_of_4": struct.pack("<I", 6) + b"\0" * 16,
    "trie_size_past_the_end": struct.pack("<I", 1 << 20) + b"\0" * 16,
    "node_outside_the_trie": struct.pack("<I", 4) + struct.pack("<I", 1000 << 10) + b"x\0",
    "value_outside_the_pool": _tiny_trie(999),
    "pool_string_without_its_nul": P.blob()[:-1],
}


def test_the_tiny_trie_of_the_malformed_cases_is_well_formed_with_a_value_inside_the_pool(tmp_path):
    pytest.importorskip("regex")
    good = _tiny_trie(0)
    assert P.Charsmap(good).lookup(b"a") == "x" and P.Charsmap(good).lookup(b"b") is None
    h = _load(_write(tmp_path, P.tokenizer_json("A", data=good)))
    try:
        ref = P.PrecompiledRef(P.tokenizer_json("A", data=good))
        assert _encode(h, b"a b xa") == ref.encode_host(b"a b xa") == ref.encode_host(b"x b xx")
    finally:
        L.lib().smt_host_tokenizer_free(h)


@pytest.mark.parametrize("kind", sorted(MALFORMED))
def test_a_malformed_character_map_is_an_error(tmp_path, kind):
    """at load, or at the lookup that meets the bad node or value: never a read outside the blob"""
    data = MALFORMED[kind]
    with pytest.raises(P.Malformed):
        P.Charsmap(data).lookup(b"a")
    path = _write(tmp_path, P.tokenizer_json("A", data=data))
    h = C.c_void_p()
    rc = L.lib().smt_host_tokenizer_load(str(path).encode(), C.byref(h))
    if rc != L.SMT_OK:
        assert b"Precompiled normalizer" in L.lib().smt_last_error() and not h
        return
    try:
        assert kind in ("node_outside_the_trie", "value_outside_the_pool")
        assert _encode(h, b"the a fox") is None and b"Precompiled normalizer" in L.lib().smt_last_error()
    finally:
        L.lib().smt_host_tokenizer_free(h)


def test_base64_that_is_none_is_an_error(tmp_path):
    tj = P.tokenizer_json("A")
    tj["normalizer"]["normalizers"][0]["precompiled_charsmap"] = "!!!not base64!!!"
    h = C.c_void_p()
    assert L.lib().smt_host_tokenizer_load(str(_write(tmp_path, tj)).encode(), C.byref(h)) != L.SMT_OK and not h


@pytest.mark.parametrize("pattern", [" *", "\\s+", "[ ]{2,}", " {2,3}", " {,2}", "ab+", " {2,}x", "", ".+", " {x,}"])
def test_other_regex_patterns_keep_the_error_with_the_pattern_named(tmp_path, pattern):
    norm = {"type": "Replace", "pattern": {"Regex": pattern}, "content": " "}
    h = C.c_void_p()
    rc = L.lib().smt_host_tokenizer_load(str(_write(tmp_path, G.tokenizer_json(norm=norm))).encode(), C.byref(h))
    err = L.lib().smt_last_error()
    assert rc != L.SMT_OK and not h and b"Regex pattern '" + pattern.encode() + b"' is not supported" in err


@pytest.mark.parametrize("pattern, text, want", [("x+", "axxb x", "a-b -"), ("b{3,}", "abbb bb bbbb", "a- bb -"), ("é{1,}", "éé é", "- -")])
def test_the_regex_forms_read_replace_whole_runs(tmp_path, pattern, text, want):
    norm = {"type": "Replace", "pattern": {"Regex": pattern}, "content": "-"}
    assert P.normalize(text, norm) == want
    plain = G.tokenizer_json(norm=None)
    h, g = _load(_write(tmp_path, G.tokenizer_json(norm=norm))), _load(_write(tmp_path, plain, "plain.json"))
    try:
        assert _encode(h, text.encode()) == _encode(g, want.encode())
    finally:
        L.lib().smt_host_tokenizer_free(h)
        L.lib().smt_host_tokenizer_free(g)


def _forms(path):
    """(the rules of the ASCII form or None, whether there is a UTF-8 form) without a device"""
    h = _load(path)
    a, b, out = C.c_int(-1), C.c_int(-1), C.c_void_p()
    try:
        rc = L.lib().smt_host_tokenizer_unigram_space_rules(h, C.byref(a), C.byref(b))
        assert rc in (L.SMT_OK, L.SMT_E_UNSUPPORTED)
        rc8 = L.lib().smt_host_tokenizer_to_device_unigram_utf8(h, None, C.byref(out))
        assert not out and rc8 in (L.SMT_E_UNSUPPORTED, L.SMT_E_HIP, L.SMT_E_INVALID)
        return ((a.value, b.value) if rc == L.SMT_OK else None), rc8 != L.SMT_E_UNSUPPORTED
    finally:
        L.lib().smt_host_tokenizer_free(h)


def test_which_tokenizers_have_a_device_form_and_with_which_space_rules(tmp_path):
    def seq(*parts):
        return {"type": "Sequence", "normalizers": list(parts)}

    pre, strip = P.precompiled_json(), {"type": "Strip", "strip_left": False, "strip_right": True}
    space = {"type": "Replace", "pattern": {"Regex": " {2,}"}, "content": " "}
    rep = dict(space, content=P.R)
    for shape in P.SHAPES:
        assert _forms(_write(tmp_path, P.tokenizer_json(shape), shape + ".json")) == (P.RULES[shape], True), shape
    assert P.RULES == {"A_ws": (1, 1), "A": (1, 0), "B": (1, 1)}
    cases = {
        "precompiled_alone": (P.tokenizer_json("A", norm=seq(pre)), (0, 0)),
        "precompiled_not_in_a_sequence": (P.tokenizer_json("A", norm=pre), (0, 0)),
        "whitespace_split_alone": (P.tokenizer_json("A_ws", norm=seq(pre)), (1, 1)),
        "lowercase_then_replace": (P.tokenizer_json("A", norm=seq({"type": "Lowercase"}, space)), (1, 0)),
        "replace_by_the_replacement": (P.tokenizer_json("A", norm=seq(pre, rep)), (1, 0)),
        "no_normalizer": (G.tokenizer_json(norm=None), (0, 0)),
        "bert": (G.tokenizer_json(norm="bert_clean", prepend="first"), (0, 0)),
        # what the rules do not state keeps the host path
        "strip_without_a_collapse": (P.tokenizer_json("A", norm=seq(pre, strip)), None),
        "strip_left": (P.tokenizer_json("A", norm=seq(pre, dict(strip, strip_left=True), space)), None),
        "replace_in_front": (P.tokenizer_json("A", norm=seq(space, pre)), None),
        "three_or_more": (P.tokenizer_json("A", norm=seq(pre, dict(space, pattern={"Regex": " {3,}"}))), None),
        "another_character": (P.tokenizer_json("A", norm=seq(pre, dict(space, pattern={"Regex": "a{2,}"}))), None),
        "another_content": (P.tokenizer_json("A", norm=seq(pre, dict(space, content="_"))), None),
        "string_replace": (P.tokenizer_json("A", norm=seq(pre, {"type": "Replace", "pattern": {"String": "  "}, "content": " "})), None),
    }
    for scheme in ("first", "never"):
        tj = P.tokenizer_json("A")
        tj["pre_tokenizer"]["prepend_scheme"] = scheme
        cases["rules_under_" + scheme] = (tj, None)
    tj = P.tokenizer_json("A_ws")
    tj["pre_tokenizer"]["pretokenizers"].reverse()
    cases["whitespace_split_behind_metaspace"] = (tj, None)
    for name, (tj, want) in cases.items():
        assert _forms(_write(tmp_path, tj, name + ".json")) == (want, want is not None), name
    out = C.c_int()
    assert L.lib().smt_host_tokenizer_unigram_space_rules(None, C.byref(out), None) == L.SMT_E_INVALID


def test_the_reference_flags_at_most_one_generated_line_in_ten(generated):
    for shape in P.SHAPES:
        ref = P.PrecompiledRef(P.tokenizer_json(shape))
        flagged = sum(ref.line(raw)[1] for raw in generated)
        named = sum(ref.line(raw)[1] for raw in NAMED)
        print(shape, "flagged of the generated", flagged, "of the named", named)
        assert flagged * 10 <= len(generated), (shape, flagged)
        assert named >= 8                     # the clusters, the characters that outgrow their bytes, the runs of 70 spaces
    assert sum(any(c >= 0x80 for c in raw) for raw in generated) > 600          # the cap is not met by generating ASCII
    assert sum(b"  " in raw for raw in generated) > 200                         # ... nor by leaving the runs out


def test_what_the_device_view_flags_by_rule():
    ref = P.PrecompiledRef(P.tokenizer_json("A_ws"))
    for name in ("eacute_decomposed", "zwj_emoji", "regional_pair", "hangul_decomposed", "half", "kabushiki", "run_70_start", "run_70_middle",
                 "run_70_end", "spaces_only", "one_space"):
        assert ref.line(P.NAMED[name]) == ([], True), name
    for name in ("hangul_precomposed", "nbsp_by_space", "ideographic_by_space", "zwsp_between_spaces", "dropped_between_spaces", "fullwidth",
                 "run_3_start", "run_3_middle", "run_3_end", "empty"):
        assert ref.line(P.NAMED[name])[1] is False, name
    assert ref.line(b"the\r\nfox")[1] is True and ref.line(b"the\rfox")[1] is False
    assert ref.line(("a" + P.R + "b").encode())[1] is True                       # a literal replacement under a rule
    keeps = P.PrecompiledRef(P.tokenizer_json("A"))                              # shape A keeps the trailing replacement, and a line of spaces
    V = {p: i for i, (p, _) in enumerate(P.build_vocab())}
    assert keeps.line(b"the   ") == ([V[P.R + "the"], V_R], False) and ref.line(b"the   ") == ([V[P.R + "the"]], False)
    assert keeps.line(b"    ") == ([V_R], False) == (keeps.encode_host(b"    "), False)
    # the measure: absorbed spaces count like dropped bytes
    assert ref.line(b"the" + b" " * 61 + b"abc")[1] is False and ref.line(b"the" + b" " * 62 + b"abc")[1] is True
    ascii_form = P.PrecompiledRef(P.tokenizer_json("A_ws"), utf8=False)
    assert ascii_form.line("the café".encode())[1] is True and ascii_form.line(b"the  fox") == ref.line(b"the  fox")


def test_the_new_entry_point_refuses_a_null_handle_loudly():
    """SMT_E_HIP on a machine without a device, SMT_E_INVALID otherwise: what the other setters of the handle answer"""
    lib = L.lib()
    want = (L.SMT_E_INVALID,) if lib.smt_device_count() > 0 else (L.SMT_E_HIP,)
    assert lib.smt_unigram_set_space_rules(None, 1, 1) in want
    assert lib.smt_unigram_set_space_rules(None, 1, 1) == lib.smt_unigram_set_long_pieces(None, L.UG_MAX_LONG)
