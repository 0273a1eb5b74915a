"""CPU: tests/unigram_long_rules_ref.py -- the reference of the long pieces under the space rules (smt_unigram_set_long_rules) --
against the host tokenizer (hf_tokenizer.cpp) and, where it imports, the `tokenizers` wheel: every named line and 1000 generated
lines per shape of tokenizer.json.  Where the device view of the reference covers a line (limit 2048, the look-back bound, the
drop_trailing cases) its ids are the whole chain's.  Four reference variants that are wrong on purpose fail on the named lines.  The
generator is held to its conditions: at most a tenth of its lines flagged by the reference, at least a fifth with a piece over 64
raw bytes.  The new export refuses a null handle and bad values without a device."""
import ctypes as C
import json

import numpy as np
import pytest

from semtools_amd import _lib as L
from tests import precompiled_ref as P
from tests import unigram_long_rules_ref as Q

NAMED = {**Q.NAMED, **Q.NAMED_UTF8, **{"p_" + k: v for k, v in P.NAMED.items()}}
N_GEN = 1000
V = {p: i for i, (p, _) in enumerate(Q.build_vocab())}
V[Q.R] = max(i for i, (p, _) in enumerate(Q.build_vocab()) if p == Q.R)
V["the"] = max(i for i, (p, _) in enumerate(Q.build_vocab()) if p == "the")


@pytest.fixture(scope="module")
def generated():
    pytest.importorskip("regex")
    return Q.lines(seed=7, n=N_GEN)


def _load(tmp_path, tj):
    path = tmp_path / "tokenizer.json"
    path.write_text(json.dumps(tj))
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


def _decodes(raw):
    try:
        raw.decode()
        return True
    except UnicodeDecodeError:
        return False


@pytest.mark.parametrize("shape", P.SHAPES)
def test_reference_equals_the_host_tokenizer(tmp_path, generated, shape):
    tj = Q.tokenizer_json(shape)
    ref = Q.LongRulesRef(tj)
    h = _load(tmp_path, tj)
    try:
        n_covered = n_long = 0
        for raw in [x for x in NAMED.values() if _decodes(x)] + generated:
            want = ref.encode_host(raw)
            assert _encode(h, raw) == want, (shape, raw[:80])
            for dev in (ref.encode(raw), ref.encode(raw, check_limit=False)):   # the device view, where it covers the line
                if dev is not None:
                    assert dev == want, (shape, raw[:80])
            n_covered += ref.encode(raw) is not None
            n_long += bool(ref.long_pieces(raw))
        assert n_covered > 900 and n_long > 250
    finally:
        L.lib().smt_host_tokenizer_free(h)


@pytest.mark.parametrize("shape", P.SHAPES)
def test_reference_equals_the_tokenizers_wheel(tmp_path, generated, shape):
    """equal ids but for EMPTY (tests/test_precompiled_ref_cpu.py): of a line whose normalised text is empty the host tokenizer makes the
    prepended replacement alone, the wheel nothing"""
    tokenizers = pytest.importorskip("tokenizers")
    tj = Q.tokenizer_json(shape)
    ref = Q.LongRulesRef(tj)
    path = tmp_path / "tokenizer.json"
    path.write_text(json.dumps(tj))
    tok = tokenizers.Tokenizer.from_file(str(path))
    for raw in [x for x in NAMED.values() if _decodes(x)] + generated:
        want = ref.encode_host(raw)
        got = tok.encode(raw.decode(), add_special_tokens=False).ids
        if got != want:
            assert raw and P.normalize(raw.decode(), ref.norm) == "" and got == [] and want == [V[Q.R]], (shape, raw[:80], got[:8], want[:8])


def test_what_the_reference_says_by_rule():
    pytest.importorskip("regex")
    ws, keeps = Q.LongRulesRef(Q.tokenizer_json("A_ws")), Q.LongRulesRef(Q.tokenizer_json("A"))
    split = Q.LongRulesRef(Q.tokenizer_json("A_ws"), collapse_runs=0, drop_trailing=1)
    old = P.PrecompiledRef(Q.tokenizer_json("A_ws"))
    the, fox, r = V[Q.R + "the"], V[Q.R + "fox"], V[Q.R]
    for k in Q.covered_only():                                                   # the old limit flags them, the new one does not
        assert old.line(Q.NAMED[k])[1] is True and ws.line(Q.NAMED[k])[1] is False and keeps.line(Q.NAMED[k])[1] is False, k
    for name, raw in NAMED.items():
        if name.startswith("flag_"):
            for ref in (ws, keeps, split):
                assert ref.line(raw) == ([], True), name
    # the measure: the owner's space one, absorbed spaces their raw bytes
    assert ws.measures(Q.NAMED["run_62_abc"]) == [4, 65, 4] and ws.measures(Q.NAMED["run_70_abc"]) == [4, 73, 4]
    assert split.measures(Q.NAMED["run_70_abc"]) == [4] + [1] * 69 + [4, 4]
    assert ws.measures(Q.NAMED["exactly_2048_through_absorbed"])[1] == 2048 and ws.line(Q.NAMED["exactly_2048_through_absorbed"])[1] is False
    assert ws.measures(Q.NAMED["over_2048_through_absorbed_only"])[1] == 2049 and ws.line(Q.NAMED["over_2048_through_absorbed_only"])[1] is True
    assert split.line(Q.NAMED["over_2048_through_absorbed_only"])[1] is False    # 1000 lone replacements and a piece of 1049
    assert ws.line(Q.NAMED["over_2048_absorbed_alone"])[1] is True
    assert ws.measures(Q.NAMED_UTF8["ideographic_22"])[1] == 1 + 21 * 3 + 12          # a SPACE character of three bytes counted as one
    # what the lines become
    assert ws.line(Q.NAMED["run_70_abc"])[0] == [the, V[Q.R + "abc"], fox] and split.line(Q.NAMED["run_70_abc"])[0] == [the] + [r] * 69 + [V[Q.R + "abc"], fox]
    assert ws.line(Q.NAMED["trailing_70"]) == ([the, fox], False) and keeps.line(Q.NAMED["trailing_70"]) == ([the, fox, r], False)
    assert ws.line(Q.NAMED["spaces_70"]) == ([], True) and keeps.line(Q.NAMED["spaces_70"]) == ([r], False)
    assert split.line(Q.NAMED["spaces_70"]) == ([r] * 69, False)
    assert ws.line(Q.NAMED["dropped_70"]) == ([], True) and keeps.line(Q.NAMED["dropped_70"]) == ([r], False)
    assert ws.line(Q.NAMED["tie_xy_40"])[0] == [the, r] + [V["xy"]] * 40         # the tie at every step: the smallest start wins
    assert ws.line(Q.NAMED["viterbi_abcd_20"])[0][:3] == [the, V[Q.R + "ab"], V["cd"]]
    assert ws.line(Q.NAMED["piece_70_twice"])[0].count(V[Q.LR.LONG_VOCAB_PIECE]) == 2
    # the look-back bound, and the witness
    assert ws.line(Q.NAMED["dropped_64_space"])[1] is False and ws.line(Q.NAMED["flag_dropped_70_space"])[1] is True
    assert ws.line(Q.NAMED["dropped_70_no_space_behind"])[1] is False
    assert ws.stats([Q.NAMED["trailing_70"], Q.NAMED["spaces_70"], Q.NAMED["flag_dropped_70_space"], b"the fox"]) == (3, 70 + 70 + 75)
    assert ws.long_pieces(Q.NAMED["flag_2049_middle"]) == [] and ws.long_pieces(Q.NAMED_UTF8["flag_mark_inside"]) is None
    ascii_form = Q.LongRulesRef(Q.tokenizer_json("A_ws"), utf8=False)
    assert ascii_form.line(Q.NAMED_UTF8["cjk_600"])[1] is True and ws.line(Q.NAMED_UTF8["cjk_600"])[1] is False
    assert ascii_form.line(Q.NAMED["url"]) == ws.line(Q.NAMED["url"])


@pytest.mark.parametrize("wrong", Q.WRONG)
def test_a_reference_that_is_wrong_on_purpose_fails_on_the_named_lines(tmp_path, wrong):
    pytest.importorskip("regex")
    failed = {}
    for shape in P.SHAPES:
        tj = Q.tokenizer_json(shape)
        good, bad = Q.LongRulesRef(tj), Q.LongRulesRef(tj, wrong=wrong)
        h = _load(tmp_path, tj)
        try:
            for name, raw in NAMED.items():
                if not _decodes(raw):
                    continue
                host = _encode(h, raw)
                assert good.line(raw, drop_unk=False) in ((host, False), ([], True)), (shape, name)
                if bad.line(raw, drop_unk=False) not in ((host, False), ([], True)) or bad.line(raw)[1] != good.line(raw)[1]:
                    failed.setdefault(shape, []).append(name)
        finally:
            L.lib().smt_host_tokenizer_free(h)
    print(wrong, {s: len(v) for s, v in failed.items()})
    assert failed.get("A_ws") and (wrong == "trailing_r_emitted" or failed.get("A")), failed


def test_the_generator_meets_its_conditions(generated):
    for shape in P.SHAPES:
        ref = Q.LongRulesRef(Q.tokenizer_json(shape))
        flagged = sum(ref.line(raw)[1] for raw in generated)
        over = sum(max(ref.measures(raw) or [0]) > Q.MAX_WORD for raw in generated)
        print(shape, "flagged", flagged, "with a piece over 64 raw bytes", over, "of", len(generated))
        assert flagged * 10 <= len(generated), (shape, flagged)
        assert over * 5 >= len(generated), (shape, over)
    assert sum(any(c >= 0x80 for c in raw) for raw in generated) > 600


def test_the_new_entry_point_refuses_a_null_handle_and_bad_values():
    """a null handle: SMT_E_HIP on a machine without a device, SMT_E_INVALID otherwise -- what the other setters of the handle answer;
    the values are checked on a live handle by tests/test_gpu_unigram_long_rules.py"""
    lib = L.lib()
    want = (L.SMT_E_INVALID,) if lib.smt_device_count() > 0 else (L.SMT_E_HIP,)
    for on in (0, 1, 2, -1):
        assert lib.smt_unigram_set_long_rules(None, on) in want
    assert lib.smt_unigram_set_long_rules(None, 1) == lib.smt_unigram_set_space_rules(None, 1, 1) == lib.smt_unigram_set_long_pieces(None, L.UG_MAX_LONG)
    assert lib.smt_unigram_set_long_rules(None, 0) in want and b"smt_unigram_set_long_rules" in lib.smt_last_error()
