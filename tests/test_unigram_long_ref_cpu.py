"""CPU: the references of the long pieces (tests/unigram_long_ref.py) before the GPU tests lean on them.  The windowed lattice equals
the existing references' quadratic one; on every named and generated long line the long references equal the host tokenizer; the
inputs stand on new ground (the long references flag none of them but the ones meant to flag, the existing references -- limit 64 --
flag every one); and three subtly wrong lattices are caught by the cases."""
import ctypes as C
import json
import random

import pytest

from semtools_amd import _lib as L
from tests import unigram_long_ref as LR
from tests import unigram_ref as U
from tests import unigram_utf8_ref as G

ASCII_CONFIGS = [(n, p, 0) for n in ("none", "lower", "bert_clean", "bert_noclean") for p in U.PREPEND] + [("none", "always", None), ("seq", "first", None)]
UTF8_CONFIGS = [(n, p, 0) for n in G.NORMS for p in G.PREPEND] + [("none", "always", None), ("seq", "first", None)]
N_GEN = 120


def _ids(c):
    return "-".join(map(str, c))


def _refs(form, norm, prepend, unk, vocab=None):
    """(tokenizer.json, the long reference, the existing reference) of one configuration"""
    if form == "ascii":
        tj = U.tokenizer_json(norm=norm, prepend=prepend, unk_id=unk, vocab=vocab)
        return tj, LR.UnigramLongRef(tj), U.UnigramRef(tj)
    tj = G.tokenizer_json(norm=norm, prepend=prepend, unk_id=unk, vocab=vocab)
    return tj, LR.UnigramLongUtf8Ref(tj, blocks=None), G.UnigramUtf8Ref(tj, blocks=None)


def _named(form):
    return dict(LR.NAMED) if form == "ascii" else {**LR.NAMED, **LR.NAMED_UTF8}


def _generated(form, unk):
    return LR.long_lines(seed=11, n=N_GEN, utf8=form == "utf8", known_only=unk is None)


CASES = [("ascii",) + c for c in ASCII_CONFIGS] + [("utf8",) + c for c in UTF8_CONFIGS]


def test_the_windowed_lattice_equals_the_quadratic_one():
    rng = random.Random(3)
    for form, vocab in (("ascii", U.build_vocab()), ("utf8", G.build_vocab()), ("ascii", LR.long_vocab())):
        tj, long_ref, old_ref = _refs(form, "none", "always", 0, vocab=vocab)
        alphabet = sorted({ch for p, _ in vocab for ch in p if ch != U.R and p not in ("<unk>", "<pad>")}) + list("zq7")
        words = [p.replace(U.R, "") for p, _ in vocab if p not in ("<unk>", "<pad>", U.R)]
        for k in range(150):
            n = rng.choice([1, 2, 3, 63, 64, 65, 130, 200]) if k < 40 else rng.randint(1, 200)
            chars = []
            while len(chars) < n:
                chars.extend(rng.choice(words) if rng.random() < 0.6 else rng.choice(alphabet))
            chars = ([U.R] if rng.random() < 0.7 else []) + chars[:n]
            want, got = [], []
            old_ref.piece(chars, want)
            long_ref.piece(chars, got)
            assert got == want, (form, "".join(chars))


def _load(tmp_path, tj):
    p = tmp_path / "tokenizer.json"
    p.write_text(json.dumps(tj))
    h = C.c_void_p()
    L.check(L.lib().smt_host_tokenizer_load(str(p).encode(), C.byref(h)))
    return h


def _encode(h, raw):
    cap = len(raw) + 16
    ids = (C.c_uint32 * cap)()
    n = C.c_uint64()
    if L.lib().smt_host_tokenizer_encode(h, raw, ids, cap, C.byref(n)) != L.SMT_OK:
        return None
    return list(ids[: n.value])


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_the_long_reference_equals_the_host_tokenizer(tmp_path, case):
    form, norm, prepend, unk = case
    tj, ref, _ = _refs(form, norm, prepend, unk)
    h = _load(tmp_path, tj)
    try:
        cuts = [x[:k] for x, k in LR.CUTS] + ([x[:k] for x, k in LR.CUTS_UTF8 if len(x) <= k] if form == "utf8" else [])
        n = 0
        for raw in list(_named(form).values()) + _generated(form, unk) + cuts:
            want = ref.encode(raw, check_limit=False)      # (the limit flags a line for the device only: the host has none)
            if want is None:
                continue
            assert _encode(h, raw) == want, (case, raw[:80])
            n += 1
        assert n >= N_GEN
    finally:
        L.lib().smt_host_tokenizer_free(h)
    tj, ref, _ = _refs(form, norm, prepend, unk, vocab=LR.long_vocab() if form == "ascii" else G.build_vocab() + [(LR.LONG_VOCAB_PIECE, -5.0)])
    h = _load(tmp_path, tj)
    try:
        for raw in LR.NAMED_LONG_VOCAB.values():
            want = ref.encode_long(raw)
            assert want is not None and _encode(h, raw) == want, (case, raw[:80])
    finally:
        L.lib().smt_host_tokenizer_free(h)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_every_input_stands_on_new_ground(case):
    """the long reference flags no generated line and no named one that is not meant to flag; the existing reference flags them all"""
    form, norm, prepend, unk = case
    _, ref, old = _refs(form, norm, prepend, unk)
    for raw in _generated(form, unk):
        assert not ref.line(raw)[1] and old.line(raw)[1], (case, raw[:80])
        assert ref.long_pieces(raw)
    bert = norm.startswith("bert")
    for name, raw in _named(form).items():
        assert old.line(raw)[1], (case, name)
        flagged = ref.line(raw)[1]
        if name.startswith("flag_"):
            assert flagged, (case, name)
        elif name.startswith("blocks_"):
            assert flagged == (unk is None) and LR.UnigramLongUtf8Ref(_refs(form, norm, prepend, unk)[0]).line(raw)[1], (case, name)   # U+0E01: in no range of BLOCKS
        elif unk is None and "unk" in name:
            continue                                       # (an unknown character without an unk id: flagged under some normalizers)
        elif name.startswith("cjk"):
            assert flagged == bert, (case, name)           # a Chinese character between two spaces: FLAG
        elif unk is None and name in ("upper", "tab_inside"):
            continue                                       # (capitals and the tab are pieces only while the normalizer leaves them)
        else:
            assert not flagged, (case, name)
    _, ref, old = _refs(form, norm, prepend, unk, vocab=LR.long_vocab() if form == "ascii" else G.build_vocab() + [(LR.LONG_VOCAB_PIECE, -5.0)])
    for name, raw in LR.NAMED_LONG_VOCAB.items():
        assert not ref.line(raw)[1] and old.line(raw)[1], (case, name)
    for raw, keep in LR.CUTS + (LR.CUTS_UTF8 if form == "utf8" else []):
        assert old.line(raw, keep_bytes=keep)[1], (case, raw[:20], keep)


def test_the_named_measures_are_what_their_names_say():
    _, ref, _ = _refs("ascii", "none", "always", 0)
    _, never, _ = _refs("ascii", "none", "never", 0)
    for m in (64, 65, 66):
        assert ref.measures(LR.NAMED["measure_%d_first" % m])[0] == m and never.measures(LR.NAMED["measure_%d_first_no_r" % m])[0] == m
        assert ref.measures(LR.NAMED["measure_%d_middle" % m])[1] == m and ref.measures(LR.NAMED["measure_%d_last" % m])[-1] == m
    assert max(ref.measures(LR.NAMED["exactly_2048_middle"])) == 2048 and max(ref.measures(LR.NAMED["flag_2049_middle"])) == 2049
    assert max(ref.measures(LR.NAMED["exactly_2048_first"])) == 2048 and max(never.measures(LR.NAMED["exactly_2048_first"])) == 2047
    for at in (64, 128, 256, 320):
        raw = LR.NAMED["across_%d" % at]
        a = raw.index(b"abcd")
        assert a < at < a + 80 and raw[a - 1:a] == b" "
    raw = LR.NAMED_LONG_VOCAB["piece_70_across_64"]
    a = raw.index(LR.LONG_VOCAB_PIECE.encode()) - 4
    assert a < 64 < a + 70
    _, clean, _ = _refs("utf8", "bert_clean", "always", 0)
    assert clean.measures(LR.NAMED_UTF8["unk_ideographic_space_measure_64"])[1:3] == [64, 65]
    assert clean.stats([LR.NAMED["measure_64_middle"], LR.NAMED["measure_65_middle"]]) == (3, 91 + 65 + 91)


WRONG = {"ties won by the largest start": dict(tie_largest=True), "starts one byte short of the longest piece": dict(window_short=1),
         "unknowns that do not fuse across a 64-position border": dict(fuse_break=64)}


@pytest.mark.parametrize("what", list(WRONG), ids=lambda w: w.replace(" ", "_"))
def test_a_wrong_lattice_fails_the_cases(what):
    """each of the three wrong lattices gives other ids than the right one on a named line AND on a generated one"""
    for form, vocab, named in (("ascii", None, LR.NAMED), ("ascii", LR.long_vocab(), LR.NAMED_LONG_VOCAB)):
        _, ref, _ = _refs(form, "none", "always", 0, vocab=vocab)
        _, bad, _ = _refs(form, "none", "always", 0, vocab=vocab)
        bad.wrong = WRONG[what]
        caught = [k for k, raw in named.items() if not ref.line(raw, drop_unk=False)[1] and bad.line(raw, drop_unk=False) != ref.line(raw, drop_unk=False)]
        if vocab is None:
            want = {"ties won by the largest start": "tie_xy_40", "starts one byte short of the longest piece": None,
                    "unknowns that do not fuse across a 64-position border": "unk_run_130"}[what]
            if want:
                assert want in caught, (what, caught)
            gen = LR.long_lines(seed=11, n=N_GEN)
            if what != "starts one byte short of the longest piece":
                assert any(bad.line(raw, drop_unk=False) != ref.line(raw, drop_unk=False) for raw in gen), what
        elif what == "starts one byte short of the longest piece":
            assert "piece_70_across_64" in caught, (what, caught)      # (the longest piece of that vocabulary is the 70-byte one)


def test_the_new_entry_points_refuse_a_null_handle_loudly():
    """SMT_E_HIP on a machine without a device, SMT_E_INVALID otherwise: never SMT_OK, never a crash"""
    lib = L.lib()
    want = (L.SMT_E_INVALID,) if lib.smt_device_count() > 0 else (L.SMT_E_HIP,)
    n, b = C.c_uint64(7), C.c_uint64(7)
    assert lib.smt_unigram_set_long_pieces(None, L.UG_MAX_LONG) in want
    assert lib.smt_unigram_long_stats(None, C.byref(n), C.byref(b)) in want and (n.value, b.value) == (7, 7)
    assert lib.smt_host_model_set_device_tokenizer_long(None, 1) == L.SMT_E_INVALID
    assert L.UG_MAX_WORD == LR.MAX_WORD == 64 and L.UG_MAX_LONG == LR.MAX_LONG == 2048
