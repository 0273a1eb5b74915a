"""GPU: the UTF-8 form of the Unigram device tokenizer (unigram_utf8_kernels.hip, smt_unigram_create_utf8) against
tests/unigram_utf8_ref.py -- ids, offsets and flags equal, for every normalizer chain and prepend scheme, every named line alone AND
packed with no separator between neighbours (a kernel that reads past a line's end would extend a piece, or finish a cut sequence, with
the next line's bytes).  The handles are the host reader's export (every code point) and, for two chains, the explicit constructor over
the blocks of the reference.  Pure-ASCII inputs give the ASCII handle's ids bit for bit; the patch path is compared with the host
tokenizer's ids for the whole batch.  Every case is a few lines of text."""
import ctypes as C
import json

import numpy as np
import pytest

import semtools_amd as smt
from semtools_amd import _lib as L
from tests import unigram_ref as U
from tests import unigram_utf8_ref as G

pytestmark = pytest.mark.gpu

CONFIGS = [(n, p, 0) for n in G.NORMS for p in G.PREPEND] + [("none", "always", None), ("seq", "first", None)]
R = G.R
V = {p: i for i, (p, _) in enumerate(G.build_vocab())}     # (the later index of a repeated piece)


def _load(tmp, tj):
    path = tmp / "tokenizer.json"
    path.write_text(json.dumps(tj))
    h = C.c_void_p()
    L.check(L.lib().smt_host_tokenizer_load(str(path).encode(), C.byref(h)))
    return h


@pytest.fixture(scope="module", params=CONFIGS, ids=lambda c: "-".join(map(str, c)))
def pair(request, gpu_ctx, tmp_path_factory):
    norm, prepend, unk = request.param
    tj = G.tokenizer_json(norm=norm, prepend=prepend, unk_id=unk)
    h = _load(tmp_path_factory.mktemp("ug8"), tj)
    tok = smt.Unigram(gpu_ctx, host_tokenizer=h, utf8=True)       # the UTF-8 device form the host reader exports: every code point
    yield tok, G.UnigramUtf8Ref(tj, blocks=None), request.param
    tok.close()
    L.lib().smt_host_tokenizer_free(h)


def _same(tok, ref, lines, **kw):
    ids, off, flg = tok.tokenize(lines, **kw)
    want = ref.batch(lines, **kw)
    assert np.array_equal(flg, want[2]), (lines[:4], flg.tolist(), want[2].tolist())
    assert np.array_equal(off, want[1]), (lines[:4], off.tolist()[:20], want[1].tolist()[:20])
    assert np.array_equal(ids, want[0]), (lines[:4], ids.tolist()[:40], want[0].tolist()[:40])
    return ids, off, flg


def _alone_and_packed(tok, ref, lines, **kw):
    for raw in lines:
        _same(tok, ref, [raw], **kw)
    return _same(tok, ref, lines, **kw)


def test_named_lines_alone_and_packed(pair):
    tok, ref, (norm, prepend, unk) = pair
    names = list(G.NAMED)
    lines = [G.NAMED[k] for k in names]
    bert = norm.startswith("bert")
    for drop in (True, False):
        _, off, flg = _alone_and_packed(tok, ref, lines, drop_unk=drop)
        f = dict(zip(names, flg.tolist()))
        assert f["empty"] == 0 and off[names.index("empty") + 1] == off[names.index("empty")]
        assert f["added_token"] == 1 and f["cjk"] == (1 if bert else 0)          # a Chinese character between two spaces: FLAG
        assert f["max_word_plus_one"] == 1 and f["max_word_plus_one_byte"] == 1 and f["first_word_over"] == 1
        assert f["first_word_at_bound_never"] == (0 if prepend == "never" else 1)
        if unk is not None:
            assert f["exactly_max_word"] == 0 and f["exactly_max_word_multibyte"] == 0 and f["first_word_at_bound"] == 0
            assert f["accented"] == 0 and f["cyrillic"] == 0 and f["hangul"] == 0 and f["four_byte"] == 0 and f["literal_replacement"] == 0
            # the SPACE character counts as one whatever its length: the 63 bytes behind a 2- or 3-byte space are a piece at the bound
            assert f["max_word_behind_nbsp"] == f["max_word_behind_ideographic_space"] == (0 if norm == "bert_clean" else 1)
            for k in names:
                if k.startswith("straddle_"):
                    assert f[k] == 0, k
        assert f["unknown_3byte"] == f["unknown_3byte_pair"] == (1 if unk is None else 0)


def test_what_the_lines_become(pair):
    tok, ref, (norm, prepend, unk) = pair
    lead = [] if prepend == "never" else [V[R]]
    one = lambda s, **kw: tok.tokenize([s.encode() if isinstance(s, str) else s], **kw)[0].tolist()   # noqa: E731
    assert one(" мир вмир") == [V[R + "мир"], V[R], V["в"], V["мир"]]                    # the later id of the repeated piece
    assert one(" дж") == [V[R], V["дж"]]                                                  # the tie: R + дж, not R+д + ж
    assert one(" привет") == [V[R + "привет"]] and one(" примир") == [V[R + "при"], V["мир"]]
    assert one(" the" + R + "fox") == [V[R + "the"], V[R + "fox"]]                        # a literal replacement starts a piece
    assert one(R + "the") == [V[R + "the"]]                                               # ... and nothing is prepended in front of it
    if unk is not None:
        assert one("か", drop_unk=False) == lead + [0] and one("かな", drop_unk=False) == lead + [0]   # two unknowns fuse
        assert one(" aかなb", drop_unk=False) == [V[R + "a"], 0, V["b"]] and one(" aかなb", drop_unk=True) == [V[R + "a"], V["b"]]
        assert one("か", drop_unk=True) == lead
    else:
        assert tok.tokenize(["か".encode()])[2].tolist() == [1]
    if norm == "seq" or norm.startswith("bert"):
        j = G.JAMO
        # NFD: a syllable becomes its jamo, and the best path ends a piece between two jamo of ONE syllable, twice
        assert one(" " + G.HANGUL) == [V[R], V[j["h"] + j["a"]], V[j["n"] + j["g"]], V[j["eu"]], V[j["l"]]]
        assert one(" CAFÉ") == [V[R + "cafe"]] and one(" cafe\u0301") == [V[R + "cafe"]]
    if norm in ("none", "lower"):
        assert one(" " + G.HANGUL) == [V[R + G.HANGUL]] and one(" café") == [V[R + "café"]]
        assert one(" 中文 中") == [V[R + "中文"], V[R], V["中"]]
    if norm == "bert_clean":
        assert one("the\u00a0fox") == ([V[R + "the"]] if prepend != "never" else [V["the"]]) + [V[R + "fox"]]   # U+00A0 is a space
        assert one(" th\u200be") == [V[R + "the"]]                                        # a DROPPED code point inside a piece
        assert one("the\u3000fox")[-1] == V[R + "fox"]
    if norm == "none" and unk is not None:
        assert one(" the\u00a0fox", drop_unk=False) == [V[R + "the"], 0, V["fox"]]        # ... and an ordinary character here
    if norm == "seq":
        assert one(" the\u0301") == [V[R + "the"]]


@pytest.mark.parametrize("name", list(G.MALFORMED))
def test_malformed_utf8_flags_its_line_and_only_its_line(pair, name):
    tok, ref, (_, _, unk) = pair
    bad = G.MALFORMED[name]
    for lines in ([bad], [bad, G.VALID_NEXT], [G.VALID_NEXT, bad, G.VALID_NEXT, bad]):
        _, _, flg = _same(tok, ref, lines)
        assert flg.tolist() == [1 if x is bad else 0 for x in lines], name


def test_all_malformed_lines_packed(pair):
    tok, ref, _ = pair
    lines = [x for bad in G.MALFORMED.values() for x in (bad, G.VALID_NEXT)]
    _, _, flg = _same(tok, ref, lines)
    assert flg.tolist() == [1, 0] * len(G.MALFORMED)


def test_the_cut(pair):
    tok, ref, (_, _, unk) = pair
    for raw, keep in G.CUTS + U.CUTS:
        _alone_and_packed(tok, ref, [raw, b"the fox", raw, b"", raw], keep_bytes=keep)
    cafe = "the café fox".encode()
    flag = lambda raw, keep: tok.tokenize([raw], keep_bytes=keep)[2].tolist()[0]   # noqa: E731
    assert flag(cafe, 7) == 0                                  # the cut in front of the character: the looked-at part is ASCII
    assert flag(cafe, 8) == 1 and flag(cafe, 9) == 1           # inside it, and behind it: a byte >= 0x80 in a line longer than the cut
    assert flag(cafe, len(cafe)) == 0 and flag(cafe[:-1], len(cafe) - 1) == 0 and flag(cafe, len(cafe) - 1) == 1
    assert flag("the café".encode(), 9) == 0 and flag("the café!".encode(), 9) == 1   # the same bytes: the line one byte shorter is covered


def test_line_counts_0_1_65(pair):
    tok, ref, _ = pair
    ids, off, flg = tok.tokenize([])
    assert ids.size == 0 and off.tolist() == [0] and flg.size == 0
    _same(tok, ref, ["привет мир".encode()])
    _same(tok, ref, G.utf8_lines(seed=5, n=65))


def test_one_long_cyrillic_line_among_short_ones(pair):
    tok, ref, _ = pair
    whole = ("привет мир дж примир, the й. " * 200).encode()[:5000].decode("utf-8", "ignore").encode()
    long_line = whole + b"a" * (5000 - len(whole))
    assert len(long_line) == 5000 and sum(c >= 0x80 for c in long_line) > 3000
    _, _, flg = _same(tok, ref, ["мир ".encode(), b"fox,"] * 10 + [long_line] + [b"a b ", "дж ".encode()] * 10)
    assert not flg.any()                                             # (no character of it is unknown: covered without an unk id too)
    _, _, flg = _same(tok, ref, [b"fox", long_line[:4999] + b"\xd0", "мир".encode()])   # ... and the same line ending inside a character
    assert flg.tolist() == [0, 1, 0]


def test_generated_lines_are_tokenized_by_the_device(pair):
    tok, ref, (_, _, unk) = pair
    lines = G.utf8_lines(seed=22, n=400)
    if unk is None:
        lines = [x for x in lines if not ref.line(x)[1]]
        assert len(lines) > 40
    for kw in (dict(), dict(keep_bytes=40, max_tokens=8, drop_unk=True), dict(max_tokens=5, drop_unk=False)):
        a = _same(tok, ref, lines, **kw)
        assert kw or a[2].mean() <= 0.1                           # the device path, not the patch, is what was compared
        b = tok.tokenize(lines, **kw)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_pure_ascii_inputs_give_the_ascii_handles_ids_bit_for_bit(gpu_ctx, tmp_path, pair):
    tok, _, (norm, prepend, unk) = pair
    h = _load(tmp_path, G.tokenizer_json(norm=norm, prepend=prepend, unk_id=unk))
    plain = smt.Unigram(gpu_ctx, host_tokenizer=h)
    try:
        lines = [x for x in U.NAMED.values() if all(c < 0x80 for c in x)] + U.ascii_lines(seed=21, n=200)
        assert len(lines) > 230
        for kw in (dict(), dict(drop_unk=False), dict(keep_bytes=9, max_tokens=4)):
            a, b = plain.tokenize(lines, **kw), tok.tokenize(lines, **kw)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), kw
        for raw, keep in U.CUTS:
            if all(c < 0x80 for c in raw):
                a, b = plain.tokenize([raw, raw], keep_bytes=keep), tok.tokenize([raw, raw], keep_bytes=keep)
                assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), (raw, keep)
    finally:
        plain.close()
        L.lib().smt_host_tokenizer_free(h)


def test_info(pair, gpu_ctx, tmp_path):
    tok, _, (norm, prepend, unk) = pair
    table, cps, utf8 = tok.info()
    assert utf8 is True and cps > 0 and table > cps
    print("unigram utf-8 table", norm, table, "bytes, code points", cps)
    if (norm, prepend) == ("seq", "always"):
        h = _load(tmp_path, G.tokenizer_json(norm=norm, prepend=prepend, unk_id=unk))
        plain = smt.Unigram(gpu_ctx, host_tokenizer=h)
        try:
            assert plain.info()[1:] == (0, False) and 0 < plain.info()[0] < table
        finally:
            plain.close()
            L.lib().smt_host_tokenizer_free(h)


# ---- the explicit constructor: the code points of the reference's blocks, everything else in no range

@pytest.mark.parametrize("norm,prepend", [("bert_clean", "first"), ("seq", "never"), ("none", "always")])
def test_built_from_ranges_equals_the_reference(gpu_ctx, norm, prepend):
    tj = G.tokenizer_json(norm=norm, prepend=prepend)
    ref = G.UnigramUtf8Ref(tj)
    bmap = np.array([0xFF if b is None else b for b in ref.map], dtype=np.uint8)
    tok = smt.Unigram(gpu_ctx, vocab=G.build_vocab(), unk_id=0, prepend=prepend, byte_map=bmap, added=U.ADDED,
                      codepoints=G.codepoint_ranges(norm))
    try:
        lines = list(G.NAMED.values()) + [x for bad in G.MALFORMED.values() for x in (bad, G.VALID_NEXT)] + G.utf8_lines(seed=9, n=120)
        _, _, flg = _same(tok, ref, lines)
        assert flg[list(G.NAMED).index("flag_codepoint")] == 1            # U+0E01 is in no range
        assert tok.info()[2] is True and tok.info()[1] > 0
    finally:
        tok.close()


def test_create_utf8_refuses_what_it_cannot_serve(gpu_ctx):
    ok = [(0xA0, 0xA0, L.WP_CP_SPACE, ""), (0xC0, 0xFF, L.WP_CP_ORDINARY, ""), (0x2581, 0x2581, L.WP_CP_SPACE, "")]
    make = lambda cps, **kw: smt.Unigram(gpu_ctx, vocab=G.build_vocab(), unk_id=0, codepoints=cps, **kw)   # noqa: E731
    make(ok).close()
    make([]).close()                                                      # no range at all: every byte >= 0x80 flags its line
    bad = {
        "alone": ok + [(0x3001, 0x3001, L.WP_CP_ALONE, "")],
        "overlapping": [(0xC0, 0xFF, L.WP_CP_ORDINARY, ""), (0xF0, 0x100, L.WP_CP_ORDINARY, "")],
        "out_of_order": [(0x400, 0x4FF, L.WP_CP_ORDINARY, ""), (0xC0, 0xFF, L.WP_CP_ORDINARY, "")],
        "more_characters_than_source_bytes": [(0xC9, 0xC9, L.WP_CP_ORDINARY, "e\u0301x")],
        "output_over_16_bytes": [(0x1F600, 0x1F600, L.WP_CP_ORDINARY, "\U0001f600" * 5)],
        "output_not_utf8": [(0xC9, 0xC9, L.WP_CP_ORDINARY, b"\xc3")],
        "ascii_range": [(0x41, 0x5A, L.WP_CP_ORDINARY, "")],
    }
    for name, cps in bad.items():
        with pytest.raises(smt.SmtError) as e:
            make(cps)
        assert e.value.code == L.SMT_E_INVALID, name
    with pytest.raises(smt.SmtError) as e:
        make(ok, added=["<pad>", "é"])
    assert e.value.code == L.SMT_E_INVALID
    out = C.c_void_p()
    prm, cps = L.SmtUnigramParams(), L.SmtWordpieceCodepoints()
    lib = L.lib()
    assert lib.smt_unigram_create_utf8(gpu_ctx._h, None, C.byref(cps), C.byref(out)) == L.SMT_E_INVALID and not out
    assert lib.smt_unigram_create_utf8(gpu_ctx._h, C.byref(prm), None, C.byref(out)) == L.SMT_E_INVALID and not out
    assert lib.smt_unigram_create_utf8(gpu_ctx._h, C.byref(prm), C.byref(cps), None) == L.SMT_E_INVALID
    assert lib.smt_unigram_info(None, None, None, None) == L.SMT_E_INVALID


# ---- the patch path: flagged lines tokenized by the host tokenizer and spliced in by pass 2

def _host_ids(h, raw, max_tokens, median, unk):
    """what tokenize_batch stores for a line: truncate to max_tokens * median characters, encode, drop unk, cap"""
    text = raw.decode("utf-8", "replace")[: max_tokens * median].encode()
    ids = np.empty(len(text) + 16, np.uint32)
    n = C.c_uint64()
    L.check(L.lib().smt_host_tokenizer_encode(h, text, L.np_ptr(ids), ids.size, C.byref(n)))
    return [t for t in ids[: n.value].tolist() if t != unk][:max_tokens]


@pytest.mark.parametrize("which", ["none", "one", "all", "first_and_last"])
def test_patched_lines_equal_the_host_path(gpu_ctx, tmp_path, which):
    import torch

    max_tokens = 6
    tj = G.tokenizer_json(norm="bert_clean", prepend="always")
    h = _load(tmp_path, tj)
    tok = smt.Unigram(gpu_ctx, host_tokenizer=h, utf8=True)
    try:
        med, unk = C.c_uint64(), C.c_int64()
        L.check(L.lib().smt_host_tokenizer_info(h, None, C.byref(unk), C.byref(med)))
        median = int(med.value)
        keep = max_tokens * median
        ref = G.UnigramUtf8Ref(tj, blocks=None)
        plain = [x for x in G.utf8_lines(seed=31, n=400) if not ref.line(x, keep_bytes=keep)[1]]
        plain = [x for x in plain if any(c >= 0x80 for c in x)][:20] + [x for x in plain if all(c < 0x80 for c in x)][:20]
        odd = ["中文 the text".encode(), b"x<pad>y the <unk> fox", ("мир " * 20 + "привет").encode(), b"<pad> the fox"]
        n = len(plain)
        assert n == 40 and len(odd[2]) > keep
        lines = {"none": plain, "one": plain[:20] + [odd[0]] + plain[20:], "all": odd * 3,
                 "first_and_last": [odd[1]] + plain[: n // 2] + [odd[2]] + plain[n // 2:] + [odd[3]]}[which]
        want = [_host_ids(h, raw, max_tokens, median, unk.value) for raw in lines]
        text, begin, lens = smt.Unigram.pack(lines)
        dev = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
        d_text = dev(np.frombuffer(text, dtype=np.uint8).copy())
        d_begin, d_len = dev(begin.view(np.int64)), dev(lens.view(np.int32))
        d_counts = torch.zeros(len(lines), dtype=torch.int32, device="cuda")
        d_flags = torch.zeros(len(lines), dtype=torch.uint8, device="cuda")
        d_nflag = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        tok.scan_device(d_text.data_ptr(), len(text), d_begin.data_ptr(), d_len.data_ptr(), len(lines), keep, max_tokens, True,
                        d_counts.data_ptr(), d_flags.data_ptr(), d_nflag.data_ptr())
        gpu_ctx.synchronize()
        flagged = np.flatnonzero(d_flags.cpu().numpy())
        assert flagged.tolist() == [i for i, raw in enumerate(lines) if ref.line(raw, keep_bytes=keep)[1]]
        assert int(d_nflag.item()) == len(flagged) == {"none": 0, "one": 1, "all": len(lines), "first_and_last": 3}[which]
        counts = d_counts.cpu().numpy()
        assert all(counts[i] == 0 for i in flagged)
        assert all(counts[i] == len(want[i]) for i in range(len(lines)) if i not in set(flagged.tolist()))
        p_ids = np.array([t for i in flagged for t in want[i]], dtype=np.uint32)
        p_off = np.zeros(len(flagged) + 1, dtype=np.uint64)
        p_off[1:] = np.cumsum([len(want[i]) for i in flagged], dtype=np.uint64)
        d_pline, d_poff = dev(flagged.astype(np.int64)), dev(p_off.view(np.int64))
        d_pids = dev(np.concatenate([p_ids, np.zeros(1, np.uint32)]).view(np.int32))
        ids_cap = min(len(text), len(lines) * keep) + len(lines) + len(p_ids)
        d_ids = torch.full((ids_cap + 1,), -1, dtype=torch.int32, device="cuda")
        d_off = torch.zeros(len(lines) + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        tok.emit_device(len(lines), d_ids.data_ptr(), ids_cap, d_off.data_ptr(), d_pline.data_ptr(), d_poff.data_ptr(), d_pids.data_ptr(),
                        len(flagged), len(p_ids))
        gpu_ctx.synchronize()
        off = d_off.cpu().numpy()
        want_off = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.int64)
        assert np.array_equal(off, want_off)
        got = d_ids.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[: off[-1]], np.array([t for w in want for t in w], dtype=np.uint32))
        assert (got[off[-1]:] == 0xFFFFFFFF).all()               # nothing written behind the last id
    finally:
        tok.close()
        L.lib().smt_host_tokenizer_free(h)
