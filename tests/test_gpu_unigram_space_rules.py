"""GPU: the space rules of the Unigram device tokenizer (unigram_rules_kernels.hip, smt_unigram_set_space_rules) against
tests/precompiled_ref.py -- ids, offsets and flags equal, for each rule combination on both forms of the handle, every named line
alone AND packed with no separator between neighbours.  The handles are the host reader's export of an XLM-R-style tokenizer.json (a
Precompiled normalizer over the character map of tests/golden); the file gives them their rules, and one configuration overrides
them to drop_trailing alone.  Rules 0, 0 give the ids of a handle on which the setter was never called, bit for bit.  Reads the
fixture and the library only.  Every case is a few lines of text."""
import ctypes as C
import json

import numpy as np
import pytest

import semtools_amd as smt
from semtools_amd import _lib as L
from tests import precompiled_ref as P
from tests import unigram_ref as U
from tests import unigram_utf8_ref as G

pytestmark = pytest.mark.gpu

# (shape of the file, collapse_runs, drop_trailing, UTF-8 form)
CONFIGS = [(s, c, d, u) for u in (True, False) for s, c, d in (("A_ws", 1, 1), ("B", 1, 1), ("A", 1, 0), ("A_ws", 0, 1))]
R = P.R
V = {p: i for i, (p, _) in enumerate(P.build_vocab())}


def _load(tmp, tj):
    path = tmp / "tokenizer.json"
    path.write_text(json.dumps(tj))
    h = C.c_void_p()
    L.check(L.lib().smt_host_tokenizer_load(str(path).encode(), C.byref(h)))
    return h


@pytest.fixture(scope="module", params=CONFIGS, ids=lambda c: "-".join(map(str, c)))
def pair(request, gpu_ctx, tmp_path_factory):
    shape, collapse, drop, utf8 = request.param
    tj = P.tokenizer_json(shape)
    h = _load(tmp_path_factory.mktemp("ugr"), tj)
    tok = smt.Unigram(gpu_ctx, host_tokenizer=h, utf8=utf8)
    if (collapse, drop) != P.RULES[shape]:
        tok.set_space_rules(collapse, drop)
    yield tok, P.PrecompiledRef(tj, collapse_runs=collapse, drop_trailing=drop, utf8=utf8), request.param
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
    tok, ref, (shape, collapse, drop, utf8) = pair
    names = list(P.NAMED)
    lines = [P.NAMED[k] for k in names]
    for drop_unk in (True, False):
        _, off, flg = _alone_and_packed(tok, ref, lines, drop_unk=drop_unk)
        f = dict(zip(names, flg.tolist()))
        assert f["empty"] == 0 and off[names.index("empty") + 1] == off[names.index("empty")]
        assert f["prose"] == 0 and f["viterbi"] == 0 and f["run_3_middle"] == 0 and f["tab_newline"] == 0
        assert f["run_70_middle"] == f["run_70_start"] == f["run_70_end"] == collapse   # the absorbed spaces count toward the measure
        assert f["one_space"] == drop and f["spaces_only"] == (collapse and drop)       # the line's only piece, and trailing
        assert f["dropped_between_spaces"] == 0
        if utf8:
            assert f["hangul_precomposed"] == 0 and f["fullwidth"] == 0 and f["nbsp_by_space"] == 0 and f["ideographic_by_space"] == 0
            assert f["zwsp_between_spaces"] == 0 and f["cyrillic"] == 0
            assert f["eacute_decomposed"] == f["zwj_emoji"] == f["regional_pair"] == f["hangul_decomposed"] == f["half"] == f["kabushiki"] == 1
        else:
            assert f["accented"] == 1 and f["fullwidth"] == 1


def test_what_the_lines_become(pair):
    tok, ref, (shape, collapse, drop, utf8) = pair
    one = lambda s, **kw: tok.tokenize([s.encode() if isinstance(s, str) else s], **kw)[0].tolist()   # noqa: E731
    between = [] if collapse else [V[R]]
    tail = [] if drop else [V[R]]
    assert one("the  fox") == [V[R + "the"]] + between + [V[R + "fox"]]
    assert one("the   fox") == [V[R + "the"]] + between * 2 + [V[R + "fox"]]
    assert one("  the fox") == between + [V[R + "the"], V[R + "fox"]]
    assert one("the fox ") == [V[R + "the"], V[R + "fox"]] + tail
    assert one("the fox   ") == [V[R + "the"], V[R + "fox"]] + (tail if collapse else [V[R]] * 2 + tail)
    assert one(" abcd  xy") == [V[R + "ab"], V["cd"]] + between + [V[R], V["xy"]]          # Viterbi and the tie rule behind a run
    if utf8:
        assert one("ﬁne　 ｆｕｌｌ") == [V[R + "fine"]] + between + [V[R + "full"]]     # U+3000 and ' ': two SPACE characters
        assert one("the ​ fox") == [V[R + "the"]] + between * 2 + [V[R + "fox"]]      # U+200B becomes a space too
        assert one("the 한글") == [V[R + "the"], V[R + "한글"]]


def _drops(ref):
    return [c for c in range(1, 32) if ref.cp_class(c)[0] == P.DROPPED]


def test_runs_at_the_borders_of_blocks_pieces_and_cuts(pair):
    tok, ref, (shape, collapse, drop, utf8) = pair
    head = b"the " * 63 + b"abc"                                   # 255 bytes: the next byte is the last of the first 256-byte block
    d = bytes(_drops(ref)[:3])
    assert len(head) == 255 and len(d) == 3                        # (the character map drops ASCII controls)
    lines = [
        head + b"   fox the",                                      # the owner in one block, absorbed spaces and the piece's text in the next
        head[1:] + b"    fox the",                                 # ... the owner and one absorbed space in the first block
        head + b" " + d[:1] + b" " + d[1:] + b"  fox",             # a run interleaved with dropped bytes, across the border
        b"the " + d[:1] + b" " + d[1:] + b"  fox " + d + b" ",     # ... and inside a block, the last space behind dropped bytes at the line's end
        d + b"  the",                                              # dropped bytes in front of the line's first space
        d + b" " + d,                                              # nothing but dropped bytes and a space
        b"the " + d[:1] * 63 + b" fox",                            # 63 dropped bytes in front of a space: inside the look-back
        b"the " + d[:1] * 64 + b" fox",                            # ... 64: the piece in front is over the measure
        b"the " + d[:1] * 70 + b" fox",                            # ... beyond the look-back bound: flagged
        b"the" + b" " * 61 + b"abc fox",                           # 1 + 60 absorbed + 3: at the bound
        b"the" + b" " * 62 + b"abc fox",                           # the measure passes 64 only because of absorbed spaces
        b"the" + b" " * 70 + b"abc",
        b" " * 64 + b"a",
        b" " * 65 + b"a",
    ]
    for long_pieces in (0, L.UG_MAX_LONG):
        tok.set_long_pieces(long_pieces)                           # while a rule is on, a piece over the measure flags its line either way
        try:
            _, _, flg = _alone_and_packed(tok, ref, lines)
            _alone_and_packed(tok, ref, lines, drop_unk=False)
            assert tok.long_stats() == (0, 0)
        finally:
            tok.set_long_pieces(0)
        f = flg.tolist()
        assert f[:5] == [0, 0, 0, 0, 0] and f[5] == drop           # nothing but dropped bytes and a space: the line's only piece
        assert f[6] == collapse and f[7] == f[8] == 1              # (the space behind the 63 is absorbed, and counts)
        assert f[9] == 0 and f[10] == f[11] == f[13] == collapse
    # a run cut by keep_bytes: the looked-at end inside the run, behind it, and inside the piece behind it
    for raw in (b"the    fox", head + b"    fox"):
        at = raw.index(b"  ")
        for keep in range(at - 1, at + 7):
            _alone_and_packed(tok, ref, [raw, b"the fox", raw, b"", raw], keep_bytes=keep)
    if utf8:
        wide = "the" + "　" * 3 + "ｆｕｌｌ"                       # three 3-byte SPACE characters, then 3-byte characters
        _alone_and_packed(tok, ref, [head + wide.encode(), (head[2:].decode() + wide).encode(), ("the" + "　" * 21 + "x").encode(),
                                     ("the" + "　" * 22 + "x").encode()])


def test_generated_lines_are_tokenized_by_the_device(pair):
    tok, ref, (shape, collapse, drop, utf8) = pair
    lines = [x for x in P.lines(seed=22, n=300) if b"\n" not in x]
    assert sum(map(len, lines)) < 65536
    for kw in (dict(), dict(keep_bytes=40, max_tokens=8, drop_unk=True), dict(max_tokens=5, drop_unk=False)):
        a = _same(tok, ref, lines, **kw)
        assert kw or not utf8 or a[2].mean() <= 0.1                # the device path, not the flags, is what was compared
        b = tok.tokenize(lines, **kw)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_line_counts_0_1_65(pair):
    tok, ref, _ = pair
    ids, off, flg = tok.tokenize([])
    assert ids.size == 0 and off.tolist() == [0] and flg.size == 0
    _same(tok, ref, [b"the  fox "])
    _same(tok, ref, P.lines(seed=5, n=65))


@pytest.mark.parametrize("utf8", [True, False])
def test_rules_0_0_are_the_handle_as_it_was(gpu_ctx, tmp_path, utf8):
    """bit for bit, by the kernels without the rules: a handle on which the setter was never called, one set to 0, 0, and one set to
    1, 1 and back"""
    tj = G.tokenizer_json(norm="bert_clean", prepend="first")
    h = _load(tmp_path, tj)
    toks = [smt.Unigram(gpu_ctx, host_tokenizer=h, utf8=utf8) for _ in range(3)]
    try:
        toks[1].set_space_rules(0, 0)
        toks[2].set_space_rules(1, 1)
        lines = list(G.NAMED.values()) + list(U.NAMED.values()) + [b"the  fox ", b"   "]
        changed = toks[2].tokenize(lines)
        toks[2].set_space_rules(0, 0)
        for kw in (dict(), dict(drop_unk=False), dict(keep_bytes=9, max_tokens=4)):
            a = toks[0].tokenize(lines, **kw)
            for t in toks[1:]:
                assert all(x.tobytes() == y.tobytes() for x, y in zip(a, t.tokenize(lines, **kw))), kw
        assert changed[0].tobytes() != toks[0].tokenize(lines)[0].tobytes()      # (the rules did change these lines)
        for bad in ((2, 0), (0, -1), (1, 7)):
            assert L.lib().smt_unigram_set_space_rules(toks[1]._h, *bad) == L.SMT_E_INVALID
        assert L.lib().smt_unigram_set_space_rules(None, 1, 1) == L.SMT_E_INVALID
    finally:
        for t in toks:
            t.close()
        L.lib().smt_host_tokenizer_free(h)
