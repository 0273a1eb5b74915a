"""GPU: the long pieces of the Unigram device tokenizer under the space rules (unigram_long_rules_kernels.hip, the hand-over in
unigram_rules_kernels.hip, smt_unigram_set_long_rules) against tests/unigram_long_rules_ref.py -- ids, offsets and flags equal for the
configurations of tests/test_gpu_unigram_space_rules.py (shapes x rules x both forms of the handle), every named line alone AND
packed with no separator between neighbours, with drop_unk on and off, and generated lines.  The witness that the long-piece kernel
answered, not the host: smt_unigram_long_stats equals the reference's count.  With the switch off the handle is the one of
tests/precompiled_ref.py, bit for bit, and with rules 0, 0 the switch changes no byte.  The handles are the host reader's export of
an XLM-R-style tokenizer.json over the character map of tests/golden.  Every case is a handful of lines of a few KB."""
import ctypes as C
import json

import numpy as np
import pytest

import semtools_amd as smt
from semtools_amd import _lib as L
from tests import precompiled_ref as P
from tests import unigram_long_rules_ref as Q
from tests import unigram_ref as U
from tests import unigram_utf8_ref as G

pytestmark = pytest.mark.gpu

# (shape of the file, collapse_runs, drop_trailing, UTF-8 form)
CONFIGS = [(s, c, d, u) for u in (True, False) for s, c, d in (("A_ws", 1, 1), ("B", 1, 1), ("A", 1, 0), ("A_ws", 0, 1))]
R = Q.R
V = {p: i for i, (p, _) in enumerate(Q.build_vocab())}
V[R] = max(i for i, (p, _) in enumerate(Q.build_vocab()) if p == R)


def _load(tmp, tj):
    path = tmp / "tokenizer.json"
    path.write_text(json.dumps(tj))
    h = C.c_void_p()
    L.check(L.lib().smt_host_tokenizer_load(str(path).encode(), C.byref(h)))
    return h


@pytest.fixture(scope="module", params=CONFIGS, ids=lambda c: "-".join(map(str, c)))
def pair(request, gpu_ctx, tmp_path_factory):
    """(device tokenizer with long pieces and the switch on, the reference, the reference without long pieces, host handle, config)"""
    shape, collapse, drop, utf8 = request.param
    tj = Q.tokenizer_json(shape)
    h = _load(tmp_path_factory.mktemp("uglr"), tj)
    tok = smt.Unigram(gpu_ctx, host_tokenizer=h, utf8=utf8)
    if (collapse, drop) != P.RULES[shape]:
        tok.set_space_rules(collapse, drop)
    tok.set_long_pieces(L.UG_MAX_LONG)
    tok.set_long_rules(True)
    yield (tok, Q.LongRulesRef(tj, collapse_runs=collapse, drop_trailing=drop, utf8=utf8),
           P.PrecompiledRef(tj, collapse_runs=collapse, drop_trailing=drop, utf8=utf8), h, request.param)
    tok.close()
    L.lib().smt_host_tokenizer_free(h)


def _same(tok, ref, lines, rows=None, **kw):
    rows = rows if rows is not None else [ref.line(raw, **kw) for raw in lines]
    ids, off, flg = tok.tokenize(lines, **kw)
    w_flg = [1 if f else 0 for _, f in rows]
    w_off = np.concatenate([[0], np.cumsum([len(i) for i, _ in rows])]).astype(np.uint64)
    w_ids = np.array([t for i, _ in rows for t in i], dtype=np.uint32)
    assert flg.tolist() == w_flg, (lines[0][:40], [i for i, (a, b) in enumerate(zip(flg.tolist(), w_flg)) if a != b][:8])
    assert np.array_equal(off, w_off), (lines[0][:40], off.tolist()[:20], w_off.tolist()[:20])
    if not np.array_equal(ids, w_ids):
        at = int(np.flatnonzero(ids != w_ids)[0])
        raise AssertionError((lines[0][:40], at, ids[max(at - 4, 0):at + 8].tolist(), w_ids[max(at - 4, 0):at + 8].tolist()))
    return ids, off, flg


def _stats_equal(tok, ref, lines, keep_bytes=0):
    """smt_unigram_long_stats after a scan of the lines on which the witness is defined"""
    defined = [raw for raw in lines if ref.long_pieces(raw, keep_bytes) is not None]
    tok.tokenize(defined, keep_bytes=keep_bytes)
    assert tok.long_stats() == ref.stats(defined, keep_bytes), (tok.long_stats(), ref.stats(defined, keep_bytes))
    return ref.stats(defined, keep_bytes)


def _named(utf8):
    """the named lines of the reference and, for what the rules did before, of tests/precompiled_ref.py; the UTF-8 lines go to the
    ASCII form too: a byte >= 0x80 inside a long piece flags the line"""
    return {**Q.NAMED, **Q.NAMED_UTF8, **{"p_" + k: v for k, v in P.NAMED.items()}}


def _host_ids(h, raw):
    ids = np.empty(len(raw) + 16, np.uint32)
    n = C.c_uint64()
    L.check(L.lib().smt_host_tokenizer_encode(h, raw, L.np_ptr(ids), ids.size, C.byref(n)))
    return ids[: n.value].tolist()


def test_named_lines_alone_and_packed(pair):
    tok, ref, _, _, (shape, collapse, drop, utf8) = pair
    named = _named(utf8)
    names, lines = list(named), list(named.values())
    for drop_unk in (True, False):
        rows = [ref.line(raw, drop_unk=drop_unk) for raw in lines]
        for raw, row in zip(lines, rows):
            _same(tok, ref, [raw], [row], drop_unk=drop_unk)
        _, _, flg = _same(tok, ref, lines, rows, drop_unk=drop_unk)
        f = dict(zip(names, flg.tolist()))
        assert all(v == 1 for k, v in f.items() if k.startswith("flag_"))
        assert f["measure_64_behind_space"] == f["measure_65_behind_space"] == f["measure_66_first"] == f["exactly_2048_middle"] == 0
        assert f["run_62_abc"] == f["run_70_abc"] == f["spaces_65_a"] == f["run_with_dropped_80"] == f["run_across_256"] == 0
        assert f["exactly_2048_through_absorbed"] == 0 and f["over_2048_through_absorbed_only"] == f["over_2048_absorbed_alone"] == collapse
        assert f["trailing_70"] == 0 and f["spaces_70"] == (collapse and drop) and f["dropped_70"] == drop
        assert f["dropped_63_space"] == f["dropped_64_space"] == f["dropped_70_no_space_behind"] == 0
        assert f["tie_xy_40"] == f["viterbi_abcd_20"] == f["piece_70_twice"] == f["two_long_pieces"] == f["unk_run_130"] == 0
        assert f["p_run_70_start"] == f["p_run_70_middle"] == f["p_run_70_end"] == 0
        for k in ("ideographic_22", "cyrillic_72", "cjk_30", "cjk_66", "cjk_198", "cjk_600", "hangul_72", "fullwidth_90"):
            assert f[k] == (0 if utf8 else 1), k
    n, b = _stats_equal(tok, ref, lines)
    assert n >= 30 and b > 65 * n                        # the long-piece kernel answered (35 pieces in the ASCII form without collapse_runs)
    one = lambda s, **kw: tok.tokenize([s], **kw)[0].tolist()   # noqa: E731
    between = [] if collapse else [V[R]]
    assert one(Q.NAMED["tie_xy_40"]) == [V[R + "the"]] + between + [V[R]] + [V["xy"]] * 40      # the tie at every step: the smallest start wins
    assert one(Q.NAMED["viterbi_abcd_20"])[: 3 + len(between)] == [V[R + "the"]] + between + [V[R + "ab"], V["cd"]]   # not greedy's R+abc, d
    assert one(Q.NAMED["trailing_70"]) == [V[R + "the"], V[R + "fox"]] + ([] if collapse else [V[R]] * 69) + ([] if drop else [V[R]])
    assert one(b"the  " + b"z" * 130, drop_unk=False) == [V[R + "the"]] + between + [V[R], 0]   # one unk across the position tiles
    if collapse:
        assert one(Q.NAMED["run_70_abc"]) == [V[R + "the"], V[R + "abc"], V[R + "fox"]]
        assert one(Q.NAMED["spaces_70"]) == ([] if drop else [V[R]])
    if utf8:
        assert one(Q.NAMED_UTF8["ideographic_22"]) == [V[R + "the"]] + between * 21 + [V[R + "full"]]


def test_the_switch_is_what_keeps_the_long_pieces_on_the_device(pair):
    """(fails without smt_unigram_set_long_rules: there the lines come back flagged whatever smt_unigram_set_long_pieces set)"""
    tok, ref, old, h, (shape, collapse, drop, utf8) = pair
    names = list(Q.covered_only())
    lines = [Q.NAMED[k] for k in names]
    ids, off, flg = tok.tokenize(lines, drop_unk=False)
    assert not flg.any()
    for i, raw in enumerate(lines):                      # the host tokenizer's ids (the reference's where the rules are not the file's)
        want = _host_ids(h, raw) if (collapse, drop) == P.RULES[shape] else ref.line(raw, drop_unk=False)[0]
        assert ids[off[i]:off[i + 1]].tolist() == want, names[i]
    n, b = tok.long_stats()
    assert n >= len(lines) and b > 65 * n and (n, b) == ref.stats(lines)
    tok.set_long_rules(False)
    try:
        mixed = lines + [P.NAMED["prose"], P.NAMED["sample"], b"the  fox "]
        got = tok.tokenize(mixed, drop_unk=False)
        want = old.batch(mixed, drop_unk=False)
        assert got[2].tolist() == [1] * len(lines) + [0, 1, 0] and tok.long_stats() == (0, 0)   # (the sample line holds a cluster)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
        for bad in (2, -1, 7):
            assert L.lib().smt_unigram_set_long_rules(tok._h, bad) == L.SMT_E_INVALID
        assert L.lib().smt_unigram_set_long_rules(None, 1) == L.SMT_E_INVALID
        assert tok.tokenize(lines)[2].all()                                      # a refused value changed nothing
        tok.set_long_rules(True)
        tok.set_long_pieces(0)                                                   # the switch alone, without a limit: inert
        got = tok.tokenize(mixed, drop_unk=False)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)) and tok.long_stats() == (0, 0)
        tok.set_long_pieces(65)                                                  # the smallest limit: measure 65 is the device's, 66 is flagged
        assert tok.tokenize([Q.NAMED["measure_64_behind_space"], Q.NAMED["measure_65_behind_space"], Q.NAMED["measure_66_last"]])[2].tolist() == [0, 0, 1]
    finally:
        tok.set_long_pieces(L.UG_MAX_LONG)
        tok.set_long_rules(True)


def test_the_cut_and_the_cap(pair):
    tok, ref, _, _, (shape, collapse, drop, utf8) = pair
    for raw, keep in Q.CUTS:
        _same(tok, ref, [raw, b"the fox", raw, b"", raw], keep_bytes=keep)
        _same(tok, ref, [raw], keep_bytes=keep)
        _stats_equal(tok, ref, [raw, b"the fox", raw], keep_bytes=keep)
    lines = [Q.NAMED["viterbi_abcd_20"], Q.NAMED["run_with_dropped_80"], b"a  " + b"z" * 70 + b"the" * 20, Q.NAMED["trailing_70"], b"the", b""]
    for mt in (1, 2, 7, 30):                              # cuts inside a long piece's tokens
        for drop_unk in (True, False):
            _same(tok, ref, lines, max_tokens=mt, drop_unk=drop_unk)
    if utf8:
        wide = ("the fox" + "　" * 40 + "中文" * 30).encode()
        for keep in (7 + 60, 7 + 120, 7 + 150):           # a non-ASCII line longer than keep_bytes is flagged as ever
            _same(tok, ref, [wide, b"the fox", wide], keep_bytes=keep)
        _same(tok, ref, [wide], keep_bytes=len(wide))


def test_generated_lines_are_tokenized_by_the_device(pair):
    tok, ref, _, _, (shape, collapse, drop, utf8) = pair
    lines = [x for x in Q.lines(seed=22, n=300) if b"\n" not in x]
    assert sum(map(len, lines)) < 65536
    for kw in (dict(), dict(keep_bytes=90, max_tokens=8, drop_unk=True), dict(max_tokens=5, drop_unk=False)):
        a = _same(tok, ref, lines, **kw)
        assert kw or not utf8 or a[2].mean() <= 0.1                # the device path, not the flags, is what was compared
        b = tok.tokenize(lines, **kw)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    n, _ = _stats_equal(tok, ref, lines)
    assert n >= (60 if utf8 else 20)
    _stats_equal(tok, ref, lines, keep_bytes=90)


def test_more_long_pieces_than_the_kernel_has_blocks(pair):
    tok, ref, _, _, _ = pair
    lines = [raw.replace(b" ", b"  ") for raw in Q.LR.many_pieces(n_lines=30, per_line=30)]
    _same(tok, ref, lines)
    n, _ = _stats_equal(tok, ref, lines)
    assert n >= 850


@pytest.mark.parametrize("utf8", [True, False])
def test_under_rules_0_0_the_switch_changes_no_byte(gpu_ctx, tmp_path, utf8):
    tj = G.tokenizer_json(norm="bert_clean", prepend="first")
    h = _load(tmp_path, tj)
    toks = [smt.Unigram(gpu_ctx, host_tokenizer=h, utf8=utf8) for _ in range(2)]
    try:
        toks[1].set_long_rules(True)
        lines = list(Q.NAMED.values()) + list(Q.LR.NAMED.values()) + list(U.NAMED.values()) + [b"the  fox ", b"   "]
        for long_pieces in (0, L.UG_MAX_LONG):
            for t in toks:
                t.set_long_pieces(long_pieces)
            for kw in (dict(), dict(drop_unk=False), dict(keep_bytes=90, max_tokens=40)):
                a, b = toks[0].tokenize(lines, **kw), toks[1].tokenize(lines, **kw)
                assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), (long_pieces, kw)
                assert toks[0].long_stats() == toks[1].long_stats() and (toks[0].long_stats() != (0, 0)) == bool(long_pieces)
    finally:
        for t in toks:
            t.close()
        L.lib().smt_host_tokenizer_free(h)
