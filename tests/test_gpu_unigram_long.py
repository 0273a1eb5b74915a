"""GPU: the long pieces of the Unigram device tokenizer (unigram_long_kernels.hip, smt_unigram_set_long_pieces) against
tests/unigram_long_ref.py -- ids, offsets and flags equal for the normalizer sets and prepend schemes of tests/test_gpu_unigram.py, both
forms of the handle, every named long line alone AND packed with no separator between neighbours, and generated lines.  The witness
that ug_long_kernel answered, not the host: smt_unigram_long_stats equals the reference's count of long pieces and their bytes
(tests/test_unigram_long_ref_cpu.py shows that the existing references flag every one of these lines).  The patch path over the whole
batch is compared with the host tokenizer's ids.  With the switch back at 0 the handle is the old one, bit for bit."""
import ctypes as C
import json

import numpy as np
import pytest

import semtools_amd as smt
from semtools_amd import _lib as L
from tests import unigram_long_ref as LR
from tests import unigram_ref as U
from tests import unigram_utf8_ref as G

pytestmark = pytest.mark.gpu

CONFIGS = [(n, p, 0) for n in ("none", "lower", "bert_clean", "bert_noclean") for p in U.PREPEND] + [("none", "always", None), ("seq", "first", None)]
FORMS = ["ascii", "utf8"]


def _load(tmp, tj):
    path = tmp / "tokenizer.json"
    path.write_text(json.dumps(tj))
    h = C.c_void_p()
    L.check(L.lib().smt_host_tokenizer_load(str(path).encode(), C.byref(h)))
    return h


def _make(gpu_ctx, tmp, form, norm, prepend, unk, vocab=None):
    """(device tokenizer with long pieces on, long reference, existing reference, host tokenizer handle)"""
    if form == "ascii":
        tj = U.tokenizer_json(norm=norm, prepend=prepend, unk_id=unk, vocab=vocab)
        ref, old = LR.UnigramLongRef(tj), U.UnigramRef(tj)
    else:
        tj = G.tokenizer_json(norm=norm, prepend=prepend, unk_id=unk, vocab=vocab)
        ref, old = LR.UnigramLongUtf8Ref(tj, blocks=None), G.UnigramUtf8Ref(tj, blocks=None)
    h = _load(tmp, tj)
    tok = smt.Unigram(gpu_ctx, host_tokenizer=h, utf8=form == "utf8")
    tok.set_long_pieces(L.UG_MAX_LONG)
    return tok, ref, old, h


@pytest.fixture(scope="module", params=[(f,) + c for f in FORMS for c in CONFIGS], ids=lambda c: "-".join(map(str, c)))
def pair(request, gpu_ctx, tmp_path_factory):
    form, norm, prepend, unk = request.param
    tok, ref, old, h = _make(gpu_ctx, tmp_path_factory.mktemp("ugl"), form, norm, prepend, unk)
    yield tok, ref, old, h, request.param
    tok.close()
    L.lib().smt_host_tokenizer_free(h)


def _same(tok, ref, lines, rows=None, **kw):
    rows = rows if rows is not None else [ref.line(raw, **kw) for raw in lines]
    ids, off, flg = tok.tokenize(lines, **kw)
    w_flg = [1 if f else 0 for _, f in rows]
    w_off = np.concatenate([[0], np.cumsum([len(i) for i, _ in rows])]).astype(np.uint64)
    w_ids = np.array([t for i, _ in rows for t in i], dtype=np.uint32)
    assert flg.tolist() == w_flg, (lines[0][:40], flg.tolist(), w_flg)
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


def _named(form):
    return dict(LR.NAMED) if form == "ascii" else {**LR.NAMED, **LR.NAMED_UTF8}


def test_named_lines_alone_and_packed(pair):
    tok, ref, old, _, (form, norm, prepend, unk) = pair
    named = _named(form)
    names, lines = list(named), list(named.values())
    for drop in (True, False):
        rows = [ref.line(raw, drop_unk=drop) for raw in lines]
        for raw, row in zip(lines, rows):
            _same(tok, ref, [raw], [row], drop_unk=drop)
        _, _, flg = _same(tok, ref, lines, rows, drop_unk=drop)
        f = dict(zip(names, flg.tolist()))
        assert f["flag_2049_middle"] == 1 and f["flag_2049_last"] == 1 and f["flag_2050_first"] == 1 and f["exactly_2048_middle"] == 0
        assert f["tie_xy_40"] == 0 and f["viterbi_abcd_20"] == 0 and f["across_320"] == 0 and f["two_long_pieces"] == 0
        assert f["unk_run_130"] == (1 if unk is None else 0) and f["qu_covers_q"] == 0
    n, b = _stats_equal(tok, ref, lines)
    assert n >= 40 and b > 65 * n                        # the new kernel answered
    v = {p: i for i, (p, _) in enumerate(U.build_vocab())}
    R = U.R
    assert tok.tokenize([b" " + b"xy" * 40])[0].tolist() == [v[R]] + [v["xy"]] * 40          # the tie at every step: the smallest start wins
    assert tok.tokenize([b" " + b"abcd" * 20])[0].tolist()[:2] == [v[R + "ab"], v["cd"]]     # not greedy's R+abc, d
    if unk is not None:
        lead = [] if prepend == "never" else [v[R]]
        assert tok.tokenize([b"z" * 130], drop_unk=False)[0].tolist() == lead + [0]          # one unk across the position tiles
        assert tok.tokenize([b"z" * 130], drop_unk=True)[0].tolist() == lead
    if norm == "bert_clean":
        assert tok.tokenize([b"\x01" * 300])[0].tolist() == ([] if prepend == "never" else [v[R]])
        assert tok.tokenize([b"the " + b"\x01\x02" * 150 + b" fox"])[0].tolist() == [v[R + "the"] if prepend != "never" else v["the"], v[R], v[R + "fox"]]


def test_generated_lines(pair):
    tok, ref, old, _, (form, _, _, unk) = pair
    lines = LR.long_lines(seed=11, n=120, utf8=form == "utf8", known_only=unk is None)
    for kw in (dict(), dict(max_tokens=9, drop_unk=False), dict(keep_bytes=150, max_tokens=40, drop_unk=True)):
        rows = [ref.line(raw, **kw) for raw in lines]
        _, _, flg = _same(tok, ref, lines, rows, **kw)
        if not kw:
            assert not flg.any()                         # the device, not the patch, is what was compared
    n, _ = _stats_equal(tok, ref, lines)
    assert n >= len(lines)
    _stats_equal(tok, ref, lines, keep_bytes=150)


def test_the_cut_and_the_cap(pair):
    tok, ref, _, _, (form, _, _, _) = pair
    cuts = LR.CUTS + (LR.CUTS_UTF8 if form == "utf8" else [])
    for raw, keep in cuts:
        lines = [raw, b"the fox", raw, b"", raw]
        _same(tok, ref, lines, keep_bytes=keep)
        _same(tok, ref, [raw], keep_bytes=keep)
    if form == "utf8":
        assert tok.tokenize([CUT[0] for CUT in LR.CUTS_UTF8[:2]], keep_bytes=100)[2].tolist() == [1, 1]   # a non-ASCII line longer than keep_bytes
        assert tok.tokenize([LR.CUTS_UTF8[1][0]], keep_bytes=184)[2].tolist() == [0]
    lines = [b"the " + b"abcd" * 20 + b" fox", b"a " + b"z" * 70 + b"the" * 20, b"mno" * 30, b"the", b""]
    for mt in (1, 2, 7, 30):                              # cuts inside a long piece's tokens
        for drop in (True, False):
            _same(tok, ref, lines, max_tokens=mt, drop_unk=drop)


def test_a_vocabulary_piece_of_70_bytes(gpu_ctx, tmp_path):
    for form in FORMS:
        vocab = LR.long_vocab() if form == "ascii" else G.build_vocab() + [(LR.LONG_VOCAB_PIECE, -5.0)]
        tok, ref, old, h = _make(gpu_ctx, tmp_path, form, "none", "always", 0, vocab=vocab)
        try:
            lines = list(LR.NAMED_LONG_VOCAB.values())
            for raw in lines:
                _same(tok, ref, [raw])
            _same(tok, ref, lines)
            big = len(vocab) - 1
            got = tok.tokenize([LR.NAMED_LONG_VOCAB["piece_70_across_64"]])[0].tolist()
            assert got.count(big) == 1
            assert tok.tokenize([LR.NAMED_LONG_VOCAB["piece_70_twice"]])[0].tolist().count(big) == 2
            assert big not in tok.tokenize([LR.NAMED_LONG_VOCAB["piece_70_one_short"]])[0].tolist()
            _stats_equal(tok, ref, lines)
        finally:
            tok.close()
            L.lib().smt_host_tokenizer_free(h)


def test_a_table_over_blocks_flags_the_code_points_outside(gpu_ctx):
    """the explicit constructor over the blocks of the reference: U+0E01 is in no range, inside a long piece it flags the line"""
    norm = "lower"
    tj = G.tokenizer_json(norm=norm, prepend="always")
    ref = LR.UnigramLongUtf8Ref(tj)
    bmap = np.array([0xFF if b is None else b for b in ref.map], dtype=np.uint8)
    tok = smt.Unigram(gpu_ctx, vocab=G.build_vocab(), unk_id=0, prepend="always", byte_map=bmap, added=U.ADDED, codepoints=G.codepoint_ranges(norm))
    try:
        tok.set_long_pieces(L.UG_MAX_LONG)
        lines = [LR.NAMED_UTF8[k] for k in LR.NAMED_UTF8 if k.startswith(("blocks_", "two_byte", "hangul", "flag_cut"))]
        for raw in lines:
            _same(tok, ref, [raw])
        _, _, flg = _same(tok, ref, lines)
        assert flg.sum() >= 2
    finally:
        tok.close()


@pytest.mark.parametrize("form", FORMS)
def test_more_long_pieces_than_the_kernel_has_blocks(gpu_ctx, tmp_path, form):
    tok, ref, _, h = _make(gpu_ctx, tmp_path, form, "none", "always", 0)
    try:
        lines = LR.many_pieces()
        _same(tok, ref, lines)
        n, _ = _stats_equal(tok, ref, lines)
        assert n >= 2900
    finally:
        tok.close()
        L.lib().smt_host_tokenizer_free(h)


def test_switch_off_is_the_old_handle(pair):
    tok, ref, old, _, (form, norm, prepend, unk) = pair
    short = U.ascii_lines(seed=5, n=200, pool=U.SAFE_POOL, seps=(" ", "  "))
    on = tok.tokenize(short)                              # zero long pieces with the switch on
    assert tok.long_stats() == (0, 0)
    tok.set_long_pieces(0)
    try:
        off = tok.tokenize(short)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(on, off))
        assert tok.long_stats() == (0, 0)
        names = ["max_word_plus_one", "first_word_over_max", "long_base64_like"]
        lines = [U.NAMED[k] for k in names] + list(LR.NAMED.values())[:12] + short[:20]
        ids, offs, flg = tok.tokenize(lines)
        want = old.batch(lines)
        assert flg[:3].tolist() == [1, 1, 1]
        assert np.array_equal(flg, want[2]) and np.array_equal(offs, want[1]) and np.array_equal(ids, want[0])
        for bad in (1, 2, 63, 64, 2049, 1 << 20):
            with pytest.raises(smt.SmtError) as e:
                tok.set_long_pieces(bad)
            assert e.value.code == L.SMT_E_INVALID
        tok.set_long_pieces(65)                           # the smallest limit: a piece of measure 65 is the device's, 66 is flagged
        lines = [b"the " + LR.word(63) + b" fox", b"the " + LR.word(64) + b" fox", b"the " + LR.word(65) + b" fox"]
        assert tok.tokenize(lines)[2].tolist() == [0, 0, 1]
    finally:
        tok.set_long_pieces(L.UG_MAX_LONG)


# ---- the patch path: flagged lines tokenized by the host tokenizer and spliced in by pass 2

def _host_ids(h, raw, max_tokens, median, unk):
    """what tokenize_batch stores for a line: truncate to max_tokens * median characters, encode, drop unk, cap"""
    text = raw.decode("utf-8")[: max_tokens * median].encode()
    ids = np.empty(len(text) + 16, np.uint32)
    n = C.c_uint64()
    L.check(L.lib().smt_host_tokenizer_encode(h, text, L.np_ptr(ids), ids.size, C.byref(n)))
    return [t for t in ids[: n.value].tolist() if t != unk][:max_tokens]


@pytest.mark.parametrize("form", FORMS)
def test_patched_lines_equal_the_host_path(gpu_ctx, tmp_path, form):
    import torch

    max_tokens = 1000
    tok, ref, old, h = _make(gpu_ctx, tmp_path, form, "lower", "always", 0)
    try:
        med, unk = C.c_uint64(), C.c_int64()
        L.check(L.lib().smt_host_tokenizer_info(h, None, C.byref(unk), C.byref(med)))
        median = int(med.value)
        keep = max_tokens * median
        gen = LR.long_lines(seed=41, n=40, utf8=form == "utf8")
        odd = [("café au lait " + "thefox" * 20).encode(), b"x<pad>y " + LR.word(100), LR.NAMED["flag_2049_middle"], ("中文 " + "the" * 30).encode()]
        lines = [odd[1]] + gen[:20] + [odd[0], odd[2]] + gen[20:] + [odd[3]]
        lines = [x for x in lines if len(x.decode()) <= keep or x.isascii()]
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
        assert 1 <= len(flagged) <= 4 and int(d_nflag.item()) == len(flagged)       # odd lines only: the generated ones are the device's
        counts = d_counts.cpu().numpy()
        assert all(counts[i] == (0 if i in set(flagged.tolist()) else len(want[i])) for i in range(len(lines)))
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
        assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.int64))
        got = d_ids.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[: off[-1]], np.array([t for w in want for t in w], dtype=np.uint32))
        assert (got[off[-1]:] == 0xFFFFFFFF).all()               # nothing written behind the last id
    finally:
        tok.close()
        L.lib().smt_host_tokenizer_free(h)
