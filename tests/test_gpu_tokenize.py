"""GPU: the device tokenizer (tokenize_kernels.hip, smt_wordpiece_*) against tests/wordpiece_ref.py -- ids, offsets and flags equal,
for the four flag sets, every named line alone AND packed with no separator between neighbours (a kernel that reads past a line's
end would extend a word with the next line's bytes).  The patch path is compared with the host tokenizer's ids for the whole batch.
The tokenizer.json files are written by hand (tests/wordpiece_ref.py): no `tokenizers` wheel here."""
import ctypes as C

import numpy as np
import pytest

import semtools_amd as smt
from semtools_amd import _lib as L
from tests import wordpiece_ref as W

pytestmark = pytest.mark.gpu

VOCAB = W.build_vocab()


def _device_tok(ctx, flags, **kw):
    return smt.WordPiece(ctx, vocab=VOCAB, unk_id=VOCAB["[UNK]"], flags=flags, added=W.ADDED, max_input_chars_per_word=W.MAX_CHARS, **kw)


@pytest.fixture(scope="module", params=list(W.FLAG_SETS))
def pair(request, gpu_ctx):
    flags = W.FLAG_SETS[request.param]
    tok = _device_tok(gpu_ctx, flags)
    yield tok, W.WordPieceRef(flags)
    tok.close()


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


def _straddler():
    """300 bytes: multi-piece words across byte offsets 63/64, 127/128 and 255/256"""
    s = bytearray(b"the " * 75)
    for at, w in ((60, b"embeddings"), (120, b"understandings"), (245, b"internationalizations")):
        s[at - 1:at + len(w) + 1] = b" " + w + b" "
    return bytes(s)


NAMED = [b"", b"   ", b"\t\t\t", b"\x01\x02\x00\x1f", b"!", b"ab\x01cd", b"a\x0bb", b"a\x0cb", b"HELLO World The TEXT", b"w" * 100, b"w" * 101,
         b"w" * 50 + b"\x01\x02" + b"w" * 50, b"w" * 50 + b"\x01" + b"w" * 51, b"theedq", b"theedq the", b"zzz", b"embeddings",
         b"caf\xc3\xa9 the", b"x[PAD]y", b"a[b]c", b"[", b"[PA", b"[UNK]", b"don't 0xDEADBEEF e-mail (again)", b"the\x7fthe", b"A\x1fB",
         b"the", b" the ", b"internationalizations understandings"]


def test_named_lines_alone_and_packed(pair):
    tok, ref = pair
    for drop in (True, False):
        _, _, flg = _alone_and_packed(tok, ref, NAMED, drop_unk=drop)
        assert flg[NAMED.index(b"x[PAD]y")] == 1 and flg[NAMED.index(b"caf\xc3\xa9 the")] == 1
        assert flg[NAMED.index(b"a[b]c")] == 0 and flg[NAMED.index(b"[")] == 0 and flg[NAMED.index(b"[PA")] == 0
    v = ref.vocab
    ids, off, _ = tok.tokenize([b"theedq", b"theedq"], drop_unk=False)
    assert ids.tolist() == [ref.unk, ref.unk] and off.tolist() == [0, 1, 2]     # two pieces found, then no ##q: ONE unk
    assert tok.tokenize([b"theedq"], drop_unk=True)[0].size == 0
    if ref.flags & W.WP_CLEAN_TEXT:
        assert tok.tokenize([b"ab\x01cd"])[0].tolist() == [v[b"abcd"]] and tok.tokenize([b"a\x0bb"])[0].tolist() == [v[b"ab"]]
    else:
        assert tok.tokenize([b"a\x0bb"])[0].tolist() == [v[b"a"], v[b"b"]]       # VT is white space without clean_text


def test_line_counts_0_1_65(pair):
    tok, ref = pair
    ids, off, flg = tok.tokenize([])
    assert ids.size == 0 and off.tolist() == [0] and flg.size == 0
    _same(tok, ref, [b"the quick fox"])
    _same(tok, ref, W.ascii_lines(seed=5, n=65))


def test_words_across_wave_and_block_boundaries(pair):
    tok, ref = pair
    s = _straddler()
    assert s[60:70] == b"embeddings" and s[120:134] == b"understandings" and s[245:266] == b"internationalizations"
    _same(tok, ref, [s])                                         # offsets of the text buffer == offsets within the line
    _same(tok, ref, [b"the fox", s, b"the"])                     # the same offsets within a line that starts elsewhere
    _same(tok, ref, [s[:60], s[60:120], s[120:245], s[245:]])    # lines that START at those words, packed: no separator
    _same(tok, ref, [s[:64], s[64:128], s[128:256], s[256:]])    # lines that END inside them: the words are cut by the line ends


def test_one_long_line_among_short_ones(pair):
    tok, ref = pair
    long_line = (b"the quick embeddings, understandings zzz; " * 120)[:5000]
    _same(tok, ref, [b"the ", b"fox,"] * 10 + [long_line] + [b"a b ", b"zzz "] * 10)


def test_keep_bytes_cuts_lines(pair):
    tok, ref = pair
    lines = [b"the embeddings fox", b"the fox", b"the understandings caf\xc3\xa9", b"caf\xc3\xa9 the understandings", b"the quick x[PAD]y",
             b"the quick xy[PAD]", b"w" * 40, b"", b"abcd" * 5]
    for keep in (13, 14, 16, 20):
        _, _, flg = _alone_and_packed(tok, ref, lines, keep_bytes=keep)
        assert flg[2] == 0 and flg[3] == 1                       # a byte >= 0x80 counts only in front of the cut
    assert _same(tok, ref, lines, keep_bytes=16)[2][5] == 0       # [PAD] straddles the cut: it does not stand in what is looked at
    assert _same(tok, ref, lines, keep_bytes=20)[2][5] == 1


def test_max_tokens_cap_after_the_unk_drop(pair):
    tok, ref = pair
    lines = [b"the quick fox again the quick fox again the", b"zzz a b c d e f g h", b"a zzz b zzz c zzz d zzz e f g h i", b"the", b"",
             b"w" * 30, b"caf\xc3\xa9 a b c d e f g h"]
    for drop in (True, False):
        _, off, _ = _alone_and_packed(tok, ref, lines, max_tokens=7, drop_unk=drop)
        assert np.diff(off.astype(np.int64)).tolist()[:3] == [7, 7, 7]
    v = ref.vocab
    assert tok.tokenize([lines[2]], max_tokens=7, drop_unk=True)[0].tolist() == [v[c] for c in (b"a", b"b", b"c", b"d", b"e", b"f", b"g")]
    assert tok.tokenize([lines[2]], max_tokens=7, drop_unk=False)[0].tolist() == [v[b"a"], ref.unk, v[b"b"], ref.unk, v[b"c"], ref.unk, v[b"d"]]


def test_ids_cap_one_short_is_refused(pair):
    tok, _ = pair
    lines = [b"the fox", b"foxes"]
    assert tok.tokenize(lines, ids_cap=12)[1].tolist() == [0, 2, 5]
    with pytest.raises(smt.SmtError) as e:
        tok.tokenize(lines, ids_cap=11)
    assert e.value.code == L.SMT_E_INVALID
    assert tok.tokenize(lines, keep_bytes=3, ids_cap=6)[1].tolist() == [0, 1, 2]
    with pytest.raises(smt.SmtError) as e:
        tok.tokenize(lines, keep_bytes=3, ids_cap=5)
    assert e.value.code == L.SMT_E_INVALID


def test_lines_out_of_order_are_refused(pair):
    tok, _ = pair
    with pytest.raises(smt.SmtError) as e:
        tok.tokenize(text=b"the fox", line_begin=[4, 0], line_len=[3, 3])
    assert e.value.code == L.SMT_E_INVALID
    # gaps between lines are fine: the bytes between them belong to no line
    ids, off, _ = tok.tokenize(text=b"the!fox", line_begin=[0, 4], line_len=[3, 3])
    assert ids.tolist() == [VOCAB["the"], VOCAB["fox"]] and off.tolist() == [0, 1, 2]


def test_fuzz_2000_lines_and_determinism(pair):
    tok, ref = pair
    lines = W.ascii_lines(seed=21, n=2000)
    for kw in (dict(), dict(keep_bytes=40, max_tokens=8, drop_unk=True), dict(max_tokens=5, drop_unk=False)):
        a = _same(tok, ref, lines, **kw)
        b = tok.tokenize(lines, **kw)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_a_repeated_piece_takes_the_later_id_and_a_vocabulary_without_unk(gpu_ctx):
    tok = smt.WordPiece(gpu_ctx, vocab=[("the", 5), ("fox", 6), ("the", 9), ("##s", 7), ("##s", 8)], unk_id=-1, flags=7)
    try:
        ids, off, flg = tok.tokenize([b"the foxs", b"dog thes"])
        assert ids.tolist() == [9, 6, 8, 9, 8] and off.tolist() == [0, 3, 5] and flg.tolist() == [0, 0]
    finally:
        tok.close()


# ---- the patch path: flagged lines tokenized by the host tokenizer and spliced in by pass 2

def _host_ids(h, raw, max_tokens, median, unk):
    """what tokenize_batch stores for a line: truncate to max_tokens * median characters, encode, drop unk, cap"""
    text = raw.decode("utf-8")[: max_tokens * median].encode()
    ids = np.empty(len(text) + 16, np.uint32)
    n = C.c_uint64()
    L.check(L.lib().smt_host_tokenizer_encode(h, text, L.np_ptr(ids), ids.size, C.byref(n)))
    return [t for t in ids[: n.value].tolist() if t != unk][:max_tokens]


@pytest.mark.parametrize("which", ["none", "one", "all", "first_and_last"])
def test_patched_lines_equal_the_host_path(gpu_ctx, tmp_path, which):
    import torch

    flags, max_tokens = 7, 6
    h = C.c_void_p()
    L.check(L.lib().smt_host_tokenizer_load(W.write_tokenizer(tmp_path / "tokenizer.json", flags).encode(), C.byref(h)))
    tok = smt.WordPiece(gpu_ctx, host_tokenizer=h)
    try:
        med, unk = C.c_uint64(), C.c_int64()
        L.check(L.lib().smt_host_tokenizer_info(h, None, C.byref(unk), C.byref(med)))
        median = int(med.value)
        plain = [x for x in W.ascii_lines(seed=31, n=120) if b"[PAD]" not in x and b"[UNK]" not in x][:40]
        odd = ["café au lait, the fox".encode(), b"x[PAD]y the [UNK] fox", "中文 the text 日本語".encode(), "é".encode() * 50 + b" the fox"]
        n = len(plain)
        lines = {"none": plain, "one": plain[:20] + [odd[0]] + plain[20:], "all": odd * 3,
                 "first_and_last": [odd[1]] + plain[: n // 2] + [odd[2]] + plain[n // 2:] + [odd[3]]}[which]
        want = [_host_ids(h, raw, max_tokens, median, unk.value) for raw in lines]
        keep = max_tokens * median
        text, begin, lens = smt.WordPiece.pack(lines)
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
        assert int(d_nflag.item()) == len(flagged) == {"none": 0, "one": 1, "all": len(lines), "first_and_last": 3}[which]
        counts = d_counts.cpu().numpy()
        assert all(counts[i] == 0 for i in flagged)
        assert all(counts[i] == len(want[i]) for i in range(len(lines)) if i not in set(flagged.tolist()))
        p_ids = np.array([t for i in flagged for t in want[i]], dtype=np.uint32)
        p_off = np.zeros(len(flagged) + 1, dtype=np.uint64)
        p_off[1:] = np.cumsum([len(want[i]) for i in flagged], dtype=np.uint64)
        d_pline, d_poff = dev(flagged.astype(np.int64)), dev(p_off.view(np.int64))
        d_pids = dev(np.concatenate([p_ids, np.zeros(1, np.uint32)]).view(np.int32))
        ids_cap = min(len(text), len(lines) * keep) + len(p_ids)
        d_ids = torch.full((ids_cap + 1,), -1, dtype=torch.int32, device="cuda")
        d_off = torch.zeros(len(lines) + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(smt.SmtError) as e:
            tok.emit_device(len(lines), d_ids.data_ptr(), ids_cap - 1, d_off.data_ptr(), d_pline.data_ptr(), d_poff.data_ptr(), d_pids.data_ptr(),
                            len(flagged), len(p_ids))
        assert e.value.code == L.SMT_E_INVALID
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
