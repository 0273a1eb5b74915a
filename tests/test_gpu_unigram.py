"""GPU: the Unigram device tokenizer (unigram_kernels.hip, smt_unigram_*) against tests/unigram_ref.py -- ids, offsets and flags equal,
for every normalizer set and prepend scheme, every named line alone AND packed with no separator between neighbours (a kernel that
reads past a line's end would extend a piece with the next line's bytes).  The patch path is compared with the host tokenizer's ids
for the whole batch.  The tokenizer.json files are written by hand (tests/unigram_ref.py): no `tokenizers` wheel here."""
import ctypes as C
import json

import numpy as np
import pytest

import semtools_amd as smt
from semtools_amd import _lib as L
from tests import unigram_ref as U

pytestmark = pytest.mark.gpu

CONFIGS = [(n, p, 0) for n in ("none", "lower", "bert_clean", "bert_noclean") for p in U.PREPEND] + [("none", "always", None), ("seq", "first", None)]


def _load(tmp, tj):
    path = tmp / "tokenizer.json"
    path.write_text(json.dumps(tj))
    h = C.c_void_p()
    L.check(L.lib().smt_host_tokenizer_load(str(path).encode(), C.byref(h)))
    return h


@pytest.fixture(scope="module", params=CONFIGS, ids=lambda c: "-".join(map(str, c)))
def pair(request, gpu_ctx, tmp_path_factory):
    norm, prepend, unk = request.param
    tj = U.tokenizer_json(norm=norm, prepend=prepend, unk_id=unk)
    h = _load(tmp_path_factory.mktemp("ug"), tj)
    tok = smt.Unigram(gpu_ctx, host_tokenizer=h)       # the device form the host reader exports
    yield tok, U.UnigramRef(tj), request.param
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
    names = list(U.NAMED)
    lines = [U.NAMED[k] for k in names]
    v = {p: i for i, (p, _) in enumerate(U.build_vocab())}
    R = U.R
    for drop in (True, False):
        _, off, flg = _alone_and_packed(tok, ref, lines, drop_unk=drop)
        f = dict(zip(names, flg.tolist()))
        assert f["byte_ge_80"] == 1 and f["added_token"] == 1 and f["added_token_prefix_only"] == (1 if unk is None else 0)
        assert f["exactly_max_word"] == 0 and f["max_word_plus_one"] == 1 and f["long_base64_like"] == 1
        assert f["first_word_exactly_max"] == 0 and f["first_word_over_max"] == 1
        assert f["one_unknown"] == (1 if unk is None else 0)    # (without an unk id the line is the host's, which raises its error)
        assert f["empty"] == 0 and off[names.index("empty") + 1] == off[names.index("empty")]
    lead = [] if prepend == "never" else [v[R]]
    assert tok.tokenize([b" abcd"])[0].tolist() == [v[R + "ab"], v["cd"]]            # greedy would take R+abc, d
    assert tok.tokenize([b" qu"])[2].tolist() == [0]                                  # q has no piece of its own, but qu covers it: no unknown on the path
    assert tok.tokenize([b" xy"])[0].tolist() == [v[R], v["xy"]]                     # the tie: R + xy, not R+x + y
    assert tok.tokenize([b" the bathe"])[0].tolist() == [v[R + "the"], v[R], v["b"], v["a"], v["the"]]   # the later id of the repeated piece
    if unk is not None:
        assert tok.tokenize([b"azzqzb"], drop_unk=False)[0].tolist() == ([v[R + "a"]] if prepend != "never" else [v["a"]]) + [0, v["b"]]
        assert tok.tokenize([b"z"], drop_unk=False)[0].tolist() == lead + [0]     # more tokens than bytes with a prepended R
        assert tok.tokenize([b"the <unk> z"], drop_unk=True)[0].tolist() == [v[R + "the"] if prepend != "never" else v["the"], v[R], v[R]]
    if norm == "bert_clean":
        assert tok.tokenize([b"\x01\x02\x7f"])[0].tolist() == lead and tok.tokenize([b"the\tfox"])[0].tolist()[-1] == v[R + "fox"]
    if norm == "none":
        assert tok.tokenize([b" the\tfox"])[0].tolist() == [v[R + "the"], v["\t"], v["fox"]]
        assert tok.tokenize([b" THE"])[0].tolist() == [v[R], v["T"], v["H"], v["E"]]
    if norm in ("lower", "bert_clean", "bert_noclean"):
        assert tok.tokenize([b" THE"])[0].tolist() == [v[R + "the"]]


def test_the_cut(pair):
    tok, ref, (_, _, unk) = pair
    for raw, keep in U.CUTS:
        _alone_and_packed(tok, ref, [raw, b"the fox", raw, b"", raw], keep_bytes=keep)
    assert tok.tokenize([b"the caf\xc3\xa9"], keep_bytes=7)[2].tolist() == [0] and tok.tokenize([b"the caf\xc3\xa9"], keep_bytes=8)[2].tolist() == [1]
    assert tok.tokenize([b"the <pad>"], keep_bytes=8)[2].tolist() == [1 if unk is None else 0]   # straddles the cut: '<' is an unknown character
    assert tok.tokenize([b"the <pad>"], keep_bytes=9)[2].tolist() == [1]


def test_max_tokens_cap_after_the_unk_drop(pair):
    tok, ref, (_, prepend, unk) = pair
    lines = [b"the fox the fox the fox the fox", b"z a b c d e f g h", b"a z b z c z d z e f g h i", b"the", b"", b"zzzz", b"caf\xc3\xa9 a b c d e"]
    for drop in (True, False):
        _, off, _ = _alone_and_packed(tok, ref, lines, max_tokens=7, drop_unk=drop)
        if unk is not None:
            assert np.diff(off.astype(np.int64)).tolist()[:3] == [7, 7, 7]


def test_line_counts_0_1_65(pair):
    tok, ref, _ = pair
    ids, off, flg = tok.tokenize([])
    assert ids.size == 0 and off.tolist() == [0] and flg.size == 0
    _same(tok, ref, [b"the search text"])
    _same(tok, ref, U.ascii_lines(seed=5, n=65))


def _straddler():
    """300 bytes: multi-piece words across byte offsets 63/64, 127/128 and 255/256"""
    s = bytearray(b"the " * 75)
    for at, w in ((60, b"abcdxy"), (122, b"searching"), (250, b"mnomnothez")):
        s[at - 1:at + len(w) + 1] = b" " + w + b" "
    return bytes(s)


def test_pieces_across_wave_and_block_boundaries(pair):
    tok, ref, _ = pair
    s = _straddler()
    assert s[60:66] == b"abcdxy" and s[122:131] == b"searching" and s[250:260] == b"mnomnothez"
    _same(tok, ref, [s])                                         # offsets of the text buffer == offsets within the line
    _same(tok, ref, [b"the fox", s, b"the"])                     # the same offsets within a line that starts elsewhere
    _same(tok, ref, [s[:60], s[60:122], s[122:250], s[250:]])    # lines that START at those words, packed: no separator
    _same(tok, ref, [s[:66], s[66:131], s[131:260], s[260:]])    # lines that END with them
    _same(tok, ref, [s[:64], s[64:128], s[128:256], s[256:]])    # lines that END inside them: the words are cut by the line ends


def test_one_long_line_among_short_ones(pair):
    tok, ref, _ = pair
    long_line = (b"the search abcd, xy mno thez; " * 200)[:5000]
    _same(tok, ref, [b"the ", b"fox,"] * 10 + [long_line] + [b"a b ", b"zq "] * 10)


def test_random_lines_are_tokenized_by_the_device(pair):
    tok, ref, (_, _, unk) = pair
    # (without an unk id an unknown character flags the line: there the pool holds only characters that are pieces)
    pool = U.SAFE_POOL if unk is not None else list("abcdefghijklmnoprstuvwxy ")
    lines = U.ascii_lines(seed=22, n=600, pool=pool, seps=(" ", "  "))
    if unk is None:
        lines = [x for x in lines if not ref.line(x)[1]]
        assert len(lines) > 300
    for kw in (dict(), dict(keep_bytes=40, max_tokens=8, drop_unk=True), dict(max_tokens=5, drop_unk=False)):
        a = _same(tok, ref, lines, **kw)
        assert not a[2].any()                                    # the device path, not the patch, is what was compared
        b = tok.tokenize(lines, **kw)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_ids_cap_one_short_is_refused(pair):
    tok, ref, (_, prepend, unk) = pair
    lines = [b"the fox", b"foxes"]
    want = ref.batch(lines)[1].tolist()
    assert tok.tokenize(lines, ids_cap=14)[1].tolist() == want   # 12 bytes + one per line
    with pytest.raises(smt.SmtError) as e:
        tok.tokenize(lines, ids_cap=13)
    assert e.value.code == L.SMT_E_INVALID
    assert tok.tokenize(lines, keep_bytes=3, ids_cap=8)[1].tolist() == ref.batch(lines, keep_bytes=3)[1].tolist()
    with pytest.raises(smt.SmtError) as e:
        tok.tokenize(lines, keep_bytes=3, ids_cap=7)
    assert e.value.code == L.SMT_E_INVALID
    with pytest.raises(smt.SmtError) as e:
        tok.tokenize(text=b"the fox", line_begin=[4, 0], line_len=[3, 3])
    assert e.value.code == L.SMT_E_INVALID


def test_built_from_a_vocabulary_equals_the_exported_form(gpu_ctx):
    tj = U.tokenizer_json(norm="bert_clean", prepend="first")
    ref = U.UnigramRef(tj)
    bmap = np.array([0xFF if b is None else b for b in ref.map], dtype=np.uint8)
    tok = smt.Unigram(gpu_ctx, vocab=U.build_vocab(), unk_id=0, prepend="first", byte_map=bmap, added=U.ADDED)
    try:
        _same(tok, ref, list(U.NAMED.values()))
        with pytest.raises(smt.SmtError):
            smt.Unigram(gpu_ctx, vocab=U.build_vocab(), replacement="_")
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

    max_tokens = 6
    h = _load(tmp_path, U.tokenizer_json(norm="lower", prepend="always"))
    tok = smt.Unigram(gpu_ctx, host_tokenizer=h)
    try:
        med, unk = C.c_uint64(), C.c_int64()
        L.check(L.lib().smt_host_tokenizer_info(h, None, C.byref(unk), C.byref(med)))
        median = int(med.value)
        plain = U.ascii_lines(seed=31, n=40, pool=U.SAFE_POOL, seps=(" ", "  "))
        odd = ["café au lait, the fox".encode(), b"x<pad>y the <unk> fox", "中文 the text 日本語".encode(), b"<pad> the fox"]
        assert max_tokens * median >= 6                          # (the cut leaves the flagged part of every odd line in front of it)
        n = len(plain)
        lines = {"none": plain, "one": plain[:20] + [odd[0]] + plain[20:], "all": odd * 3,
                 "first_and_last": [odd[1]] + plain[: n // 2] + [odd[2]] + plain[n // 2:] + [odd[3]]}[which]
        want = [_host_ids(h, raw, max_tokens, median, unk.value) for raw in lines]
        keep = max_tokens * median
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
        ref = U.UnigramRef(U.tokenizer_json(norm="lower", prepend="always"))
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
        with pytest.raises(smt.SmtError) as e:                   # one short of the rule: refused, nothing enqueued
            tok.emit_device(len(lines), d_ids.data_ptr(), ids_cap - 1, d_off.data_ptr(), d_pline.data_ptr(), d_poff.data_ptr(), d_pids.data_ptr(),
                            len(flagged), len(p_ids))
        assert e.value.code == L.SMT_E_INVALID
        gpu_ctx.synchronize()
        assert (d_ids.cpu().numpy() == -1).all() and (d_off.cpu().numpy() == 0).all()
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
