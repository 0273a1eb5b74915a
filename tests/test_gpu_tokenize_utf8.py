"""GPU: the UTF-8 form of the device tokenizer (wordpiece_utf8_kernels.hip, smt_wordpiece_create_utf8) against
tests/wordpiece_utf8_ref.py -- ids, offsets and flags equal, for the four flag sets, each line alone AND packed with no separator
between neighbours.  The code-point table comes from the reference's own rules (U8.codepoint_ranges); the patch path takes the table
the host tokenizer exports and is compared with the host tokenizer's ids."""
import ctypes as C

import numpy as np
import pytest

import semtools_amd as smt
from semtools_amd import _lib as L
from tests import wordpiece_ref as W
from tests import wordpiece_utf8_ref as U8

pytestmark = pytest.mark.gpu

VOCAB = U8.build_vocab()
E_ACUTE, ZHONG, HAN, GRIN = "é", "中", "한", "\U0001f600"      # 2, 3, 3 (three jamo under strip_accents) and 4 bytes


def _device_tok(ctx, flags, utf8=True, **kw):
    cps = U8.codepoint_ranges(flags) if utf8 else None
    return smt.WordPiece(ctx, vocab=VOCAB, unk_id=VOCAB["[UNK]"], flags=flags, added=W.ADDED, max_input_chars_per_word=W.MAX_CHARS,
                         codepoints=cps, **kw)


@pytest.fixture(scope="module", params=list(W.FLAG_SETS))
def pair(request, gpu_ctx):
    flags = W.FLAG_SETS[request.param]
    tok = _device_tok(gpu_ctx, flags)
    yield tok, U8.WordPieceUtf8Ref(flags, VOCAB)
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


def test_an_accented_word_is_tokenized_on_the_device(pair, gpu_ctx):
    """fails on a library without the UTF-8 form: there the line is flagged"""
    tok, ref = pair
    raw = b"caf\xc3\xa9 the"
    ids, off, flg = tok.tokenize([raw])
    word = "cafe" if ref.flags & W.WP_LOWERCASE else "café"
    assert flg.tolist() == [0] and ids.tolist() == [VOCAB[word], VOCAB["the"]] and off.tolist() == [0, 2]
    old = _device_tok(gpu_ctx, ref.flags, utf8=False)
    try:
        assert old.tokenize([raw])[2].tolist() == [1]             # the ASCII form keeps flagging it
    finally:
        old.close()


NAMED = ["", " ", "café the", "Café CAFÉ café", "naïve über Über", "λόγος Λόγος και",
         "привет мир Мир й",
         # combining marks dropped inside a word (strip_accents), flagged without it
         "thé̀fox", "é́́mbeddings", "́the", "thé",
         # CJK characters alone, with and without neighbours; Unicode punctuation alone
         ZHONG + "文", "the" + ZHONG + "文fox", ZHONG + " x文y", ZHONG * 5, "　" + ZHONG + "　",
         "“the” fox—again…", "«fox»", "…", "——",
         # NBSP and U+2003 are spaces
         "the fox again", "  ", "the ",
         # Hangul: under strip_accents a syllable becomes its jamo and the pieces split inside it
         HAN + "글", HAN, HAN + "글x", "x" + HAN, HAN + " " + HAN,
         # 4-byte characters, kana, a dropped format character, U+FFFD, multi-character lowerings
         "ok" + GRIN + " " + GRIN + GRIN, "\U0001d400\U0001d401", "かな か", "x�y", "x​y", "x­y", "ﬁx ǆ İ ß Ω",
         "[PAD] café", "x[UNK]é", "þþ the", "the 〮 fox", "the ͸ fox", "\U00010300 the"]
NAMED = [s.encode() for s in NAMED]


def test_named_lines_alone_and_packed(pair):
    tok, ref = pair
    for drop in (True, False):
        _alone_and_packed(tok, ref, NAMED, drop_unk=drop)
    v = ref.vocab
    if ref.flags & W.WP_LOWERCASE:
        assert tok.tokenize([HAN.encode()])[0].tolist() == [v[U8.JAMO_HA], v["##" + U8.JAMO_N]]
        assert tok.tokenize([(HAN + "글").encode()])[0].tolist() == [v[U8.JAMO_HA], v["##" + U8.JAMO_N + U8.JAMO_G], v["##" + U8.JAMO_EUL]]
        assert tok.tokenize(["thé̀fox".encode()])[2].tolist() == [0]
    else:
        assert tok.tokenize([(HAN + "글").encode()])[0].tolist() == [v[HAN], v["##글"]]
        assert tok.tokenize(["thé̀fox".encode()])[2].tolist() == [1]
    want = [v["the"], v[ZHONG], v["文"], v["fox"]] if ref.flags & W.WP_NORMALIZER else [ref.unk]     # (the normalizer spaces them)
    assert tok.tokenize([("the" + ZHONG + "文fox").encode()], drop_unk=False)[0].tolist() == want
    assert tok.tokenize(["the fox again".encode()])[0].tolist() == [v["the"], v["fox"], v["again"]]
    assert tok.tokenize(["“the”".encode()])[0].tolist() == [v["“"], v["the"], v["”"]]
    assert tok.tokenize(["the \U00010300 fox".encode()])[2].tolist() == [1]        # a code point in no range is FLAG


def test_a_word_of_100_and_of_101_two_byte_letters(pair):
    tok, ref = pair
    v = ref.vocab
    e = "e" if ref.flags & W.WP_LOWERCASE else E_ACUTE
    _alone_and_packed(tok, ref, [(E_ACUTE * 100).encode(), (E_ACUTE * 101).encode(), (E_ACUTE * 50 + "­" + E_ACUTE * 50).encode()], drop_unk=False)
    assert tok.tokenize([(E_ACUTE * 100).encode()], drop_unk=False)[0].tolist() == [v[e]] + [v["##" + e]] * 99
    assert tok.tokenize([(E_ACUTE * 101).encode()], drop_unk=False)[0].tolist() == [ref.unk]


def _straddlers():
    """300-byte lines in which a 2-, 3- or 4-byte character lies across byte offset 64, 128 or 256 -- every split of its bytes --, the
    offset each character starts at, and the same bytes cut into lines AT those characters and THROUGH them"""
    out = []
    for ch, word in ((E_ACUTE, "caf" + E_ACUTE + "s"), (ZHONG, "ab" + ZHONG + "cd"), (HAN, "x" + HAN + "글"), (GRIN, "ok" + GRIN)):
        w, lead = word.encode(), len(word[: word.index(ch)].encode())
        for shift in range(1, len(ch.encode())):
            s = bytearray(b"the " * 75)
            starts = []
            for edge in (64, 128, 256):
                at = edge - shift - lead                      # the character's first byte stands `shift` bytes in front of the edge
                s[at - 1:at + len(w) + 1] = b" " + w + b" "
                starts.append(edge - shift)
            assert len(s) == 300 and all(bytes(s[a:a + len(ch.encode())]).decode() == ch for a in starts)
            out.append((bytes(s), starts))
    return out


def test_characters_across_wave_and_block_boundaries(pair):
    tok, ref = pair
    whole, shifted, at_chars, through = [], [], [], []
    for s, starts in _straddlers():
        whole.append([s])                                                          # offsets of the text buffer == offsets within the line
        shifted += [b"the fox", s, b"the"]
        at_chars.append([s[:starts[0]], s[starts[0]:starts[1]], s[starts[1]:starts[2]], s[starts[2]:]])   # lines that START at them
        through.append([s[:64], s[64:128], s[128:256], s[256:]])                 # lines cut THROUGH them: malformed on both sides
    for lines in whole + at_chars + through + [shifted]:
        _same(tok, ref, lines)
    assert all(tok.tokenize(lines)[2].tolist() == [1, 1, 1, 1] for lines in through)
    assert all(tok.tokenize(lines)[2].sum() == 0 for lines in at_chars + whole)


MALFORMED = [b"a\x80b", b"\x80", b"\xbf\xbfab", b"caf\xc3", b"\xe4\xb8", b"\xf0\x9f\x98", b"ab\xe4\xb8x", b"\xc0\xaf", b"\xc1\xbf", b"\xe0\x80\xaf",
             b"\xe0\x9f\xbf", b"\xf0\x80\x80\xaf", b"\xf0\x8f\xbf\xbf", b"\xed\xa0\x80", b"\xed\xbf\xbf", b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80",
             b"\xf8\x88\x80\x80\x80", b"\xfe", b"\xff", b"\xc3\xa9\xa9", b"\xe4\xb8\xad\xad", b"\xf0\x9f\x98\x80\x80", b"the \xc3"]


def test_malformed_utf8_is_flagged_and_the_neighbours_are_untouched(pair):
    tok, ref = pair
    for bad in MALFORMED:
        ids, off, flg = _same(tok, ref, [b"the fox", bad, b"again the"], drop_unk=False)
        assert flg.tolist() == [0, 1, 0] and ids.tolist() == [VOCAB["the"], VOCAB["fox"], VOCAB["again"], VOCAB["the"]], bad
        _same(tok, ref, [bad])                                  # alone: the text ends inside or right behind the sequence
        _same(tok, ref, [b"the", bad])
    # a sequence cut by a line's end is not mended by the next line's first bytes
    _, _, flg = _same(tok, ref, [b"caf\xc3", b"\xa9 the", b"the \xe4", b"\xb8\xad", b"the"])
    assert flg.tolist() == [1, 1, 1, 1, 0]
    _same(tok, ref, [b"the fox"] + MALFORMED + [b"again"])


def test_keep_bytes_on_both_sides_of_the_cut(pair):
    tok, ref = pair
    raw = ("the caf" + E_ACUTE).encode()                            # 9 bytes: the accent's two at 7 and 8
    lines = [raw, raw + b" fox again", b"the fox again the", ("the " + ZHONG).encode(), (ZHONG + " the fox").encode(), b"x[PAD]y", b""]
    for keep in (3, 4, 5, 6, 7, 8, 9, 10, 13):
        _alone_and_packed(tok, ref, lines, keep_bytes=keep)
    assert tok.tokenize([raw], keep_bytes=7)[2].tolist() == [0]    # the kept bytes are ASCII: cut by bytes
    assert tok.tokenize([raw], keep_bytes=8)[2].tolist() == [1]    # a byte >= 0x80 in front of the cut of a line longer than the cut
    assert tok.tokenize([raw], keep_bytes=9)[2].tolist() == [0]    # a line no longer than the cut has no cut
    assert tok.tokenize([raw + b" fox"], keep_bytes=9)[2].tolist() == [1]


def test_max_tokens_cap_after_the_unk_drop(pair):
    tok, ref = pair
    lines = [("caf" + E_ACUTE + " the fox again the caf" + E_ACUTE + " fox again the").encode(), "þþ a b c d e f g h".encode(),
             ("a þ b þ c þ d þ e f g h i").encode(), (ZHONG * 9).encode(), (E_ACUTE * 30).encode(), b""]
    for drop in (True, False):
        _, off, _ = _alone_and_packed(tok, ref, lines, max_tokens=7, drop_unk=drop)
        assert np.diff(off.astype(np.int64)).tolist()[:3] == [7, 7, 7]
        assert int(off[4] - off[3]) == (7 if ref.flags & W.WP_NORMALIZER else 0 if drop else 1)    # nine words, or one unknown word
    v = ref.vocab
    assert tok.tokenize([lines[2]], max_tokens=7, drop_unk=True)[0].tolist() == [v[c] for c in "abcdefg"]
    assert tok.tokenize([lines[2]], max_tokens=7, drop_unk=False)[0].tolist() == [v["a"], ref.unk, v["b"], ref.unk, v["c"], ref.unk, v["d"]]


def test_fuzz_1500_mixed_lines_and_determinism(pair):
    tok, ref = pair
    lines = U8.utf8_lines(seed=33, n=1500)
    for kw in (dict(), dict(keep_bytes=40, max_tokens=8, drop_unk=True), dict(max_tokens=5, drop_unk=False)):
        a = _same(tok, ref, lines, **kw)
        b = tok.tokenize(lines, **kw)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    covered = sum(ref.covered(raw) for raw in lines if any(c >= 0x80 for c in raw))
    assert covered > 300                                            # in every flag set the device does tokenize non-ASCII lines


def test_pure_ascii_lines_give_the_bytes_of_the_ascii_form(pair, gpu_ctx):
    tok, ref = pair
    old = _device_tok(gpu_ctx, ref.flags, utf8=False)
    try:
        lines = W.ascii_lines(seed=34, n=1000) + [b"", b"w" * 100, b"w" * 101, b"x[PAD]y"]
        for kw in (dict(), dict(keep_bytes=30, max_tokens=6, drop_unk=True), dict(drop_unk=False)):
            a, b = tok.tokenize(lines, **kw), old.tokenize(lines, **kw)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    finally:
        old.close()


def test_create_validates_the_code_points(gpu_ctx):
    O, S, A, D, F = U8.ORDINARY, U8.SPACE, U8.ALONE, U8.DROPPED, U8.FLAG
    good = [(0x80, 0xBF, D, ""), (0xC9, 0xC9, O, "e"), (0xE9, 0xE9, O, ""), (0x2014, 0x2014, A, ""), (0xAC00, 0xAC00, O, "가")]
    smt.WordPiece(gpu_ctx, vocab=VOCAB, unk_id=1, codepoints=good).close()
    smt.WordPiece(gpu_ctx, vocab=VOCAB, unk_id=1, codepoints=[]).close()         # every code point >= U+0080 is FLAG
    bad = {"out of order": [(0xE9, 0xE9, O, ""), (0xC9, 0xC9, O, "")],
           "overlapping": [(0x80, 0xC9, O, ""), (0xC9, 0xD0, O, "")],
           "first > last": [(0xD0, 0xC9, O, "")],
           "below U+0080": [(0x41, 0x41, O, "")],
           "above U+10FFFF": [(0x10FFFF, 0x110000, O, "")],
           "unknown class": [(0xC9, 0xC9, 5, "")],
           "output not UTF-8": [(0xC9, 0xC9, O, b"\xc3")],
           "overlong output": [(0xC9, 0xC9, O, b"\xc0\xaf")],
           "more characters than source bytes": [(0xC9, 0xC9, O, "abc")],
           "output on a range": [(0xC9, 0xCA, O, "e")],
           "output on DROPPED": [(0xC9, 0xC9, D, "e")],
           "output on FLAG": [(0xC9, 0xC9, F, "e")],
           "ALONE of two characters": [(0x2014, 0x2014, A, "--")],
           "SPACE of two characters": [(0x2003, 0x2003, S, "  ")]}
    for what, cps in bad.items():
        with pytest.raises(smt.SmtError) as e:
            smt.WordPiece(gpu_ctx, vocab=VOCAB, unk_id=1, codepoints=cps)
        assert e.value.code == L.SMT_E_INVALID, what
    with pytest.raises(smt.SmtError) as e:
        smt.WordPiece(gpu_ctx, vocab=VOCAB, unk_id=1, codepoints=good, added=["[MÄSK]"])
    assert e.value.code == L.SMT_E_INVALID
    # offsets that decrease are refused as a whole, before any output byte is read: the first range's ten bytes are not in the pool
    first, last = np.array([0xC9, 0xE9], np.uint32), np.array([0xC9, 0xE9], np.uint32)
    cls, off = np.zeros(2, np.uint8), np.array([0, 10, 5], np.uint32)
    cps = L.SmtWordpieceCodepoints(L.np_ptr(first), L.np_ptr(last), L.np_ptr(cls), b"eeeee", L.np_ptr(off), 2)
    prm, out = L.SmtWordpieceParams(), C.c_void_p()
    assert L.lib().smt_wordpiece_create_utf8(gpu_ctx._h, C.byref(prm), C.byref(cps), C.byref(out)) == L.SMT_E_INVALID and not out
    assert b"non-decreasing" in L.lib().smt_last_error()


# ---- the patch path: the table the host tokenizer exports; flagged lines tokenized by the host tokenizer and spliced in by pass 2

def _host_ids(h, raw, max_tokens, median, unk):
    """what tokenize_batch stores for a line: truncate to max_tokens * median characters, encode, drop unk, cap"""
    text = raw.decode("utf-8")[: max_tokens * median].encode()
    ids = np.empty(len(text) + 16, np.uint32)
    n = C.c_uint64()
    L.check(L.lib().smt_host_tokenizer_encode(h, text, L.np_ptr(ids), ids.size, C.byref(n)))
    return [t for t in ids[: n.value].tolist() if t != unk][:max_tokens]


@pytest.mark.parametrize("name", ["norm_clean_lower", "norm_clean"])
def test_patched_lines_equal_the_host_path(gpu_ctx, tmp_path, name):
    import torch

    flags, max_tokens = W.FLAG_SETS[name], 64
    h = C.c_void_p()
    L.check(L.lib().smt_host_tokenizer_load(W.write_tokenizer(tmp_path / "tokenizer.json", flags, vocab=VOCAB).encode(), C.byref(h)))
    tok = smt.WordPiece(gpu_ctx, host_tokenizer=h, utf8=True)
    try:
        med, unk = C.c_uint64(), C.c_int64()
        L.check(L.lib().smt_host_tokenizer_info(h, None, C.byref(unk), C.byref(med)))
        median = int(med.value)
        keep = max_tokens * median
        ref = U8.WordPieceUtf8Ref(flags, VOCAB, blocks=None)
        lines = [x for x in U8.utf8_lines(seed=35, n=300) if b"\x00" not in x]
        lines += [b"x[PAD]y the [UNK] fox", ("caf" + E_ACUTE + " ").encode() * 50, b"the fox " * 50, ("the 〮 fox").encode(), ("thé fox").encode()]
        want = [_host_ids(h, raw, max_tokens, median, unk.value) for raw in lines]
        expect_flagged = [i for i, raw in enumerate(lines) if ref.line(raw, keep_bytes=keep)[1]]
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
        assert flagged.tolist() == expect_flagged and int(d_nflag.item()) == len(flagged)
        assert keep < 250 and lines.index(("caf" + E_ACUTE + " ").encode() * 50) in flagged and lines.index(b"the fox " * 50) not in flagged
        on_device = [i for i, raw in enumerate(lines) if i not in set(flagged.tolist()) and any(c >= 0x80 for c in raw)]
        assert len(flagged) > 3 and len(on_device) > 60            # non-ASCII lines do stay on the device
        counts = d_counts.cpu().numpy()
        fl = set(flagged.tolist())
        assert all(counts[i] == (0 if i in fl else len(want[i])) for i in range(len(lines)))
        p_ids = np.array([t for i in flagged for t in want[i]], dtype=np.uint32)
        p_off = np.zeros(len(flagged) + 1, dtype=np.uint64)
        p_off[1:] = np.cumsum([len(want[i]) for i in flagged], dtype=np.uint64)
        d_pline, d_poff = dev(flagged.astype(np.int64)), dev(p_off.view(np.int64))
        d_pids = dev(np.concatenate([p_ids, np.zeros(1, np.uint32)]).view(np.int32))
        ids_cap = min(len(text), len(lines) * keep) + len(p_ids)
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
