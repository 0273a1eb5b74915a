"""GPU: smt_lower_device / smt_lower_lines (lower_kernels.hip) against tests/lower_ref.py -- line by line the bytes of the host layer's
to_lowercase, ill-formed lines flagged and copied unchanged, the layout of the contract.  Every comparison is byte for byte; every
device call presets out_text to 0x5A with a guard area behind it and checks that nothing at or beyond the total was written."""
import numpy as np
import pytest
import torch

import semtools_amd as smt
from semtools_amd import _lib as L
from tests import lower_ref as R

pytestmark = pytest.mark.gpu

GUARD = 256
FILL = 0x5A


@pytest.fixture(scope="module")
def lower(gpu_ctx):
    h = smt.Lower(gpu_ctx)
    yield h
    h.close()


def _device(ctx, h, text, begin, lens, tail=b"", out_cap=None):
    """smt_lower_device on the text with `tail` standing in the allocation behind text_bytes -> (Result, n_flagged, the whole out buffer)"""
    n, tb = len(lens), len(text)
    cap = tb + tb // 2 if out_cap is None else out_cap
    d_text = torch.from_numpy(np.frombuffer(bytes(text) + bytes(tail) + b"\0", dtype=np.uint8).copy()).cuda()
    d_begin = torch.from_numpy(np.ascontiguousarray(begin, dtype=np.uint64).view(np.int64).copy()).cuda() if n else torch.zeros(1, dtype=torch.int64, device="cuda")
    d_len = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.uint32).view(np.int32).copy()).cuda() if n else torch.zeros(1, dtype=torch.int32, device="cuda")
    d_out = torch.full((cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    d_obegin = torch.full((n + 2,), -1, dtype=torch.int64, device="cuda")
    d_olen = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
    d_flags = torch.full((n + 1,), 7, dtype=torch.uint8, device="cuda")
    d_nflag = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    h.lower_device(d_text.data_ptr(), tb, d_begin.data_ptr(), d_len.data_ptr(), n, d_out.data_ptr(), cap, d_obegin.data_ptr(), d_olen.data_ptr(),
                   d_flags.data_ptr(), d_nflag.data_ptr())
    ctx.synchronize()
    ob = d_obegin.cpu().numpy().view(np.uint64)
    assert ob[n + 1] == np.uint64(0xFFFFFFFFFFFFFFFF) and d_olen.cpu().numpy()[n] == -1 and d_flags.cpu().numpy()[n] == 7   # nothing behind the arrays
    out = d_out.cpu().numpy()
    total = int(ob[n])
    res = R.Result(out[:total].tobytes(), ob[:n + 1].copy(), d_olen.cpu().numpy()[:n].view(np.uint32).copy(), d_flags.cpu().numpy()[:n].copy())
    return res, int(d_nflag.cpu().numpy()[0]), out


def _check(ctx, h, text, begin, lens, want, tail=b""):
    got, n_flagged, out = _device(ctx, h, text, begin, lens, tail=tail)
    assert np.array_equal(got.flags != 0, want.flags != 0), (np.flatnonzero(got.flags).tolist()[:10], np.flatnonzero(want.flags).tolist()[:10])
    assert n_flagged == int(np.count_nonzero(want.flags))
    bad = np.flatnonzero(got.len != want.len)
    assert bad.size == 0, (bad[:5].tolist(), got.len[bad[:5]].tolist(), want.len[bad[:5]].tolist())
    assert np.array_equal(got.begin, want.begin)
    if got.text != want.text:
        a, b = np.frombuffer(got.text, np.uint8), np.frombuffer(want.text, np.uint8)
        at = int(np.flatnonzero(a != b)[0])
        line = int(np.searchsorted(want.begin, at, side="right")) - 1
        raise AssertionError(("first differing byte", at, "line", line, got.text[at - 8:at + 8], want.text[at - 8:at + 8]))
    assert (out[len(want.text):] == FILL).all(), "bytes were written at or beyond out_begin[n_lines]"
    return got


CASES = list(R.cases())
_ALL = {}


def _all_code_points():
    if not _ALL:
        text, begin, lens = R.pack(R.all_code_point_lines())
        _ALL["case"] = (text, begin, lens, R.lower_lines(text, begin, lens))
    return _ALL["case"]


@pytest.mark.parametrize("name", CASES)
def test_named_case(name, lower, gpu_ctx):
    c = R.cases()[name]
    got = _check(gpu_ctx, lower, c.text, c.begin, c.len, R.reference(name))
    assert set(np.flatnonzero(got.flags).tolist()) == set(c.flagged)


def test_nul_and_every_ascii_byte_directly(lower, gpu_ctx):
    """the C-string reference cannot hold NUL: checked against the rule itself"""
    text = bytes(range(128)) * 3
    begin, lens = np.array([0, 128, 256], np.uint64), np.array([128, 128, 128], np.uint32)
    got, n_flagged, _ = _device(gpu_ctx, lower, text, begin, lens)
    want = bytes(b + 32 if 65 <= b <= 90 else b for b in text)
    assert got.text == want and n_flagged == 0 and got.len.tolist() == [128] * 3 and want[0] == 0 and want[128] == 0


def test_every_code_point(lower, gpu_ctx):
    """every code point U+0080 .. U+10FFFF except the surrogates, 64 per line: every run, the strides, the negative deltas, the multi
    entry, U+03A3 among its neighbours"""
    text, begin, lens, want = _all_code_points()
    assert not want.flags.any() and want.text != text and len(lens) > 17000
    _check(gpu_ctx, lower, text, begin, lens, want)


def test_f0_at_the_end_of_the_text_flags_and_does_not_decode_what_stands_behind_it(lower, gpu_ctx):
    lines = [b"Clean LINE", b"ok \xf0"]
    text, begin, lens = R.pack(lines)
    want = R.lower_lines(text, begin, lens)
    assert want.flags.tolist() == [0, 1]
    got = _check(gpu_ctx, lower, text, begin, lens, want, tail=b"\x9f\x98\x80")
    assert got.text.endswith(b"ok \xf0") and got.len.tolist() == [10, 4]
    # ... and the same F0 as the last byte of a line in the middle, the next line starting with the three bytes
    lines = [b"A\xf0", b"\x9f\x98\x80B", b"C"]
    text, begin, lens = R.pack(lines)
    want = R.lower_lines(text, begin, lens)
    assert want.flags.tolist() == [1, 1, 0]
    _check(gpu_ctx, lower, text, begin, lens, want)


CUSTOM = dict(runs=[(0x100, 0x10C, 1, 3),                        # stride 3: U+0100, 0103, 0106, 0109, 010C move, the others stay
                    (0x2100, 0x2119, 0x41 - 0x2100, 1),           # a negative delta that shrinks three bytes to one: -> A .. Z
                    (0x10400, 0x10401, 40, 1)],
              multi=[(0x3A3, [0x73]),                             # final_sigma off: U+03A3 is a code point like any other
                     (0x10500, [0xE9, 0x62, 0x63])],              # three code points: four bytes -> 2 + 1 + 1
              cased=[(0x100, 0x10C)], ignorable=[(0x300, 0x36F)], final_sigma=False)


def _custom_ref(s):
    """the reference for CUSTOM: a dictionary"""
    m = {0x3A3: "s", 0x10500: "\u00e9bc", 0x10400: chr(0x10428), 0x10401: chr(0x10429)}
    for cp in range(0x100, 0x10D, 3):
        m[cp] = chr(cp + 1)
    for cp in range(0x2100, 0x211A):
        m[cp] = chr(cp - 0x2100 + 0x41)
    return "".join(m.get(ord(ch), chr(ord(ch) + 32) if "A" <= ch <= "Z" else ch) for ch in s)


def test_custom_tables(gpu_ctx):
    assert smt.Lower.check_tables(CUSTOM) == L.SMT_OK
    h = smt.Lower(gpu_ctx, tables=CUSTOM)
    try:
        strs = ["".join(map(chr, range(0x100, 0x110))), "".join(map(chr, range(0x20FE, 0x211C))) * 20, "\U00010400\U00010401\U00010402",
                "a\u03a3 \u03a3b a\u03a3.", "\U00010500" * 300 + "X", "\u00c9 stays: no run covers it", "Ascii STILL Lowers", "\u0130"]
        lines = [s.encode() for s in strs]
        text, begin, lens = R.pack(lines)
        want = R.lower_lines(text, begin, lens, lower=lambda ln: _custom_ref(ln.decode()).encode())
        assert want.text != R.lower_lines(text, begin, lens).text
        _check(gpu_ctx, h, text, begin, lens, want)
    finally:
        h.close()
    with pytest.raises(smt.SmtError) as e:
        smt.Lower(gpu_ctx, tables=dict(CUSTOM, runs=[(0x100, 0x10C, 1, 0)]))
    assert e.value.code == L.SMT_E_INVALID


def test_capacity(lower, gpu_ctx):
    c = R.cases()["length_changes"]
    tb = len(c.text)
    bound = tb + tb // 2
    with pytest.raises(smt.SmtError) as e:
        _device(gpu_ctx, lower, c.text, c.begin, c.len, out_cap=bound - 1)
    assert e.value.code == L.SMT_E_INVALID
    with pytest.raises(smt.SmtError) as e:
        lower.lower(text=c.text, line_begin=c.begin, line_len=c.len, out_cap=bound - 1)
    assert e.value.code == L.SMT_E_INVALID
    # nothing was written by the refused device call: it is refused before anything is enqueued -- a fresh buffer handed to a
    # refused call stays as it was
    n = len(c.len)
    d_out = torch.full((bound + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    d_ob = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_misc = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
    d_text = torch.from_numpy(np.frombuffer(c.text, dtype=np.uint8).copy()).cuda()
    d_begin = torch.from_numpy(c.begin.view(np.int64).copy()).cuda()
    d_len = torch.from_numpy(c.len.view(np.int32).copy()).cuda()
    d_flags = torch.full((n + 1,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(smt.SmtError):
        lower.lower_device(d_text.data_ptr(), tb, d_begin.data_ptr(), d_len.data_ptr(), n, d_out.data_ptr(), bound - 1, d_ob.data_ptr(),
                           d_misc.data_ptr(), d_flags.data_ptr(), d_misc.data_ptr() + 4 * n)
    gpu_ctx.synchronize()
    assert (d_out.cpu().numpy() == FILL).all() and (d_ob.cpu().numpy() == -1).all() and (d_misc.cpu().numpy() == -1).all()
    assert (d_flags.cpu().numpy() == 7).all()
    # at the bound the call works, device form and host form
    _check(gpu_ctx, lower, c.text, c.begin, c.len, R.reference("length_changes"))
    want = R.reference("length_changes")
    text, ob, ol, fl = lower.lower(text=c.text, line_begin=c.begin, line_len=c.len, out_cap=bound)
    assert text == want.text and np.array_equal(ob, want.begin) and np.array_equal(ol, want.len) and not fl.any()


def test_the_host_form_checks_the_line_list_and_lowers_packed_lines(lower):
    text, ob, ol, fl = lower.lower(["HeLLo", "", "ÉCOLE aΣ", b"bad \xff", "K"])
    assert text == "hello\u00e9cole a\u03c2".encode() + b"bad \xff" + b"k" and ol.tolist() == [5, 0, 10, 5, 1] and fl.tolist() == [0, 0, 0, 1, 0]
    assert ob.tolist() == [0, 5, 5, 15, 20, 21]
    assert lower.lower([])[1].tolist() == [0]
    with pytest.raises(smt.SmtError) as e:
        lower.lower(text=b"abcdef", line_begin=np.array([3, 0], np.uint64), line_len=np.array([3, 3], np.uint32))
    assert e.value.code == L.SMT_E_INVALID
    with pytest.raises(smt.SmtError) as e:
        lower.lower(text=b"abcdef", line_begin=np.array([0, 2], np.uint64), line_len=np.array([3, 3], np.uint32))
    assert e.value.code == L.SMT_E_INVALID


def test_two_runs_of_the_largest_case_give_identical_bytes(lower, gpu_ctx):
    text, begin, lens, _ = _all_code_points()
    a, na, out_a = _device(gpu_ctx, lower, text, begin, lens)
    b, nb, out_b = _device(gpu_ctx, lower, text, begin, lens)
    assert a.text == b.text and np.array_equal(out_a, out_b) and np.array_equal(a.begin, b.begin) and np.array_equal(a.len, b.len) and na == nb == 0
