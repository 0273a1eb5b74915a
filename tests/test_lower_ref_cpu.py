"""CPU: tests/lower_ref.py is a sound yardstick for the device lower-casing (tests/test_gpu_lower.py) -- its named cases hold what
their names say, the flagged lines are the constructed ones, subtly wrong lowerings each fail a named case -- and
smt_lower_tables_check (host only) refuses what include/semtools_hip.h says it refuses and passes the library's own tables."""
import numpy as np
import pytest

import semtools_amd as smt
from semtools_amd import _lib as L
from tests import lower_ref as R


def test_every_case_holds_what_its_name_says_and_flags_the_constructed_lines():
    cases = R.cases()
    assert len(cases) > 25
    for name, c in cases.items():
        lines = R._lines_of(c.text, c.begin, c.len)
        for h in c.holds:
            assert any(h in ln for ln in lines), (name, h)
        ref = R.reference(name)
        assert set(np.flatnonzero(ref.flags).tolist()) == set(c.flagged), name
        ends = (c.begin + c.len).tolist()
        assert all(e <= b for e, b in zip(ends, c.begin.tolist()[1:])) and (not ends or ends[-1] <= len(c.text)), name
        # the layout of the contract
        assert ref.begin[0] == 0 and np.array_equal(np.diff(ref.begin.astype(np.int64)), ref.len.astype(np.int64)) and ref.begin[-1] == len(ref.text)
        assert all(int(o) <= int(n) + int(n) // 2 for o, n in zip(ref.len, c.len)), name
        for i in c.flagged:
            assert ref.text[int(ref.begin[i]):int(ref.begin[i + 1])] == lines[i], (name, i)
    sizes = {n: int(c.len.max()) if len(c.len) else 0 for n, c in cases.items()}
    assert [sizes["line_of_%d" % n] for n in (255, 256, 257, 1023, 1024, 1025)] == [255, 256, 257, 1023, 1024, 1025]
    assert len(cases["no_lines"].len) == 0 and not cases["only_empty_lines"].len.any() and len(cases["lines_4097"].len) == 4097
    assert sizes["mixed_100000"] == 100000 and sizes["one_byte_line"] == 1
    g = cases["gaps"]
    gaps = (g.begin[1:] - (g.begin[:-1] + g.len[:-1])).tolist()
    assert gaps == [1, 1000, 1000, 1000] and len(g.text) == int(g.begin[-1]) + int(g.len[-1])
    gap_bytes = g.text[int(g.begin[1]) + int(g.len[1]):int(g.begin[2])]
    assert R.SIGMA.encode() in gap_bytes and any(65 <= b <= 90 for b in gap_bytes)
    assert bytes(range(128)) in cases["ascii_all_128"].text


def test_lengths_change_both_ways_as_the_contract_lists_them():
    want = {R.DOT_I: (2, 3), R.A_STROKE: (2, 3), R.T_STROKE: (2, 3), R.KELVIN: (3, 1), R.ANGSTROM: (3, 2), R.OHM: (3, 2), R.SHARP_S: (3, 2)}
    for ch, (n_in, n_out) in want.items():
        raw = ch.encode()
        assert (len(raw), len(R.host_lower(raw))) == (n_in, n_out), hex(ord(ch))
    assert R.host_lower(R.DOT_I.encode()) == ("i" + R.DOT_ABOVE).encode()
    assert R.host_lower(b"A\0Z\0") == b"a\0z\0"


def test_final_sigma_of_the_reference():
    low = [R.host_lower(w.encode()).decode() for w in R.SIGMA_WORDS]
    s, f = R.SMALL_SIGMA, R.FINAL_SIGMA
    assert low[:8] == [s, "a" + f, s + "a", "a" + f + ".", "a" + s + "'b", "a'" + f, "οδυσσευς"[:-1] + f, "." + s]
    ref = R.reference("sigma_neighbour_lines")
    lines = [ref.text[int(a):int(b)].decode() for a, b in zip(ref.begin[:-1], ref.begin[1:])]
    assert lines[:4] == ["a" + f, "b", "a", s]          # the neighbouring line is no context
    for n in (300, 2000):
        ref = R.reference("sigma_marks_%d" % n)
        lines = [ref.text[int(a):int(b)].decode() for a, b in zip(ref.begin[:-1], ref.begin[1:])]
        m = R.ACUTE * n
        assert lines == ["a" + m + f, s + m + "b", "a" + s + m + "b", "a" + f + m, m + s, "a" + m + f + m + "."]


def test_the_second_lowering_agrees_with_the_reference_on_the_named_cases():
    for name, c in R.cases().items():
        if name in ("mixed_100000", "lines_4097"):
            continue
        got = R.lower_lines(c.text, c.begin, c.len, lower=R.py_lower)
        ref = R.reference(name)
        assert got.text == ref.text and np.array_equal(got.begin, ref.begin), name


def _same(a, b):
    return a.text == b.text and np.array_equal(a.begin, b.begin) and np.array_equal(a.len, b.len) and np.array_equal(a.flags, b.flags)


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_a_subtly_wrong_lowering_fails_its_named_case(mutant):
    name = R.MUTANT_FAILS[mutant]
    c = R.cases()[name]
    assert not _same(R.MUTANTS[mutant](c.text, c.begin, c.len), R.reference(name)), (mutant, name)


def test_all_code_point_lines_cover_every_scalar_value():
    lines = R.all_code_point_lines()
    assert len(lines) == (0x110000 - 0x80 - 0x800 + 63) // 64
    assert lines[0].decode()[0] == "\x80" and lines[-1].decode()[-1] == "\U0010ffff"
    assert sum(len(ln.decode()) for ln in lines[:50] + lines[-50:]) == 64 * 99 + len(lines[-1].decode())


# ---- smt_lower_tables_check

GOOD = dict(runs=[(0xC0, 0xDE, 32, 1), (0x100, 0x12E, 1, 2), (0x212A, 0x212A, -0x212A + 0x6B, 1)], multi=[(0x130, [0x69, 0x307])],
            cased=[(0xC0, 0xFF), (0x391, 0x3A9)], ignorable=[(0xAD, 0xAD), (0x300, 0x36F)], final_sigma=True)


def _bad(**change):
    t = dict(GOOD)
    t.update(change)
    return t


REFUSED = {
    "runs out of order": _bad(runs=[(0x100, 0x12E, 1, 2), (0xC0, 0xDE, 32, 1)]),
    "runs overlapping": _bad(runs=[(0xC0, 0xDE, 32, 1), (0xDE, 0xF0, 1, 1)]),
    "run last < first": _bad(runs=[(0xDE, 0xC0, 32, 1)]),
    "stride 0": _bad(runs=[(0xC0, 0xDE, 32, 0)]),
    "delta below 0": _bad(runs=[(0xC0, 0xDE, -0xC1, 1)]),
    "delta above U+10FFFF": _bad(runs=[(0x10FF00, 0x10FFFF, 1, 1)]),
    "delta onto a surrogate": _bad(runs=[(0xD000, 0xD7FF, 1, 1)]),
    "delta onto a surrogate with a stride": _bad(runs=[(0xD000, 0xD7FF, 0x100, 0x7FF)]),
    "multi n 0": _bad(multi=[(0x130, 0, [0x69, 0, 0])]),
    "multi n 4": _bad(multi=[(0x130, 4, [0x69, 0x69, 0x69])]),
    "multi target above U+10FFFF": _bad(multi=[(0x130, [0x110000])]),
    "multi target a surrogate": _bad(multi=[(0x130, [0xD800])]),
    "multi code point in a run": _bad(multi=[(0xC5, [0x69])]),
    "run below U+0080": _bad(runs=[(0x41, 0x5A, 32, 1)]),
    "multi below U+0080": _bad(multi=[(0x49, [0x69, 0x307])]),
    "cased below U+0080": _bad(cased=[(0x41, 0x5A), (0xC0, 0xFF)]),
    "ignorable below U+0080": _bad(ignorable=[(0x27, 0x27)]),
    "cased out of order": _bad(cased=[(0x391, 0x3A9), (0xC0, 0xFF)]),
    "ignorable overlapping": _bad(ignorable=[(0x300, 0x36F), (0x36F, 0x370)]),
    "cased last < first": _bad(cased=[(0xFF, 0xC0)]),
    "a two-byte code point grown to four": _bad(runs=[(0x700, 0x7FF, 0x10000, 1)]),
    "a multi entry grown past half": _bad(multi=[(0x130, [0x307, 0x307])]),
}


def test_the_good_tables_and_the_built_in_ones_pass():
    assert smt.Lower.check_tables(GOOD) == L.SMT_OK
    assert smt.Lower.check_tables(dict(final_sigma=False)) == L.SMT_OK          # empty tables: ASCII only
    # a stride that steps over the surrogates is fine; so is a 3-code-point entry that grows four bytes to six
    assert smt.Lower.check_tables(_bad(runs=[(0xD000, 0xE800, 1, 0x1800)], multi=[(0x10400, [0xE9, 0xE9, 0xE9])])) == L.SMT_OK
    assert L.lib().smt_lower_tables_check(None) == L.SMT_OK, L.lib().smt_last_error()     # NULL: the library's own tables


@pytest.mark.parametrize("why", sorted(REFUSED))
def test_tables_check_refuses(why):
    assert smt.Lower.check_tables(REFUSED[why]) == L.SMT_E_INVALID, why
    assert L.lib().smt_last_error()
