"""The contract of smt_lower_device (include/semtools_hip.h, "lower-casing") restated in Python, and the named cases the GPU tests run.

lower_lines(text, begin, len): every line alone through the host layer's to_lowercase (smt_host_to_lowercase -- existing host code, the
reference for the bytes), lines that are not strictly valid UTF-8 flagged and copied unchanged, the outputs back to back.  The strict
validity check is Python's own UTF-8 decoder: it refuses lone continuation bytes, cut sequences, overlong forms, surrogates, values
above U+10FFFF and the bytes that lead nothing, which is the list of the contract.

py_lower is a second, slow lowering with switches for the ways a device implementation can go subtly wrong; with every switch off it
agrees with the reference on the named cases (tests/test_lower_ref_cpu.py), so a switch is the only difference of its mutant."""
import collections
import ctypes as C
import functools
import unicodedata

import numpy as np

from semtools_amd import _lib as L

SIGMA, SMALL_SIGMA, FINAL_SIGMA = "\u03a3", "\u03c3", "\u03c2"
DOT_I, DOT_ABOVE, ACUTE = "\u0130", "\u0307", "\u0301"
KELVIN, ANGSTROM, OHM, SHARP_S = "\u212a", "\u212b", "\u2126", "\u1e9e"
A_STROKE, T_STROKE, ALPHA = "\u023a", "\u023e", "\u0391"

Case = collections.namedtuple("Case", "text begin len flagged holds")
Result = collections.namedtuple("Result", "text begin len flags")


def host_lower(line):
    """to_lowercase of the host layer on one line's bytes.  The C string cannot hold NUL: NUL is neither cased nor case-ignorable, so
    it ends every Final_Sigma look, and the pieces between NULs lowered alone give the line's bytes."""
    lib = L.lib()
    out = []
    for piece in bytes(line).split(b"\0"):
        p = lib.smt_host_to_lowercase(piece)
        out.append(C.string_at(p))
        lib.smt_host_free(p)
    return b"\0".join(out)


def strictly_valid(line):
    try:
        bytes(line).decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def pack(lines, gaps=None):
    """lines back to back; gaps[i] = bytes standing in front of line i (between the lines, owned by none)"""
    text, begin, lens = bytearray(), [], []
    for i, ln in enumerate(lines):
        if gaps and gaps.get(i):
            text += gaps[i]
        begin.append(len(text))
        lens.append(len(ln))
        text += ln
    return bytes(text), np.array(begin, dtype=np.uint64), np.array(lens, dtype=np.uint32)


def lower_lines(text, begin, lens, lower=host_lower):
    """-> Result(out text, out_begin uint64 [n + 1], out_len uint32 [n], flags uint8 [n])"""
    out, out_begin, out_len, flags = bytearray(), [0], [], []
    for b, n in zip(np.asarray(begin).tolist(), np.asarray(lens).tolist()):
        line = text[b:b + n]
        ok = strictly_valid(line)
        low = lower(line) if ok else line
        flags.append(0 if ok else 1)
        out += low
        out_len.append(len(low))
        out_begin.append(len(out))
    return Result(bytes(out), np.array(out_begin, dtype=np.uint64), np.array(out_len, dtype=np.uint32), np.array(flags, dtype=np.uint8))


# ---- the second lowering, with switches

def _ignorable(ch):
    return ch in "'.:^`·" or unicodedata.category(ch) in ("Mn", "Me", "Cf", "Lm", "Sk")


def _cased(ch):
    return ch.lower() != ch or ch.upper() != ch


def py_lower(line, sigma="rule", ignorable_is_cased=False, dot_above=True, before="", after=""):
    """one valid line lowered character by character.  sigma "small": U+03A3 always becomes U+03C3; ignorable_is_cased: a
    case-ignorable character ends the Final_Sigma look as a cased one; dot_above False: U+0130 loses its U+0307; before / after:
    characters of the neighbouring lines that the look may (wrongly) see."""
    s = bytes(line).decode("utf-8")
    ctx = before + s + after
    out = []
    for i, ch in enumerate(s):
        if ch == SIGMA:
            j = len(before) + i

            def look(seq):
                for c in seq:
                    if _ignorable(c):
                        if ignorable_is_cased:
                            return True
                        continue
                    return _cased(c)
                return False

            final = sigma == "rule" and look(reversed(ctx[:j])) and not look(ctx[j + 1:])
            out.append(FINAL_SIGMA if final else SMALL_SIGMA)
        elif ch == DOT_I:
            out.append("i" + DOT_ABOVE if dot_above else "i")
        else:
            out.append(ch.lower())
    return "".join(out).encode("utf-8")


# ---- the wrong lowerings: each takes (text, begin, lens) like lower_lines

def _lines_of(text, begin, lens):
    return [text[b:b + n] for b, n in zip(np.asarray(begin).tolist(), np.asarray(lens).tolist())]


def _with(lower_of_line):
    """a lower_lines whose valid lines go through lower_of_line(i, lines)"""
    def run(text, begin, lens):
        lines = _lines_of(text, begin, lens)
        it = iter(range(len(lines)))
        return lower_lines(text, begin, lens, lower=lambda _line: lower_of_line(next(i for i in it if strictly_valid(lines[i])), lines))
    return run


def _neighbour_context(i, lines):
    def edge(j, last):
        if j < 0 or j >= len(lines) or not strictly_valid(lines[j]):
            return ""
        s = lines[j].decode("utf-8")
        return s[-1:] if last else s[:1]
    return py_lower(lines[i], before=edge(i - 1, True), after=edge(i + 1, False))


def _length_preserving(text, begin, lens):
    r = lower_lines(text, begin, lens)
    b = np.concatenate([np.asarray(begin, dtype=np.uint64), np.array([r.begin[-1]], dtype=np.uint64)]) if len(lens) else r.begin
    return Result(r.text, b, r.len, r.flags)


def _lax_decoder(text, begin, lens):
    """the host function's decode: what is not strictly valid passes through byte by byte, and an overlong two-byte form is decoded"""
    out, out_begin, out_len = bytearray(), [0], []
    for line in _lines_of(text, begin, lens):
        low = host_lower(line).replace(b"\xc1\x81", b"a")
        out += low
        out_len.append(len(low))
        out_begin.append(len(out))
    return Result(bytes(out), np.array(out_begin, dtype=np.uint64), np.array(out_len, dtype=np.uint32), np.zeros(len(out_len), dtype=np.uint8))


def _gaps_counted(text, begin, lens):
    b = np.asarray(begin).tolist()
    n = np.asarray(lens).tolist()
    grown = [(b[i + 1] - b[i]) if i + 1 < len(b) else n[i] for i in range(len(b))]
    return lower_lines(text, begin, np.array(grown, dtype=np.uint32))


MUTANTS = {
    "Final_Sigma context taken from the neighbouring line": _with(_neighbour_context),
    "U+03A3 always U+03C3": _with(lambda i, lines: py_lower(lines[i], sigma="small")),
    "U+0130 without its U+0307": _with(lambda i, lines: py_lower(lines[i], dot_above=False)),
    "positions assumed length-preserving": _length_preserving,
    "the lax decoder": _lax_decoder,
    "a case-ignorable treated as cased": _with(lambda i, lines: py_lower(lines[i], ignorable_is_cased=True)),
    "gap bytes counted": _gaps_counted,
}
# the named case each mutant must fail
MUTANT_FAILS = {
    "Final_Sigma context taken from the neighbouring line": "sigma_neighbour_lines",
    "U+03A3 always U+03C3": "sigma_words",
    "U+0130 without its U+0307": "drift_blocks",
    "positions assumed length-preserving": "drift_blocks",
    "the lax decoder": "ill_formed_overlong_c1",
    "a case-ignorable treated as cased": "sigma_words",
    "gap bytes counted": "gaps",
}


# ---- the named cases

ILL_FORMED = collections.OrderedDict([
    ("lone_80", b"\x80"), ("c3_cut", b"\xc3"), ("e2_82_cut", b"\xe2\x82"), ("c0_80", b"\xc0\x80"), ("e0_80_80", b"\xe0\x80\x80"),
    ("surrogate", b"\xed\xa0\x80"), ("above_10ffff", b"\xf4\x90\x80\x80"), ("f8_lead", b"\xf8\x88\x80\x80\x80"),
])
SIGMA_WORDS = [SIGMA, "a" + SIGMA, SIGMA + "a", "a" + SIGMA + ".", "a" + SIGMA + "'b", "a'" + SIGMA, "ΟΔΥΣΣΕΥΣ",
               "." + SIGMA, "A" + SIGMA + " " + SIGMA + "A", ALPHA + SIGMA + ACUTE]


def _enc(lines):
    return [x.encode("utf-8") if isinstance(x, str) else bytes(x) for x in lines]


def _mixed_line(n_bytes, seed):
    """one valid line of exactly n_bytes: upper-case ASCII words, Latin-1 and Greek capitals with final sigmas, the characters whose
    length changes, CJK and a 4-byte character"""
    rng = np.random.default_rng(seed)
    parts = ["HELLO World", "ÉCOLE ÜBER", "ΟΔΥΣΣΕΥΣ Σ", DOT_I + "STANBUL", "300 " + KELVIN + " " + ANGSTROM + OHM,
             SHARP_S + A_STROKE + T_STROKE, "中文", "\U00010400\U0001f600", "a" + SIGMA + ACUTE * 3 + ".", "Mixed CASE text", "ПРИВЕТ"]
    out = bytearray()
    while len(out) < n_bytes:
        out += (parts[int(rng.integers(len(parts)))] + " ").encode("utf-8")
    out = out[:n_bytes]
    while not strictly_valid(out):                   # a character cut by the end: ASCII in its place
        k = len(out) - 1
        while (out[k] & 0xC0) == 0x80:
            k -= 1
        out[k:] = b"X" * (len(out) - k)
    return bytes(out)


def all_code_point_lines():
    """every code point U+0080 .. U+10FFFF except the surrogates, 64 per line"""
    cps = [cp for cp in range(0x80, 0x110000) if not 0xD800 <= cp <= 0xDFFF]
    return ["".join(map(chr, cps[i:i + 64])).encode("utf-8", "surrogatepass") for i in range(0, len(cps), 64)]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case(text, begin, len, flagged line numbers as constructed, holds: byte strings some line of the case must contain)"""
    out = collections.OrderedDict()

    def add(name, lines, flagged=(), holds=(), gaps=None):
        text, begin, lens = pack(_enc(lines), gaps)
        out[name] = Case(text, begin, lens, frozenset(flagged), tuple(h.encode("utf-8") if isinstance(h, str) else h for h in holds))

    add("no_lines", [])
    add("only_empty_lines", [""] * 700)
    add("one_byte_line", ["Q"], holds=["Q"])
    add("ascii_all_128", [bytes(range(128)), bytes(range(127, -1, -1)), b"\0", b"A\0Z"], holds=[b"\0", b"A", b"Z", b"\x7f"])
    for n in (255, 256, 257, 1023, 1024, 1025):
        add("line_of_%d" % n, ["x", _mixed_line(n, n), "Y"], holds=["HELLO", SIGMA])
    add("lines_4097", [("Line %d " % i + ("É" if i % 7 == 0 else "") + (SIGMA if i % 11 == 0 else "")) if i % 13 else "" for i in range(4097)],
        holds=["É", SIGMA])
    add("mixed_100000", [_mixed_line(100000, 7)], holds=[KELVIN, DOT_I, SIGMA, "\U00010400"])
    add("gaps", ["aB", "C" + SIGMA, "d", SIGMA + "E", ""], holds=[SIGMA],
        gaps={1: b"Z", 2: ("UPPER " + SIGMA + "A ").encode("utf-8") * 100, 3: SIGMA.encode("utf-8") * 500, 4: b"Q" * 1000})
    five_k = KELVIN * 5000, DOT_I * 5000, "Plain ASCII Line " * 40
    add("drift_blocks", list(five_k), holds=[KELVIN, DOT_I])
    add("drift_blocks_one_byte_between", [five_k[0], "A", five_k[1], "B", five_k[2], "C"], holds=[KELVIN, DOT_I])
    add("length_changes", [DOT_I, A_STROKE, T_STROKE, KELVIN, ANGSTROM, OHM, SHARP_S, (DOT_I + KELVIN) * 200, "x" + ANGSTROM * 129 + A_STROKE * 130],
        holds=[DOT_I, KELVIN, SHARP_S])
    add("sigma_words", SIGMA_WORDS, holds=["a" + SIGMA + ".", "a'" + SIGMA, "." + SIGMA])
    add("sigma_neighbour_lines", ["a" + SIGMA, "b", "a", SIGMA, "a" + SIGMA, SIGMA + "b", "x."], holds=["a" + SIGMA])
    for n in (300, 2000):
        add("sigma_marks_%d" % n, ["a" + ACUTE * n + SIGMA, SIGMA + ACUTE * n + "b", "a" + SIGMA + ACUTE * n + "b", "a" + SIGMA + ACUTE * n,
                                   ACUTE * n + SIGMA, "a" + ACUTE * n + SIGMA + ACUTE * n + "."], holds=[ACUTE * n + SIGMA])
    for name, bad in ILL_FORMED.items():
        lines = ["Clean UPPER " + SIGMA, b"AB" + bad + b"cd", "Éclean", bad + b"XY", "Clean TWO", b"xy" + bad, "aB" + SIGMA, b"", bad, "Z"]
        add("ill_formed_" + name, lines, flagged=(1, 3, 5, 8), holds=[bad])
    add("ill_formed_overlong_c1", ["Clean", b"X\xc1\x81Y", "É"], flagged=(1,), holds=[b"\xc1\x81"])
    add("ill_formed_cut_between_lines", [b"CAF\xc3", b"\xa9X", "Clean " + SIGMA], flagged=(0, 1), holds=[b"\xc3"])
    add("ill_formed_long_line", [b"UPPER \xc3\x89 " * 300 + b"\xff" + b" MORE " * 300, "Clean"], flagged=(0,), holds=[b"\xff"])
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    c = cases()[name]
    return lower_lines(c.text, c.begin, c.len)
