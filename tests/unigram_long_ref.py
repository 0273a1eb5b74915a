"""Plain-Python restatement of the Unigram device tokenizer with long pieces on (DESIGN 4.9 "long pieces"): the references of
tests/unigram_ref.py and tests/unigram_utf8_ref.py with the piece limit a parameter (`max_long`, the same measure: raw bytes, the
SPACE character or a prepended R counted as one) and with a lattice whose starts are bounded by the vocabulary's longest piece --
the existing one tries every start and is quadratic.  It still PULLS, smallest start first, strictly better replaces: the tie rule
is written from the rule, not copied from the kernel.

Also here: what smt_unigram_long_stats counts, the named long lines, and a seeded generator of lines with long pieces."""
import random

from tests import unigram_ref as U
from tests import unigram_utf8_ref as G

R = U.R
MAX_WORD = U.MAX_WORD
MAX_LONG = 2048                  # SMT_UG_MAX_LONG


def lattice(chars, pieces, max_piece_bytes, unk_score, unk, tie_largest=False, window_short=0, fuse_break=0):
    """Viterbi over the characters of one piece -> [(id, unknown)] of the best path with consecutive unknowns fused.  For every end
    the starts run from the smallest whose text fits the longest piece (the one character in front of the end always runs: the
    unknown edge) upwards.  The three keyword arguments make it WRONG on purpose (tests/test_unigram_long_ref_cpu.py): ties won by the
    largest start; starts bounded `window_short` bytes short of the longest piece; unknowns that do not fuse across a multiple of
    `fuse_break` positions."""
    n = len(chars)
    at = [0] * (n + 1)                                           # bytes in front of character i
    for i, ch in enumerate(chars):
        at[i + 1] = at[i] + len(ch.encode())
    best = [(0.0, None, None, False)] + [None] * n               # (sum, start, id, unknown)
    lo = 0
    for end in range(1, n + 1):
        while at[end] - at[lo] > max_piece_bytes - window_short and lo < end - 1:
            lo += 1
        node = None
        for start in range(lo, end):                             # smallest start first, strictly better replaces: ties keep the smaller
            text = "".join(chars[start:end])
            hit = pieces.get(text) if at[end] - at[start] <= max_piece_bytes - window_short else None
            if hit is not None:
                cand = hit[1] + best[start][0]
                if node is None or cand > node[0] or (tie_largest and cand == node[0]):
                    node = (cand, start, hit[0], False)
            elif end - start == 1:                               # no piece covers exactly this character
                cand = unk_score + best[start][0]
                if node is None or cand > node[0] or (tie_largest and cand == node[0]):
                    node = (cand, start, unk, True)
        best[end] = node
    path, e = [], n
    while e > 0:
        path.append((e,) + best[e][2:])
        e = best[e][1]
    out, prev_unk = [], False
    for e, tid, is_unk in reversed(path):
        if is_unk and prev_unk and not (fuse_break and (e - 1) % fuse_break == 0):
            continue
        out.append((tid, is_unk))
        prev_unk = is_unk
    return out


class _Long:
    """mixed into a reference in front of it: the limit a parameter, the lattice windowed"""
    max_long = MAX_LONG
    wrong = {}                                                   # keyword arguments of lattice(): a wrong lattice on purpose

    def piece(self, chars, ids):
        for tid, is_unk in lattice(chars, self.pieces, self.max_piece_bytes, self.unk_score, self.unk, **self.wrong):
            if is_unk and self.unk is None:
                raise U.Flagged("an unknown character and no unk id")
            ids.append(tid)

    def measures(self, raw):
        """the measure of every piece of a line (after the cut), or None: the line's bytes or characters are not covered"""
        units = self._units(raw)
        if units is None:
            return None
        out, first = [0], self.prepend != "never"
        for src, is_space in units:
            if is_space:
                out.append(1)
            else:
                out[-1] += src
        out[0] += 1 if first else 0
        return out

    def encode_long(self, raw):
        m = self.measures(raw)
        if m is not None and max(m) > self.max_long:
            return None
        return self.encode(raw, check_limit=False)

    def long_pieces(self, raw, keep_bytes=0):
        """the measures of the pieces the long-piece kernel tokenizes (over MAX_WORD, at most max_long), or None where the witness is
        not defined: a line whose looked-at part is not covered (the pieces in front of the offending byte still count), or a
        non-ASCII line longer than keep_bytes (its multi-byte SPACE characters own no piece)"""
        if keep_bytes and len(raw) > keep_bytes:
            raw = raw[:keep_bytes]
            if any(c >= 0x80 for c in raw):
                return None
        m = self.measures(raw)
        return None if m is None else [x for x in m if MAX_WORD < x <= self.max_long]

    def stats(self, lines, keep_bytes=0):
        """(pieces, raw bytes) as smt_unigram_long_stats reports them for a batch of lines on which the witness is defined"""
        got = [x for raw in lines for x in self.long_pieces(raw, keep_bytes)]
        return len(got), sum(got)


class UnigramLongRef(_Long, U.UnigramRef):
    def __init__(self, tj, max_long=MAX_LONG):
        super().__init__(tj)
        self.max_long = max_long

    def _units(self, raw):
        if any(c >= 0x80 for c in raw):
            return None
        return [(1, self.map[c] == 0x20) for c in raw]

    def line(self, raw, keep_bytes=0, max_tokens=0, drop_unk=True):
        if keep_bytes:
            raw = raw[:keep_bytes]
        ids = self.encode_long(raw)
        if ids is None:
            return [], True
        if drop_unk and self.unk is not None:
            ids = [t for t in ids if t != self.unk]
        if max_tokens:
            ids = ids[:max_tokens]
        return ids, False


class UnigramLongUtf8Ref(_Long, G.UnigramUtf8Ref):
    def __init__(self, tj, blocks=G.BLOCKS, max_long=MAX_LONG):
        super().__init__(tj, blocks=blocks)
        self.max_long = max_long

    def _units(self, raw):
        units = self.units(raw)
        return None if units is None else [(src, cls == G.SPACE) for src, cls, _ in units]

    def line(self, raw, keep_bytes=0, max_tokens=0, drop_unk=True):
        if keep_bytes and len(raw) > keep_bytes:
            raw = raw[:keep_bytes]
            if any(c >= 0x80 for c in raw):
                return [], True
        ids = self.encode_long(raw)
        if ids is None:
            return [], True
        if drop_unk and self.unk is not None:
            ids = [t for t in ids if t != self.unk]
        if max_tokens:
            ids = ids[:max_tokens]
        return ids, False


# ---- the named long lines.  A name that starts with "flag_" is meant to be flagged under every configuration, one that starts with
# "cjk" under handle_chinese_chars, one that starts with "blocks_" by a table over the blocks of the reference; one that holds "unk"
# has a character without a piece on its best path under some normalizer (flagged while the tokenizer has no unk id); every other
# one is covered everywhere.

def word(n, unit=b"abcd"):
    """n bytes of the unit repeated"""
    return (unit * (n // len(unit) + 1))[:n]


LONG = word(90, b"the")          # certainly a long piece: a line that holds it is on new ground under every prepend scheme


def across(at, n=80, unit=b"abcd", lead=30):
    """a line whose long piece of n bytes starts `lead` bytes in front of byte offset `at` of the line"""
    head = (b"the " * 100)[: at - lead - 1] + b" "
    line = head + word(n, unit) + b" fox"
    assert len(head) == at - lead and n > lead
    return line


LONG_VOCAB_PIECE = "abcdefghij" * 7      # 70 bytes: longer than a wave has lanes, longer than the old limit


def long_vocab():
    return U.build_vocab() + [(LONG_VOCAB_PIECE, -5.0)]


NAMED = {}
for _m in (64, 65, 66):          # the measure (the space counted) at the old limit and just over it; LONG keeps the line on new ground
    NAMED["measure_%d_first" % _m] = word(_m - 1) + b" fox " + LONG             # (one less under `never`)
    NAMED["measure_%d_first_no_r" % _m] = word(_m) + b" fox " + LONG            # (the measure under `never`, one more otherwise)
    NAMED["measure_%d_middle" % _m] = b"the " + word(_m - 1) + b" fox " + LONG
    NAMED["measure_%d_last" % _m] = LONG + b" the " + word(_m - 1)
NAMED.update({
    "exactly_2048_middle": b"the " + word(2047) + b" fox",
    "exactly_2048_last": b"the " + word(2047, b"mno"),
    "exactly_2048_first": word(2047) + b" x",                                     # with a prepended R; 2047 under `never`
    "flag_2049_middle": b"the " + word(2048) + b" fox",
    "flag_2049_last": b"the " + word(2048),
    "flag_2050_first": word(2050) + b" x",
    "flag_5000_one_piece": word(5000, b"the"),
    "across_64": across(64), "across_128": across(128), "across_256": across(256), "across_320": across(320),
    "across_64_from_63": across(64, lead=1), "across_256_long": across(256, n=700, unit=b"mnothe"),
    "two_long_pieces": b"the " + word(70) + b" " + word(130, b"xy") + b" fox",
    "two_long_pieces_touching_lines_end": word(100, b"mno") + b" " + word(65),
    "long_against_short": b"a " + word(70) + b" b x " + word(66, b"the") + b" a",
    "long_between_doubled_spaces": b"the  " + word(70) + b"  fox",
    "tie_xy_40": b"the " + b"xy" * 40,
    "tie_xy_40_first": b"xy" * 40,
    "last_bits_mno_30": b"a " + b"mno" * 30,
    "last_bits_mno_30_first": b"mno" * 30 + b" mnomno",
    "viterbi_abcd_20": b"the " + b"abcd" * 20,
    "viterbi_abcd_20_first": b"abcd" * 20 + b" abcd",
    "words_of_pieces": b"see " + b"thesearchtextfoxesing" * 9,
    "unk_run_130": b"the " + b"z" * 130 + b" fox",
    "unk_run_130_between": b"a" + b"z" * 130 + b"b the",
    "unk_runs_and_pieces": b"the " + (b"zz" + b"the" + b"q") * 30,
    "qu_covers_q": b"the " + b"qu" * 40,                                        # q has no piece of its own, qu covers it: no unknown on the path
    "unk_base64_like": b"see " + b"QUJD" * 40,
    "unk_url_like": b"see https://example.org/search/text/" + b"a1b2" * 20 + b".the?x=12 fox",
    "unk_dropped_inside": b"the " + b"ab\x01cd\x7f" * 15 + b" fox",               # dropped under bert_clean, unknown characters otherwise
    "unk_300_dropped": b"the " + b"\x01\x02" * 150 + b" fox",                     # under bert_clean: R alone
    "unk_300_dropped_first": b"\x01" * 300,                                       # under bert_clean: R alone, or nothing under `never`
    "unk_300_dropped_then_space": b"\x02" * 300 + b" the",
    "tab_inside": b"the " + word(70) + b"\t" + word(70),                          # one piece under none (the tab is a piece), two under bert_clean
    "upper": b"the " + b"THEAB" * 16,
})
# (vocabulary with one piece of 70 bytes) the piece straddles position 64 of its long piece, stands at its start, and is cut one short
NAMED_LONG_VOCAB = {
    "piece_70_across_64": b"the " + b"xy" * 20 + LONG_VOCAB_PIECE.encode() + b"mno" * 5,
    "piece_70_first": LONG_VOCAB_PIECE.encode() + b"the",
    "piece_70_twice": b"a " + LONG_VOCAB_PIECE.encode() * 2,
    "piece_70_one_short": b"the " + b"xy" * 20 + LONG_VOCAB_PIECE.encode()[:-1] + b" " + LONG_VOCAB_PIECE.encode()[1:] * 2,
}
# (line, keep_bytes): the cut at the old limit, one over, and inside a long piece
CUTS = [(b"the " + b"a" * 100, 4 + 64), (b"the " + b"a" * 100, 4 + 65), (b"the " + b"abcd" * 100, 4 + 90), (word(300, b"xy"), 130),
        (b"the " + word(3000), 4 + 2047), (b"the " + word(3000), 4 + 2048)]

HANGUL = G.HANGUL
NAMED_UTF8 = {
    "cjk_22": "中文" * 11,                                                    # 66 raw bytes: FLAG under handle_chinese_chars
    "cjk_22_behind_space": "the " + "中文" * 11 + " 中",
    "cjk_300": "the " + "中文中" * 100,
    "hangul_24": "the " + HANGUL * 12,                                            # under NFD: jamo, three nodes per syllable, across position 64
    "hangul_first": HANGUL * 11 + " " + HANGUL,
    "hangul_odd_offset": "a " + "x" + HANGUL * 30,
    "two_byte": "the " + "привет" * 6 + " мир",
    "two_byte_tie": "the " + "дж" * 20,
    "two_byte_first_odd": "a" + "мир" * 12,
    "unk_three_byte": "the " + "か" * 30,
    "four_byte": "the " + "\U0001f600" * 20,
    "cjk_mixed_widths": "the " + "aé中\U0001f600мир" * 8,
    "accents": "see " + "caféétéüber" * 6,                       # under NFD + StripAccents the marks drop
    "unk_ideographic_space": "the\u3000" + word(70).decode() + "\u3000fox",       # a SPACE of three bytes counted as one under bert_clean
    "unk_ideographic_space_measure_64": "the\u3000" + word(63).decode() + "\u3000" + word(64).decode() + " " + LONG.decode(),
    "unk_nbsp": "the\u00a0" + word(64).decode(),
    "literal_replacement": "the" + R + word(70).decode() + R + "fox",
    "unk_dropped_zwsp": "the " + "ab\u200bcd" * 12 + " fox",                      # U+200B: dropped by clean_text
    "unk_dropped_marks": "the " + "é" * 30,
    "unk_300_dropped": "the " + "\u200b" * 100 + " fox",
    "blocks_codepoint": "the " + word(70).decode() + "ก" + word(10).decode() + " fox",       # U+0E01: in no range of BLOCKS
    "blocks_codepoint_early": "the " + word(10).decode() + "ก" + word(70).decode(),
}
NAMED_UTF8 = {k: v.encode() for k, v in NAMED_UTF8.items()}
# every malformed form as the LAST bytes of a line, inside a long piece (the next line follows directly when packed), and in its middle
for _k, _v in G.MALFORMED.items():
    NAMED_UTF8["flag_" + _k] = b"the " + word(70) + _v[4:]
    NAMED_UTF8["flag_" + _k + "_inside"] = b"the " + word(70) + _v[4:] + word(70, b"mno")
NAMED_UTF8["flag_fourth_continuation_inside"] = b"the " + word(70) + "é".encode() + b"\x80" + word(70, b"mno")
# (line, keep_bytes): a non-ASCII line longer than keep_bytes is flagged as ever; one that fits is not
CUTS_UTF8 = [(("the " + "мир" * 30).encode(), 100), (("the " + "мир" * 30).encode(), 184), (b"the " + word(200) + "мир".encode(), 150)]

KNOWN_WORDS = ["the", "fox", "search", "text", "abcd", "abc", "xy", "mno", "nomn", "a", "x", "bathe", "12", "er,", "foxes", "mn", "no", "theing"]
KNOWN_UTF8_WORDS = ["привет", "мир", "примир", "дж", "дждж", "вет", HANGUL, HANGUL[0], "\U0001f600", "λογος"]
UNKNOWN_BITS = ["z", "q", "zq", "7", "(", "/", ":", "_", "-", "%"]
UTF8_BITS = ["café", "Café", "été", "Über", "naïve", "Привет", "か", "かな", "ΛΟΓΟΣ", "ß", "café"]


def long_lines(seed, n, utf8=False, known_only=False):
    """n lines (bytes); each holds at least one piece of 65 .. 300 raw bytes built of vocabulary words (and, unless known_only,
    characters without a piece), among short words; one line in eight holds a piece of up to 2000 bytes.  No byte the ASCII byte
    maps drop or turn into a space, no CJK character, no first byte of an added token."""
    rng = random.Random(seed)
    bits = list(KNOWN_WORDS) + (KNOWN_UTF8_WORDS if utf8 else [])
    if not known_only:
        bits += UNKNOWN_BITS + U.WORDS + (UTF8_BITS if utf8 else [])

    def long_word(lo, hi):
        want, w = rng.randint(lo, hi), ""
        while len(w.encode()) < want:
            w += rng.choice(bits)
        return w

    out = []
    while len(out) < n:
        parts = [rng.choice(KNOWN_WORDS) for _ in range(rng.randint(0, 8))]
        for _ in range(rng.randint(1, 3)):
            parts.insert(rng.randrange(len(parts) + 1), long_word(66, 300))
        if len(out) % 8 == 7:
            parts.insert(rng.randrange(len(parts) + 1), long_word(600, 2000))
        out.append(rng.choice([" ", " ", "  "]).join(parts).encode())
    return out


def many_pieces(n_lines=100, per_line=30):
    """n_lines * per_line long pieces of 65 .. 72 raw bytes: more than the long-piece kernel has blocks"""
    units = [b"abcd", b"xy", b"mno", b"the", b"searchtext"]
    return [b" ".join(word(64 + (i + j) % 8, units[(i * 7 + j) % len(units)]) for j in range(per_line)) for i in range(n_lines)]
