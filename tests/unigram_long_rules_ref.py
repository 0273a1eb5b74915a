"""Plain-Python restatement of the Unigram device tokenizer with long pieces on UNDER THE SPACE RULES (DESIGN 4.9 "long pieces under
the space rules", smt_unigram_set_long_rules): tests/precompiled_ref.py's PrecompiledRef with the piece limit a parameter (`max_long`)
and tests/unigram_long_ref.py's windowed lattice.  Written from the rules:

  the measure     of a piece is its raw bytes, the owner's SPACE character (or the prepended R of the line's first piece) counted
                  as one; under collapse_runs an absorbed space counts its raw bytes like a dropped character.  Over max_long: flagged.
  the look-back   a SPACE character with more than MAX_WORD raw bytes of dropped characters directly in front of it flags the line,
                  whatever the limit: a bound of the device form, implied by the measure while the limit was MAX_WORD.
  drop_trailing   a piece without a kept character at the line's end emits nothing, whatever its length; as the line's only piece it
                  flags the line.
  stats()         what smt_unigram_long_stats counts: the pieces measured to their end within the limit, each with its measure --
                  a piece drop_trailing leaves without a token among them.

Also here: the vocabulary (precompiled_ref.build_vocab() joined with unigram_long_ref.long_vocab()), the named lines, the reference
variants that are wrong on purpose, and a seeded generator."""
import random

from tests import precompiled_ref as P
from tests import unigram_long_ref as LR
from tests import unigram_ref as U

R = P.R
MAX_WORD = P.MAX_WORD
MAX_LONG = LR.MAX_LONG
SPACE, DROPPED, ORDINARY = P.SPACE, P.DROPPED, P.ORDINARY
# what a reference may get wrong on purpose (tests/test_unigram_long_rules_ref_cpu.py: each fails on the named lines)
WRONG = ("absorbed_not_measured", "trailing_r_emitted", "tie_largest", "skip_stops_at_dropped")


def build_vocab():
    v = list(P.build_vocab())
    return v + [x for x in LR.long_vocab() if x not in v]


def tokenizer_json(shape="A_ws", **kw):
    return P.tokenizer_json(shape, vocab=build_vocab(), **kw)


class LongRulesRef(LR._Long, P.PrecompiledRef):
    def __init__(self, tj, collapse_runs=None, drop_trailing=None, utf8=True, max_long=MAX_LONG, wrong=None):
        super().__init__(tj, collapse_runs=collapse_runs, drop_trailing=drop_trailing, utf8=utf8)
        assert wrong is None or wrong in WRONG
        self.max_long = max_long
        self.mistake = wrong
        self.wrong = {"tie_largest": True} if wrong == "tie_largest" else {}

    def _walk(self, units):
        """-> (the measures of the line's pieces, the normalised text as a list of characters, whether the look-back bound is passed)"""
        measures, text, prev_space, back, far = [1], [], False, 0, False          # (the first piece's prepended R counts one)
        for src, cls, o in units:
            if cls == SPACE:
                far = far or back > MAX_WORD
            if cls == SPACE and not (self.collapse and prev_space):
                measures.append(1)
                text.append(self.rep)
            elif not (cls == SPACE and self.mistake == "absorbed_not_measured"):
                measures[-1] += src                   # an absorbed space counts like a dropped character: its raw bytes
            if cls == ORDINARY:
                text.extend(o)
            back = back + src if cls == DROPPED else 0
            if cls != DROPPED or self.mistake == "skip_stops_at_dropped":
                prev_space = cls == SPACE
        return measures, text, far

    def measures(self, raw):
        units = self.units(raw)
        return None if units is None else self._walk(units)[0]

    def encode(self, raw, check_limit=True):
        """ids of a line (bytes) under the space rules with the limit max_long, or None when the line is flagged"""
        units = self.units(raw)
        if units is None:
            return None
        if not raw:
            return []
        measures, text, far = self._walk(units)
        if check_limit and (far or max(measures) > self.max_long):
            return None
        if self.drop_trailing and (not text or text[-1] == self.rep):
            if len(text) <= 1:
                return None                           # the line's only piece: the host's
            if self.mistake != "trailing_r_emitted":
                text.pop()
        if not text or text[0] != self.rep:
            text.insert(0, self.rep)
        pieces = []
        for ch in text:
            if ch == self.rep or not pieces:
                pieces.append([])
            pieces[-1].append(ch)
        ids = []
        try:
            for p in pieces:
                self.piece(p, ids)
        except U.Flagged:
            return None
        return ids


# ---- the named lines.  A name that starts with "flag_" is flagged under every rule combination and both forms.
word = LR.word
D = b"\x01"                       # an ASCII control: the character map drops it
HEAD = b"the " * 55               # 220 bytes, the last a space: what follows starts 36 bytes in front of the 256-byte block border
NAMED = {}
for _m in (64, 65, 66):           # the measure (the space, or the prepended R, counted) at the old limit and just over it
    NAMED["measure_%d_behind_space" % _m] = b"the " + word(_m - 1) + b" fox"
    NAMED["measure_%d_first" % _m] = word(_m - 1) + b" fox"
    NAMED["measure_%d_last" % _m] = b"the " + word(_m - 1, b"mno")
for _n in range(62, 71):          # 1 + (n - 1) absorbed + 3: the measure passes 64 in the absorbed run, or just behind it
    NAMED["run_%d_abc" % _n] = b"the" + b" " * _n + b"abc fox"
NAMED.update({
    "exactly_2048_middle": b"the " + word(2047) + b" fox",
    "exactly_2048_last": b"the " + word(2047, b"mno"),
    "exactly_2048_first": word(2047) + b" x",
    "flag_2049_middle": b"the " + word(2048) + b" fox",
    "flag_2049_first": word(2048) + b" x",
    "exactly_2048_through_absorbed": b"the" + b" " * 1000 + word(1048) + b" fox",     # 1 + 999 + 1048 under collapse_runs
    "over_2048_through_absorbed_only": b"the" + b" " * 1001 + word(1048) + b" fox",   # 2049 under collapse_runs, 1049 without
    "over_2048_absorbed_alone": b"the" + b" " * 2100 + b"fox",                        # the skip phase passes the limit on its own
    "spaces_65_a": b" " * 65 + b"a",
    "spaces_64_a": b" " * 64 + b"a",
    "run_with_dropped_80": b"the " + (D + b" \x02\x03  ") * 8 + word(80) + b" fox",
    "run_with_dropped_ends_dropped": b"the " + (b"  " + D) * 30 + word(70, b"xy") + b" a",
    "trailing_70": b"the fox" + b" " * 70,                     # nothing, or R
    "trailing_70_dropped": b"the fox " + (D + b" ") * 40,
    "spaces_70": b" " * 70,                                    # flagged under drop_trailing, the lone R without it
    "dropped_70": D * 70,                                      # the line's first piece, nothing kept: flagged under drop_trailing
    "dropped_63_space": b"the " + D * 63 + b" fox",            # the look-back bound: inside,
    "dropped_64_space": b"the " + D * 64 + b" fox",            # at,
    "flag_dropped_70_space": b"the " + D * 70 + b" fox",       # and beyond it
    "flag_dropped_70_first_space": D * 70 + b" the",
    "dropped_64_first_space": D * 64 + b" the",
    "dropped_70_no_space_behind": b"the " + D * 70 + b"fox",   # no SPACE looks back over them
    "piece_across_256": HEAD + word(80) + b" fox",
    "piece_700_across_256": HEAD + word(700, b"mnothe") + b" fox",
    "run_across_256": HEAD + b" " * 79 + b"abcd fox",
    "run_and_piece_across_256": HEAD[:-20] + b" " * 30 + word(90, b"the") + b" fox",
    "two_long_pieces": b"the  " + word(70) + b"   " + word(130, b"xy") + b"  fox",
    "tie_xy_40": b"the  " + b"xy" * 40,                        # the words of unigram_long_ref behind a doubled space
    "viterbi_abcd_20": b"the  " + b"abcd" * 20,
    "last_bits_mno_30": b"a  " + b"mno" * 30,
    "words_of_pieces": b"see  " + b"thesearchtextfoxesing" * 9,
    "unk_run_130": b"the  " + b"z" * 130 + b"  fox",
    "qu_covers_q": b"the  " + b"qu" * 40,
    "piece_70_across_64": b"the  " + b"xy" * 20 + LR.LONG_VOCAB_PIECE.encode() + b"mno" * 5,
    "piece_70_twice": b"a  " + LR.LONG_VOCAB_PIECE.encode() * 2,
    "url": b"see  https://example.org/search/text/" + b"a1b2" * 20 + b".the?x=12  fox",
    "tab_inside": b"the " + word(70) + b"\t" + word(70),
})
NAMED_UTF8 = {
    "ideographic_22": "the" + "　" * 22 + "ｆｕｌｌ",                     # 66 raw bytes of absorbed 3-byte spaces
    "ideographic_30_mixed": "the" + "　  " * 10 + "fox",
    "cyrillic_72": "the  " + "привет" * 6 + " мир",
    "cyrillic_tie": "the  " + "дж" * 20,
    "cjk_30": "  " + "中文" * 5,
    "cjk_66": "中文" * 11 + "  ",
    "cjk_198": "  " + "中文中" * 22 + "  ",
    "cjk_600": "  " + "中文" * 100 + "  ",
    "cjk_behind_words": "the fox  " + "文中" * 40 + "  text",
    "hangul_72": "the  " + "한글" * 12,
    "fullwidth_90": "a  " + "ｆｕｌｌ" * 8 + " b",
    "flag_mark_inside": "the " + word(70).decode() + "é" + word(10).decode(),        # a FLAG code point inside a long piece
    "flag_mark_in_the_run": "the" + " " * 70 + "́abc",                                # ... and behind an absorbed run
    "flag_zwj_inside": "the  " + word(100).decode() + "‍" + "fox",
}
NAMED_UTF8 = {k: v.encode() for k, v in NAMED_UTF8.items()}
NAMED_UTF8.update({
    "flag_lone_continuation_inside": b"the " + word(70) + b"\x80" + word(10, b"mno"),
    "flag_cut_2_at_the_end": b"the  " + word(70) + b"\xc3",
    "flag_cut_3_inside": b"the " + word(70) + b"\xe3\x81" + word(70, b"mno"),
    "flag_malformed_in_the_run": b"the" + b" " * 70 + b"\xc0\xaf fox",
    "flag_fourth_continuation": b"the " + word(70) + "é".encode() + b"\x80" + word(70, b"mno"),
})
# (line, keep_bytes): the looked-at end inside a long absorbed run, just behind it, and inside the long piece behind it
_CUT = b"the" + b" " * 100 + word(100) + b" fox"
CUTS = [(_CUT, 3 + 50), (_CUT, 3 + 64), (_CUT, 3 + 65), (_CUT, 3 + 100), (_CUT, 3 + 101), (_CUT, 3 + 140), (_CUT, 3 + 200), (_CUT, 3 + 201),
        (b"the " + word(3000), 4 + 2047), (b"the " + word(3000), 4 + 2048), (HEAD + b" " * 79 + b"abcd fox", 256), (HEAD + word(80) + b" fox", 257)]


def covered_only(names=None):
    """the named lines (both dicts) that hold a long piece and only covered characters: every form and rule combination that knows
    long pieces tokenizes them -- tests/test_gpu_unigram_long_rules.py: the test that fails without the feature"""
    pick = ["measure_65_behind_space", "measure_66_first", "measure_66_last", "exactly_2048_middle", "run_with_dropped_80", "piece_across_256",
            "two_long_pieces", "tie_xy_40", "viterbi_abcd_20", "piece_70_twice", "url"]
    return {k: NAMED[k] for k in (names or pick)}


_URL_BITS = LR.KNOWN_WORDS + ["a1b2", "-12", "_x", "/", "/", ".", "?x=12"]
_CJK_BITS = ["中文", "中", "文", "中文中", "한글", "カ"]


def lines(seed, n):
    """n lines (bytes): precompiled_ref.lines, and in two lines of five one thing more -- a URL-like word of 65 .. 160 bytes, text of a
    script written without spaces (66 .. 200 bytes), or a run of 64 .. 90 spaces or mixed Unicode spaces in front of a word."""
    rng = random.Random(seed)
    out = []
    for i, raw in enumerate(P.lines(rng.randrange(1 << 30), n)):
        kind = i % 5
        if kind in (1, 3):
            s = raw.decode()
            words = s.split(" ")
            at = rng.randrange(len(words) + 1)
            pick = rng.randrange(3)
            if pick == 0:
                w, want = "https://example.org/", rng.randint(65, 160)
                while len(w) < want:
                    w += rng.choice(_URL_BITS)
            elif pick == 1:
                w, want = "", rng.randint(66, 200)
                while len(w.encode()) < want:
                    w += rng.choice(_CJK_BITS)
            else:
                w = rng.choice([" ", " ", "　", "  "]) * rng.randint(64, 90) + rng.choice(LR.KNOWN_WORDS)
            words.insert(at, w)
            raw = " ".join(words).encode()
        out.append(raw)
    return out
