"""Plain-Python restatement of what a UTF-8 line becomes under a per-character normalizer -> Metaspace -> Unigram, and of which lines
the device tokenizer's UTF-8 form covers (DESIGN 4.9 "Unigram over UTF-8 lines").  Written from the rules -- `unicodedata` for
categories, canonical decomposition and combining class -- not from hf_tokenizer.cpp's tables, so the two can disagree.  The
normalizer runs over the WHOLE line in `normalize`; `classify` states the per-code-point answer the device table is built from, the
encoder works from that answer, and tests/test_unigram_utf8_ref_cpu.py asserts that the two agree on covered lines.  Extends
tests/unigram_ref.py by import: the lattice (UnigramRef.piece, which PULLS where the kernel pushes), the ASCII byte map, the ASCII
vocabulary and named lines are that module's.

Also here: the code-point range builder of the kernel-level tests, a vocabulary with non-ASCII pieces, the named lines, and a seeded
generator of mixed-script lines drawn from code points Unicode 3.2 already assigns."""
import functools
import random
import unicodedata

from tests import unigram_ref as U
from tests import wordpiece_utf8_ref as W8

R = U.R
MAX_WORD = U.MAX_WORD
ORDINARY, SPACE, ALONE, DROPPED, FLAG = 0, 1, 2, 3, 4
NORMALIZERS = U.NORMALIZERS
NORMS = ["none", "lower", "bert_clean", "bert_noclean", "seq"]
PREPEND = U.PREPEND
# the code points >= U+0080 the kernel-level tests give the device a statement for (everything else is in no range: FLAG); the
# replacement character's own code point is among them
BLOCKS = tuple(sorted(list(W8.BLOCKS) + [(ord(R), ord(R))]))


def _norm_of(norm):
    return NORMALIZERS[norm] if isinstance(norm, str) else norm


def has_nfd(n):
    """NFD in the chain, directly or through BertNormalizer's strip_accents (None follows lowercase)"""
    if n is None:
        return False
    t = n["type"]
    if t == "NFD":
        return True
    if t == "BertNormalizer":
        sa = n.get("strip_accents")
        return n.get("lowercase", True) if sa is None else bool(sa)
    if t == "Sequence":
        return any(has_nfd(c) for c in n["normalizers"])
    return False


def normalize(s, n):
    """a normalizer (a tokenizer.json dict or None) over a whole str"""
    if n is None:
        return s
    t = n["type"]
    if t == "Sequence":
        for c in n["normalizers"]:
            s = normalize(s, c)
        return s
    if t == "Lowercase":
        return "".join(ch.lower() for ch in s)                    # per character: no Final_Sigma context
    if t == "NFD":
        return unicodedata.normalize("NFD", s)
    if t == "StripAccents":
        return "".join(ch for ch in s if unicodedata.category(ch) != "Mn")
    if t == "BertNormalizer":
        if n.get("clean_text", True):
            out = []
            for ch in s:
                if ch in "\t\n\r":
                    out.append(" ")
                elif ord(ch) == 0 or ord(ch) == 0xFFFD or unicodedata.category(ch).startswith("C"):
                    continue
                else:
                    out.append(" " if W8.is_white_space(ch) else ch)
            s = "".join(out)
        if n.get("handle_chinese_chars", True):
            s = "".join(" " + ch + " " if W8.is_chinese_char(ch) else ch for ch in s)
        if has_nfd(n):
            s = "".join(ch for ch in unicodedata.normalize("NFD", s) if unicodedata.category(ch) != "Mn")
        if n.get("lowercase", True):
            s = "".join(ch.lower() for ch in s)
        return s
    raise ValueError(t)


@functools.lru_cache(maxsize=None)
def classify(cp, norm, rep=R):
    """(class, output) of one code point >= U+0080 under NORMALIZERS[norm]: what the device table says.  output "": itself (or
    none, for SPACE / DROPPED / FLAG)"""
    return classify_under(cp, _norm_of(norm), rep)


def classify_under(cp, n, rep=R):
    """classify() for a normalizer given as a tokenizer.json dict (or None)"""
    ch = chr(cp)
    s = normalize(ch, n)
    if s == "":
        return DROPPED, ""
    if s == " " or s == rep:
        return SPACE, ""                                           # (Metaspace splits at a literal replacement as at a replaced space)
    if " " in s or rep in s:
        return FLAG, ""                                            # a Chinese character between its two spaces
    if len(s) > len(ch.encode()):
        return FLAG, ""
    if has_nfd(n) and any(unicodedata.combining(c) for c in s):
        return FLAG, ""
    return ORDINARY, "" if s == ch else s


@functools.lru_cache(maxsize=None)
def codepoint_ranges(norm, blocks=BLOCKS, rep=R):
    """[(first, last, class, output)] over `blocks`: equal neighbours merged, FLAG code points left out (no range: FLAG)"""
    out = []
    for a, b in blocks:
        for cp in range(a, b + 1):
            if 0xD800 <= cp <= 0xDFFF:
                continue
            k, o = classify(cp, norm, rep)
            if k == FLAG:
                continue
            if out and o == "" and out[-1][3] == "" and out[-1][2] == k and out[-1][1] + 1 == cp:
                out[-1] = (out[-1][0], cp, k, "")
            else:
                out.append((cp, cp, k, o))
    return out


# conjoining jamo, as NFD makes them of 한글: h a n | g eu l
JAMO = dict(h="ᄒ", a="ᅡ", n="ᆫ", g="ᄀ", eu="ᅳ", l="ᆯ")


def build_vocab():
    """unigram_ref.build_vocab() (the ids stay) + non-ASCII pieces: accented and Cyrillic words with and without R; the six jamo of
    한글 alone, the pair h+a, and the pair n+g that runs from INSIDE the first syllable into the second (the best path of the word under
    NFD ends a piece between two jamo of one syllable); the two syllables precomposed; CJK characters alone and as a word; a repeated
    Cyrillic piece whose first entry would lose; the tie of xy in Cyrillic (R+д, ж = -7 = R, дж: the smaller start of the last edge
    wins: R, дж); a 4-byte character.  No score below the lowest of the ASCII vocabulary: the unknown's cost stays."""
    v = list(U.build_vocab())
    v += [("café", -4.5), (R + "cafe", -3.8), ("cafe", -4.2), ("été", -4.0), (R + "über", -3.0), (R + "uber", -3.1), ("ü", -5.0), ("ï", -5.0)]
    v += [("мир", -9.0)]
    v += [(c, -5.0) for c in "приветмй"] + [("М", -5.5), ("П", -5.5)]
    v += [(R + "привет", -3.0), ("привет", -4.0), ("мир", -3.5), (R + "мир", -3.0), ("вет", -3.2), (R + "при", -3.3)]
    v += [(R + "д", -3.0), ("дж", -5.0), ("д", -4.0), ("ж", -4.0)]
    v += [(JAMO[k], -5.0) for k in ("h", "a", "n", "g", "eu", "l")]
    v += [(JAMO["h"] + JAMO["a"], -4.0), (JAMO["n"] + JAMO["g"], -3.0), ("한", -4.0), ("글", -4.0), (R + "한글", -3.0)]
    v += [("中", -4.0), ("文", -4.0), ("中文", -3.0), (R + "中文", -2.5)]
    v += [("\U0001f600", -5.0), (R + "\U0001f600", -4.0), ("λ", -5.0), ("ο", -5.0), ("σ", -5.0), ("ς", -5.0), ("γ", -5.0), ("Λ", -5.5)]
    assert min(s for _, s in v) == min(s for _, s in U.build_vocab())
    return v


def tokenizer_json(norm="none", prepend="always", unk_id=0, vocab=None, **kw):
    return U.tokenizer_json(norm=norm, prepend=prepend, unk_id=unk_id, vocab=vocab or build_vocab(), **kw)


class UnigramUtf8Ref(U.UnigramRef):
    """blocks: the code points the device table covers (None: all of them, as the host layer's export)"""

    def __init__(self, tj, blocks=BLOCKS):
        super().__init__(tj)
        self.norm = tj.get("normalizer")
        self.blocks = blocks
        self._cls = {}

    def cp_class(self, cp):
        """(class, output) of a code point >= U+0080 as the device table has it"""
        got = self._cls.get(cp)
        if got is None:
            if self.blocks is not None and not any(a <= cp <= b for a, b in self.blocks):
                got = (FLAG, "")
            else:
                k, o = classify_under(cp, self.norm, self.rep)
                got = (k, o if o or k != ORDINARY else chr(cp))
            self._cls[cp] = got
        return got

    def units(self, raw):
        """[(source bytes, class, output characters)] of a line's characters, or None: an added token, malformed UTF-8 (strict:
        overlong forms, surrogates and values above U+10FFFF are errors) or a FLAG code point"""
        if any(a in raw for a in self.added):
            return None
        try:
            s = raw.decode("utf-8")
        except UnicodeDecodeError:
            return None
        out = []
        for ch in s:
            cp = ord(ch)
            if cp < 0x80:
                m = self.map[cp]
                out.append((1, DROPPED, "") if m is None else (1, SPACE, "") if m == 0x20 else (1, ORDINARY, chr(m)))
            else:
                k, o = self.cp_class(cp)
                if k == FLAG:
                    return None
                out.append((len(ch.encode()), k, o))
        return out

    def covered(self, raw):
        return self.units(raw) is not None

    def encode(self, raw, check_limit=True):
        """ids of a line (bytes), or None when the line is flagged"""
        units = self.units(raw)
        if units is None:
            return None
        if not raw:
            return []
        if check_limit:                       # the raw bytes between two SPACE characters, that character counted as ONE
            seg, k = 0, 0
            for src, cls, _ in units:
                if cls == SPACE:
                    k, seg = k + 1, 1
                else:
                    seg += src
                if seg + (1 if k == 0 and self.prepend != "never" else 0) > MAX_WORD:
                    return None
        text = []
        for _, cls, o in units:
            if cls == SPACE:
                text.append(self.rep)
            elif cls == ORDINARY:
                text.extend(o)
        if self.prepend != "never" and (not text or text[0] != self.rep):
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

    def line(self, raw, keep_bytes=0, max_tokens=0, drop_unk=True):
        """-> (ids, flagged) after truncate -> encode -> unk drop -> cap.  A line longer than keep_bytes is cut by BYTES, and flagged
        when the kept part holds a byte >= 0x80 (the host layer cuts by characters)"""
        if keep_bytes and len(raw) > keep_bytes:
            raw = raw[:keep_bytes]
            if any(c >= 0x80 for c in raw):
                return [], True
        ids = self.encode(raw)
        if ids is None:
            return [], True
        if drop_unk and self.unk is not None:
            ids = [t for t in ids if t != self.unk]
        if max_tokens:
            ids = ids[:max_tokens]
        return ids, False



def _straddle(ch, at, before, after=""):
    """a line in which the lead byte of `ch` stands at byte offset at - 1 and its continuation bytes from `at`: 'the ' words, then
    `before` + ch + `after` as one word"""
    head = (b"the " * 80)[: at - 1 - len(before.encode()) - 1] + b" "
    line = head + (before + ch + after).encode() + b" the fox"
    assert line[at - 1] == ch.encode()[0] and len(head) + len(before.encode()) == at - 1
    return line


HANGUL = "한글"
NAMED = {
    "empty": b"",
    "accented": "the café fox".encode(),
    "accented_upper": "CAFÉ Über été".encode(),
    "cyrillic": "привет мир Привет Мир".encode(),
    "cyrillic_repeated_piece": "мир вмир".encode(),
    "cyrillic_tie": "дж a дждж".encode(),
    "cyrillic_viterbi": "приветик примир".encode(),
    "hangul": HANGUL.encode(),                                     # under NFD: R, h+a, n+g, eu, l -- a piece ends inside each syllable
    "hangul_inner": ("the " + HANGUL + " " + HANGUL[0] + " fox").encode(),
    "jamo_literal": (JAMO["h"] + JAMO["a"] + JAMO["n"] + JAMO["g"]).encode(),
    "cjk": "中文 the 中 文中文".encode(),      # FLAG under handle_chinese_chars
    "four_byte": "the \U0001f600 \U0001f600\U0001f600 fox".encode(),
    "unknown_3byte": "か".encode(),
    "unknown_3byte_pair": "かな".encode(),                 # two unknowns fuse into one unk
    "unknown_between": "aかなb the".encode(),
    "literal_replacement": ("the" + R + "fox " + R + R + "a").encode(),
    "replacement_first": (R + "the fox").encode(),
    "nbsp": "the\u00a0fox".encode(),                               # a space under bert_clean, an ordinary (unknown) character under none
    "ideographic_space": "the\u3000fox".encode(),                  # a 3-byte SPACE under bert_clean
    "dropped_zwsp": "th\u200be fox".encode(),                      # U+200B: Cf, dropped by clean_text
    "dropped_mark": "the\u0301 fo\u0308x".encode(),                # combining marks: dropped by StripAccents, ordinary without it
    "greek_sigma": "ΛΟΓΟΣ λογος".encode(),
    # the measure: raw bytes against SMT_UG_MAX_WORD, the SPACE character counted as one
    "exactly_max_word": ("the " + "м" * 30 + "abc fox").encode(),                 # 1 + 63 raw bytes
    "exactly_max_word_multibyte": ("the " + "か" * 21 + " fox").encode(),          # 1 + 63 raw bytes of 3-byte characters
    "max_word_plus_one": ("the " + "м" * 32 + " fox").encode(),                   # 1 + 64: flagged
    "max_word_plus_one_byte": ("the " + "м" * 30 + "abcd fox").encode(),
    "max_word_behind_nbsp": ("the\u00a0" + "м" * 30 + "abc fox").encode(),      # (63 bytes behind a 2-byte character)
    "max_word_behind_ideographic_space": ("the\u3000" + "м" * 30 + "abc fox").encode(),
    "first_word_at_bound": ("м" * 31 + "a x").encode(),                           # 63 raw bytes: at the bound with a prepended R
    "first_word_at_bound_never": ("м" * 32 + " x").encode(),                      # 64: flagged unless the scheme is `never`
    "first_word_over": ("м" * 32 + "a x").encode(),                               # 65: flagged always
    "added_token": "мир <pad> мир".encode(),
    "added_token_prefix_only": "мир <pa мир".encode(),
    "flag_codepoint": "the ก fox".encode(),                   # U+0E01: in no range of BLOCKS
}
for _name, _ch in (("2", "é"), ("3", "か"), ("4", "\U0001f600")):
    for _at in (64, 256):
        NAMED["straddle_%s_at_%d_piece_before" % (_name, _at)] = _straddle(_ch, _at, "caf")          # the owner's piece begins in front
        NAMED["straddle_%s_at_%d_piece_after" % (_name, _at)] = _straddle(_ch, _at, "", "the")       # the character follows the space
# every malformed form, as the LAST bytes of a line (the next line follows directly when packed)
MALFORMED = {
    "lone_continuation": b"the \x80",
    "lone_continuation_after_ascii": b"the a\xbf",
    "cut_2": b"the \xc3",
    "cut_3": b"the \xe3\x81",
    "cut_4": b"the \xf0\x9f\x98",
    "overlong_2": b"the \xc0\xaf",
    "overlong_c1": b"the \xc1\xbf",
    "overlong_3": b"the \xe0\x80\xaf",
    "overlong_4": b"the \xf0\x80\x80\xaf",
    "surrogate": b"the \xed\xa0\x80",
    "above_10ffff": b"the \xf4\x90\x80\x80",
    "leads_nothing_f5": b"the \xf5\x80\x80\x80",
    "leads_nothing_ff": b"the \xff",
    "bad_continuation": b"the \xc3\x28",
    "fourth_continuation": "the é".encode() + b"\x80",
}
VALID_NEXT = "été the fox".encode()         # (its first byte is a lead byte: a cut sequence in front of it must not swallow it)
# (line, keep_bytes): the cut at, before and inside a multi-byte character; a non-ASCII line longer than keep_bytes is flagged
CUTS = [("the café fox".encode(), 7), ("the café fox".encode(), 8), ("the café fox".encode(), 9), ("the café".encode(), 9),
        ("the café".encode(), 8), ("the café!".encode(), 9), ("мир мир".encode(), 13), ("мир мир".encode(), 12),
        ("мир мир".encode(), 3), ("the fox мир".encode(), 7), (b"the <pad>", 8), (b"abcd", 3)]

ASCII_WORDS = U.WORDS
UTF8_WORDS = ["café", "Café", "CAFÉ", "cafe\u0301", "été", "Über", "über", "naïve", "привет", "Привет", "мир", "Мир",
              "примир", "ветер", "дж", "дждж", "й", HANGUL, HANGUL[0], HANGUL[1] + "x", "\U0001f600", "ok\U0001f600", "か", "かな",
              "λογος", "ΛΟΓΟΣ", "Σ", "ẞ", "İ", "ß", "ǅx", R + "a", "a" + R + "b"]
CJK_WORDS = ["中文", "中", "文x"]
_GEN_BLOCKS = [(0xA0, 0x24F), (0x300, 0x36F), (0x370, 0x3FF), (0x400, 0x4FF), (0x2000, 0x206F), (0x2600, 0x26FF), (0x3040, 0x30FF),
               (0xAC00, 0xD7A3), (0x1D400, 0x1D7FF)]
SEPS = [" ", "  ", "\t", " ", "\n", "\u00a0", "\u3000", " ", "\u2003"]


@functools.lru_cache(maxsize=None)
def _gen_pools():
    old = unicodedata.ucd_3_2_0
    return [[chr(c) for c in range(a, b + 1) if old.category(chr(c)) != "Cn"] for a, b in _GEN_BLOCKS]


def utf8_lines(seed, n):
    """n lines (bytes) of mixed scripts: words of the vocabulary's scripts joined by ASCII and Unicode white space (one line in
    twenty with a CJK word, which the Bert chains flag); words drawn from one block each, at most 8 characters; every fourth line
    pure ASCII.  The pool holds no code point the reference flags under a chain without handle_chinese_chars, and no word comes near
    SMT_UG_MAX_WORD raw bytes: the CPU test checks that the reference flags at most one line in ten."""
    rng = random.Random(seed)
    pools = _gen_pools()
    out = []
    while len(out) < n:
        parts = [rng.choice(UTF8_WORDS) if rng.random() < 0.5 else rng.choice(ASCII_WORDS) for _ in range(rng.randint(1, 12))]
        if rng.random() < 0.05:
            parts.insert(rng.randrange(len(parts) + 1), rng.choice(CJK_WORDS))
        out.append(rng.choice(SEPS).join(parts).encode())
        words = []
        for _ in range(rng.randint(1, 8)):
            blk = rng.choice(pools)
            words.append("".join(rng.choice(blk) if rng.random() < 0.7 else rng.choice("abcdexy") for _ in range(rng.randint(1, 8))))
        out.append(" ".join(words).encode())
        blk = rng.choice(pools)
        out.append(rng.choice(SEPS).join("".join(rng.choice(blk) for _ in range(rng.randint(1, 6))) for _ in range(rng.randint(1, 8))).encode())
        out.append(U.ascii_lines(rng.randrange(1 << 30), 1, pool=U.SAFE_POOL, seps=(" ", "  "))[0])
    return out[:n]

