"""Plain-Python restatement of what a UTF-8 line becomes under BertNormalizer -> BertPreTokenizer -> WordPiece, and of which lines the
device tokenizer's UTF-8 form covers (DESIGN 4.9 "WordPiece over UTF-8 lines").  Written from the rules -- `unicodedata` for
categories, canonical decomposition and combining class, the CJK ranges and the punctuation test of the `tokenizers` crate -- not from
hf_tokenizer.cpp's tables, so the two can disagree.  The normalizer runs over the WHOLE line here; `classify` states the per-code-point
answer the device table is built from, and tests/test_wordpiece_utf8_ref_cpu.py asserts that the two agree on covered lines.

Also here: the code-point range builder of the kernel-level tests, a vocabulary that extends wordpiece_ref.build_vocab() with
non-ASCII pieces, and a seeded generator of mixed lines drawn from code points Unicode 3.2 already assigns (three table versions --
this module's, the host tokenizer's, the `tokenizers` wheel's -- cannot disagree about them)."""
import functools
import random
import unicodedata

import numpy as np

from tests import wordpiece_ref as W

ORDINARY, SPACE, ALONE, DROPPED, FLAG = 0, 1, 2, 3, 4
WHITE_SPACE = set(range(0x9, 0xE)) | {0x20, 0x85, 0xA0, 0x1680} | set(range(0x2000, 0x200B)) | {0x2028, 0x2029, 0x202F, 0x205F, 0x3000}
CJK = [(0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F), (0x2B920, 0x2CEAF), (0xF900, 0xFAFF),
       (0x2F800, 0x2FA1F)]
# the code points >= U+0080 the kernel-level tests give the device a statement for (everything else is in no range: FLAG)
BLOCKS = [(0x80, 0x4FF), (0x1100, 0x11FF), (0x2000, 0x206F), (0x2600, 0x26FF), (0x3000, 0x30FF), (0x4E00, 0x9FFF), (0xAC00, 0xD7A3),
          (0xFFFD, 0xFFFD), (0x1D400, 0x1D7FF), (0x1F600, 0x1F64F), (0x20000, 0x200FF)]


def is_white_space(ch):
    return ord(ch) in WHITE_SPACE


def is_bert_punc(ch):
    return ord(ch) in W.PUNCT or unicodedata.category(ch).startswith("P")


def is_chinese_char(ch):
    return any(a <= ord(ch) <= b for a, b in CJK)


def normalize(s, flags):
    """BertNormalizer over a whole str: clean_text, Chinese characters spaced, strip_accents (follows lowercase), lowercase"""
    if not flags & W.WP_NORMALIZER:
        return s
    if flags & W.WP_CLEAN_TEXT:
        out = []
        for ch in s:
            if ch in "\t\n\r":
                out.append(" ")
            elif ord(ch) == 0 or ord(ch) == 0xFFFD or unicodedata.category(ch).startswith("C"):
                continue                                   # (VT, FF and U+0085 are controls first, white space second: removed)
            else:
                out.append(" " if is_white_space(ch) else ch)
        s = "".join(out)
    s = "".join(" " + ch + " " if is_chinese_char(ch) else ch for ch in s)       # handle_chinese_chars
    if flags & W.WP_LOWERCASE:
        s = "".join(ch for ch in unicodedata.normalize("NFD", s) if unicodedata.category(ch) != "Mn")
        s = "".join(ch.lower() for ch in s)                                          # per character: no Final_Sigma context
    return s


@functools.lru_cache(maxsize=None)
def classify(cp, flags):
    """(class, output) of one code point >= U+0080: what the device table says.  output "": itself (or none, for SPACE / DROPPED / FLAG)"""
    ch = chr(cp)
    s = normalize(ch, flags)
    if s == "":
        return DROPPED, ""
    if len(s) > len(ch.encode()) or any(unicodedata.combining(c) for c in s):
        return FLAG, ""
    core = s.strip("".join(chr(c) for c in WHITE_SPACE))
    if core == "":
        return SPACE, ""
    kinds = {SPACE if is_white_space(c) else ALONE if is_bert_punc(c) else ORDINARY for c in core}
    if core == s:
        if kinds == {ORDINARY}:
            return ORDINARY, "" if s == ch else s
        if kinds == {ALONE} and len(s) == 1:
            return ALONE, "" if s == ch else s
        return FLAG, ""
    if s == " " + core + " " and len(core) == 1 and kinds == {ORDINARY}:
        return ALONE, "" if core == ch else core
    return FLAG, ""


@functools.lru_cache(maxsize=None)
def codepoint_ranges(flags, blocks=tuple(BLOCKS)):
    """[(first, last, class, output)] over `blocks`: equal neighbours merged, FLAG code points left out (no range: FLAG)"""
    out = []
    for a, b in blocks:
        for cp in range(a, b + 1):
            if 0xD800 <= cp <= 0xDFFF:
                continue
            k, o = classify(cp, flags)
            if k == FLAG:
                continue
            if out and o == "" and out[-1][3] == "" and out[-1][2] == k and out[-1][1] + 1 == cp:
                out[-1] = (out[-1][0], cp, k, "")
            else:
                out.append((cp, cp, k, o))
    return out


def build_vocab():
    """wordpiece_ref.build_vocab() + non-ASCII pieces: accented and plain forms, Greek and Cyrillic words and letters, two Chinese
    characters, jamo (so that a syllable's pieces split INSIDE it under strip_accents), Unicode punctuation, a 4-byte emoji"""
    vocab = dict(W.build_vocab())
    pieces = ["café", "cafe", "é", "##é", "e", "naïve", "naive", "über", "uber", "##ï", "##ü",
              "λόγος", "λογος", "λ", "##ο", "##ό", "##γ", "##ς", "##σ", "και", "Λ",
              "привет", "мир", "п", "##р", "##и", "##в", "##е", "##т", "##й", "М", "##ир",
              "中", "文", JAMO_HA, "##" + JAMO_N, "##" + JAMO_N + JAMO_G, "##" + JAMO_EUL, "##" + JAMO_G, "\ud55c", "##\uae00",
              "“", "”", "—", "…", "«", "😀", "##😀", "ok😀", "か", "##な", "𝐀", "##𝐁"]
    for p in pieces:
        if p not in vocab:
            vocab[p] = len(vocab)
    return vocab


class WordPieceUtf8Ref:
    """blocks: the code points the device table covers (None: all of them, as the host layer's export)"""

    def __init__(self, flags, vocab=None, max_chars=W.MAX_CHARS, prefix="##", unk="[UNK]", added=W.ADDED, blocks=tuple(BLOCKS)):
        self.vocab = dict(vocab or build_vocab())
        self.flags, self.max_chars, self.prefix = flags, max_chars, prefix
        self.unk = self.vocab[unk]
        self.added = [a.encode() for a in added]
        self.blocks = blocks

    def cp_class(self, cp):
        if cp < 0x80:
            return None
        if self.blocks is not None and not any(a <= cp <= b for a, b in self.blocks):
            return FLAG
        return classify(cp, self.flags)[0]

    def decode(self, raw):
        """the str of a line, or None: malformed UTF-8 (strict: overlong forms, surrogates and values above U+10FFFF are errors)"""
        try:
            return raw.decode("utf-8")
        except UnicodeDecodeError:
            return None

    def covered(self, raw):
        s = self.decode(raw)
        return s is not None and not any(a in raw for a in self.added) and not any(self.cp_class(ord(ch)) == FLAG for ch in s)

    def word(self, w, ids):
        if len(w) > self.max_chars:
            ids.append(self.unk)
            return
        sub, start = [], 0
        while start < len(w):
            end = len(w)
            while end > start:
                cand = w[start:end] if start == 0 else self.prefix + w[start:end]
                if cand in self.vocab:
                    break
                end -= 1
            if end == start:
                ids.append(self.unk)
                return
            sub.append(self.vocab[cand])
            start = end
        ids.extend(sub)

    def encode_str(self, s):
        """ids of a str through the whole pipeline (no added tokens, no flag rules)"""
        s, ids, i = normalize(s, self.flags), [], 0
        while i < len(s):
            if is_white_space(s[i]):
                i += 1
                continue
            b = i
            if is_bert_punc(s[i]):
                i += 1
            else:
                while i < len(s) and not is_white_space(s[i]) and not is_bert_punc(s[i]):
                    i += 1
            self.word(s[b:i], ids)
        return ids

    def encode(self, raw):
        """ids of a line (bytes), or None when the line is not covered"""
        if not self.covered(raw):
            return None
        return self.encode_str(raw.decode("utf-8"))

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
        if drop_unk:
            ids = [t for t in ids if t != self.unk]
        if max_tokens:
            ids = ids[:max_tokens]
        return ids, False

    def batch(self, lines, keep_bytes=0, max_tokens=0, drop_unk=True):
        ids, offsets, flags = [], [0], []
        for raw in lines:
            got, flagged = self.line(raw, keep_bytes, max_tokens, drop_unk)
            ids.extend(got)
            offsets.append(len(ids))
            flags.append(1 if flagged else 0)
        return np.array(ids, dtype=np.uint32), np.array(offsets, dtype=np.uint64), np.array(flags, dtype=np.uint8)


# conjoining jamo, as NFD makes them of \ud55c\uae00: h a n | g eu l
JAMO_HA, JAMO_N, JAMO_G, JAMO_EUL = "\u1112\u1161", "\u11ab", "\u1100", "\u1173\u11af"


UTF8_WORDS = ["café", "Café", "CAFÉ", "café", "naïve", "Über", "λόγος", "Λόγος", "και", "привет", "Мир", "мир", "й", "中文", "中", "文x",
              "한글", "한", "“the”", "a—b", "wait…", "«fox»", "か", "かな", "x y", "a b", "ẹ́", "ﬁx", "ǆ", "İ", "ß", "Ω", "ǅx"]
_GEN_BLOCKS = [(0xA0, 0x24F), (0x300, 0x36F), (0x370, 0x3FF), (0x400, 0x4FF), (0x2000, 0x206F), (0x2600, 0x26FF), (0x3040, 0x30FF),
               (0x4E00, 0x9FFF), (0xAC00, 0xD7A3), (0x1D400, 0x1D7FF), (0x20000, 0x200FF)]


@functools.lru_cache(maxsize=None)
def _gen_pools():
    old = unicodedata.ucd_3_2_0
    return [[chr(c) for c in range(a, b + 1) if old.category(chr(c)) != "Cn"] for a, b in _GEN_BLOCKS]


def utf8_lines(seed, n):
    """n lines (bytes): words of W.WORDS and UTF8_WORDS joined by ASCII and Unicode white space; draws from ASCII and the blocks; and
    every fourth line pure ASCII"""
    rng = random.Random(seed)
    pools = _gen_pools()
    out = []
    while len(out) < n:
        parts = [rng.choice(UTF8_WORDS) if rng.random() < 0.4 else rng.choice(W.WORDS) for _ in range(rng.randint(1, 12))]
        out.append(rng.choice([" ", "  ", "\t", " ", "  ", "\n"]).join(parts).encode())
        chars = []
        for _ in range(rng.randint(1, 40)):
            r = rng.random()
            chars.append(rng.choice(W.ASCII_POOL) if r < 0.5 else rng.choice(rng.choice(pools)))
        out.append("".join(chars).encode())
        blk = rng.choice(pools)
        out.append(" ".join("".join(rng.choice(blk) for _ in range(rng.randint(1, 6))) for _ in range(rng.randint(1, 8))).encode())
        out.append(W.ascii_lines(rng.randrange(1 << 30), 1)[0])
    return out[:n]
