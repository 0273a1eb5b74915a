"""Plain-Python restatement of what a pure-ASCII line becomes under BertNormalizer -> BertPreTokenizer -> WordPiece, with the truncate,
unk-drop and cap steps of the host layer's tokenize_batch.  Longest candidate first, exactly as hf_tokenizer.cpp's encode_ascii tries
them; written from the rules, not from that code's table (semtools_amd/csrc/wordpiece_bytes.h), so the two can disagree.

Also here: the hand-written tokenizer.json files of the device tokenizer's tests (no `tokenizers` wheel needed) and the two seeded
generators of ASCII lines tests/test_tokenizer.py uses for the host tokenizer (`words` joined by white space, draws from `ascii_pool`)."""
import json
import random
import string

import numpy as np

WP_NORMALIZER, WP_CLEAN_TEXT, WP_LOWERCASE = 1, 2, 4
FLAG_SETS = {"norm_clean_lower": 7, "norm_clean": 3, "norm_only": 1, "no_norm": 0}
PUNCT = set(range(0x21, 0x30)) | set(range(0x3A, 0x41)) | set(range(0x5B, 0x61)) | set(range(0x7B, 0x7F))
ADDED = ["[PAD]", "[UNK]"]
MAX_CHARS = 100
NO_CONTINUATION = "qzQZ7"    # letters / digits WITHOUT a ## piece: a word that needs one there has an unmatched tail


def build_vocab():
    """piece -> id.  [PAD], [UNK]; every ASCII letter, digit and punctuation character; every letter and digit but NO_CONTINUATION as a
    ## piece; a few dozen words; ## suffixes of every length 2 .. 12.  Greedy matching therefore meets multi-step matches
    (embeddings = em ##bed ##d ##ings ...), full-word first matches (the) and unmatched tails (zzz: z, then no ##z)."""
    pieces = list(ADDED)
    pieces += list(string.ascii_lowercase + string.ascii_uppercase + string.digits)
    pieces += [chr(c) for c in sorted(PUNCT)]
    pieces += ["##" + c for c in string.ascii_lowercase + string.ascii_uppercase + string.digits if c not in NO_CONTINUATION]
    pieces += ["the", "quick", "search", "text", "em", "embed", "cosine", "fox", "again", "mail", "don", "semi", "colon", "dead", "beef", "be",
               "a_b", "Search", "TEXT", "The", "token", "word", "pre", "un", "under", "stand", "understand", "over", "line", "file", "in",
               "inter", "nation", "national", "ab", "abc", "abcd", "cd", "0x", "1e", "12", "123", "xx", "yy", "wor", "ww"]
    pieces += ["##ed", "##er", "##ly", "##ing", "##ings", "##tion", "##ation", "##ations", "##ization", "##izations", "##abilities",
               "##istically", "##ifications", "##izationally", "##bed", "##dings", "##d", "##cd", "##bcd", "##ww", "##DEAD", "##BEEF", "##xx"]
    vocab = {}
    for p in pieces:
        if p not in vocab:
            vocab[p] = len(vocab)
    return vocab


def tokenizer_json(flags, vocab=None, max_chars=MAX_CHARS):
    """the tokenizer.json (a dict for json.dump) of a flag set: WordPiece with an explicit vocabulary, BertPreTokenizer, and a
    BertNormalizer unless flags == 0"""
    vocab = vocab or build_vocab()
    norm = None
    if flags & WP_NORMALIZER:
        norm = {"type": "BertNormalizer", "clean_text": bool(flags & WP_CLEAN_TEXT), "handle_chinese_chars": True, "strip_accents": None,
                "lowercase": bool(flags & WP_LOWERCASE)}
    return {"version": "1.0", "truncation": None, "padding": None,
            "added_tokens": [{"id": vocab[t], "content": t, "single_word": False, "lstrip": False, "rstrip": False, "normalized": False,
                              "special": True} for t in ADDED],
            "normalizer": norm, "pre_tokenizer": {"type": "BertPreTokenizer"}, "post_processor": None, "decoder": None,
            "model": {"type": "WordPiece", "unk_token": "[UNK]", "continuing_subword_prefix": "##", "max_input_chars_per_word": max_chars,
                      "vocab": vocab}}


def write_tokenizer(path, flags, **kw):
    with open(path, "w") as f:
        json.dump(tokenizer_json(flags, **kw), f)
    return str(path)


def unigram_json():
    """a small Unigram / Metaspace tokenizer.json: no device form"""
    vocab = [["<unk>", 0.0], ["▁", -2.0]] + [[c, -3.0] for c in string.ascii_lowercase] + [["▁the", -1.5], ["ing", -2.5]]
    return {"version": "1.0", "truncation": None, "padding": None, "added_tokens": [], "normalizer": None,
            "pre_tokenizer": {"type": "Metaspace", "replacement": "▁", "prepend_scheme": "always", "split": True},
            "post_processor": None, "decoder": None, "model": {"type": "Unigram", "unk_id": 0, "vocab": vocab, "byte_fallback": False}}


class WordPieceRef:
    def __init__(self, flags, vocab=None, max_chars=MAX_CHARS, prefix="##", unk="[UNK]", added=ADDED):
        self.vocab = {k.encode(): v for k, v in (vocab or build_vocab()).items()}
        self.flags, self.max_chars, self.prefix = flags, max_chars, prefix.encode()
        self.unk = self.vocab[unk.encode()]
        self.added = [a.encode() for a in added]

    def normalize(self, raw):
        """the normalized bytes of a pure-ASCII line"""
        if not self.flags & WP_NORMALIZER:
            return raw
        out = bytearray()
        for c in raw:
            if self.flags & WP_CLEAN_TEXT:
                if c in (0x09, 0x0A, 0x0D):
                    out.append(0x20)
                    continue
                if c < 0x20 or c == 0x7F:          # NUL, the controls (VT and FF among them), DEL: dropped, the neighbours join
                    continue
            if self.flags & WP_LOWERCASE and 0x41 <= c <= 0x5A:
                c += 32
            out.append(c)
        return bytes(out)

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
            if end == start:                       # an unmatched tail: ONE unk for the word, the pieces found are taken back
                ids.append(self.unk)
                return
            sub.append(self.vocab[cand])
            start = end
        ids.extend(sub)

    def encode(self, raw):
        """ids of a line (bytes), or None when the line is not covered: a byte >= 0x80, or an added token standing in it"""
        if any(c >= 0x80 for c in raw) or any(a in raw for a in self.added):
            return None
        s, ids, i = self.normalize(raw), [], 0
        while i < len(s):
            c = s[i]
            if (0x09 <= c <= 0x0D) or c == 0x20:   # white space (without clean_text VT and FF are still here, as white space)
                i += 1
                continue
            b = i
            if c in PUNCT:
                i += 1
            else:
                while i < len(s) and not ((0x09 <= s[i] <= 0x0D) or s[i] == 0x20 or s[i] in PUNCT):
                    i += 1
            self.word(s[b:i], ids)
        return ids

    def line(self, raw, keep_bytes=0, max_tokens=0, drop_unk=True):
        """-> (ids, flagged) after truncate -> encode -> unk drop -> cap, the order of the host layer"""
        if keep_bytes:
            raw = raw[:keep_bytes]
        ids = self.encode(raw)
        if ids is None:
            return [], True
        if drop_unk:
            ids = [t for t in ids if t != self.unk]
        if max_tokens:
            ids = ids[:max_tokens]
        return ids, False

    def batch(self, lines, keep_bytes=0, max_tokens=0, drop_unk=True):
        """-> (ids uint32, offsets uint64 [n + 1], flags uint8 [n]); a flagged line has no ids"""
        ids, offsets, flags = [], [0], []
        for raw in lines:
            got, flagged = self.line(raw, keep_bytes, max_tokens, drop_unk)
            ids.extend(got)
            offsets.append(len(ids))
            flags.append(1 if flagged else 0)
        return np.array(ids, dtype=np.uint32), np.array(offsets, dtype=np.uint64), np.array(flags, dtype=np.uint8)


WORDS = ["the", "quick", "Search", "TEXT", "embeddings", "cosine", "x", "fox,", "(again)", "a_b", "e-mail", "1e-5", "0xDEADBEEF", "[UNK]",
         "[PAD]", "[", "]", "<unk>", "zzzqqqxxyy", "w" * 101, "don't", "semi;colon", "q" * 100, "understandings", "internationalizations",
         "abcd", "w" * 100, "The7"]
ASCII_POOL = [chr(c) for c in range(1, 128)]


def ascii_lines(seed, n):
    """n lines (bytes), alternately from the two generators of tests/test_tokenizer.py: words joined by white space, draws from the pool"""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        parts = [rng.choice(WORDS) for _ in range(rng.randint(1, 14))]
        out.append(rng.choice([" ", "  ", "\t", "\n", " \r\n"]).join(parts).encode())
        out.append("".join(rng.choice(ASCII_POOL) for _ in range(rng.randint(1, 80))).encode())
    return out[:n]
