"""Plain-Python restatement of what a pure-ASCII line becomes under a per-byte normalizer -> Metaspace -> Unigram, with the truncate,
unk-drop and cap steps of the host layer's tokenize_batch -- the rules of DESIGN.md 4.9 "Unigram", written from the rules: the
lattice here PULLS (for every end position all starts, smallest first) where hf_tokenizer.cpp's unigram() and the kernel push, so
the tie rule -- among equal f64 sums for one end the smallest start wins -- is stated a second time, not copied.

UnigramRef reads a tokenizer.json (a dict): the hand-written one below, or one the `tokenizers` wheel trained.  Also here: the
hand-written vocabulary of the device tokenizer's tests, the writer of its tokenizer.json files, the named lines and a seeded
generator of ASCII lines."""
import json
import random
import string

import numpy as np

R = "▁"
MAX_WORD = 64                    # SMT_UG_MAX_WORD: the raw bytes of one piece (its space, dropped bytes and a prepended R counted)
ADDED = ["<pad>"]
NORMALIZERS = {
    "none": None,
    "lower": {"type": "Lowercase"},
    "seq": {"type": "Sequence", "normalizers": [{"type": "NFD"}, {"type": "Lowercase"}, {"type": "StripAccents"}]},
    "bert_clean": {"type": "BertNormalizer", "clean_text": True, "handle_chinese_chars": True, "strip_accents": None, "lowercase": True},
    "bert_noclean": {"type": "BertNormalizer", "clean_text": False, "handle_chinese_chars": True, "strip_accents": None, "lowercase": True},
}
PREPEND = ["always", "first", "never"]


def build_vocab():
    """[(piece, score)], the id of a piece is its index.  Holds: a word where Viterbi and greedy longest match differ (abcd: greedy
    takes R+abc, d; the best path is R+ab, cd); two segmentations of equal f64 sum (xy: R+x, y = -7 = R, xy: the smaller start of the
    last edge wins: R, xy); sums that differ in the last bits only (mno: scores that are no dyadic fractions); R alone, twice (the
    later entry wins); a repeated piece whose first entry would lose (the); pieces with a non-ASCII byte, one of them the longest;
    ASCII characters without a single piece (q, z, 7, most punctuation): the unknown; the literal text of the unk token."""
    v = [("<unk>", 0.0), ("<pad>", 0.0), (R, -9.0), ("the", -20.0)]
    for c in string.ascii_lowercase:
        if c not in "qz":
            v.append((c, {"m": -3.1, "n": -3.2, "o": -3.3}.get(c, -4.0)))
    v += [(c, -4.5) for c in "THEAB"] + [(c, -4.25) for c in "12.,"] + [("\t", -6.0)]
    v += [(R + "ab", -2.0), (R + "abc", -2.5), ("cd", -1.0), ("abc", -3.5)]
    v += [(R + "x", -3.0), ("xy", -5.0)]
    v += [("mn", -6.3), ("no", -6.5), (R + "m", -3.7)]
    v += [(R, -2.0), ("the", -2.5), (R + "the", -1.5), ("ing", -2.5), (R + "a", -3.0), (R + "fox", -2.25), ("fox", -3.0), ("er", -2.75), ("The", -3.0),
          (R + "search", -2.0), ("search", -3.0), ("es", -3.5), (R + "q", -8.0), ("qu", -5.0), ("text", -3.0), (R + "text", -2.0), ("s", -3.9)]
    v += [("é", -5.0), (R + "café", -4.0), ("aéb", -4.0), ("é" * 12, -7.0)]
    return v


def tokenizer_json(norm="none", prepend="always", unk_id=0, vocab=None, added=ADDED, replacement=R, split=True, pre_sequence=False):
    """the tokenizer.json (a dict for json.dump): Unigram with the explicit vocabulary behind one Metaspace"""
    vocab = vocab or build_vocab()
    names = [p for p, _ in vocab]
    ms = {"type": "Metaspace", "replacement": replacement, "prepend_scheme": prepend, "split": split}
    return {"version": "1.0", "truncation": None, "padding": None,
            "added_tokens": [{"id": names.index(t), "content": t, "single_word": False, "lstrip": False, "rstrip": False, "normalized": False,
                              "special": True} for t in added],
            "normalizer": NORMALIZERS[norm] if isinstance(norm, str) else norm,
            "pre_tokenizer": {"type": "Sequence", "pretokenizers": [ms]} if pre_sequence else ms, "post_processor": None, "decoder": None,
            "model": {"type": "Unigram", "unk_id": unk_id, "vocab": [[p, s] for p, s in vocab], "byte_fallback": False}}


def write_tokenizer(path, **kw):
    with open(path, "w") as f:
        json.dump(tokenizer_json(**kw), f)
    return str(path)


def byte_map(norm):
    """what every byte < 0x80 becomes under a normalizer (a tokenizer.json dict or None): a byte, or None = dropped"""
    m = list(range(128))

    def apply(n):
        if n is None:
            return
        t = n["type"]
        if t == "Sequence":
            for c in n["normalizers"]:
                apply(c)
        elif t == "Lowercase":
            for c in range(128):
                if m[c] is not None and 0x41 <= m[c] <= 0x5A:
                    m[c] += 32
        elif t in ("NFD", "StripAccents"):
            pass                                       # no ASCII character decomposes or is a mark
        elif t == "BertNormalizer":
            for c in range(128):
                b = m[c]
                if b is None:
                    continue
                if n.get("clean_text", True):
                    if b in (0x09, 0x0A, 0x0D):
                        b = 0x20
                    elif b < 0x20 or b == 0x7F:        # NUL, the controls (VT and FF among them), DEL
                        b = None
                if b is not None and n.get("lowercase", True) and 0x41 <= b <= 0x5A:
                    b += 32
                m[c] = b
        else:
            raise ValueError(t)

    apply(norm)
    return m


class Flagged(Exception):
    pass


class UnigramRef:
    def __init__(self, tj):
        model = tj["model"]
        self.pieces = {}
        for i, (p, s) in enumerate(model["vocab"]):
            self.pieces[p] = (i, float(s))           # a repeated piece: the later entry, id and score
        self.max_piece_bytes = max((len(p.encode()) for p, _ in model["vocab"]), default=0)
        self.unk_score = min((float(s) for _, s in model["vocab"]), default=0.0) - 10.0
        self.unk = model.get("unk_id")
        pre = tj["pre_tokenizer"]
        if pre["type"] == "Sequence":
            (pre,) = pre["pretokenizers"]
        assert pre["type"] == "Metaspace" and pre.get("split", True)
        self.rep = pre["replacement"]
        self.prepend = pre["prepend_scheme"]
        self.map = byte_map(tj.get("normalizer"))
        self.added = [a["content"].encode() for a in tj.get("added_tokens", []) if not a.get("normalized") and a["content"].isascii()]

    def piece(self, chars, ids):
        """Viterbi over the characters of one piece; appends its ids"""
        n = len(chars)
        best = [(0.0, None, None, False)] + [None] * n          # (sum, start, id, unknown)
        for end in range(1, n + 1):
            node = None
            for start in range(end):                             # smallest start first, strictly better replaces: ties keep the smaller
                text = "".join(chars[start:end])
                hit = self.pieces.get(text) if len(text.encode()) <= self.max_piece_bytes else None
                if hit is not None:
                    cand = hit[1] + best[start][0]
                    if node is None or cand > node[0]:
                        node = (cand, start, hit[0], False)
                elif end - start == 1:                           # no piece covers exactly this character
                    cand = self.unk_score + best[start][0]
                    if node is None or cand > node[0]:
                        node = (cand, start, self.unk, True)
            best[end] = node
        path, e = [], n
        while e > 0:
            path.append(best[e])
            e = best[e][1]
        prev_unk = False
        for _, _, tid, unk in reversed(path):
            if unk and prev_unk:
                continue                                         # consecutive unknowns fuse
            if unk and self.unk is None:
                raise Flagged("an unknown character and no unk id")
            ids.append(tid)
            prev_unk = unk

    def encode(self, raw, check_limit=True):
        """ids of a line (bytes), or None when the line is flagged"""
        if any(c >= 0x80 for c in raw) or any(a in raw for a in self.added):
            return None
        if not raw:
            return []
        if check_limit:                                          # the raw bytes between two spaces, the space itself counted
            seg, k = 0, 0
            for c in raw:
                if self.map[c] == 0x20:
                    k, seg = k + 1, 1
                else:
                    seg += 1
                if seg + (1 if k == 0 and self.prepend != "never" else 0) > MAX_WORD:
                    return None
        text = [self.rep if self.map[c] == 0x20 else chr(self.map[c]) for c in raw if self.map[c] is not None]
        if self.prepend != "never" and (not text or text[0] != self.rep):    # (an unflagged line is one section, and the first)
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
        except Flagged:
            return None
        return ids

    def line(self, raw, keep_bytes=0, max_tokens=0, drop_unk=True):
        """-> (ids, flagged) after truncate -> encode -> unk drop -> cap, the order of the host layer"""
        if keep_bytes:
            raw = raw[:keep_bytes]
        ids = self.encode(raw)
        if ids is None:
            return [], True
        if drop_unk and self.unk is not None:
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


NAMED = {
    "empty": b"",
    "one_space": b" ",
    "spaces_only": b"   ",
    "only_dropped": b"\x01\x02\x7f",                 # dropped under clean_text (one piece: R), unknown characters otherwise
    "dropped_then_space": b"\x01 the",
    "leading_space": b" the fox",
    "trailing_space": b"the fox ",
    "doubled_spaces": b"the  fox   text",
    "viterbi_vs_greedy": b"abcd",
    "viterbi_vs_greedy_inner": b"the abcd abc",
    "tie": b"xy",
    "tie_inner": b"a xy xyxy",
    "last_bits": b"mno mnomno nomn",
    "one_unknown": b"thez",
    "unknown_run": b"azzqzb the",                    # z z q z: one fused unk between a and b
    "unknown_only": b"zzz",
    "unknown_covered_by_a_longer_piece": b"qu quq",  # q has no single piece, qu covers it
    "literal_unk_text": b"the <unk> fox",            # the piece <unk> carries the unk id: dropped with it
    "byte_ge_80": b"the caf\xc3\xa9 fox",
    "added_token": b"the <pad> fox",
    "added_token_prefix_only": b"the <pa fox <",
    "exactly_max_word": b"the " + b"a" * (MAX_WORD - 1) + b" fox",
    "max_word_plus_one": b"the " + b"a" * MAX_WORD + b" fox",
    "first_word_exactly_max": b"b" * (MAX_WORD - 1) + b" x",     # (one less without a prepended R: still under the limit)
    "first_word_over_max": b"b" * (MAX_WORD + 1),
    "long_base64_like": b"see " + b"QUJD" * 40,
    "tab": b"the\tfox",
    "newline_cr": b"the\nfox\r\ntext",
    "upper": b"THE The tHE",
    "dropped_inside": b"th\x01e f\x02\x03ox",
    "repeated_piece": b"the bathe",
    "one_byte": b"a",                                # with a prepended R: two tokens from one byte
    "one_byte_unknown": b"z",
    "punctuation": b"the, fox. 12 7 (x)",
    "prose": b"the search text es foxes searching a fox",
}
# (line, keep_bytes): the cut
CUTS = [(b"the caf\xc3\xa9", 7), (b"the caf\xc3\xa9", 8), (b"the <pad>", 6), (b"the <pad>", 8), (b"the <pad>", 9), (b"the searching", 9),
        (b"abcd", 3), (b"a b c d", 1), (b"xy xy", 4), (b"the " + b"a" * 100, 4 + MAX_WORD - 1), (b"the " + b"a" * 100, 4 + MAX_WORD)]

WORDS = ["the", "fox", "search", "searching", "text", "texts", "abcd", "abc", "xy", "xyxy", "mno", "nomn", "a", "x", "qu", "zq", "thez", "The",
         "THE", "bathe", "12", "7.", "er,", "foxes", "mn", "no", "abcdxy", "theing", "z"]
# no first byte of an added token ('<'), no byte >= 0x80
SAFE_POOL = [chr(c) for c in range(1, 128) if chr(c) != "<"]


def ascii_lines(seed, n, pool=None, max_word=MAX_WORD - 2, seps=(" ", "  ", "\t", "\n", " \r\n")):
    """n lines (bytes), alternately words joined by white space and draws from `pool` (default: every ASCII byte but NUL) cut into
    runs of at most max_word bytes by spaces"""
    rng = random.Random(seed)
    pool = pool or [chr(c) for c in range(1, 128)]
    out = []
    while len(out) < n:
        parts = [rng.choice(WORDS) for _ in range(rng.randint(1, 14))]
        out.append(rng.choice(seps).join(parts).encode())
        draw = [rng.choice(pool) for _ in range(rng.randint(1, 80))]
        for i in range(rng.randint(0, max_word), len(draw), max_word):
            draw[i] = " "
        out.append("".join(draw).encode())
    return out[:n]
