"""Plain-Python restatement of an XLM-R-style tokenizer -- a `Precompiled` sentencepiece normalizer, a regex `Replace` that collapses
runs of spaces, Metaspace, Unigram -- and of what the device tokenizer covers of it under its space rules (DESIGN 4.9 "Behind a
Precompiled normalizer").  Written from the rules: the character map is walked here from the blob's bytes, the text is cut into
extended grapheme clusters by the `regex` module's \\X (imported only where a whole line is normalised: the device-side part needs
the blob alone), the lattice is tests/unigram_ref.py's.

Two views of one tokenizer:
  * PrecompiledRef.encode_host: the whole chain over the whole line, as the host tokenizer and the `tokenizers` wheel run it;
  * PrecompiledRef.encode / .line / .batch: what the device form answers -- a per-character table (classify), the two space rules,
    the measure -- or that the line is flagged.
tests/test_precompiled_ref_cpu.py asserts that the two agree on every line the second covers.

Also here: the three shapes of tokenizer.json in circulation, the named lines, and a seeded generator of mixed-script lines drawn
from code points Unicode 13 assigns."""
import base64
import functools
import os
import random
import struct
import unicodedata

from tests import unigram_ref as U
from tests import unigram_utf8_ref as G
from tests import wordpiece_utf8_ref as W8

R = U.R
MAX_WORD = U.MAX_WORD
ORDINARY, SPACE, DROPPED, FLAG = G.ORDINARY, G.SPACE, G.DROPPED, G.FLAG
BLOB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nmt_nfkc_charsmap.bin")
SHAPES = ["A_ws", "A", "B"]
# (collapse_runs, drop_trailing) of each shape's device form
RULES = {"A_ws": (1, 1), "A": (1, 0), "B": (1, 1)}


@functools.lru_cache(maxsize=None)
def blob():
    with open(BLOB_PATH, "rb") as f:
        return f.read()


class Malformed(Exception):
    pass


class Charsmap:
    """the blob: u32 LE trie size, the darts-clone units, the pool of NUL-terminated strings"""

    def __init__(self, data):
        if len(data) < 4:
            raise Malformed("header")
        (size,) = struct.unpack_from("<I", data, 0)
        if size % 4 or size > len(data) - 4:
            raise Malformed("trie size")
        self.units = struct.unpack_from("<%dI" % (size // 4), data, 4)
        self.pool = data[4 + size:]
        if self.pool and self.pool[-1] != 0:
            raise Malformed("the last string has no NUL")

    @staticmethod
    def _offset(unit):
        return (unit >> 10) << ((unit & 0x200) >> 6)

    def lookup(self, key):
        """the FIRST result of the common-prefix search over key (bytes): the normalised str, or None"""
        if not self.units:
            return None
        node = self._offset(self.units[0])
        for c in key:
            if c == 0:
                return None
            node ^= c
            if node >= len(self.units):
                raise Malformed("node")
            unit = self.units[node]
            if unit & 0x800000FF != c:
                return None
            node ^= self._offset(unit)
            if (unit >> 8) & 1:
                if node >= len(self.units):
                    raise Malformed("node")
                value = self.units[node] & 0x7FFFFFFF
                if value >= len(self.pool):
                    raise Malformed("value")
                return self.pool[value:self.pool.index(b"\0", value)].decode()
        return None

    def chars(self, s):
        """every character of s looked up on its own; a miss keeps it"""
        out = []
        for ch in s:
            hit = self.lookup(ch.encode())
            out.append(ch if hit is None else hit)
        return "".join(out)

    def normalize(self, s):
        """the text cut into extended grapheme clusters; one shorter than 6 bytes is looked up whole, otherwise (or on a miss) its
        characters one by one"""
        import regex
        out = []
        for cluster in regex.findall(r"\X", s):
            hit = self.lookup(cluster.encode()) if len(cluster.encode()) < 6 else None
            out.append(self.chars(cluster) if hit is None else hit)
        return "".join(out)


@functools.lru_cache(maxsize=None)
def charsmap():
    return Charsmap(blob())


def precompiled_json(data=None):
    return {"type": "Precompiled", "precompiled_charsmap": base64.b64encode(blob() if data is None else data).decode()}


def normalizer_json(shape, data=None):
    pre = precompiled_json(data)
    if shape == "B":
        return {"type": "Sequence", "normalizers": [pre, {"type": "Strip", "strip_left": False, "strip_right": True},
                                                    {"type": "Replace", "pattern": {"Regex": " {2,}"}, "content": R}]}
    return {"type": "Sequence", "normalizers": [pre, {"type": "Replace", "pattern": {"Regex": " {2,}"}, "content": " "}]}


def build_vocab():
    """unigram_utf8_ref.build_vocab() (the ids stay) + what nmt_nfkc makes of the sample line: the ligature and the full-width word
    spelled out, a Roman numeral, a katakana syllable with its voiced mark composed and apart"""
    v = list(G.build_vocab())
    v += [(R + "fine", -3.0), ("fi", -4.0), (R + "full", -3.0), ("XII", -4.0), (R + "No", -3.5), ("5", -4.25), ("ß", -5.0), (R + "x", -3.0),
          ("2", -4.25), ("ガ", -4.0), ("カ", -4.5), ("゙", -5.0), (R + "é", -4.0), ("é", -4.5)]
    return v


def tokenizer_json(shape="A_ws", vocab=None, data=None, norm=None, **kw):
    tj = U.tokenizer_json(norm=norm or normalizer_json(shape, data), prepend="always", vocab=vocab or build_vocab(), **kw)
    if shape == "A_ws":
        tj["pre_tokenizer"] = {"type": "Sequence", "pretokenizers": [{"type": "WhitespaceSplit"}, tj["pre_tokenizer"]]}
    return tj


def _parse_run_regex(pattern):
    """(character, least count) of the one regex form read: a literal character and {n,} or +"""
    c, rest = pattern[0], pattern[1:]
    assert c not in "\\.^$*+?()[]{}|"
    if rest == "+":
        return c, 1
    assert rest[0] == "{" and rest.endswith(",}") and rest[1:-2].isdigit()
    return c, int(rest[1:-2])


def normalize(s, n):
    """unigram_utf8_ref.normalize + Precompiled, Strip, Replace"""
    if n is None:
        return s
    t = n["type"]
    if t == "Sequence":
        for c in n["normalizers"]:
            s = normalize(s, c)
        return s
    if t == "Precompiled":
        return Charsmap(base64.b64decode(n["precompiled_charsmap"])).normalize(s) if "_map" not in n else n["_map"].normalize(s)
    if t == "Strip":
        b, e = 0, len(s)
        while n.get("strip_left", True) and b < e and W8.is_white_space(s[b]):
            b += 1
        while n.get("strip_right", True) and e > b and W8.is_white_space(s[e - 1]):
            e -= 1
        return s[b:e]
    if t == "Replace":
        if "String" in n["pattern"]:
            return s.replace(n["pattern"]["String"], n["content"])
        c, least = _parse_run_regex(n["pattern"]["Regex"])
        out, i = [], 0
        while i < len(s):
            j = i
            while j < len(s) and s[j] == c:
                j += 1
            if j - i >= least:
                out.append(n["content"])
            else:
                out.append(s[i:max(j, i + 1)])
            i = max(j, i + 1)
        return "".join(out)
    return G.normalize(s, n)


def joins(cp):
    """the code point can stand in one extended grapheme cluster with a neighbour: Extend, ZWJ, SpacingMark, Prepend, the conjoining
    jamo, a Regional_Indicator, CR and LF (with each other).  From `unicodedata` and the ranges UAX #29 names, not from the `regex`
    module: Mn / Me and the Other_Grapheme_Extend characters are Extend; Mc is SpacingMark but for the few that are Extend."""
    if cp in (0x0D, 0x0A, 0x200C, 0x200D):
        return True
    if 0x1100 <= cp <= 0x11FF or 0xA960 <= cp <= 0xA97C or 0xD7B0 <= cp <= 0xD7FB:   # jamo L, V, T
        return True
    if 0x1F1E6 <= cp <= 0x1F1FF or 0x1F3FB <= cp <= 0x1F3FF or 0xE0020 <= cp <= 0xE007F:   # regional indicators, emoji modifiers, tags
        return True
    cat = unicodedata.category(chr(cp))
    if cat in ("Mn", "Me", "Mc"):
        return True
    if cp in (0xFF9E, 0xFF9F):                                      # Other_Grapheme_Extend of category Lm
        return True
    # Prepend: the prepended concatenation marks (Cf) and a few letters
    return cp in (0x0600, 0x0601, 0x0602, 0x0603, 0x0604, 0x0605, 0x06DD, 0x070F, 0x08E2, 0x0D4E, 0x110BD, 0x110CD, 0x111C2, 0x111C3, 0x1193F,
                  0x11941, 0x11A3A, 0x11A84, 0x11A85, 0x11A86, 0x11A87, 0x11A88, 0x11A89, 0x11D46)


class PrecompiledRef(U.UnigramRef):
    """utf8 = False: the ASCII form (a byte >= 0x80 flags the line)"""

    def __init__(self, tj, collapse_runs=None, drop_trailing=None, utf8=True):
        plain = dict(tj, normalizer=None, pre_tokenizer={"type": "Metaspace", "replacement": R, "prepend_scheme": "always", "split": True})
        super().__init__(plain)
        pre = tj["pre_tokenizer"]
        self.ws_split = pre["type"] == "Sequence" and pre["pretokenizers"][0]["type"] == "WhitespaceSplit"
        self.norm = tj["normalizer"]
        parts = self.norm["normalizers"]
        assert parts[0]["type"] == "Precompiled"
        self.cmap = Charsmap(base64.b64decode(parts[0]["precompiled_charsmap"]))
        self.norm = dict(self.norm, normalizers=[dict(parts[0], _map=self.cmap)] + parts[1:])
        strips = any(p["type"] == "Strip" for p in parts)
        self.collapse = int(any(p["type"] == "Replace" for p in parts)) if collapse_runs is None else collapse_runs
        self.drop_trailing = int(self.ws_split or strips) if drop_trailing is None else drop_trailing
        self.utf8 = utf8
        self._cls = {}
        assert tj["pre_tokenizer"].get("prepend_scheme", "always") == "always"

    # ---- the whole chain over the whole line
    def encode_host(self, raw):
        s = normalize(raw.decode(), self.norm)
        words = [s]
        if self.ws_split:
            words, cur = [], []
            for ch in s + " ":
                if W8.is_white_space(ch):
                    if cur:
                        words.append("".join(cur))
                    cur = []
                else:
                    cur.append(ch)
        ids = []
        if not raw:
            return ids
        for w in words:
            w = w.replace(" ", self.rep)
            if not w.startswith(self.rep):
                w = self.rep + w
            pieces = []
            for ch in w:
                if ch == self.rep or not pieces:
                    pieces.append([])
                pieces[-1].append(ch)
            for p in pieces:
                self.piece(p, ids)
        return ids

    # ---- the device form
    def cp_class(self, cp):
        """(class, output) of one character as the device table has it: what the character map makes of the one-character string
        (Strip and the regex Replace are the space rules, not the table)"""
        got = self._cls.get(cp)
        if got is None:
            ch = chr(cp)
            s = self.cmap.chars(ch)
            rules = self.collapse or self.drop_trailing
            if cp >= 0x80 and (joins(cp) or (unicodedata.category(ch).startswith("C") and s == ch)):
                got = (FLAG, "")                  # joins a neighbour into one cluster; unassigned or private and unknown to the map
            elif (rules and cp == ord(self.rep)) or (self.drop_trailing and any(c != " " and W8.is_white_space(c) for c in s)):
                got = (FLAG, "")                  # a literal replacement beside a space is no run; Strip and WhitespaceSplit cut at any white space
            elif s == "":
                got = (DROPPED, "")
            elif s == " " or s == self.rep:
                got = (SPACE, "")
            elif " " in s or self.rep in s or len(s) > len(ch.encode()):
                got = (FLAG, "")
            elif cp < 0x80 and (len(s) != 1 or ord(s) >= 0x80):
                got = (FLAG, "")
            else:
                got = (ORDINARY, s)
            self._cls[cp] = got
        return got

    def units(self, raw):
        if any(a in raw for a in self.added) or b"\r\n" in raw:      # (CR LF is one cluster, looked up whole)
            return None
        if not self.utf8 and any(c >= 0x80 for c in raw):
            return None
        try:
            s = raw.decode("utf-8")
        except UnicodeDecodeError:
            return None
        out = []
        for ch in s:
            k, o = self.cp_class(ord(ch))
            if k == FLAG:
                return None
            out.append((len(ch.encode()), k, o))
        return out

    def encode(self, raw, check_limit=True):
        """ids of a line (bytes) under the space rules, or None when the line is flagged"""
        units = self.units(raw)
        if units is None:
            return None
        if not raw:
            return []
        text, seg, n_space, prev_space = [], 0, 0, False
        for src, cls, o in units:
            if cls == SPACE and not (self.collapse and prev_space):
                n_space, seg = n_space + 1, 1
                text.append(self.rep)
            else:                                 # an absorbed space counts like a dropped character: its raw bytes
                seg += src
            if check_limit and seg + (1 if n_space == 0 else 0) > MAX_WORD:
                return None
            if cls == ORDINARY:
                text.extend(o)
            if cls != DROPPED:
                prev_space = cls == SPACE
        if self.drop_trailing and (not text or text[-1] == self.rep):
            if len(text) <= 1:
                return None                       # the line's only piece: a chain that strips and one that splits differ, the host's
            text.pop()                            # the replacement alone at the line's end
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

    def line(self, raw, keep_bytes=0, max_tokens=0, drop_unk=True):
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


SAMPLE = "ﬁne  Straße ｆｕｌｌ  x² ｶﾞ é Ⅻ №5​ 한글"
NAMED = {
    "sample": SAMPLE.encode(),
    "empty": b"",
    "spaces_only": b"    ",
    "one_space": b" ",
    "eacute_decomposed": "the é fox".encode(),
    "zwj_emoji": "a \U0001f468‍\U0001f469‍\U0001f467 b".encode(),
    "regional_pair": "the \U0001f1e9\U0001f1ea fox".encode(),
    "hangul_precomposed": "the 한글 fox".encode(),
    "hangul_decomposed": ("the " + unicodedata.normalize("NFD", "한글") + " fox").encode(),
    "half": "a ½ b".encode(),
    "kabushiki": "the ㍿ fox".encode(),
    "nbsp_by_space": "the  fox  text".encode(),
    "ideographic_by_space": "the　 fox 　text".encode(),
    "zwsp_between_spaces": "the ​ fox".encode(),
    "dropped_between_spaces": b"the \x01 \x02\x03  fox",
    "tab_newline": b"the\t fox \n text",
    "fullwidth": "ｔｈｅ　ｆｏｘ".encode(),
    "accented": "the café fox".encode(),
    "cyrillic": "привет  мир".encode(),
    "cjk": "中文  the 中".encode(),
    "prose": b"the search text es foxes searching a fox",
    "viterbi": b"abcd  xy mno",
}
for _n in (1, 2, 3, 70):
    NAMED["run_%d_start" % _n] = b" " * _n + b"the fox"
    NAMED["run_%d_middle" % _n] = b"the" + b" " * _n + b"fox"
    NAMED["run_%d_end" % _n] = b"the fox" + b" " * _n

_GEN_BLOCKS = [(0xA0, 0x24F), (0x370, 0x3FF), (0x400, 0x4FF), (0x2010, 0x2016), (0x3041, 0x3096), (0x30A1, 0x30FA), (0x4E00, 0x4FFF),
               (0xAC00, 0xD7A3), (0xFF01, 0xFF5E), (0xFF66, 0xFF9D), (0x1D400, 0x1D454), (0x1F600, 0x1F64F)]
_WORDS = [w for w in G.UTF8_WORDS if R not in w and "\u0301" not in w] + ["ﬁne", "Straße", "ｆｕｌｌ", "x²", "Ⅻ", "№5", "한글", "ｶ", "カ"]
_RARE = ["é", "½", "㍿", "\U0001f1e9\U0001f1ea", "\U0001f468‍\U0001f469", unicodedata.normalize("NFD", "한"), "ｶﾞ", "ﷺ", "क्ष"]
_SEPS = [" ", "  ", "   ", " ", "\t", " ", "　", " ​ ", " "]


@functools.lru_cache(maxsize=None)
def _gen_pools():
    return [[chr(c) for c in range(a, b + 1) if unicodedata.category(chr(c)) != "Cn"] for a, b in _GEN_BLOCKS]


def lines(seed, n):
    """n lines (bytes) of mixed scripts joined by single and repeated ASCII and Unicode spaces, some with spaces at either end; one
    line in thirty holds a sequence that joins into a cluster or outgrows its bytes (flagged); every fourth line is pure ASCII"""
    rng = random.Random(seed)
    pools = _gen_pools()
    out = []

    def ends(s):
        return rng.choice(["", "", "", " ", "  "]) + s + rng.choice(["", "", "", " ", "   "])

    while len(out) < n:
        parts = [rng.choice(_WORDS) if rng.random() < 0.5 else rng.choice(U.WORDS) for _ in range(rng.randint(1, 12))]
        if rng.random() < 0.12:
            parts.insert(rng.randrange(len(parts) + 1), rng.choice(_RARE))
        out.append(ends(rng.choice(_SEPS).join(parts)).encode())
        words = []
        for _ in range(rng.randint(1, 8)):
            blk = rng.choice(pools)
            words.append("".join(rng.choice(blk) if rng.random() < 0.7 else rng.choice("abcdexy") for _ in range(rng.randint(1, 8))))
        out.append(ends(rng.choice(_SEPS).join(words)).encode())
        blk = rng.choice(pools)
        out.append(rng.choice(_SEPS).join("".join(rng.choice(blk) for _ in range(rng.randint(1, 6))) for _ in range(rng.randint(1, 8))).encode())
        out.append(ends(U.ascii_lines(rng.randrange(1 << 30), 1, pool=[c for c in U.SAFE_POOL if c not in "\n\r"], seps=(" ", "  ", "   "))[0].decode()).encode())
    return out[:n]
