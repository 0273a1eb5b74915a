"""The host layer's ingest with the device tokenizer route off and on, same box, same process, same order:
N prose-like ASCII lines through smt_host_search_content (split + tokenize + K1 + one search), lines/s end to end, the phase times of
the host layer's timer, pass 1's bytes/s from the kernel profile, and a second corpus in which every tenth line is flagged (a
Latin-1 word).  The tokenizer.json is written here: a WordPiece vocabulary over the corpus' own words (the most frequent whole, the
tail through ## pieces).  The process pins itself to --cpus CPUs first (default 16, what an ordinary deployment has; 0 = all it is
given), so the host tokenizer's threads and the route's copy threads share that many.  Each setting gets one discarded warm-up call
(first-use allocations), then three timed ones.  Merges its result under the key cpus_<n> into profiles/device_tokenizer.json.
--model unigram runs the same lines through a synthetic Unigram vocabulary of the same size behind BertNormalizer -> Metaspace (the
other device tokenizer) and writes profiles/device_tokenizer_unigram.json.
--utf8 measures the UTF-8 form of the WordPiece route instead (settings off / 1 / 2, alternated in one process, one warm-up call each
discarded, best of three with the spread, every timed call ends in a device synchronise): a text in which every tenth line holds a
non-ASCII character (curly quotes, an accented word, a CJK phrase), the pure-ASCII text (pass 1 of the UTF-8 kernel against the ASCII
kernel: the price of 2 where it is not needed), the same lines transliterated into Cyrillic letters (every word non-ASCII, the
vocabulary transliterated with them) and rewritten as CJK characters without spaces (every character a word of its own), and the size
of the code-point table.  Writes profiles/device_tokenizer_utf8.json.
--model unigram --utf8 does the same for the UTF-8 form of the Unigram route, on the same four texts, behind NFD -> Lowercase ->
StripAccents -> Metaspace (no handle_chinese_chars: a spaced Chinese character is a FLAG behind Metaspace), with the covered share of
every text (device_tokenized_lines_per_call).  Writes profiles/device_tokenizer_unigram_utf8.json.
--model unigram --long measures the long pieces of the Unigram route (smt_host_model_set_device_tokenizer_long) with the same tokenizer
and protocol: settings off / 2 / 2 with long pieces, on the CJK text without spaces (a line is one piece), on the ASCII text with a
100-byte URL-like word in every tenth line, and on the plain ASCII text (no long piece: what the switch costs where it is not
needed); with pass 1's time, the long-piece kernel's own time and smt_unigram_long_stats of the text's first 20000 lines.  Writes
profiles/device_tokenizer_unigram_long.json.
--model unigram --precompiled measures an XLM-R-style chain -- Precompiled (the nmt_nfkc character map of tests/golden) -> Replace(" {2,}")
-> WhitespaceSplit -> Metaspace, the same synthetic vocabulary -- with the protocol and the four texts of --utf8, and the ASCII text with
two doubled spaces in every tenth line (the space rules at work).  Writes profiles/device_tokenizer_precompiled.json.
--model unigram --precompiled --long measures the long pieces under the space rules (smt_unigram_set_long_rules, which the long switch
of the host layer sets too) on that chain with the protocol of --long: settings off / 2 / 2 with long pieces, on the CJK text without
spaces, on the ASCII text with a 100-byte URL-like word in every tenth line, and on the ASCII text with two doubled spaces in every
tenth line (no long piece: what the hand-over branch of the rules kernels and the second launch cost where they are not needed).
Setting 2 without the switch is what the chain did before the switch covered it.  Writes
profiles/device_tokenizer_precompiled_long.json.
--ignore-case measures the ingest of an ignore_case search (every line through to_lowercase before it is embedded) with the WordPiece
tokenizer, the vocabulary and the protocol of --utf8, the route at setting 2, on three texts with capitals: the pure-ASCII prose with
every word capitalised and every fifth one in upper case, the same with a non-ASCII line with capitals in every tenth place, and the
prose transliterated into Cyrillic with every word capitalised.  Settings, alternated in one process: host_lower (the route on,
SEMTOOLS_DEVICE_LOWER=0: each batch lowered on the host by the thread that packs it), device_lower (lowered on the GPU), no_ignore_case
(the same text without the option: the ceiling) and route_off (no device route: lowered on the tokenizer's threads).  --parent-build
runs in a tree whose library has no device lower-casing -- a build of the parent commit, where every line is lowered up front on the
calling thread -- and measures ignore_case / no_ignore_case there; its result goes under the key parent_build.  --files measures the
same settings through smt_host_session_open on a file of the text (load_documents: where the parent lowered one line at a time on the
calling thread) instead of smt_host_search_content (where it already used eight threads); under the key through_load_documents.
--kernels TEXT runs
smt_lower_device alone five times on one of the three texts, for a kernel trace taken from outside.  Writes profiles/device_lower.json.

    python tools/bench_device_tokenizer.py [--model wordpiece|unigram] [--utf8|--long|--precompiled [--long]|--ignore-case [--files] [--parent-build] | --ignore-case --kernels TEXT] [--lines 1000000] [--cpus 16] [--out profiles/device_tokenizer.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time
import zlib

import math

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["SEMTOOLS_EAGER_MODEL"] = "1"     # the whole table is resident from the start, for both settings

import torch  # noqa: E402,F401  (one HIP runtime per process: torch's, loaded first)

import semtools_amd as smt  # noqa: E402
from semtools_amd import _lib as L  # noqa: E402
from semtools_amd import host  # noqa: E402
from tests import precompiled_ref as P  # noqa: E402
from tests import synth  # noqa: E402
from tests import unigram_ref as U  # noqa: E402
from tests import wordpiece_ref as W  # noqa: E402

SYL = ["ta", "re", "mi", "con", "ver", "sion", "al", "ing", "er", "pro", "de", "ment", "un", "st", "or", "an", "en", "ti", "ly", "ex", "per", "for",
       "qu", "ob", "ject", "sys", "tem", "da", "ta", "in", "dex", "se", "arch", "vec", "tor", "to", "ken", "li", "ne", "fi", "le"]


def make_words(n, rng):
    words = set()
    while len(words) < n:
        words.add("".join(SYL[i] for i in rng.integers(0, len(SYL), size=int(rng.integers(1, 5)))))
    return sorted(words)


def make_lines(n_distinct, words, rng):
    lines = []
    for _ in range(n_distinct):
        k = int(rng.integers(5, 21))
        ws = [words[int(r)] for r in (rng.zipf(1.2, size=k) - 1) % len(words)]
        ws[0] = ws[0].capitalize()
        if k > 8:
            ws[k // 2] += ","
        lines.append(" ".join(ws) + ".")
    return lines


def make_vocab(words):
    vocab = dict(W.build_vocab())
    for c in W.NO_CONTINUATION:
        vocab.setdefault("##" + c, len(vocab))
    for s in SYL:
        vocab.setdefault("##" + s, len(vocab))
    for w in words[: len(words) * 3 // 4]:      # three quarters of the words are pieces; the rest split into syllables
        vocab.setdefault(w, len(vocab))
    return vocab


def make_unigram_vocab(words):
    """[(piece, score)]: <unk>, R, every printable ASCII character, the syllables bare and behind R, three quarters of the words behind R (the
    rest split into syllables by the lattice); scores fall with the logarithm of the rank, as a trained model's do"""
    pieces = ["<unk>", U.R] + [chr(c) for c in range(0x21, 0x7F)] + SYL + [U.R + s for s in SYL]
    pieces += [U.R + w for w in words[: len(words) * 3 // 4]] + [U.R + w.capitalize() for w in words[:2000]]
    seen, vocab = set(), []
    for p in pieces:
        if p not in seen:
            seen.add(p)
            vocab.append((p, 0.0 if p == "<unk>" else -(4.0 + math.log(len(vocab) + 1.0))))
    return vocab


def unigram_utf8_vocab(vocab):
    """the Unigram vocabulary + the non-ASCII pieces of the --utf8 texts: the accented words, the curly quotes, the CJK characters
    bare and behind R, and every alphabetic ASCII piece transliterated into Cyrillic letters"""
    seen = {p for p, _ in vocab}
    extra = [U.R + "cafe", U.R + "café", U.R + "naive", U.R + "naïve", "“", "”", U.R + "“"]
    for c in ["中", "文", "字", "符"] + CJK_POOL:
        extra += [c, U.R + c]
    for p, _ in vocab:
        body = p[len(U.R):] if p.startswith(U.R) else p
        if body.isascii() and body.isalpha():
            extra.append(p.translate(CYRILLIC))
    vocab = list(vocab)
    for p in extra:
        if p not in seen:
            seen.add(p)
            vocab.append((p, -(4.0 + math.log(len(vocab) + 1.0))))
    return vocab


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def phases_now():
    return json.loads(host._take_text(L.lib().smt_host_timing_json()) or "{}")


def run(ctx, model, content_b, query_b, n_lines, repeats=3):
    warm = C.c_void_p()   # discarded: buffers grown on first use, the route's table upload
    L.check(L.lib().smt_host_search_content(model._h, query_b, b"<stdin>", content_b, 0, 3, float("nan"), 0, 0, 0, C.byref(warm)))
    host._take_text(warm)
    before = phases_now()
    ctx.prof_reset()
    best, first = None, ""
    for _ in range(repeats):
        out = C.c_void_p()
        t0 = time.perf_counter()
        L.check(L.lib().smt_host_search_content(model._h, query_b, b"<stdin>", content_b, 0, 3, float("nan"), 0, 0, 0, C.byref(out)))
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
        first = host._take_text(out).split("\n")[0]
    after = phases_now()
    phases = {k: round((v - before.get(k, 0.0)) / repeats, 3) for k, v in after.items() if k.startswith("within_embed") and v - before.get(k, 0.0) > 0}
    kernels = {}
    for name in ("tokenize", "tokenize_emit", "embed"):
        n, ms = ctx.prof_read(name)
        if n:
            kernels[name] = {"launches": n, "total_ms": round(ms, 3)}
    res = {"seconds": round(best, 4), "lines_per_s": round(n_lines / best), "text_MB_per_s": round(len(content_b) / best / 1e6, 1),
           "phases_ms_per_call": phases, "kernel_ms_over_%d_calls" % repeats: kernels, "first_hit": first[:80],
           "device_tokenized_lines": model.device_tokenized_lines()}
    if "tokenize" in kernels:
        res["pass1_GB_per_s"] = round(len(content_b) * repeats / (kernels["tokenize"]["total_ms"] * 1e-3) / 1e9, 2)
    return res


NON_ASCII = [lambda ln: ln.replace(" ", " \u201c", 1).replace(",", "\u201d,", 1), lambda ln: ln.replace(" ", " caf\u00e9 na\u00efve ", 1),
             lambda ln: ln.replace(" ", " \u4e2d\u6587\u5b57\u7b26 ", 1)]


CYRILLIC = str.maketrans("abcdefghijklmnopqrstuvwxyz" + "ABCDEFGHIJKLMNOPQRSTUVWXYZ",
                         "абвгдежзиклмнопрстуфхцчшщы" + "АБВГДЕЖЗИКЛМНОПРСТУФХЦЧШЩЫ")   # (no й: NFD splits it)
CJK_POOL = [chr(0x4E00 + 3 * i) for i in range(2000)]


def to_cjk(line):
    """every word becomes one to three characters of CJK_POOL (chosen by its CRC), written without spaces; , and . stay"""
    out = []
    for w in line.split(" "):
        tail = w[-1] if w[-1:] in (",", ".") else ""
        h = zlib.crc32(w.lower().encode())
        out.append("".join(CJK_POOL[(h >> (11 * k)) % len(CJK_POOL)] for k in range(1 + h % 3)) + tail)
    return "".join(out)


def run_utf8(ctx, d, corpus, n_lines, repeats=3):
    """off / 1 / 2 on one text: a model per setting, a discarded warm-up call each, then `repeats` rounds that visit the settings in
    turn; every timed call ends in a device synchronise"""
    content_b = ("\n".join(corpus) + "\n").encode()
    query_b = corpus[17].encode()
    models = {name: host.StaticModel(ctx, model_dir=d, device_tokenizer=mode) for name, mode in (("off", 0), ("1", 1), ("2", 2))}
    times = {name: [] for name in models}
    pass1 = {name: [0, 0.0] for name in models}
    first = {}

    def call(m):
        out = C.c_void_p()
        L.check(L.lib().smt_host_search_content(m._h, query_b, b"<stdin>", content_b, 0, 3, float("nan"), 0, 0, 0, C.byref(out)))
        ctx.synchronize()
        return host._take_text(out).split("\n")[0]

    for m in models.values():
        call(m)
    for _ in range(repeats):
        for name, m in models.items():
            ctx.prof_reset()
            t0 = time.perf_counter()
            first[name] = call(m)
            times[name].append(time.perf_counter() - t0)
            n, ms = ctx.prof_read("tokenize")
            pass1[name][0] += n
            pass1[name][1] += ms
    entry = {"text_bytes": len(content_b)}
    for name, m in models.items():
        best = min(times[name])
        res = {"seconds_best": round(best, 4), "seconds_all": [round(t, 4) for t in times[name]],
               "spread_percent": round(100.0 * (max(times[name]) - best) / best, 1), "lines_per_s": round(n_lines / best),
               "device_tokenized_lines_per_call": m.device_tokenized_lines() // (repeats + 1), "first_hit": first[name][:80]}
        if pass1[name][0]:
            res["pass1_ms_per_call"] = round(pass1[name][1] / repeats, 3)
            res["pass1_launches_per_call"] = pass1[name][0] // repeats
            res["pass1_GB_per_s"] = round(len(content_b) * repeats / (pass1[name][1] * 1e-3) / 1e9, 2)
        entry[name] = res
        m.close()
    entry["same_first_hit"] = len(set(first.values())) == 1
    entry["2_over_1"] = round(entry["2"]["lines_per_s"] / entry["1"]["lines_per_s"], 3)
    entry["2_over_off"] = round(entry["2"]["lines_per_s"] / entry["off"]["lines_per_s"], 3)
    entry["1_over_off"] = round(entry["1"]["lines_per_s"] / entry["off"]["lines_per_s"], 3)
    print("measured:", {name: entry[name]["lines_per_s"] for name in ("off", "1", "2")}, "lines/s", flush=True)
    return entry


def lower_texts(lines):
    """the three texts of --ignore-case"""
    def caps(ln):
        return " ".join(w.upper() if i % 5 == 4 else w.capitalize() for i, w in enumerate(ln.split(" ")))
    ascii_caps = [caps(ln) for ln in lines]
    odd = ["\u00c9COLE \u00dcBER Caf\u00e9 NA\u00cfVE", "\u039f\u0394\u03a5\u03a3\u03a3\u0395\u03a5\u03a3 \u039a\u0391\u0399 \u039b\u039f\u0393\u039f\u03a3", "\u0130STANBUL 300 \u212a \u4e2d\u6587"]
    mixed = [ln.replace(" ", " " + odd[(i // 10) % 3] + " ", 1) if i % 10 == 0 else ln for i, ln in enumerate(ascii_caps)]
    cyrillic = [" ".join(w.capitalize() for w in ln.translate(CYRILLIC).split(" ")) for ln in lines]
    return (("ascii_with_capitals", ascii_caps), ("every_tenth_line_non_ascii_with_capitals", mixed), ("cyrillic_capitalised_words", cyrillic))


def run_lower(ctx, d, corpus, n_lines, repeats=3, parent=False, files_dir=None):
    """the settings of --ignore-case on one text: a model per setting, a discarded warm-up call each, then `repeats` rounds that visit
    the settings in turn; every timed call ends in a device synchronise"""
    content_b = ("\n".join(corpus) + "\n").encode()
    query_b = corpus[17].encode()
    if parent:
        settings = (("ignore_case", 2, None, 1), ("no_ignore_case", 2, None, 0))
    else:
        settings = (("host_lower", 2, False, 1), ("device_lower", 2, True, 1), ("no_ignore_case", 2, True, 0), ("route_off", 0, True, 1))
    models, ic = {}, {}
    for name, mode, dev_lower, ignore_case in settings:
        models[name] = host.StaticModel(ctx, model_dir=d, device_tokenizer=mode) if dev_lower is None else \
            host.StaticModel(ctx, model_dir=d, device_tokenizer=mode, device_lower=dev_lower)
        ic[name] = ignore_case
    times = {name: [] for name in models}
    prof = {name: {"lower": [0, 0.0], "tokenize": [0, 0.0]} for name in models}
    phases = {name: {} for name in models}
    first = {}

    path = None
    if files_dir:
        path = os.path.join(files_dir, "corpus.txt")
        with open(path, "wb") as f:
            f.write(content_b)

    def call(name):
        if path:                                     # smt_host_session_open: read, split, (lower,) tokenize, K1
            s = host.Session(models[name], [path], ignore_case=bool(ic[name]))
            n = s.lines
            s.close()
            ctx.synchronize()
            return "%d lines" % n
        out = C.c_void_p()
        L.check(L.lib().smt_host_search_content(models[name]._h, query_b, b"<stdin>", content_b, 0, 3, float("nan"), ic[name], 0, 0, C.byref(out)))
        ctx.synchronize()
        return host._take_text(out).split("\n")[0]

    for name in models:
        call(name)
    for _ in range(repeats):
        for name in models:
            ctx.prof_reset()
            before = phases_now()
            t0 = time.perf_counter()
            first[name] = call(name)
            times[name].append(time.perf_counter() - t0)
            for k, v in phases_now().items():
                if (k.startswith("within_embed") or k in ("split_lines", "tokenize_and_embed")) and v - before.get(k, 0.0) > 0:
                    phases[name][k] = phases[name].get(k, 0.0) + v - before.get(k, 0.0)
            for key, acc in prof[name].items():
                n, ms = ctx.prof_read(key)
                acc[0] += n
                acc[1] += ms
    entry = {"text_bytes": len(content_b)}
    for name, m in models.items():
        best = min(times[name])
        res = {"seconds_best": round(best, 4), "seconds_all": [round(t, 4) for t in times[name]],
               "spread_percent": round(100.0 * (max(times[name]) - best) / best, 1), "lines_per_s": round(n_lines / best),
               "device_tokenized_lines_per_call": m.device_tokenized_lines() // (repeats + 1), "first_hit": first[name][:80],
               "phases_ms_per_call": {k: round(v / repeats, 2) for k, v in sorted(phases[name].items())}}
        if not parent:
            res["device_lowered_lines_per_call"] = m.device_lowered_lines() // (repeats + 1)
        if prof[name]["lower"][0]:
            res["lower_ms_per_call"] = round(prof[name]["lower"][1] / repeats, 3)      # the three launches and the two prefix sums, by events
            res["lower_GB_per_s"] = round(len(content_b) * repeats / (prof[name]["lower"][1] * 1e-3) / 1e9, 2)
        if prof[name]["tokenize"][0]:
            res["pass1_ms_per_call"] = round(prof[name]["tokenize"][1] / repeats, 3)
        entry[name] = res
        m.close()
    lowered = [n for n in models if ic[n]]
    entry["same_first_hit_among_the_lowering_settings"] = len({first[n] for n in lowered}) == 1
    if not parent:
        entry["device_over_host_lower"] = round(entry["device_lower"]["lines_per_s"] / entry["host_lower"]["lines_per_s"], 3)
        entry["device_lower_over_no_ignore_case"] = round(entry["device_lower"]["lines_per_s"] / entry["no_ignore_case"]["lines_per_s"], 3)
        a, b = entry["device_lower"], entry["host_lower"]
        entry["device_lower_slower_beyond_the_spreads"] = a["seconds_best"] > max(b["seconds_all"])
    print("measured:", {name: entry[name]["lines_per_s"] for name in models}, "lines/s", flush=True)
    return entry


def run_lower_kernels(ctx, corpus, repeats=5):
    """smt_lower_device alone on one text, `repeats` times behind a warm-up call: for a kernel trace taken from outside"""
    text, begin, lens = smt.Lower.pack([ln.encode() for ln in corpus])
    n, tb = len(lens), len(text)
    cap = tb + tb // 2
    d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    d_begin = torch.from_numpy(begin.view(np.int64)).cuda()
    d_len = torch.from_numpy(lens.view(np.int32)).cuda()
    d_out = torch.zeros(cap + 16, dtype=torch.uint8, device="cuda")
    d_ob = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_ol = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    d_fl = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")
    d_nf = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    h = smt.Lower(ctx)
    times = []
    for _ in range(repeats + 1):
        t0 = time.perf_counter()
        h.lower_device(d_text.data_ptr(), tb, d_begin.data_ptr(), d_len.data_ptr(), n, d_out.data_ptr(), cap, d_ob.data_ptr(), d_ol.data_ptr(),
                       d_fl.data_ptr(), d_nf.data_ptr())
        ctx.synchronize()
        times.append(time.perf_counter() - t0)
    h.close()
    res = {"text_bytes": tb, "lines": n, "lowered_bytes": int(d_ob[n].item()), "flagged_lines": int(d_nf[0].item()), "calls_traced": repeats + 1,
           "call_seconds_best_host_clock": round(min(times[1:]), 6)}
    print(json.dumps(res), flush=True)
    return res


def run_long(ctx, d, corpus, n_lines, repeats=3, rules=False):
    """off / 2 / 2 with long pieces on one text: a model per setting, a discarded warm-up call each, then `repeats` rounds that visit
    the settings in turn; every timed call ends in a device synchronise"""
    content_b = ("\n".join(corpus) + "\n").encode()
    query_b = corpus[17].encode()
    models = {}
    for name, mode, long_pieces in (("off", 0, False), ("2", 2, False), ("2_long", 2, True)):
        models[name] = host.StaticModel(ctx, model_dir=d, device_tokenizer=mode)
        models[name].set_device_tokenizer_long(long_pieces)
    times = {name: [] for name in models}
    prof = {name: {"tokenize": [0, 0.0], "tokenize_long": [0, 0.0]} for name in models}
    first = {}

    def call(m):
        out = C.c_void_p()
        L.check(L.lib().smt_host_search_content(m._h, query_b, b"<stdin>", content_b, 0, 3, float("nan"), 0, 0, 0, C.byref(out)))
        ctx.synchronize()
        return host._take_text(out).split("\n")[0]

    for m in models.values():
        call(m)
    for _ in range(repeats):
        for name, m in models.items():
            ctx.prof_reset()
            t0 = time.perf_counter()
            first[name] = call(m)
            times[name].append(time.perf_counter() - t0)
            for key, acc in prof[name].items():
                n, ms = ctx.prof_read(key)
                acc[0] += n
                acc[1] += ms
    entry = {"text_bytes": len(content_b)}
    for name, m in models.items():
        best = min(times[name])
        res = {"seconds_best": round(best, 4), "seconds_all": [round(t, 4) for t in times[name]],
               "spread_percent": round(100.0 * (max(times[name]) - best) / best, 1), "lines_per_s": round(n_lines / best),
               "device_tokenized_lines_per_call": m.device_tokenized_lines() // (repeats + 1), "first_hit": first[name][:80]}
        if prof[name]["tokenize"][0]:
            res["pass1_ms_per_call"] = round(prof[name]["tokenize"][1] / repeats, 3)
            res["pass1_launches_per_call"] = prof[name]["tokenize"][0] // repeats
        if prof[name]["tokenize_long"][0]:
            res["long_kernel_ms_per_call"] = round(prof[name]["tokenize_long"][1] / repeats, 3)
        entry[name] = res
        m.close()
    h = C.c_void_p()      # the witness, on the handle itself: the route keeps its own inside
    L.check(L.lib().smt_host_tokenizer_load(os.path.join(d, "tokenizer.json").encode(), C.byref(h)))
    tok = smt.Unigram(ctx, host_tokenizer=h, utf8=True)
    tok.set_long_pieces(L.UG_MAX_LONG)
    if rules:                                        # (the handle of a Precompiled chain has its space rules from the file)
        tok.set_long_rules(True)
    flags = tok.tokenize([ln.encode() for ln in corpus[:20000]])[2]
    pieces, raw = tok.long_stats()
    entry["long_stats_of_first_20000_lines"] = {"long_pieces": pieces, "raw_bytes": raw, "flagged_lines": int(flags.sum())}
    tok.close()
    L.lib().smt_host_tokenizer_free(h)
    entry["same_first_hit"] = len(set(first.values())) == 1
    for a, b in (("2_long", "2"), ("2_long", "off"), ("2", "off")):
        entry["%s_over_%s" % (a, b)] = round(entry[a]["lines_per_s"] / entry[b]["lines_per_s"], 3)
    print("measured:", {name: entry[name]["lines_per_s"] for name in models}, "lines/s", flush=True)
    return entry


def url_like(i):
    """a word of 100 bytes: scheme, host and a path of syllables chosen by i"""
    w = "https://" + SYL[i % len(SYL)] + SYL[(i // 7) % len(SYL)] + ".example.org"
    k = i
    while len(w) < 100:
        w += "/" + SYL[k % len(SYL)] + SYL[(k // 3) % len(SYL)] + str(k % 97)
        k = k * 31 + 7
    return w[:100]


def measure_long(ctx, d, lines, n_lines, result, precompiled=False):
    result["what"] = "host-layer ingest (smt_host_search_content), device tokenizer route off / 2 (UTF-8 form) / 2 with long pieces"
    result["note"] = ("kernel profiling events are on in all settings; per setting one warm-up call is discarded, then three rounds visit "
                      "off, 2, 2_long in turn; every timed call ends in a device synchronise; seconds_best is the best of 3, spread_percent "
                      "(max - best) / best; long_kernel_ms_per_call is ug_long_kernel alone, inside pass1_ms_per_call")
    result["cjk_no_spaces"] = run_long(ctx, d, [to_cjk(ln) for ln in lines], n_lines, rules=precompiled)
    urls = [ln.replace(" ", " " + url_like(i) + " ", 1) if i % 10 == 0 else ln for i, ln in enumerate(lines)]
    result["every_tenth_line_a_100_byte_url"] = run_long(ctx, d, urls, n_lines, rules=precompiled)
    if precompiled:
        doubled = [ln.replace(" ", "  ", 2) if i % 10 == 0 else ln for i, ln in enumerate(lines)]
        result["ascii_every_tenth_line_doubled_spaces_no_long_piece"] = run_long(ctx, d, doubled, n_lines, rules=True)
    else:
        result["ascii_no_long_piece"] = run_long(ctx, d, lines, n_lines)


def measure_on_off(ctx, d, corpora, n_lines, result):
    for corpus_name, corpus in corpora:
        content_b = ("\n".join(corpus) + "\n").encode()
        query_b = corpus[17].encode()
        entry = {"text_bytes": len(content_b)}
        for setting, on in (("off", False), ("on", True)):
            m = host.StaticModel(ctx, model_dir=d, device_tokenizer=on)
            entry[setting] = run(ctx, m, content_b, query_b, n_lines)
            m.close()
        entry["on_over_off"] = round(entry["on"]["lines_per_s"] / entry["off"]["lines_per_s"], 3)
        entry["same_first_hit"] = entry["on"]["first_hit"] == entry["off"]["first_hit"]
        result[corpus_name] = entry


def measure_utf8(ctx, d, lines, n_lines, result, unigram=False, precompiled=False):
    result["what"] = "host-layer ingest (smt_host_search_content), device tokenizer route off / 1 (ASCII form) / 2 (UTF-8 form)"
    result["note"] = ("kernel profiling events are on in all settings; per setting one warm-up call is discarded, then three rounds visit "
                      "off, 1, 2 in turn; every timed call ends in a device synchronise; seconds_best is the best of 3, spread_percent "
                      "(max - best) / best")
    h = C.c_void_p()
    L.check(L.lib().smt_host_tokenizer_load(os.path.join(d, "tokenizer.json").encode(), C.byref(h)))
    t0 = time.perf_counter()
    tok = (smt.Unigram if unigram else smt.WordPiece)(ctx, host_tokenizer=h, utf8=True)
    result["code_point_table"] = {"create_seconds": round(time.perf_counter() - t0, 3), "table_bytes": tok.info()[0],
                                  "code_point_bytes": tok.info()[1]}
    tok.close()
    L.lib().smt_host_tokenizer_free(h)
    mixed = [NON_ASCII[(i // 10) % 3](ln) if i % 10 == 0 else ln for i, ln in enumerate(lines)]
    result["every_tenth_line_non_ascii"] = run_utf8(ctx, d, mixed, n_lines)
    result["ascii"] = run_utf8(ctx, d, lines, n_lines)
    result["cyrillic"] = run_utf8(ctx, d, [ln.translate(CYRILLIC) for ln in lines], n_lines)
    result["cjk_no_spaces"] = run_utf8(ctx, d, [to_cjk(ln) for ln in lines], n_lines)
    if precompiled:
        doubled = [ln.replace(" ", "  ", 2) if i % 10 == 0 else ln for i, ln in enumerate(lines)]
        result["ascii_every_tenth_line_doubled_spaces"] = run_utf8(ctx, d, doubled, n_lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utf8", action="store_true")
    ap.add_argument("--long", action="store_true", help="the long pieces of the Unigram route (with --model unigram)")
    ap.add_argument("--precompiled", action="store_true", help="an XLM-R-style chain in front of the Unigram route (with --model unigram)")
    ap.add_argument("--ignore-case", action="store_true", help="the ingest of an ignore_case search: where the lines are lowered")
    ap.add_argument("--parent-build", action="store_true", help="with --ignore-case: the library has no device lower-casing (a build of the parent commit)")
    ap.add_argument("--files", action="store_true", help="with --ignore-case: through smt_host_session_open on a file (load_documents)")
    ap.add_argument("--kernels", default=None, help="with --ignore-case: smt_lower_device alone on this text (for a kernel trace)")
    ap.add_argument("--lines", type=int, default=1_000_000)
    ap.add_argument("--cpus", type=int, default=16)
    ap.add_argument("--model", choices=["wordpiece", "unigram"], default="wordpiece")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    unigram = a.model == "unigram"
    if a.ignore_case:
        if unigram or a.utf8 or a.long or a.precompiled:
            ap.error("--ignore-case goes alone (WordPiece, the vocabulary of --utf8)")
        a.utf8 = True
        a.out = a.out or os.path.join(ROOT, "profiles", "device_lower.json")
    if a.long:
        if not unigram or a.utf8:
            ap.error("--long goes with --model unigram, without --utf8")
        a.utf8 = True                                # the vocabulary, the texts and the tokenizer of the UTF-8 profile
        a.out = a.out or os.path.join(ROOT, "profiles", "device_tokenizer_precompiled_long.json" if a.precompiled else "device_tokenizer_unigram_long.json")
    elif a.precompiled:
        if not unigram or a.utf8:
            ap.error("--precompiled goes with --model unigram, without --utf8")
        a.utf8 = True                                # the vocabulary, the texts and the protocol of the UTF-8 profile
        a.out = a.out or os.path.join(ROOT, "profiles", "device_tokenizer_precompiled.json")
    if a.out is None:
        name = ("device_tokenizer_unigram_utf8.json" if unigram else "device_tokenizer_utf8.json") if a.utf8 else \
            "device_tokenizer_unigram.json" if unigram else "device_tokenizer.json"
        a.out = os.path.join(ROOT, "profiles", name)
    if a.cpus and hasattr(os, "sched_setaffinity"):
        os.sched_setaffinity(0, sorted(os.sched_getaffinity(0))[: a.cpus])
    rng = np.random.default_rng(7)
    words = make_words(30_000, rng)
    vocab = make_unigram_vocab(words) if unigram else make_vocab(words)
    if a.utf8 and unigram:
        vocab = unigram_utf8_vocab(vocab)
    elif a.utf8:
        for p in ["cafe", "café", "naive", "naïve", "\u201c", "\u201d", "\u4e2d", "\u6587", "\u5b57", "\u7b26"] + CJK_POOL:
            vocab.setdefault(p, len(vocab))
        for p in [p for p in vocab if p.replace("##", "", 1).isalpha() and p.isascii() and p.replace("##", "", 1).islower()]:
            vocab.setdefault(p.translate(CYRILLIC), len(vocab))
    distinct = make_lines(20_000, words, rng)
    lines = [distinct[i % len(distinct)] for i in range(a.lines)]
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    ctx = smt.Context(0)
    ctx.prof_enable(True)
    result = {"what": "host-layer ingest (smt_host_search_content: split + tokenize + K1 + one search), device tokenizer route off / on",
              "lines": a.lines, "cpus_available": cores, "gpu": torch.cuda.get_device_name(0), "vocabulary_pieces": len(vocab),
              "host_cpu": cpu_model(), "tokenizer": "BertNormalizer -> Metaspace -> Unigram" if unigram else "BertNormalizer -> BertPreTokenizer -> WordPiece",
              "note": "kernel profiling events are on in both settings; per setting one warm-up call is discarded, seconds is the best of 3 "
                      "timed calls, phases are the mean of those 3; 'off' runs before 'on' in the same process"}
    with tempfile.TemporaryDirectory() as d:
        from safetensors.numpy import save_file

        save_file({"embeddings": synth.table(len(vocab), seed=2)}, os.path.join(d, "model.safetensors"))
        if a.precompiled:
            result["tokenizer"] = "Precompiled(nmt_nfkc) -> Replace(' {2,}') -> WhitespaceSplit -> Metaspace -> Unigram"
            with open(os.path.join(d, "tokenizer.json"), "w") as f:
                json.dump(P.tokenizer_json("A_ws", vocab=vocab, added=[]), f)
        elif unigram and a.utf8:      # (a chain without handle_chinese_chars: behind Metaspace a spaced Chinese character is a FLAG)
            result["tokenizer"] = "NFD -> Lowercase -> StripAccents -> Metaspace -> Unigram"
            U.write_tokenizer(os.path.join(d, "tokenizer.json"), norm="seq", prepend="always", vocab=vocab, added=[])
        elif unigram:
            U.write_tokenizer(os.path.join(d, "tokenizer.json"), norm="bert_clean", prepend="always", vocab=vocab, added=[])
        else:
            W.write_tokenizer(os.path.join(d, "tokenizer.json"), 7, vocab=vocab)
        with open(os.path.join(d, "config.json"), "w") as f:
            json.dump({"normalize": True, "unk_token": "<unk>" if unigram else "[UNK]"}, f)
        if a.ignore_case and a.kernels:
            result = {"what": "smt_lower_device alone, for a kernel trace", a.kernels: run_lower_kernels(ctx, dict(lower_texts(lines))[a.kernels])}
        elif a.ignore_case:
            result["what"] = "host-layer ingest of an ignore_case search (smt_host_search_content), by where the lines are lowered"
            result["note"] = ("route at setting 2 (UTF-8 form) but for route_off; kernel profiling events are on in all settings; per setting one "
                              "warm-up call is discarded, then three rounds visit the settings in turn; every timed call ends in a device "
                              "synchronise; seconds_best is the best of 3, spread_percent (max - best) / best; lower_ms_per_call is the three "
                              "launches of smt_lower_device and its two prefix sums, by events")
            if a.files:
                result["what"] = "host-layer ingest of an ignore_case session (smt_host_session_open on one file: load_documents), by where the lines are lowered"
            for name, corpus in lower_texts(lines):
                result[name] = run_lower(ctx, d, corpus, a.lines, parent=a.parent_build, files_dir=d if a.files else None)
        elif a.long:
            measure_long(ctx, d, lines, a.lines, result, a.precompiled)
        elif a.utf8:
            measure_utf8(ctx, d, lines, a.lines, result, unigram, a.precompiled)
        else:
            flagged = [ln.replace(" ", " café ", 1) if i % 10 == 0 else ln for i, ln in enumerate(lines)]
            measure_on_off(ctx, d, (("ascii", lines), ("ten_percent_flagged", flagged)), a.lines, result)
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    merged = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            merged = json.load(f)
    key = "cpus_%d" % cores
    if a.ignore_case and a.kernels:
        merged.setdefault(key, {}).setdefault("kernels_alone", {}).update({a.kernels: result[a.kernels]})
    elif a.ignore_case and a.files:
        sub = merged.setdefault(key, {}).setdefault("through_load_documents", {})
        if a.parent_build:
            sub["parent_build"] = result
        else:
            sub.update(result)
    elif a.ignore_case and a.parent_build:
        merged.setdefault(key, {})["parent_build"] = result
    elif a.ignore_case and key in merged:
        merged[key].update(result)
    else:
        merged[key] = result
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
