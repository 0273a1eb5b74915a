"""The host layer's ingest with the device tokenizer route off and on, same box, same process, same order:
N prose-like ASCII lines through smt_host_search_content (split + tokenize + K1 + one search), lines/s end to end, the phase times of
the host layer's timer, pass 1's bytes/s from the kernel profile, and a second corpus in which every tenth line is flagged (a
Latin-1 word).  The tokenizer.json is written here: a WordPiece vocabulary over the corpus' own words (the most frequent whole, the
tail through ## pieces).  The process pins itself to --cpus CPUs first (default 16, what an ordinary deployment has; 0 = all it is
given), so the host tokenizer's threads and the route's copy threads share that many.  Each setting gets one discarded warm-up call
(first-use allocations), then three timed ones.  Merges its result under the key cpus_<n> into profiles/device_tokenizer.json.
--model unigram runs the same lines through a synthetic Unigram vocabulary of the same size behind BertNormalizer -> Metaspace (the
other device tokenizer) and writes profiles/device_tokenizer_unigram.json.

    python tools/bench_device_tokenizer.py [--model wordpiece|unigram] [--lines 1000000] [--cpus 16] [--out profiles/device_tokenizer.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import math

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["SEMTOOLS_EAGER_MODEL"] = "1"     # the whole table is resident from the start, for both settings

import torch  # noqa: E402,F401  (one HIP runtime per process: torch's, loaded first)

import semtools_amd as smt  # noqa: E402
from semtools_amd import _lib as L  # noqa: E402
from semtools_amd import host  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1_000_000)
    ap.add_argument("--cpus", type=int, default=16)
    ap.add_argument("--model", choices=["wordpiece", "unigram"], default="wordpiece")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    unigram = a.model == "unigram"
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "device_tokenizer_unigram.json" if unigram else "device_tokenizer.json")
    if a.cpus and hasattr(os, "sched_setaffinity"):
        os.sched_setaffinity(0, sorted(os.sched_getaffinity(0))[: a.cpus])
    rng = np.random.default_rng(7)
    words = make_words(30_000, rng)
    vocab = make_unigram_vocab(words) if unigram else make_vocab(words)
    distinct = make_lines(20_000, words, rng)
    lines = [distinct[i % len(distinct)] for i in range(a.lines)]
    flagged = [ln.replace(" ", " café ", 1) if i % 10 == 0 else ln for i, ln in enumerate(lines)]
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
        if unigram:
            U.write_tokenizer(os.path.join(d, "tokenizer.json"), norm="bert_clean", prepend="always", vocab=vocab, added=[])
        else:
            W.write_tokenizer(os.path.join(d, "tokenizer.json"), 7, vocab=vocab)
        with open(os.path.join(d, "config.json"), "w") as f:
            json.dump({"normalize": True, "unk_token": "<unk>" if unigram else "[UNK]"}, f)
        for corpus_name, corpus in (("ascii", lines), ("ten_percent_flagged", flagged)):
            content_b = ("\n".join(corpus) + "\n").encode()
            query_b = corpus[17].encode()
            entry = {"text_bytes": len(content_b)}
            for setting, on in (("off", False), ("on", True)):
                m = host.StaticModel(ctx, model_dir=d, device_tokenizer=on)
                entry[setting] = run(ctx, m, content_b, query_b, a.lines)
                m.close()
            entry["on_over_off"] = round(entry["on"]["lines_per_s"] / entry["off"]["lines_per_s"], 3)
            entry["same_first_hit"] = entry["on"]["first_hit"] == entry["off"]["first_hit"]
            result[corpus_name] = entry
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    merged = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            merged = json.load(f)
    merged["cpus_%d" % cores] = result
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
