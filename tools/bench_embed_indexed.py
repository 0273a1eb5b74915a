#!/usr/bin/env python3
"""K1 (embed_kernels.hip) over indexed tables: kernel time of smt_embed_device read with smt_prof_read("embed"), one process, one GPU.

Workload (the sizes of bench_embed_typed.py): ~32 M tokens over 8 M ragged lines (0..8 tokens), uniform ids and Zipf s = 1.1 ids.
Per case: warm-up launches, then REPS single launches timed one by one; median, min, max and spread (max - min) / median.

  (a) indirection  a plain model against an indexed model with the identity mapping and unit weights over the SAME table (V rows):
                   the cost of the extra link alone, F32 and I8, uniform and Zipf ids.
  (b) shrunken     n_tokens = 500 k tokens over 32 Ki I8 rows (random many-to-one mapping, weights in [0.25, 4]) against the plain
                   500 k-row I8 and F32 tables: what a vocabulary-quantised model buys.
  (c) plain        the plain kernels of this library; run the script again with --lib <older libsemtools_hip.so> --label parent for
                   the other side (a library without the indexed creators runs the plain cases only).

Cases run in the order listed in the output ("order"); the box is named in "device".

  tools/bench_embed_indexed.py --out profiles/embed_indexed.json [--lib PATH --label parent]"""
import argparse
import ctypes as C
import json
import os
import statistics

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM = 256
KINDS = {"f32": (0, 4), "i8": (2, 1)}


def bind(path):
    import torch  # noqa: F401  (first: one HIP runtime per process)

    L = C.CDLL(path)
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    L.smt_last_error.restype = C.c_char_p
    L.smt_ctx_create.argtypes = [i32, C.POINTER(vp)]
    L.smt_ctx_destroy.argtypes = [vp]
    L.smt_ctx_destroy.restype = None
    L.smt_ctx_synchronize.argtypes = [vp]
    L.smt_prof_enable.argtypes = [vp, i32]
    L.smt_prof_reset.argtypes = [vp]
    L.smt_prof_read.argtypes = [vp, C.c_char_p, C.POINTER(u64), C.POINTER(C.c_double)]
    L.smt_model_create_from_device_typed.argtypes = [vp, vp, i32, u64, u32, i32, C.POINTER(vp)]
    L.smt_model_destroy.argtypes = [vp]
    L.smt_model_destroy.restype = None
    L.smt_embed_device.argtypes = [vp, vp, vp, u64, u32, vp]
    L.indexed = hasattr(L, "smt_model_create_from_device_indexed")
    if L.indexed:
        L.smt_model_create_from_device_indexed.argtypes = [vp, vp, i32, u64, u32, vp, vp, u64, i32, C.POINTER(vp)]
    return L


def ok(L, rc):
    if rc != 0:
        raise RuntimeError(f"error {rc}: {L.smt_last_error().decode(errors='replace')}")


def workload(n_ids, n_lines, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 9, size=n_lines)
    offsets = np.zeros(n_lines + 1, dtype=np.uint64)
    np.cumsum(lens, out=offsets[1:])
    n_tok = int(offsets[-1])
    uniform = rng.integers(0, n_ids, size=n_tok, dtype=np.int64).astype(np.uint32)
    ranks = rng.zipf(1.1, size=n_tok).astype(np.uint64)
    zipf = ((ranks * np.uint64(2654435761)) % np.uint64(n_ids)).astype(np.uint32)     # rank r -> a fixed id somewhere in the range
    return offsets, {"uniform": uniform, "zipf_1.1": zipf}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "semtools_amd", "lib", "libsemtools_hip.so"))
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None)
    ap.add_argument("--v", type=int, default=4_000_000, help="rows of the table of (a) and (c)")
    ap.add_argument("--tokens", type=int, default=500_000, help="n_tokens of (b)")
    ap.add_argument("--rows", type=int, default=32 * 1024, help="n_rows of (b)")
    ap.add_argument("--lines", type=int, default=8_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    import torch

    L = bind(args.lib)
    ctx = C.c_void_p()
    ok(L, L.smt_ctx_create(0, C.byref(ctx)))
    ok(L, L.smt_prof_enable(ctx, 1))
    d_out = torch.empty((args.lines, DIM), dtype=torch.float32, device="cuda")
    g = torch.Generator(device="cuda")
    g.manual_seed(9)
    results, order = [], []

    def table_of(kind, rows):
        base = torch.randn((rows, DIM), generator=g, device="cuda", dtype=torch.float32) * 0.1
        return base if kind == "f32" else torch.clamp(torch.round(base * 400), -127, 127).to(torch.int8)

    def measure(part, case, kind, model, offsets, idsets, d_off, extra):
        for name, ids in idsets.items():
            d_ids = torch.from_numpy(ids.view(np.int32)).cuda()
            torch.cuda.synchronize()
            run = lambda: ok(L, L.smt_embed_device(model, C.c_void_p(d_ids.data_ptr()), C.c_void_p(d_off.data_ptr()), args.lines, 2048,
                                                   C.c_void_p(d_out.data_ptr())))
            for _ in range(args.warmup):
                run()
            ok(L, L.smt_ctx_synchronize(ctx))
            ms = []
            for _ in range(args.reps):
                ok(L, L.smt_prof_reset(ctx))
                run()
                n, t = C.c_uint64(), C.c_double()
                ok(L, L.smt_prof_read(ctx, b"embed", C.byref(n), C.byref(t)))
                ms.append(t.value)
            med = statistics.median(ms)
            r = dict(part=part, case=case, table=kind, ids=name, tokens=int(offsets[-1]), lines=args.lines, median_ms=round(med, 4),
                     min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), spread=round((max(ms) - min(ms)) / med, 4), reps=args.reps, **extra)
            results.append(r)
            order.append(f"{part}:{case}:{kind}:{name}")
            print(json.dumps(r), flush=True)
            del d_ids

    def model_of(table, kind, rows, mapping=None, weights=None, n_tokens=0):
        m = C.c_void_p()
        torch.cuda.synchronize()
        if mapping is None and weights is None:
            ok(L, L.smt_model_create_from_device_typed(ctx, C.c_void_p(table.data_ptr()), KINDS[kind][0], rows, DIM, 1, C.byref(m)))
        else:
            ok(L, L.smt_model_create_from_device_indexed(ctx, C.c_void_p(table.data_ptr()), KINDS[kind][0], rows, DIM,
                                                         C.c_void_p(mapping.data_ptr()), C.c_void_p(weights.data_ptr()), n_tokens, 1, C.byref(m)))
        return m

    # ---- (a) + (c): the same table plain and behind an identity mapping with unit weights
    offsets, idsets = workload(args.v, args.lines, 5)
    d_off = torch.from_numpy(offsets.view(np.int64)).cuda()
    for kind in ("f32", "i8"):
        table = table_of(kind, args.v)
        m = model_of(table, kind, args.v)
        measure("a_c", "plain", kind, m, offsets, idsets, d_off, dict(n_rows=args.v, n_tokens=args.v))
        L.smt_model_destroy(m)
        if L.indexed:
            ident = torch.arange(args.v, dtype=torch.int32, device="cuda")
            ones = torch.ones(args.v, dtype=torch.float32, device="cuda")
            m = model_of(table, kind, args.v, ident, ones, args.v)
            measure("a", "identity_mapping_unit_weights", kind, m, offsets, idsets, d_off, dict(n_rows=args.v, n_tokens=args.v))
            L.smt_model_destroy(m)
            del ident, ones
        del table
    # ---- (b): 500 k tokens over 32 Ki I8 rows against plain 500 k-row tables
    offsets, idsets = workload(args.tokens, args.lines, 6)
    d_off = torch.from_numpy(offsets.view(np.int64)).cuda()
    for kind in ("i8", "f32"):
        table = table_of(kind, args.tokens)
        m = model_of(table, kind, args.tokens)
        measure("b", "plain_full_vocabulary", kind, m, offsets, idsets, d_off, dict(n_rows=args.tokens, n_tokens=args.tokens))
        L.smt_model_destroy(m)
        del table
    if L.indexed:
        table = table_of("i8", args.rows)
        mapping = torch.randint(0, args.rows, (args.tokens,), generator=g, device="cuda", dtype=torch.int32)
        weights = torch.rand(args.tokens, generator=g, device="cuda", dtype=torch.float32) * 3.75 + 0.25
        m = model_of(table, "i8", args.rows, mapping, weights, args.tokens)
        measure("b", "indexed_shrunken", "i8", m, offsets, idsets, d_off, dict(n_rows=args.rows, n_tokens=args.tokens))
        L.smt_model_destroy(m)
    out = dict(label=args.label, lib=os.path.basename(args.lib), device=torch.cuda.get_device_name(0), order=order, results=results)
    L.smt_ctx_destroy(ctx)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(dict(label=args.label, cases=len(results))))


if __name__ == "__main__":
    main()
