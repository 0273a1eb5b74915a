#!/usr/bin/env python3
"""K1 (embed_kernels.hip) over f32, half and int8 tables: kernel time of smt_embed_device read with smt_prof_read("embed").

Workload: ~32 M tokens over 8 M lines (ragged, 0..8 tokens), a table of V = 4 M rows, uniform ids and Zipf s = 1.1 ids (ranks
scattered over the table).  Per case: warm-up launches, then REPS single launches timed one by one; median, min, max and the
spread (max - min) / median are reported, with bytes gathered per token and the fraction of the HBM peak they amount to.

The script binds the library with ctypes by itself (--lib), so the same file measures an older build of the library: one without
the typed creators runs the f32 case only (that is the "parent" line of profiles/embed_typed.json).

  tools/bench_embed_typed.py --out profiles/embed_typed.json [--lib PATH --label parent] [--host-load-v 500000]

--host-load-v V also times smt_host_model_from_dir on a synthetic F16 model directory of V rows, plus the first call that needs
the whole table (33 000 three-token lines)."""
import argparse
import ctypes as C
import json
import os
import statistics
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_TBS = 8.0      # MI355X: 8 TB/s
DIM = 256
KINDS = {"f32": (0, 4), "f16": (1, 2), "i8": (2, 1)}


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
    L.smt_model_create_from_device.argtypes = [vp, vp, u64, u32, i32, C.POINTER(vp)]
    L.smt_model_destroy.argtypes = [vp]
    L.smt_model_destroy.restype = None
    L.smt_embed_device.argtypes = [vp, vp, vp, u64, u32, vp]
    L.typed = hasattr(L, "smt_model_create_from_device_typed")
    if L.typed:
        L.smt_model_create_from_device_typed.argtypes = [vp, vp, i32, u64, u32, i32, C.POINTER(vp)]
    L.smt_host_model_from_dir.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
    L.smt_host_model_destroy.argtypes = [vp]
    L.smt_host_model_destroy.restype = None
    L.smt_host_encode.argtypes = [vp, C.POINTER(C.c_char_p), u64, u32, vp]
    return L


def ok(L, rc):
    if rc != 0:
        raise RuntimeError(f"error {rc}: {L.smt_last_error().decode(errors='replace')}")


def workload(V, n_lines, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 9, size=n_lines)
    offsets = np.zeros(n_lines + 1, dtype=np.uint64)
    np.cumsum(lens, out=offsets[1:])
    n_tok = int(offsets[-1])
    uniform = rng.integers(0, V, size=n_tok, dtype=np.int64).astype(np.uint32)
    ranks = rng.zipf(1.1, size=n_tok).astype(np.uint64)
    zipf = ((ranks * np.uint64(2654435761)) % np.uint64(V)).astype(np.uint32)     # rank r -> a fixed row somewhere in the table
    return offsets, {"uniform": uniform, "zipf_1.1": zipf}


def bench_kernel(L, args):
    import torch

    ctx = C.c_void_p()
    ok(L, L.smt_ctx_create(0, C.byref(ctx)))
    ok(L, L.smt_prof_enable(ctx, 1))
    V, n_lines = args.v, args.lines
    offsets, idsets = workload(V, n_lines, 5)
    n_tok = int(offsets[-1])
    d_off = torch.from_numpy(offsets.view(np.int64)).cuda()
    d_out = torch.empty((n_lines, DIM), dtype=torch.float32, device="cuda")
    g = torch.Generator(device="cuda")
    g.manual_seed(9)
    base = torch.randn((V, DIM), generator=g, device="cuda", dtype=torch.float32) * 0.1
    results = []
    for kind in ("f32", "f16", "i8"):
        code, elem = KINDS[kind]
        if kind != "f32" and not L.typed:
            continue
        if kind == "f32":
            table = base
        elif kind == "f16":
            table = base.half()
        else:
            table = torch.clamp(torch.round(base * 400), -127, 127).to(torch.int8)
        torch.cuda.synchronize()
        model = C.c_void_p()
        if L.typed:
            ok(L, L.smt_model_create_from_device_typed(ctx, C.c_void_p(table.data_ptr()), code, V, DIM, 1, C.byref(model)))
        else:
            ok(L, L.smt_model_create_from_device(ctx, C.c_void_p(table.data_ptr()), V, DIM, 1, C.byref(model)))
        for name, ids in idsets.items():
            d_ids = torch.from_numpy(ids.view(np.int32)).cuda()
            torch.cuda.synchronize()
            run = lambda: ok(L, L.smt_embed_device(model, C.c_void_p(d_ids.data_ptr()), C.c_void_p(d_off.data_ptr()), n_lines, 2048,
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
            row_bytes = DIM * elem
            tbs = n_tok * row_bytes / (med * 1e-3) / 1e12
            r = {"label": args.label, "table": kind, "ids": name, "V": V, "n_lines": n_lines, "n_tokens": n_tok, "reps": args.reps,
                 "warmup": args.warmup, "median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                 "spread": round((max(ms) - min(ms)) / med, 4), "bytes_per_token": row_bytes, "table_bytes": V * row_bytes,
                 "gathered_TB_per_s": round(tbs, 3), "fraction_of_hbm_peak": round(tbs / HBM_PEAK_TBS, 3)}
            print(json.dumps(r), flush=True)
            results.append(r)
            del d_ids
        L.smt_model_destroy(model)
        if kind != "f32":
            del table
    L.smt_ctx_destroy(ctx)
    return results


def bench_host_load(L, args):
    """smt_host_model_from_dir on an F16 directory of V rows, and the first call that needs the whole table."""
    from safetensors.numpy import save_file

    V = args.host_load_v
    with tempfile.TemporaryDirectory() as d:
        rng = np.random.default_rng(4)
        save_file({"embeddings": (rng.standard_normal((V, DIM), dtype=np.float32) * 0.1).astype(np.float16)}, os.path.join(d, "model.safetensors"))
        with open(os.path.join(d, "vocab.txt"), "w") as f:
            f.write("".join(f"w{i}\n" for i in range(V - 1)) + "[UNK]\n")
        with open(os.path.join(d, "config.json"), "w") as f:
            json.dump({"normalize": True, "unk_token": "[UNK]"}, f)
        n = 33_000
        toks = rng.integers(0, V - 1, size=(n, 3))
        texts = (C.c_char_p * n)(*[f"w{a} w{b} w{c}".encode() for a, b, c in toks])
        out = np.empty((n, DIM), dtype=np.float32)
        ctx = C.c_void_p()
        ok(L, L.smt_ctx_create(0, C.byref(ctx)))
        rows = []
        for rep in range(3):          # (the first repetition reads the file cold and pays one-time runtime set-up)
            h = C.c_void_p()
            t0 = time.perf_counter()
            ok(L, L.smt_host_model_from_dir(ctx, d.encode(), C.byref(h)))
            t1 = time.perf_counter()
            ok(L, L.smt_host_encode(h, texts, n, 2048, out.ctypes.data_as(C.c_void_p)))
            t2 = time.perf_counter()
            L.smt_host_model_destroy(h)
            rows.append({"from_dir_ms": round((t1 - t0) * 1e3, 2), "first_full_table_encode_ms": round((t2 - t1) * 1e3, 2),
                         "total_ms": round((t2 - t0) * 1e3, 2)})
        L.smt_ctx_destroy(ctx)
    r = {"label": args.label, "host_load": "F16 model directory", "V": V, "repetitions": rows}
    print(json.dumps(r), flush=True)
    return [r]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "semtools_amd", "lib", "libsemtools_hip.so"))
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None, help="JSON file; results are appended to the list it holds")
    ap.add_argument("--v", type=int, default=4_000_000)
    ap.add_argument("--lines", type=int, default=8_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-load-v", type=int, default=0)
    ap.add_argument("--skip-kernel", action="store_true")
    args = ap.parse_args()
    L = bind(args.lib)
    results = [] if args.skip_kernel else bench_kernel(L, args)
    if args.host_load_v:
        results += bench_host_load(L, args)
    if args.out:
        old = []
        if os.path.exists(args.out):
            with open(args.out) as f:
                old = json.load(f)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(old + results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
