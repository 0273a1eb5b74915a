"""What a compaction costs, in one process on one GPU: smt_corpus_compact (rows moved HBM to HBM in place, compact.hip) against
the method the workspace store used before it -- smt_corpus_read_rows of every live extent into a host buffer and
smt_corpus_append_host into a fresh corpus in runs of up to 64 Ki rows (Store::compact_if_sparse's copy through the host).

Sizes 1 M and 10 M rows; keep lists: documents of 20 rows with every second one dead, and a single dead row at position 0.
Host clock around call + synchronize, median of --reps runs, each in-place run on a fresh copy of the corpus.  Also the bytes/s
the in-place move achieved, counting 2 x the moved bytes for direct steps and 4 x for bounced ones, beside the 8 TB/s peak.
Prints one JSON line and writes it to --out (default profiles/compact_ab.json).  Run it under `timeout`."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import semtools_amd as smt  # noqa: E402
from semtools_amd import _lib as L  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = 65536
PEAK_TBS = 8.0


def keep_lists(n):
    docs = [(b, min(b + 20, n)) for b in range(0, n, 40)]          # documents of 20 rows, every second one dead
    return {"docs20_every_second_dead": docs, "one_dead_row_at_0": [(1, n)]}


def plan(keep, n_rows, bounce):
    """compact.hip's planner: (rows moved by direct steps, rows moved by bounced steps, enqueues)"""
    begins = np.array([b for b, e in keep], dtype=np.int64)
    lens = np.array([e - b for b, e in keep], dtype=np.int64)
    prefix = np.concatenate([[0], np.cumsum(lens)])
    new_rows = int(prefix[-1])
    off = np.nonzero(begins != prefix[:-1])[0]
    if not len(off):
        return 0, 0, 0
    v, direct, bounced, enq = int(prefix[off[0]]), 0, 0, 0
    while v < new_rows:
        ri = int(np.searchsorted(prefix, v, side="right")) - 1
        delta = int(begins[ri]) - int(prefix[ri])
        if delta >= bounce:
            w = min(delta, new_rows - v)
            direct += w
            enq += 1
        else:
            w = min(bounce, new_rows - v)
            bounced += w
            enq += 2
        v += w
    return direct, bounced, enq


def fill(ctx, n, block):
    c = smt.Corpus(ctx, capacity_rows=n)
    at = 0
    while at < n:
        m = min(len(block), n - at)
        c.append(block[:m])
        at += m
    return c


def through_the_host(ctx, src, keep, buf):
    """the store's old compaction: every live extent read into the run buffer, one append per run; returns the fresh corpus"""
    lib = L.lib()
    fresh = C.c_void_p()
    L.check(lib.smt_corpus_create(ctx._h, L.DIM, 0, C.byref(fresh)))
    base = buf.ctypes.data
    run_rows = 0
    first = C.c_uint64(0)
    for b, e in keep:
        n = e - b
        if run_rows and run_rows + n > RUN:
            L.check(lib.smt_corpus_append_host(fresh, C.c_void_p(base), run_rows, C.byref(first)))
            run_rows = 0
        L.check(lib.smt_corpus_read_rows(src._h, b, n, C.c_void_p(base + run_rows * 1024)))
        run_rows += n
    if run_rows:
        L.check(lib.smt_corpus_append_host(fresh, C.c_void_p(base), run_rows, C.byref(first)))
    return smt.Corpus(ctx, _handle=fresh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_ab.json"))
    args = ap.parse_args()
    ctx = smt.Context(0)
    rng = np.random.default_rng(3)
    block = np.ascontiguousarray(rng.standard_normal((RUN, 256), dtype=np.float32))
    out = {"tool": "ab_compact", "reps": args.reps, "bounce_rows": 65536, "peak_TBps": PEAK_TBS, "legs": []}
    for n in [int(s) for s in args.sizes.split(",")]:
        for name, keep in keep_lists(n).items():
            kept = sum(e - b for b, e in keep)
            direct, bounced, enq = plan(keep, n, 65536)
            t_in, moved = [], 0
            for rep in range(args.reps + 1):                        # (the first run warms up: scratch, code objects)
                c = fill(ctx, n, block)
                ctx.synchronize()
                t0 = time.perf_counter()
                moved = c.compact(keep)
                ctx.synchronize()
                t_in.append((time.perf_counter() - t0) * 1e3)
                probe = [0, kept // 2, kept - 1]
                for v in probe:                                     # the moved rows are the ones the list names
                    src = v // 20 * 40 + v % 20 if name.startswith("docs20") else v + 1
                    assert c.rows == kept and np.array_equal(c.read_rows(v, 1)[0], block[src % RUN]), (name, v)
                c.close()
            assert moved == direct + bounced, (moved, direct, bounced)
            src_c = fill(ctx, n, block)
            buf = np.empty((max(RUN, max(e - b for b, e in keep)), 256), dtype=np.float32)
            t_host = []
            for rep in range(args.reps + 1):
                ctx.synchronize()
                t0 = time.perf_counter()
                fresh = through_the_host(ctx, src_c, keep, buf)
                ctx.synchronize()
                t_host.append((time.perf_counter() - t0) * 1e3)
                assert fresh.rows == kept
                fresh.close()
            src_c.close()
            del buf
            ms_in, ms_host = float(np.median(t_in[1:])), float(np.median(t_host[1:]))
            traffic = (2 * direct + 4 * bounced) * 1024
            out["legs"].append({"rows": n, "keep": name, "kept_rows": kept, "rows_moved": moved, "direct_rows": direct,
                                "bounced_rows": bounced, "enqueues": enq, "in_place_ms": round(ms_in, 3),
                                "through_host_ms": round(ms_host, 1), "speedup": round(ms_host / ms_in, 1),
                                "traffic_bytes": traffic, "achieved_TBps": round(traffic / (ms_in * 1e-3) / 1e12, 3),
                                "share_of_peak": round(traffic / (ms_in * 1e-3) / 1e12 / PEAK_TBS, 3)})
            print(json.dumps(out["legs"][-1]), flush=True)
    ctx.close()
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
