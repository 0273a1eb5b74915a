"""What carrying an IVF index through a compaction costs, against the path it replaces, in one process on one GPU.

Corpus: the bench's 20 000-topic generative model (bench.py bench_c5), --rows rows (the documented runs: 1 M and 10 M), per-list PCA
codes; the keep list is every second 1000-row "document".  Timed, as whole calls with the clock stopped behind a synchronise:
  carry     IvfPq.compact(keep)                                  (smt_ivfpq_compact: the rows move, the index follows)
  replaced  Corpus.compact(keep) + IvfPq.close() + IvfPq(...)    (the rows move, the index is destroyed and built again)
A compaction consumes its corpus, so every call gets a fresh one: the rows are appended again and the index is loaded from the file
the first build wrote -- outside the clock.  Each side runs --reps calls behind one warm-up call and every call's time is kept.
Then recall@10 (1000 queries, nprobe 8, rerank 128) of the carried index and of the rebuilt one against the exact answer on the
compacted corpus.  No gate: the feature does not depend on a ratio.  Results are merged into --out under the key rows_<rows>."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--nlist", type=int, default=0, help="0 = 4096 at >= 4 M rows, else 1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_compact.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import semtools_amd as smt
    from tests import synth

    n = args.rows
    nlist = args.nlist or (4096 if n >= 4_000_000 else 1024)
    dev = torch.device("cuda:0")
    gen = synth.clustered_model_torch(20000, 8, 11, dev)
    xh = synth.clustered_sample_torch(gen, n, 12).cpu().numpy()
    q = synth.clustered_sample_torch(gen, args.nq, 13).cpu().numpy()
    del gen
    torch.cuda.empty_cache()
    ctx = smt.Context(0)
    keep = [(b, min(b + 1000, n)) for b in range(0, n, 2000)]
    kept = sum(e - b for b, e in keep)
    index_file = os.path.join(tempfile.mkdtemp(prefix="ab_ivf_compact_"), "full.ivf")

    def fresh():
        """an uncompacted corpus with its index (built once, loaded from its file afterwards)"""
        c = smt.Corpus(ctx)
        c.append(xh)
        if os.path.exists(index_file):
            ix = smt.IvfPq.load(c, index_file)
        else:
            ix = smt.IvfPq(c, nlist=nlist, train_iters=10, local_pca=True)
            ix.save(index_file)
        ctx.synchronize()
        return c, ix

    def carry():
        c, ix = fresh()
        t0 = time.perf_counter()
        moved, dropped = ix.compact(keep)
        ctx.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        assert c.rows == kept and dropped == n - kept and ix.info()["rows"] == kept
        return ms, c, ix

    def replaced():
        c, ix = fresh()
        t0 = time.perf_counter()
        c.compact(keep)
        ix.close()
        ix = smt.IvfPq(c, nlist=nlist, train_iters=10, local_pca=True)
        ctx.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, c, ix

    def series(fn):
        """every call's ms behind one warm-up call; the last call's corpus and index stay for the recall figures"""
        out, c, ix = [], None, None
        for i in range(args.reps + 1):
            if c is not None:
                ix.close(); c.close()
            ms, c, ix = fn()
            if i:
                out.append(round(ms, 3))
        return out, c, ix

    def recall(c, ix):
        exact = c.search(q, top_k=10)
        got = ix.search(q, top_k=10, nprobe=8, rerank=128)
        return round(sum(len(set(r.tolist()) & set(e.tolist())) for (r, _), (e, _) in zip(got, exact)) / (args.nq * 10), 4)

    res = dict(rows=n, kept_rows=kept, keep_ranges=len(keep), nlist=nlist, coding="per-list PCA", reps=args.reps,
               corpus="20000 topics (bench.py bench_c5)", keep_list="every second 1000-row document",
               note="one device lease, one process; wall-clock of whole calls behind one warm-up call, every call kept")
    ms, c, ix = series(carry)
    res["carry_ms"] = ms
    res["carry_recall_at_10"] = recall(c, ix)
    ix.close(); c.close()
    ms, c, ix = series(replaced)
    res["replaced_ms"] = ms
    res["rebuilt_recall_at_10"] = recall(c, ix)
    res["rebuild_alone_ms"] = {k: round(v, 3) for k, v in ix.info()["build_ms"].items()}
    ix.close(); c.close()
    res["carry_ms_mean"] = round(float(np.mean(res["carry_ms"])), 3)
    res["replaced_ms_mean"] = round(float(np.mean(res["replaced_ms"])), 3)
    all_res = json.load(open(args.out)) if os.path.exists(args.out) else {}
    all_res[f"rows_{n}"] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(all_res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    os.remove(index_file)
    os.rmdir(os.path.dirname(index_file))
    ctx.close()


if __name__ == "__main__":
    main()
