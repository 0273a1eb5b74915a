"""IVF index searched inside row ranges: one GPU step per invocation, results merged into profiles/ivf_ranges.json.

Corpus: the bench's 20 000-topic generative model (bench.py bench_c5), 10 M rows, per-list PCA codes, nlist 4096; the subset is every
second 1000-row "document".  --index PATH keeps the built index in a file, so that the invocations of one session (and both
libraries) search the same index without building it again.  Steps (--step):
  ranged      the ranged search against the exact range-filtered smt_search of the same subset -- the path it replaces -- in the same
              process.  Both go through their HOST entry points (queries up, answer down, unpacked), both are warmed up by one call
              before the clock starts (the exact search's first call also stages its range plan), both are the mean of the same
              number of calls: per 1000 queries and per single query.  Beside them the ranged search through its device entry point,
              the unfiltered search of the same process, the mask build alone (profiling events around ivf_range_mask_kernel, in a
              pass of its own after the timings), and recall@10 of the ranged search against the exact answer at nprobe 8 / 32.
  unfiltered  smt_ivfpq_search_device without ranges, 1000 queries, nprobe 8, rerank 128: --samples samples, each the mean of --reps
              calls back to back behind one warm-up call.  --tree DIR imports semtools_amd from another checkout (the parent commit,
              built there), so that a driver can alternate this commit and its parent on one device; --label names the sample series
              in the JSON.  A digest of the answer is recorded per label: the two libraries must return the same bytes.
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["ranged", "unfiltered"], required=True)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--label", default="this_commit")
    ap.add_argument("--index", default=None, help="index file: loaded when it exists, else built and saved there")
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_ranges.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)                      # tests.synth
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    import torch

    import semtools_amd as smt
    from tests import synth

    dev = torch.device("cuda:0")
    gen = synth.clustered_model_torch(20000, 8, 11, dev)
    x = synth.clustered_sample_torch(gen, args.rows, 12)
    q = synth.clustered_sample_torch(gen, args.nq, 13).cpu().numpy()
    del gen
    torch.cuda.synchronize()
    ctx = smt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    corpus = smt.Corpus(ctx, device_ptr=x.data_ptr(), rows=args.rows)
    if args.index and os.path.exists(args.index):
        ix = smt.IvfPq.load(corpus, args.index)
    else:
        ix = smt.IvfPq(corpus, nlist=args.nlist, train_iters=10, local_pca=True)
        if args.index:
            ix.save(args.index)
    k, rerank = 10, 128
    qd = torch.from_numpy(q).to(dev)
    o_rows = torch.empty((args.nq, k), dtype=torch.int64, device=dev)
    o_dist = torch.empty((args.nq, k), dtype=torch.float64, device=dev)

    def timed(fn, reps):
        """ms per call: one warm-up call, then `reps` calls back to back, the clock stopped behind a device synchronise"""
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    res = {}
    if os.path.exists(args.out):
        res = json.load(open(args.out))
    res.setdefault("config", dict(rows=args.rows, nlist=args.nlist, nq=args.nq, top_k=k, rerank=rerank, coding="per-list PCA",
                                  corpus="20000 topics (bench.py bench_c5)", subset="every second 1000-row document",
                                  note="one device lease per driver run; wall-clock of whole calls unless said otherwise"))
    if args.step == "unfiltered":
        series = res.setdefault("unfiltered_ms_per_1000_queries", {}).setdefault(args.label, [])
        for _ in range(args.samples):
            ms = timed(lambda: ix.search_device(qd.data_ptr(), args.nq, k, 8, rerank, 0, o_rows.data_ptr(), o_dist.data_ptr()), args.reps)
            series.append(round(ms, 4))
        digest = hashlib.sha256(o_rows.cpu().numpy().tobytes() + o_dist.cpu().numpy().tobytes()).hexdigest()[:16]
        res.setdefault("unfiltered_answer_digest", {}).setdefault(args.label, [])
        if digest not in res["unfiltered_answer_digest"][args.label]:
            res["unfiltered_answer_digest"][args.label].append(digest)
    else:
        ranges = smt.PackedRanges([(b, min(b + 1000, args.rows)) for b in range(0, args.rows, 2000)])
        out = dict(entry="host entry points, one warm-up call, mean of the calls that follow", calls_per_1000_queries_figure=10,
                   calls_per_single_query_figure=50)
        exact_ms = timed(lambda: corpus.search(q, top_k=k, ranges=ranges), 10)
        exact_one = timed(lambda: corpus.search(q[0], top_k=k, ranges=ranges), 50)
        out["exact_filtered_ms_per_1000_queries"] = round(exact_ms, 4)
        out["exact_filtered_ms_single_query"] = round(exact_one, 4)
        for nprobe in (8, 32):
            ms = timed(lambda: ix.search(q, top_k=k, nprobe=nprobe, rerank=rerank, ranges=ranges), 10)
            one = timed(lambda: ix.search(q[0], top_k=k, nprobe=nprobe, rerank=rerank, ranges=ranges), 50)
            plain = timed(lambda: ix.search(q, top_k=k, nprobe=nprobe, rerank=rerank), 10)
            dev_ms = timed(lambda: ix.search_device(qd.data_ptr(), args.nq, k, nprobe, rerank, 0, o_rows.data_ptr(), o_dist.data_ptr(),
                                                    ranges=ranges), 10)
            dev_one = timed(lambda: ix.search_device(qd.data_ptr(), 1, k, nprobe, rerank, 0, o_rows.data_ptr(), o_dist.data_ptr(),
                                                     ranges=ranges), 50)
            out[f"nprobe{nprobe}"] = dict(ranged_ms_per_1000_queries=round(ms, 4), ranged_ms_single_query=round(one, 4),
                                          unfiltered_ms_per_1000_queries_same_process=round(plain, 4),
                                          ranged_device_entry_ms_per_1000_queries=round(dev_ms, 4),
                                          ranged_device_entry_ms_single_query=round(dev_one, 4))
        exact = corpus.search(q, top_k=k, ranges=ranges)
        for nprobe in (8, 32):
            got = ix.search(q, top_k=k, nprobe=nprobe, rerank=rerank, ranges=ranges)
            hit = sum(len(set(r.tolist()) & set(e.tolist())) for (r, _), (e, _) in zip(got, exact))
            out[f"nprobe{nprobe}"]["recall_at_10_vs_exact_filtered"] = round(hit / (args.nq * k), 4)
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(20):
            ix.search_device(qd.data_ptr(), 1, k, 8, rerank, 0, o_rows.data_ptr(), o_dist.data_ptr(), ranges=ranges)
        torch.cuda.synchronize()
        n_m, ms_m = ctx.prof_read("ivf_mask")
        ctx.prof_enable(False)
        out["mask_build_ms"] = round(ms_m / max(n_m, 1), 4)
        out["mask_build_ranges"] = ranges.n
        res["ranged"] = out
    u = res.get("unfiltered_ms_per_1000_queries", {})
    if u:
        summ = {lab: dict(median=float(np.median(v)), min=min(v), max=max(v), samples=len(v)) for lab, v in u.items()}
        if "parent" in summ and "this_commit" in summ:
            summ["this_commit_median_within_parent_spread"] = bool(summ["parent"]["min"] <= summ["this_commit"]["median"] <= summ["parent"]["max"])
            summ["this_commit_median_not_above_parent_max"] = bool(summ["this_commit"]["median"] <= summ["parent"]["max"])
        res["unfiltered_summary"] = summ
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res.get("ranged") if args.step == "ranged" else res.get("unfiltered_summary")), flush=True)
    ix.close(); corpus.close(); ctx.close()


if __name__ == "__main__":
    main()
