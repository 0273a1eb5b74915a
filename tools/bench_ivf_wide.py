"""Wide IVF searches (top_k 57 ... 1024 from the candidate pool): times, kernel shares and recall, written to profiles/ivf_wide.json.

Corpus: the bench's 20 000-topic generative model (bench.py bench_c5), 10 M rows, per-list PCA codes, nlist 4096.  One process, one
device lease.  For nprobe in {8, 32} x rerank in {128, 512} x nq in {1, 1000}:
  narrow_k56     smt_ivfpq_search_device at top_k = 56: the narrow route, the first comparison figure
  wide_k100/1000 smt_ivfpq_search_wide_device
each as ms per call (one warm-up call, then the mean of the calls that follow, the clock stopped behind a device synchronise) with
the ADC and finish (narrow: select) kernels' microseconds per call from the library's profiling events, taken in a pass of their own.
The second comparison figure is the exact large-k route, smt_search_topk_device at the same k: what a caller who wants 100 hits has
without this route.  Recall@100 and recall@1000 are against that exact answer.  The single-query finish is also timed over the largest
pool there is (nprobe 512 x 512 slots = 256 Ki keys).  The expectations the figures are held against are spelled out in the file."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summarise(res):
    """The expectations the figures are held against, each with its ratios and a verdict worked out from them."""
    def ratio(a, b):
        return round(a / b, 3) if a and b else None

    checks = {}
    for nqk, leg in res["legs"].items():
        for name, v in leg.items():
            if not name.startswith("nprobe"):
                continue
            for k in (100, 1000):
                w, n = v[f"wide_k{k}"], v["narrow_k56"]
                checks[f"{nqk}_{name}_k{k}"] = dict(wide_adc_over_narrow_adc=ratio(w["ivf_adc"], n["ivf_adc"]),
                                                    finish_over_adc=ratio(w["ivf_finish"], w["ivf_adc"]),
                                                    wide_call_over_narrow_call=ratio(w["ms_per_call"], n["ms_per_call"]),
                                                    exact_large_k_over_wide_call=ratio(leg["exact_large_k_ms_per_call"][f"k{k}"], w["ms_per_call"]))

    def span(key, pick):
        v = [c[key] for name, c in checks.items() if pick(name) and c[key] is not None]
        return [min(v), max(v)] if v else None

    def batch(name):
        return not name.startswith("nq1_")

    adc = span("wide_adc_over_narrow_adc", batch)
    fin100 = span("finish_over_adc", lambda n: batch(n) and n.endswith("_k100"))
    fin1000 = span("finish_over_adc", lambda n: batch(n) and n.endswith("_k1000"))
    one = span("finish_over_adc", lambda n: not batch(n))
    res["expectations"] = dict(
        wide_adc_within_a_few_per_cent_of_narrow_adc=dict(
            why="same bytes read, more keys written, no block merge", batch_ratio_min_max=adc,
            one_query_ratio_min_max=span("wide_adc_over_narrow_adc", lambda n: not batch(n)),
            verdict="confirmed" if adc and 0.9 <= adc[0] and adc[1] <= 1.1 else "refuted"),
        batch_finish_well_under_its_adc_time=dict(
            finish_over_adc_at_k100_min_max=fin100, finish_over_adc_at_k1000_min_max=fin1000,
            verdict="confirmed" if fin1000 and fin1000[1] < 0.5 else
                    "refuted: at k = 1000 the finish reaches or passes the ADC time" if fin100 and fin100[1] < 1.0 else "refuted"),
        single_query_finish_over_a_large_pool_may_be_the_weak_spot=dict(
            finish_over_adc_min_max=one, large_pools_us=res.get("single_query_finish_over_a_large_pool_us"),
            verdict="confirmed: one block's finish costs more than the query's ADC scan" if one and one[0] > 1.0 else "refuted"),
        against_the_two_comparison_figures=dict(
            wide_call_over_narrow_k56_call_min_max=span("wide_call_over_narrow_call", lambda n: True),
            exact_large_k_call_over_wide_call_min_max=span("exact_large_k_over_wide_call", lambda n: True)),
        ratios=checks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--index", default=None, help="index file: loaded when it exists, else built and saved there")
    ap.add_argument("--box", default="MI355X (gfx950)")
    ap.add_argument("--commit", default=None, help="names the commit in the file (default: git rev-parse of this checkout)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_wide.json"))
    ap.add_argument("--resummarise", default=None, metavar="FILE",
                    help="no GPU: read a result file, work the expectations out of its figures again, write it to --out")
    args = ap.parse_args()
    if args.resummarise:
        res = json.load(open(args.resummarise))
        if args.commit:
            res["config"]["commit"] = args.commit
        summarise(res)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({k: v.get("verdict") for k, v in res["expectations"].items() if isinstance(v, dict) and "verdict" in v}))
        return
    sys.path.insert(0, ROOT)
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
    qd = torch.from_numpy(q).to(dev)
    o_rows = torch.empty((args.nq, 1024), dtype=torch.int64, device=dev)
    o_dist = torch.empty((args.nq, 1024), dtype=torch.float64, device=dev)

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    def kernels_us(fn, reps, names):
        """microseconds per call of the named profiling pairs, in a pass of its own"""
        fn()
        torch.cuda.synchronize()
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out = {}
        for name in names:
            n, ms = ctx.prof_read(name)
            out[name] = round(ms / reps * 1e3, 2) if n else None
        ctx.prof_enable(False)
        return out

    def ivf(nq, k, nprobe, rerank, wide):
        return lambda: ix.search_device(qd.data_ptr(), nq, k, nprobe, rerank, 0, o_rows.data_ptr(), o_dist.data_ptr(), wide=wide)

    def exact(nq, k):
        return lambda: corpus.search_topk_device(qd.data_ptr(), nq, k, 0, o_rows.data_ptr(), o_dist.data_ptr())

    def rows_of(nq, k):
        torch.cuda.synchronize()
        return o_rows.view(-1)[:nq * k].view(nq, k).cpu().numpy()   # (the answers are [nq][k], packed at the buffer's start)

    commit = args.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
            commit = (commit + " + this change") if commit else "this change"
        except OSError:
            commit = "this change"
    res = dict(config=dict(rows=args.rows, nlist=args.nlist, coding="per-list PCA", corpus="20000 topics (bench.py bench_c5)",
                           box=args.box, commit=commit,
                           entry="device entry points; ms per call = one warm-up call, then the mean of the calls that follow",
                           kernel_us="per call, from the library's profiling events (ivf_adc; ivf_finish = the pool's finish, "
                                     "select = the narrow route's select stage), in a pass of their own"))
    legs = {}
    for nq, reps in ((1, 30), (args.nq, 4)):
        ex = {}
        for k in (100, 1000):
            ex[k] = round(timed(exact(nq, k), max(2, reps // 2)), 4)
        legs[f"nq{nq}"] = dict(exact_large_k_ms_per_call={f"k{k}": v for k, v in ex.items()})
        for nprobe in (8, 32):
            for rerank in (128, 512):
                leg = {}
                leg["narrow_k56"] = dict(ms_per_call=round(timed(ivf(nq, 56, nprobe, rerank, False), reps), 4),
                                         **kernels_us(ivf(nq, 56, nprobe, rerank, False), reps, ("ivf_adc", "select")))
                for k in (100, 1000):
                    leg[f"wide_k{k}"] = dict(ms_per_call=round(timed(ivf(nq, k, nprobe, rerank, True), reps), 4),
                                             **kernels_us(ivf(nq, k, nprobe, rerank, True), reps, ("ivf_adc", "ivf_finish")))
                legs[f"nq{nq}"][f"nprobe{nprobe}_rerank{rerank}"] = leg
    res["legs"] = legs

    # recall against the exact answer
    recall = {}
    for k in (100, 1000):
        exact(args.nq, k)()
        want = rows_of(args.nq, k)
        for nprobe in (8, 32):
            for rerank in (128, 512):
                ivf(args.nq, k, nprobe, rerank, True)()
                got = rows_of(args.nq, k)
                hit = sum(len(set(g.tolist()) & set(w.tolist())) for g, w in zip(got, want))
                recall.setdefault(f"recall_at_{k}", {})[f"nprobe{nprobe}_rerank{rerank}"] = round(hit / (args.nq * k), 4)
    res["recall_vs_exact"] = recall

    # the single-query finish over a large pool: one block, eight radix passes
    big = {}
    for nprobe in (32, 512):
        for k in (100, 1000):
            us = kernels_us(ivf(1, k, nprobe, 512, True), 20, ("ivf_adc", "ivf_finish"))
            big[f"P{nprobe * 512 // 1024}Ki_k{k}"] = dict(pool_keys=nprobe * 512, **us)
    res["single_query_finish_over_a_large_pool_us"] = big

    summarise(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(recall=recall, big=big)), flush=True)
    ix.close(); corpus.close(); ctx.close()


if __name__ == "__main__":
    main()
