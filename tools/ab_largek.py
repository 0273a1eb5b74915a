"""A/B of the large-k routes in one process: tuning key largek_sampled 1 (sampled threshold, collect, exact finish: topk_large.hip)
against 0 (all keys + radix sort: largek.hip), host-form smt_search, wall ms per call.  Legs: 1 query x 1 M rows at k = 57, 100,
1000; 256 queries x 10 M rows at k = 100 next to k = 10 (the K3 sweep); the fraction of device-form answers that were not PROVED.
Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import semtools_amd as smt  # noqa: E402


def unit(n, dev, g):
    x = torch.empty(n, 256, device=dev)
    for b in range(0, n, 2_000_000):
        e = min(n, b + 2_000_000)
        c = torch.randn(e - b, 256, device=dev, generator=g)
        x[b:e] = c / c.norm(dim=1, keepdim=True)
    return x


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    ctx = smt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    out = {"tool": "ab_largek"}
    x1 = unit(1_000_000, dev, g)
    c1 = smt.Corpus(ctx, device_ptr=x1.data_ptr(), rows=1_000_000)
    q1 = torch.nn.functional.normalize(torch.randn(64, 256, device=dev, generator=g), dim=1)
    qh = q1.cpu().numpy()
    for k in (57, 100, 1000):
        for rep in range(2):   # alternate the routes
            for s in (1, 0):
                ctx.set_tuning("largek_sampled", s)
                ms = timed(lambda: c1.search(qh[:1], top_k=k), 20)
                out.setdefault(f"1x1M_k{k}_{'sampled' if s else 'allkeys'}_ms", []).append(round(ms, 4))
    ctx.set_tuning("largek_sampled", 1)
    # fallback fraction of the device form: 64 queries x 1 M rows at each k
    st = torch.empty(64, dtype=torch.int32, device=dev)
    n_bad = n_all = 0
    for k in (57, 100, 1000):
        rows = torch.empty((64, k), dtype=torch.int64, device=dev)
        dist = torch.empty((64, k), dtype=torch.float64, device=dev)
        c1.search_topk_device(q1.data_ptr(), 64, k, 0, rows.data_ptr(), dist.data_ptr(), st.data_ptr())
        torch.cuda.synchronize()
        n_bad += int((st != 0).sum())
        n_all += 64
    out["device_not_proved_fraction_1M"] = n_bad / n_all
    c1.close()
    del x1
    x10 = unit(10_000_000, dev, g)
    c10 = smt.Corpus(ctx, device_ptr=x10.data_ptr(), rows=10_000_000)
    q10 = torch.nn.functional.normalize(torch.randn(256, 256, device=dev, generator=g), dim=1).cpu().numpy()
    out["256x10M_k10_ms"] = round(timed(lambda: c10.search(q10, top_k=10), 3), 3)
    for s in (1, 0):
        ctx.set_tuning("largek_sampled", s)
        out[f"256x10M_k100_{'sampled' if s else 'allkeys'}_ms"] = round(timed(lambda: c10.search(q10, top_k=100), 2), 3)
    ctx.set_tuning("largek_sampled", 1)
    ctx.uncertain_count(reset=True)
    c10.search(q10, top_k=100)
    out["256x10M_k100_not_proved_fraction"] = ctx.uncertain_count(reset=True) / 256
    c10.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
