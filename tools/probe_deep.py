"""Counter runs for groups of sixteen against groups of eight (scan_deep_kernel against scan_wide_kernel), and the worst case.

  rocprofv3 --pmc FETCH_SIZE SQ_INSTS_VALU SQ_WAVE_CYCLES SQ_WAIT_INST_ANY --output-format csv -d DIR -o p -- \
      python tools/probe_deep.py counters LIMIT [rows]   400 steps after 300 over two corpora in turn (as bench.py) at the group limit
      LIMIT (7: scan_take, scan_wide_kernel; 15: scan_deep, scan_deep_kernel).  Counter collection serialises kernels: the host is
      far ahead of them, and the scans find their successors' descriptors waiting
  rocprofv3 --pmc ... -- python tools/probe_deep.py worst LIMIT [one]   the worst case for the same run and fold: 65 536 rows whose
      distance to sixteen queries falls with the row number (the steep corpus of tests/test_gpu_scan_deep.py), so every row inserts
      in every list.  The corpus scans faster than the host issues calls: each batch of 64 calls is queued behind two calls over
      a 4 M-row corpus, one per internal stream, so that the scans find their successors' descriptors waiting and wait for nothing
      themselves.  `one`: three corpora of the same rows at different addresses in turn, so that every pass serves one call
  python tools/probe_deep.py fold DIR [out.json]   the counter run per LEADER (a launch that ran the row loop) and per call served"""
import collections, csv, glob, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KERNELS = ("scan_deep_kernel", "scan_wide_kernel", "scan_pair_kernel", "scan_topk_kernel")


def fold(d):
    """per kernel: the leaders (launches with more than a tenth of the largest SQ_INSTS_VALU: an absorbed launch ends before its
    first row), the median of every counter and of the duration per leader"""
    by = collections.defaultdict(lambda: collections.defaultdict(float))
    dur, name = {}, {}
    for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            kern = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
            if kern is None:
                continue
            key = (f, r["Dispatch_Id"])
            by[key][r["Counter_Name"]] += float(r["Counter_Value"])
            dur[key] = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            name[key] = kern
    med = lambda xs: sorted(xs)[len(xs) // 2]
    res = {}
    for kern in KERNELS:
        keys = [k for k in by if name[k] == kern]
        if not keys:
            continue
        top = max(by[k]["SQ_INSTS_VALU"] for k in keys)
        lead = [k for k in keys if by[k]["SQ_INSTS_VALU"] > top / 10]
        res[kern] = {"launches": len(keys), "leaders": len(lead), "dur_per_leader_median_us": round(med([dur[k] for k in lead]), 1)}
        for c in sorted(by[lead[0]]):
            res[kern][c + "_per_leader_median"] = med([by[k][c] for k in lead])
        # the leaders of FULL groups: within a tenth of the largest SQ_INSTS_VALU (a pass of fewer calls issues fewer instructions)
        full = [k for k in lead if by[k]["SQ_INSTS_VALU"] > 0.9 * top]
        res[kern]["full_groups"] = {"leaders": len(full), "dur_median_us": round(med([dur[k] for k in full]), 1),
                                    **{c + "_median": med([by[k][c] for k in full]) for c in sorted(by[full[0]])}}
    return res


def main():
    mode = sys.argv[1]
    if mode == "fold":
        report = json.dumps(fold(sys.argv[2]), indent=1)
        if len(sys.argv) > 3:
            open(sys.argv[3], "w").write(report + "\n")
        print(report)
        return
    import torch
    import semtools_amd as smt
    limit = int(sys.argv[2])
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(59)
    if mode == "worst":
        rows, one = 65_536, len(sys.argv) > 3 and sys.argv[3] == "one"
        basis = torch.linalg.qr(torch.randn(256, 18, device=dev, generator=g, dtype=torch.float64))[0].T
        theta = torch.linspace(1.5, 0.1, rows, device=dev, dtype=torch.float64)
        x = (torch.cos(theta)[:, None] * basis[0] + torch.sin(theta)[:, None] * basis[1]).float().contiguous()
        data = [x, x.clone(), x.clone()] if one else [x]
        qs = (basis[0] + 0.2 * basis[2:18]).float().contiguous()
        batches = 10
        xb = torch.randn(4_000_000, 256, device=dev, generator=g)
    else:
        rows = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
        data = []
        for _ in range(2):
            x = torch.randn(rows, 256, device=dev, generator=g); x /= x.norm(dim=1, keepdim=True)
            data.append(x)
        qs = torch.randn(16, 256, device=dev, generator=g); qs /= qs.norm(dim=1, keepdim=True)
        batches = 11
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    ctx = smt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    corpora = [smt.Corpus(ctx, device_ptr=t.data_ptr(), rows=rows) for t in data]
    blocker = smt.Corpus(ctx, device_ptr=xb.data_ptr(), rows=4_000_000) if mode == "worst" else None
    calls = 64
    out = torch.empty((calls + 2, 2, 10), dtype=torch.int64, device=dev)
    st = torch.full((calls + 2,), 7, dtype=torch.int32, device=dev)
    ctx.set_tuning("prof_select", 0)
    ctx.set_tuning("async_select", 1)
    ctx.set_tuning("scan_take" if limit < 8 else "scan_deep", limit)
    g0, d0 = ctx.scan_groups_wide(), ctx.scan_groups_deep()
    for b in range(batches):
        for j in range(calls, calls + 2 if blocker else calls):
            blocker.search_topk_device(qs[0].data_ptr(), 1, 10, 0, out[j, 0].data_ptr(), out[j, 1].data_ptr(), out_status_ptr=st[j:].data_ptr())
        for i in range(calls):
            corpora[i % len(corpora)].search_topk_device(qs[(i // 2) % 16].data_ptr(), 1, 10, 0, out[i, 0].data_ptr(), out[i, 1].data_ptr(),
                                                         out_status_ptr=st[i:].data_ptr())
        ctx.synchronize()
    ok = bool((st[:calls].cpu() == 0).all())
    if mode == "worst":
        ok = ok and bool((out[:calls, 0].cpu() == torch.arange(rows - 1, rows - 11, -1)).all())
    print(json.dumps({"mode": mode, "limit": limit, "rows": rows, "calls": batches * calls,
                      "launches_by_calls_served": [b - a for a, b in zip(g0, ctx.scan_groups_wide())],
                      "deep_launches_by_calls_served": [b - a for a, b in zip(d0, ctx.scan_groups_deep())], "status_0": ok}))


if __name__ == "__main__":
    main()
