"""What do scan_wide_kernel's top-k list inserts cost?  One 1 M-row corpus in two row orders, (a) random and (b) the same rows sorted
by ascending distance to the query, one query repeated so that groups of eight form (scan_take = 7, the same query eight times in a
group).  In order (b) a wave's first k' rows are its best: it stops inserting after them, and the row loads, the reductions, the
candidate tests and the block tail are those of order (a).  The difference between the orders is the inserts.

  python tools/probe_insert_cost.py time [rows] [rounds] [out.json]    median us per pipelined step, orders alternated in one process
  rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVE_CYCLES SQ_WAIT_INST_ANY --output-format csv -d DIR -o p -- \
      python tools/probe_insert_cost.py counters random|sorted [rows]  400 steps after 300 for the counter run (one order per run)
  rocprofv3 --pmc ... -- python tools/probe_insert_cost.py worst       the worst case, for the same counter run and fold: 65 536 rows whose
      distance to eight queries falls with the row number (the steep corpus of tests/test_gpu_scan_wide.py), so every row inserts
      in all eight lists.  The corpus scans faster than the host issues calls: each batch of 64 calls is queued behind ~5 ms of
      copies on the caller's stream, so that the scans find their successors' descriptors waiting and wait for nothing themselves
  python tools/probe_insert_cost.py fold DIR [out.json]                the counter run per LEADER (a launch that ran the row loop)
(tools/summarize_pmc.py DIR gives the same run averaged over every launch, absorbed ones included.)"""
import collections, csv, glob, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def fold(d):
    """per scan_wide_kernel leader: the median of every counter and of the duration; leaders are the launches with more than a
    tenth of the largest SQ_INSTS_VALU (an absorbed launch ends before its first row)"""
    by = collections.defaultdict(lambda: collections.defaultdict(float))
    dur = {}
    for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if "scan_wide_kernel" not in r["Kernel_Name"]:
                continue
            by[(f, r["Dispatch_Id"])][r["Counter_Name"]] += float(r["Counter_Value"])
            dur[(f, r["Dispatch_Id"])] = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    if not by:
        return {"launches": 0}
    top = max(v["SQ_INSTS_VALU"] for v in by.values())
    lead = [k for k, v in by.items() if v["SQ_INSTS_VALU"] > top / 10]
    med = lambda xs: sorted(xs)[len(xs) // 2]
    res = {"launches": len(by), "leaders": len(lead), "dur_per_leader_median_us": round(med([dur[k] for k in lead]), 1)}
    for c in sorted(by[lead[0]]):
        res[c + "_per_leader_median"] = med([by[k][c] for k in lead])
    return res


def worst(torch, smt, rows=65_536, batches=10, calls=64):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(59)
    basis = torch.linalg.qr(torch.randn(256, 10, device=dev, generator=g, dtype=torch.float64))[0].T
    theta = torch.linspace(1.5, 0.1, rows, device=dev, dtype=torch.float64)
    x = (torch.cos(theta)[:, None] * basis[0] + torch.sin(theta)[:, None] * basis[1]).float().contiguous()
    qs = (basis[0] + 0.2 * basis[2:10]).float().contiguous()
    big = torch.ones(256 << 20, dtype=torch.float32, device=dev); big2 = torch.empty_like(big)
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    ctx = smt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    c = smt.Corpus(ctx, device_ptr=x.data_ptr(), rows=rows)
    out = torch.empty((calls, 2, 10), dtype=torch.int64, device=dev)
    st = torch.full((calls,), 7, dtype=torch.int32, device=dev)
    ctx.set_tuning("prof_select", 0)
    ctx.set_tuning("async_select", 1)
    ctx.set_tuning("scan_take", 7)
    g0 = ctx.scan_groups_wide()
    for b in range(batches):
        for _ in range(10):
            torch.mul(big, 1.0, out=big2)
        for i in range(calls):
            c.search_topk_device(qs[(i // 2) % 8].data_ptr(), 1, 10, 0, out[i, 0].data_ptr(), out[i, 1].data_ptr(), out_status_ptr=st[i:].data_ptr())
        ctx.synchronize()
    ok = bool((st.cpu() == 0).all()) and bool((out[:, 0].cpu() == torch.arange(rows - 1, rows - 11, -1)).all())
    print(json.dumps({"rows": rows, "calls": batches * calls, "launches_by_calls_served": [b - a for a, b in zip(g0, ctx.scan_groups_wide())],
                      "status_0_and_the_last_rows": ok}))


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    if mode == "fold":
        report = json.dumps(fold(sys.argv[2]), indent=1)
        if len(sys.argv) > 3:
            open(sys.argv[3], "w").write(report + "\n")
        print(report)
        return
    import torch
    import semtools_amd as smt
    if mode == "worst":
        return worst(torch, smt)
    if mode == "counters":
        orders, rows, rounds, out_path = (sys.argv[2],), int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000, 1, None
    else:
        orders = ("random", "sorted")
        rows = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
        rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
        out_path = sys.argv[4] if len(sys.argv) > 4 else None
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(3)
    x = torch.randn(rows, 256, device=dev, generator=g); x /= x.norm(dim=1, keepdim=True)
    q = torch.randn(1, 256, device=dev, generator=g); q /= q.norm(dim=1, keepdim=True)
    data = {"random": x}
    if "sorted" in orders:
        data["sorted"] = x[torch.argsort((x.double() @ q[0].double()), descending=True)].contiguous()   # nearest first
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    ctx = smt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    corpora = {o: smt.Corpus(ctx, device_ptr=data[o].data_ptr(), rows=rows) for o in orders}
    out = torch.empty((64, 2, 10), dtype=torch.int64, device=dev)
    st = torch.full((2048,), 7, dtype=torch.int32, device=dev)

    def run(n, c):
        for i in range(n):
            c.search_topk_device(q.data_ptr(), 1, 10, 0, out[i % 64, 0].data_ptr(), out[i % 64, 1].data_ptr(), out_status_ptr=st[i % 2048:].data_ptr())
        ctx.synchronize()
    ctx.set_tuning("prof_select", 0)
    ctx.set_tuning("async_select", 1)
    ctx.set_tuning("scan_take", 7)
    steps = 400 if mode == "counters" else 2000
    res = {o: [] for o in orders}
    for r in range(rounds):
        for o in orders:
            run(300, corpora[o])
            st.fill_(7)
            g0 = ctx.scan_groups_wide()
            t0 = time.perf_counter(); run(steps, corpora[o]); step = (time.perf_counter() - t0) / steps * 1e6
            g1 = ctx.scan_groups_wide()
            ok = bool((st[:steps].cpu() == 0).all()) and bool((out[:, 0] == out[0, 0]).all())
            res[o].append({"step_us": round(step, 2), "launches_by_calls_served": [b - a for a, b in zip(g0, g1)], "status_0_and_one_answer": ok})
            print(json.dumps({"round": r, "order": o, **res[o][-1]}), file=sys.stderr, flush=True)
    summary = {o: {"median_step_us": sorted(x["step_us"] for x in v)[len(v) // 2], "min": min(x["step_us"] for x in v),
                   "max": max(x["step_us"] for x in v), "all_ok": all(x["status_0_and_one_answer"] for x in v)} for o, v in res.items()}
    if len(orders) == 2:
        a, b = summary["random"]["median_step_us"], summary["sorted"]["median_step_us"]
        summary["sorted_faster_by_pct"] = round(100.0 * (a - b) / a, 2)
    report = json.dumps({"rows": rows, "rounds": rounds, "steps": steps, "scan_take": 7, "summary": summary, "by_order": res}, indent=1)
    if out_path:
        open(out_path, "w").write(report + "\n")
    print(report)


if __name__ == "__main__":
    main()
