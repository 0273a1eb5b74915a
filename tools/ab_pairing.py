"""A/B of grouped one-query scans (tuning keys scan_take = 0 .. 7 and scan_deep = 8 .. 15 later calls taken along; scan_gate_pct swept
at the limit of fifteen) in ONE process on one box, settings alternated: the wall time per pipelined step (async select, scan_overlap,
no events) over two 1 M-row corpora used in turn (as bench.py) and over one corpus alone, how many launches took calls along
(smt_debug_scan_pairs) and how many calls each launch served (smt_debug_scan_groups_wide, eight entries, for the limits up to seven;
smt_debug_scan_groups_deep, sixteen entries, above), and the answers and status words compared with the limit 0.  T(n), what one corpus
pass serving n calls costs, is step x n at the limit n - 1 (the streams are always busy).  "sync":
one call, synchronise, repeat -- the latency of a call when the GPU is not behind, where nothing can be taken along and the
group-capable kernel must cost what the plain one does.  python tools/ab_pairing.py [rows] [rounds] [out.json]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import semtools_amd as smt
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = torch.device("cuda:0")
g = torch.Generator(device=dev); g.manual_seed(3)
x = torch.randn(rows, 256, device=dev, generator=g); x /= x.norm(dim=1, keepdim=True)
x2 = torch.randn(rows, 256, device=dev, generator=g); x2 /= x2.norm(dim=1, keepdim=True)
q = torch.randn(16, 256, device=dev, generator=g); q /= q.norm(dim=1, keepdim=True)
torch.cuda.synchronize()
torch.cuda.set_stream(torch.cuda.Stream(dev))
ctx = smt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
both = [smt.Corpus(ctx, device_ptr=t.data_ptr(), rows=rows) for t in (x, x2)]
out = torch.empty((64, 2, 10), dtype=torch.int64, device=dev)
st = torch.full((2048,), 7, dtype=torch.int32, device=dev)
def run(n, corpora, sync_each=False):
    for i in range(n):
        corpora[i % len(corpora)].search_topk_device(q[i % 16].data_ptr(), 1, 10, 0, out[i % 64, 0].data_ptr(), out[i % 64, 1].data_ptr(),
                                                     out_status_ptr=st[i % 2048:].data_ptr())
        if sync_each: torch.cuda.synchronize()
    ctx.synchronize()
def groups():
    return ctx.scan_groups_wide() + ctx.scan_groups_deep()
ctx.set_tuning("prof_select", 0)
ctx.set_tuning("async_select", 1)
# (limit, scan_gate_pct, scan_pair_wait_us): the sixteen group limits at the shipped gate, then the gate swept at the limit of fifteen
settings = [(take, 50, 0) for take in range(16)] + [(15, 0, 0), (15, 25, 0), (15, 75, 0), (15, 100, 0)]
loads = {"two_corpora": (both, False, settings), "one_corpus": (both[:1], False, settings),
         "sync": (both, True, [settings[0], settings[7], settings[15]])}
res, ref = {}, {}
for r in range(rounds):
    for load, (corpora, sync_each, todo) in loads.items():
        for pair, gate, wait_us in todo:
            ctx.set_tuning("scan_take" if pair < 8 else "scan_deep", pair)
            ctx.set_tuning("scan_gate_pct", gate)
            ctx.set_tuning("scan_pair_wait_us", wait_us)
            run(300, corpora, sync_each)
            st.fill_(7)
            c0, g0 = ctx.scan_pairs(), groups()
            t0 = time.perf_counter(); run(2000, corpora, sync_each); step = (time.perf_counter() - t0) / 2000 * 1e6
            c1, g1 = ctx.scan_pairs(), groups()
            ans = out.cpu().numpy().copy()
            ref.setdefault(load, ans)
            same = bool((ans == ref[load]).all()) and bool((st[:2000].cpu() == 0).all())
            key = f"{load}/" + ("off" if pair == 0 else f"take{pair}_gate{gate}")
            by = [b - a for a, b in zip(g0, g1)]
            res.setdefault(key, []).append({"step_us": round(step, 2), "pass_us": round(step * (pair + 1), 1), "paired": c1[0] - c0[0],
                                            "alone": c1[1] - c0[1], "absorbed": c1[2] - c0[2], "launches_by_calls_served": by[:8],
                                            "deep_launches_by_calls_served": by[8:], "answers_and_status_match": same})
            print(json.dumps({"round": r, "setting": key, **res[key][-1]}), file=sys.stderr, flush=True)
ctx.set_tuning("scan_gate_pct", -1)
ctx.set_tuning("scan_pair_wait_us", 0)
summary = {k: {"median_step_us": sorted(x["step_us"] for x in v)[len(v) // 2], "min": min(x["step_us"] for x in v),
               "max": max(x["step_us"] for x in v), "median_pass_us": sorted(x["pass_us"] for x in v)[len(v) // 2],
               "paired_of_2000": [x["paired"] for x in v],
               "launches_by_calls_served": [x["launches_by_calls_served"] for x in v],
               "deep_launches_by_calls_served": [x["deep_launches_by_calls_served"] for x in v],
               "all_match": all(x["answers_and_status_match"] for x in v)} for k, v in res.items()}
report = json.dumps({"rows": rows, "rounds": rounds, "summary": summary, "by_setting": res}, indent=1)
if len(sys.argv) > 3:
    open(sys.argv[3], "w").write(report + "\n")
else:
    print(report)
