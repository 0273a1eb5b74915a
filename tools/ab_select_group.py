"""A/B of the one-select-launch-per-pass route and the lighter pipeline call (tuning keys select_group and ov_skip_ready) in ONE process,
settings alternated, at the group limit of fifteen: wall time per pipelined step and host time to issue a step over two 1 M-row
corpora used in turn (as bench.py), the select launches by calls served (smt_debug_select_groups), the ready events recorded
(smt_debug_ov_ready), and the answers and status words compared with both switches off.  Then, with host_timing = 1, what the
runtime calls of one pipeline call cost the host (clock_gettime around each, smt_debug_host_timing), and "sync": one call,
synchronise, repeat.  python tools/ab_select_group.py [out.json] [rows] [rounds]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import semtools_amd as smt
rows = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
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
def run(n, sync_each=False):
    t0 = time.perf_counter()
    for i in range(n):
        both[i % 2].search_topk_device(q[i % 16].data_ptr(), 1, 10, 0, out[i % 64, 0].data_ptr(), out[i % 64, 1].data_ptr(),
                                       out_status_ptr=st[i % 2048:].data_ptr())
        if sync_each: torch.cuda.synchronize()
    issued = time.perf_counter() - t0
    ctx.synchronize()
    return issued, time.perf_counter() - t0
ctx.set_tuning("prof_select", 0)
ctx.set_tuning("async_select", 1)
ctx.set_tuning("scan_deep", 15)
KINDS = ("stream_queries", "ready_event", "scan_launch", "select_launch", "aux_event", "whole_call")
res, ref = {}, None
for r in range(rounds):
    for group, skip in ((0, 0), (1, 1), (0, 1), (1, 0)):
        ctx.set_tuning("select_group", group)
        ctx.set_tuning("ov_skip_ready", skip)
        run(300)
        st.fill_(7)
        s0, r0 = ctx.select_groups(), ctx.ov_ready_records()
        issued, total = run(2000)
        s1, r1 = ctx.select_groups(), ctx.ov_ready_records()
        ans = out.cpu().numpy().copy()
        ref = ans if ref is None else ref
        same = bool((ans == ref).all()) and bool((st[:2000].cpu() == 0).all())
        key = f"select_group{group}_ov_skip_ready{skip}"
        res.setdefault(key, []).append({"step_us": round(total / 2000 * 1e6, 2), "host_issue_us": round(issued / 2000 * 1e6, 2),
                                        "select_launches_by_calls_served": [b - a for a, b in zip(s0, s1)], "ready_events": r1 - r0,
                                        "answers_and_status_match": same})
        print(json.dumps({"round": r, "setting": key, **res[key][-1]}), file=sys.stderr, flush=True)
host = {}
for group, skip in ((0, 0), (1, 1)):
    ctx.set_tuning("select_group", group)
    ctx.set_tuning("ov_skip_ready", skip)
    run(300)
    ctx.set_tuning("host_timing", 1)
    issued, total = run(2000)
    ns, calls = ctx.host_timing()
    ctx.set_tuning("host_timing", 0)
    host[f"select_group{group}_ov_skip_ready{skip}"] = {"calls": calls, "host_issue_us_with_timing": round(issued / 2000 * 1e6, 2),
                                                        "us_per_call": {k: round(v / max(calls, 1) / 1e3, 2) for k, v in zip(KINDS, ns)}}
    print(json.dumps(host), file=sys.stderr, flush=True)
sync = {}
for group, skip in ((0, 0), (1, 1)):
    ctx.set_tuning("select_group", group)
    ctx.set_tuning("ov_skip_ready", skip)
    run(100, True)
    sync[f"select_group{group}_ov_skip_ready{skip}"] = round(run(1000, True)[1] / 1000 * 1e6, 2)
ctx.set_tuning("select_group", 1)
ctx.set_tuning("ov_skip_ready", 1)
summary = {k: {"median_step_us": sorted(v_["step_us"] for v_ in v)[len(v) // 2], "min": min(v_["step_us"] for v_ in v),
               "max": max(v_["step_us"] for v_ in v), "median_host_issue_us": sorted(v_["host_issue_us"] for v_ in v)[len(v) // 2],
               "all_match": all(v_["answers_and_status_match"] for v_ in v)} for k, v in res.items()}
report = json.dumps({"rows": rows, "rounds": rounds, "summary": summary, "host_breakdown": host, "sync_call_us": sync, "by_setting": res}, indent=1)
print(json.dumps({"summary": summary, "host_breakdown": host, "sync_call_us": sync}), file=sys.stderr, flush=True)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(report + "\n")
else:
    print(report)
