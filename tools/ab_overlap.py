"""A/B of the one-query pipeline's overlapped scans (tuning key scan_overlap; scan_gate_pct = the start gate) in ONE process on one
box: alternating settings, the wall time per pipelined step (async select, no events) over two 1 M-row corpora used in turn (as
bench.py), and the answers and status words compared with scan_overlap = 0.  python tools/ab_overlap.py [rows] [rounds] [gates] > out.json
"gates": the gate settings only, with the machine's hardware queue count and the four streams bench.py's process uses (no aux stream;
the answers are compared with the first setting's)."""
import json, os, sys, time
gates_only = len(sys.argv) > 3 and sys.argv[3] == "gates"
# the A/B alternates with scan_overlap = 0, whose aux stream is a fifth stream of this process (torch's default, the caller's, aux and
# the two scan streams): with 4 hardware queues two of them would share one and serialise -- give each its own
if not gates_only:
    os.environ["GPU_MAX_HW_QUEUES"] = "8"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import semtools_amd as smt
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda:0")
g = torch.Generator(device=dev); g.manual_seed(3)
x = torch.randn(rows, 256, device=dev, generator=g); x /= x.norm(dim=1, keepdim=True)
x2 = torch.randn(rows, 256, device=dev, generator=g); x2 /= x2.norm(dim=1, keepdim=True)
q = torch.randn(16, 256, device=dev, generator=g); q /= q.norm(dim=1, keepdim=True)
torch.cuda.synchronize()
torch.cuda.set_stream(torch.cuda.Stream(dev))
ctx = smt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
corpora = [smt.Corpus(ctx, device_ptr=t.data_ptr(), rows=rows) for t in (x, x2)]
out = torch.empty((64, 2, 10), dtype=torch.int64, device=dev)
st = torch.full((2048,), 7, dtype=torch.int32, device=dev)
def run(n):
    for i in range(n):
        corpora[i & 1].search_topk_device(q[i % 16].data_ptr(), 1, 10, 0, out[i % 64, 0].data_ptr(), out[i % 64, 1].data_ptr(),
                                          out_status_ptr=st[i % 2048:].data_ptr())
    ctx.synchronize()
ctx.set_tuning("prof_select", 0)
ctx.set_tuning("async_select", 1)
settings = [(0, 0), (1, 0), (1, 50), (1, 75), (1, 90), (1, 97), (1, 100)][1 if gates_only else 0:]
res, ref = {}, None
for r in range(rounds):
    for ov, gate in settings:
        ctx.set_tuning("scan_overlap", ov)
        ctx.set_tuning("scan_gate_pct", gate)
        run(300)
        st.fill_(7)
        t0 = time.perf_counter(); run(2000); step = (time.perf_counter() - t0) / 2000 * 1e6
        ans = out.cpu().numpy().copy()
        if ref is None: ref = ans
        same = bool((ans == ref).all()) and bool((st[:2000].cpu() == 0).all())
        key = "off" if ov == 0 else f"gate{gate}"
        res.setdefault(key, []).append({"pipelined_step_us": round(step, 2), "answers_and_status_match": same})
        print(json.dumps({"round": r, "setting": key, **res[key][-1]}), file=sys.stderr, flush=True)
summary = {k: {"median_step_us": sorted(x["pipelined_step_us"] for x in v)[len(v) // 2],
               "min": min(x["pipelined_step_us"] for x in v), "max": max(x["pipelined_step_us"] for x in v),
               "all_match": all(x["answers_and_status_match"] for x in v)} for k, v in res.items()}
print(json.dumps({"rows": rows, "rounds": rounds, "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "summary": summary, "by_setting": res}, indent=1))
