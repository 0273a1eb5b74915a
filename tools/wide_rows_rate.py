"""Byte rate of the wide scan (scan_slab_kernel, 512 / 768 / 1024 dimensions) beside the 256 scan over the SAME number of bytes, in one
process: one query over 2^20 / S rows at each width, kernel time by HIP events (every launch bracketed), the widths alternating
round by round; median and spread over the rounds.  python tools/wide_rows_rate.py > profiles/wide_rows.json"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import semtools_amd as smt
ROUNDS, WARM, TIMED = 9, 30, 200
dev = torch.device("cuda:0")
g = torch.Generator(device=dev); g.manual_seed(11)
torch.cuda.set_stream(torch.cuda.Stream(dev))
ctx = smt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
ctx.set_tuning("prof_select", 0)
cases = {}
for D in (256, 512, 768, 1024):
    rows = (1 << 20) // (D // 256)
    x = torch.randn(rows, D, device=dev, generator=g); x /= x.norm(dim=1, keepdim=True)
    q = torch.randn(8, D, device=dev, generator=g); q /= q.norm(dim=1, keepdim=True)
    torch.cuda.synchronize()
    cases[D] = dict(x=x, q=q, rows=rows, corpus=smt.Corpus(ctx, device_ptr=x.data_ptr(), rows=rows, dim=D), us=[])
out = torch.empty((2, 10), dtype=torch.int64, device=dev)
st = torch.zeros(1, dtype=torch.int32, device=dev)
def run(c, n):
    for i in range(n):
        c["corpus"].search_topk_device(c["q"][i % 8].data_ptr(), 1, 10, 0, out[0].data_ptr(), out[1].data_ptr(), out_status_ptr=st.data_ptr())
    ctx.synchronize()
for r in range(ROUNDS):
    for D, c in cases.items():
        run(c, WARM)
        ctx.prof_enable(True); ctx.prof_reset(); run(c, TIMED)
        n, ms = ctx.prof_read("scan" if D == 256 else "scan_slab"); ctx.prof_enable(False)
        assert n > 0, (D, n)
        c["us"].append(ms / n * 1e3)
res = {"what": "one query, top_k 10, scan kernel time by HIP events; bytes = rows x D x 4", "rounds": ROUNDS, "launches_per_round": TIMED, "widths": {}}
for D, c in cases.items():
    med = statistics.median(c["us"])
    nbytes = c["rows"] * D * 4
    res["widths"][str(D)] = {"rows": c["rows"], "bytes": nbytes, "kernel_us_median": round(med, 2), "kernel_us_min": round(min(c["us"]), 2),
                             "kernel_us_max": round(max(c["us"]), 2), "tb_per_s_median": round(nbytes / med / 1e6, 3),
                             "tb_per_s_min": round(nbytes / max(c["us"]) / 1e6, 3), "tb_per_s_max": round(nbytes / min(c["us"]) / 1e6, 3)}
base = res["widths"]["256"]["tb_per_s_median"]
for D in ("512", "768", "1024"):
    res["widths"][D]["rate_over_256"] = round(res["widths"][D]["tb_per_s_median"] / base, 3)
print(json.dumps(res, indent=1))
