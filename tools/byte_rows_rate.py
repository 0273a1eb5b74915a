"""Byte and row rate of the byte scan (scan_byte_kernel, rows of 256 int8) beside the half scan and the f32 256 scan over the SAME
number of bytes, in one process: one query over 1 GiB of rows each -- 2^22 byte rows, 2^21 half rows, 2^20 f32 rows -- kernel time
by HIP events (every launch bracketed), the three alternating round by round; median and spread over the rounds.
python tools/byte_rows_rate.py > profiles/byte_rows.json   (the other keys of that file are added by hand: its "notes")"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import semtools_amd as smt
ROUNDS, WARM, TIMED = 9, 30, 200
dev = torch.device("cuda:0")
g = torch.Generator(device=dev); g.manual_seed(11)
torch.cuda.set_stream(torch.cuda.Stream(dev))
ctx = smt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
ctx.set_tuning("prof_select", 0)
cases = {}
for name, tdt, ndt, rows, kernel in (("f32", torch.float32, np.float32, 1 << 20, "scan"), ("f16", torch.float16, np.float16, 1 << 21, "scan_half"),
                                     ("i8", torch.int8, np.int8, 1 << 22, "scan_byte")):
    x = torch.randn(rows, 256, device=dev, generator=g)
    if tdt == torch.int8:   # the library's rounding rule (include/semtools_hip.h, "BYTE ROWS")
        x = torch.round(x * (127.0 / x.abs().amax(dim=1, keepdim=True))).to(tdt).contiguous()
    else:
        x /= x.norm(dim=1, keepdim=True)
        x = x.to(tdt).contiguous()
    q = torch.randn(8, 256, device=dev, generator=g); q /= q.norm(dim=1, keepdim=True)
    torch.cuda.synchronize()
    cases[name] = dict(x=x, q=q, rows=rows, bytes=rows * 256 * x.element_size(), kernel=kernel, us=[],
                       corpus=smt.Corpus(ctx, device_ptr=x.data_ptr(), rows=rows, dtype=ndt))
out = torch.empty((2, 10), dtype=torch.int64, device=dev)
st = torch.zeros(1, dtype=torch.int32, device=dev)
def run(c, n):
    for i in range(n):
        c["corpus"].search_topk_device(c["q"][i % 8].data_ptr(), 1, 10, 0, out[0].data_ptr(), out[1].data_ptr(), out_status_ptr=st.data_ptr())
    ctx.synchronize()
for r in range(ROUNDS):
    for c in cases.values():
        run(c, WARM)
        ctx.prof_enable(True); ctx.prof_reset(); run(c, TIMED)
        n, ms = ctx.prof_read(c["kernel"]); ctx.prof_enable(False)
        assert n > 0, (c["kernel"], n)
        c["us"].append(ms / n * 1e3)
res = {"what": "one query, top_k 10, scan kernel time by HIP events over 1 GiB of rows; f32 = the 256 scan, f16 = scan_half_kernel, "
               "i8 = scan_byte_kernel", "rounds": ROUNDS, "launches_per_round": TIMED, "rows_as": {}}
for name, c in cases.items():
    med, lo, hi = statistics.median(c["us"]), min(c["us"]), max(c["us"])
    res["rows_as"][name] = {"rows": c["rows"], "bytes": c["bytes"], "kernel_us_median": round(med, 2), "kernel_us_min": round(lo, 2),
                            "kernel_us_max": round(hi, 2), "tb_per_s_median": round(c["bytes"] / med / 1e6, 3),
                            "tb_per_s_min": round(c["bytes"] / hi / 1e6, 3), "tb_per_s_max": round(c["bytes"] / lo / 1e6, 3),
                            "grows_per_s_median": round(c["rows"] / med / 1e3, 3), "grows_per_s_min": round(c["rows"] / hi / 1e3, 3),
                            "grows_per_s_max": round(c["rows"] / lo / 1e3, 3)}
b = res["rows_as"]["i8"]
for other in ("f32", "f16"):
    a = res["rows_as"][other]
    res["i8_over_" + other] = {"byte_rate": round(b["tb_per_s_median"] / a["tb_per_s_median"], 3),
                               "row_rate": round(b["grows_per_s_median"] / a["grows_per_s_median"], 3)}
print(json.dumps(res, indent=1))
