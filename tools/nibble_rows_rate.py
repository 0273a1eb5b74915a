"""Byte and row rate of the nibble scan (scan_nibble_kernel, rows of 256 int4) beside the byte scan and the f32 256 scan over the SAME
number of bytes, in one process: one query over 1 GiB of rows each -- 2^23 nibble rows, 2^22 byte rows, 2^20 f32 rows -- kernel time
by HIP events (every launch bracketed), the three alternating round by round; median and spread over the rounds.  The four-query
pass of the nibble and byte scans the same way (byte_batch_min = 0: the byte corpus stays on its scan).  As information only:
recall@10 of a nibble corpus against the f32 corpus of the same rows (the bench's generator: normal rows, normalised).
python tools/nibble_rows_rate.py > profiles/nibble_rows.json   (the other keys of that file are added by hand: its "notes")"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import semtools_amd as smt
from semtools_amd import _lib as L
ROUNDS, WARM, TIMED = 9, 30, 200
dev = torch.device("cuda:0")
g = torch.Generator(device=dev); g.manual_seed(11)
torch.cuda.set_stream(torch.cuda.Stream(dev))
ctx = smt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
ctx.set_tuning("prof_select", 0)
ctx.set_tuning("byte_batch_min", 0)
def stored(x, kind):
    """the library's rounding rules (include/semtools_hip.h, "BYTE ROWS", "NIBBLE ROWS") in torch; i4 comes back packed"""
    if kind == "f32":
        return x
    q = torch.round(x * ((127.0 if kind == "i8" else 7.0) / x.abs().amax(dim=1, keepdim=True))).to(torch.int8)
    if kind == "i8":
        return q
    q = q.to(torch.int16)
    return ((q[:, 0::2] & 15) | ((q[:, 1::2] & 15) << 4)).to(torch.uint8)
def make(rows, kind):
    parts = []
    for b in range(0, rows, 1 << 20):
        x = torch.randn(min(1 << 20, rows - b), 256, device=dev, generator=g)
        x /= x.norm(dim=1, keepdim=True)
        parts.append(stored(x, kind).contiguous())
    return parts[0] if len(parts) == 1 else torch.cat(parts)
cases = {}
for name, code, rows, kernel in (("f32", L.ROWS_F32, 1 << 20, "scan"), ("i8", L.ROWS_I8, 1 << 22, "scan_byte"), ("i4", L.ROWS_I4, 1 << 23, "scan_nibble")):
    x = make(rows, name)
    q = torch.randn(8, 256, device=dev, generator=g); q /= q.norm(dim=1, keepdim=True)
    torch.cuda.synchronize()
    cases[name] = dict(x=x, q=q, rows=rows, bytes=x.numel() * x.element_size(), kernel=kernel, us={1: [], 4: []},
                       corpus=smt.Corpus(ctx, device_ptr=x.data_ptr(), rows=rows, dtype=code))
out = torch.empty((2, 4, 10), dtype=torch.int64, device=dev)
st = torch.zeros(4, dtype=torch.int32, device=dev)
def run(c, nq, n):
    for i in range(n):
        c["corpus"].search_topk_device(c["q"][(4 * i) % 8:].data_ptr(), nq, 10, 0, out[0].data_ptr(), out[1].data_ptr(), out_status_ptr=st.data_ptr())
    ctx.synchronize()
for r in range(ROUNDS):
    for nq in (1, 4):
        for name, c in cases.items():
            if nq == 4 and name == "f32":
                continue   # (the 256 kernels group queries their own way: not this family's pass)
            run(c, nq, WARM)
            ctx.prof_enable(True); ctx.prof_reset(); run(c, nq, TIMED)
            n, ms = ctx.prof_read(c["kernel"]); ctx.prof_enable(False)
            assert n > 0, (c["kernel"], n)
            c["us"][nq].append(ms / n * 1e3)
res = {"what": "top_k 10, scan kernel time by HIP events over 1 GiB of rows; f32 = the 256 scan, i8 = scan_byte_kernel, i4 = "
               "scan_nibble_kernel; one_query = the one-slot kernels, four_queries = one pass of the four-slot kernels",
       "rounds": ROUNDS, "launches_per_round": TIMED, "one_query": {}, "four_queries": {}}
for nq, key in ((1, "one_query"), (4, "four_queries")):
    for name, c in cases.items():
        us = c["us"][nq]
        if not us:
            continue
        med, lo, hi = statistics.median(us), min(us), max(us)
        res[key][name] = {"rows": c["rows"], "bytes": c["bytes"], "kernel_us_median": round(med, 2), "kernel_us_min": round(lo, 2),
                          "kernel_us_max": round(hi, 2), "tb_per_s_median": round(c["bytes"] / med / 1e6, 3),
                          "tb_per_s_min": round(c["bytes"] / hi / 1e6, 3), "tb_per_s_max": round(c["bytes"] / lo / 1e6, 3),
                          "grows_per_s_median": round(c["rows"] / med / 1e3, 3), "grows_per_s_min": round(c["rows"] / hi / 1e3, 3),
                          "grows_per_s_max": round(c["rows"] / lo / 1e3, 3)}
b = res["one_query"]["i4"]
for other in ("f32", "i8"):
    a = res["one_query"][other]
    res["i4_over_" + other] = {"byte_rate": round(b["tb_per_s_median"] / a["tb_per_s_median"], 3),
                               "row_rate": round(b["grows_per_s_median"] / a["grows_per_s_median"], 3)}
# recall@10, information only: the library promises exactness over what is stored, not closeness to the f32 rows
x = make(1 << 18, "f32")
xq = stored(x, "i4").contiguous()
Q = np.ascontiguousarray(make(64, "f32").cpu().numpy())
torch.cuda.synchronize()
full, nib = smt.Corpus(ctx, device_ptr=x.data_ptr(), rows=1 << 18), smt.Corpus(ctx, device_ptr=xq.data_ptr(), rows=1 << 18, dtype="int4")
hits = [len(set(a[0].tolist()) & set(b_[0].tolist())) for a, b_ in zip(full.search(Q, top_k=10), nib.search(Q, top_k=10))]
res["recall_at_10_vs_f32"] = {"rows": 1 << 18, "queries": 64, "mean": round(sum(hits) / 640.0, 4), "worst_query": min(hits) / 10.0}
print(json.dumps(res, indent=1))
