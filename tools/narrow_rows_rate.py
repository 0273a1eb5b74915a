"""Byte and row rate of the narrow scan (scan_narrow_kernel, rows of 64 floats) beside the f32 256 scan and the byte scan over the SAME
number of bytes, in one process: one query over 1 GiB of rows each -- 2^22 narrow rows, 2^20 rows of 256 floats, 2^22 byte rows --
kernel time by HIP events (every launch bracketed), the three alternating round by round; median and spread over the rounds.  The
four-query pass of the narrow and byte scans the same way (byte_batch_min = 0: the byte corpus stays on its scan).  K1: Zipf ids
over a 64-wide f32 table (embed_narrow_kernel) beside the 256 kernel on the same ids, alternating as well.
python tools/narrow_rows_rate.py > profiles/narrow_rows.json   (the other keys of that file are added by hand: its "notes")"""
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
def make(rows, dim, kind):
    parts = []
    for b in range(0, rows, 1 << 20):
        x = torch.randn(min(1 << 20, rows - b), dim, device=dev, generator=g)
        x /= x.norm(dim=1, keepdim=True)
        if kind == "i8":   # the library's rounding rule (include/semtools_hip.h, "BYTE ROWS")
            x = torch.round(x * (127.0 / x.abs().amax(dim=1, keepdim=True))).to(torch.int8)
        parts.append(x.contiguous())
    return parts[0] if len(parts) == 1 else torch.cat(parts)
cases = {}
for name, dim, code, rows, kernel in (("f32_64", 64, L.ROWS_F32, 1 << 22, "scan_narrow"), ("f32_256", 256, L.ROWS_F32, 1 << 20, "scan"),
                                      ("i8_256", 256, L.ROWS_I8, 1 << 22, "scan_byte")):
    x = make(rows, dim, "i8" if code == L.ROWS_I8 else "f32")
    q = torch.randn(8, dim, device=dev, generator=g); q /= q.norm(dim=1, keepdim=True)
    torch.cuda.synchronize()
    cases[name] = dict(x=x, q=q, rows=rows, bytes=x.numel() * x.element_size(), kernel=kernel, us={1: [], 4: []},
                       corpus=smt.Corpus(ctx, device_ptr=x.data_ptr(), rows=rows, dtype=code, dim=dim))
out = torch.empty((2, 4, 10), dtype=torch.int64, device=dev)
st = torch.zeros(4, dtype=torch.int32, device=dev)
def run(c, nq, n):
    for i in range(n):
        c["corpus"].search_topk_device(c["q"][(4 * i) % 8:].data_ptr(), nq, 10, 0, out[0].data_ptr(), out[1].data_ptr(), out_status_ptr=st.data_ptr())
    ctx.synchronize()
def timed(kernel, fn, warm, n):
    fn(warm)
    ctx.prof_enable(True); ctx.prof_reset(); fn(n)
    k, ms = ctx.prof_read(kernel); ctx.prof_enable(False)
    assert k > 0, (kernel, k)
    return ms / k * 1e3
# K1: 2^16 lines of Zipf ids (mean about 24 tokens, max_tokens 512) over tables of 2^15 rows
rs = np.random.default_rng(3)
V, n_lines = 1 << 15, 1 << 16
lens = np.minimum(rs.geometric(1 / 24.0, n_lines), 512)
ids = torch.from_numpy(np.minimum(rs.zipf(1.2, int(lens.sum())) - 1, V - 1).astype(np.int32)).to(dev)
offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)
k1 = {}
for name, dim, kernel in (("f32_64", 64, "embed_narrow"), ("f32_256", 256, "embed")):
    t = torch.randn(V, dim, device=dev, generator=g)
    o = torch.empty((n_lines, dim), device=dev)
    torch.cuda.synchronize()
    k1[name] = dict(t=t, o=o, dim=dim, kernel=kernel, us=[], model=smt.Model(ctx, device_ptr=t.data_ptr(), V=V, dim=dim))
def run_k1(c, n):
    for _ in range(n):
        c["model"].embed_device(ids.data_ptr(), offs.data_ptr(), n_lines, 512, c["o"].data_ptr())
    ctx.synchronize()
for r in range(ROUNDS):
    for nq in (1, 4):
        for name, c in cases.items():
            if nq == 4 and name == "f32_256":
                continue   # (the 256 kernels group queries their own way: not this family's pass)
            c["us"][nq].append(timed(c["kernel"], lambda n: run(c, nq, n), WARM, TIMED))
    for c in k1.values():
        c["us"].append(timed(c["kernel"], lambda n: run_k1(c, n), 5, 20))
def spread(us):
    return statistics.median(us), min(us), max(us)
res = {"what": "top_k 10, scan kernel time by HIP events over 1 GiB of rows; f32_64 = scan_narrow_kernel, f32_256 = the 256 scan, i8_256 "
               "= scan_byte_kernel; one_query = the one-slot kernels, four_queries = one pass of the four-slot kernels; k1 = the pooling "
               "kernel alone over 2^16 lines of Zipf ids",
       "rounds": ROUNDS, "launches_per_round": TIMED, "one_query": {}, "four_queries": {}, "k1": {}}
for nq, key in ((1, "one_query"), (4, "four_queries")):
    for name, c in cases.items():
        if not c["us"][nq]:
            continue
        med, lo, hi = spread(c["us"][nq])
        res[key][name] = {"rows": c["rows"], "bytes": c["bytes"], "kernel_us_median": round(med, 2), "kernel_us_min": round(lo, 2),
                          "kernel_us_max": round(hi, 2), "tb_per_s_median": round(c["bytes"] / med / 1e6, 3),
                          "tb_per_s_min": round(c["bytes"] / hi / 1e6, 3), "tb_per_s_max": round(c["bytes"] / lo / 1e6, 3),
                          "grows_per_s_median": round(c["rows"] / med / 1e3, 3), "grows_per_s_min": round(c["rows"] / hi / 1e3, 3),
                          "grows_per_s_max": round(c["rows"] / lo / 1e3, 3)}
b = res["one_query"]["f32_64"]
for other in ("f32_256", "i8_256"):
    a = res["one_query"][other]
    res["f32_64_over_" + other] = {"byte_rate": round(b["tb_per_s_median"] / a["tb_per_s_median"], 3),
                                   "row_rate": round(b["grows_per_s_median"] / a["grows_per_s_median"], 3)}
for name, c in k1.items():
    med, lo, hi = spread(c["us"])
    res["k1"][name] = {"lines": n_lines, "tokens": int(lens.sum()), "kernel_us_median": round(med, 2), "kernel_us_min": round(lo, 2),
                       "kernel_us_max": round(hi, 2), "gtokens_per_s_median": round(int(lens.sum()) / med / 1e3, 3),
                       "gathered_gb_per_s_median": round(int(lens.sum()) * c["dim"] * 4 / med / 1e3, 1)}
print(json.dumps(res, indent=1))
