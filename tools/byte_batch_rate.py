"""Batched byte route (batch_byte.hip) against the scan passes of four it replaces: 1 GiB of byte rows (4 Mi rows of 256 int8),
top_k 10, the device form (smt_search_topk_device_ex) with nq = 4 .. 1000 queries, host clock around calls that end in a
synchronise.  One process, two settings of the same context taking turns round by round (nine rounds, the order alternating), so
both see the same drift of the machine: "scan" (byte_batch_min = 0: what the parent commit runs) and "batched" (the route forced on
at every nq).  Per cell: median and spread of ms per call, queries/s, whether the settings answered with the same bytes (asserted),
and -- from a profiled pass of its own -- the row rate of batch_byte_kernel alone.  --resources prints the build's register / LDS /
scratch report of the unit (no GPU needed); --merge FILE adds a JSON object (that report, what the list tests printed) to the profile.
python tools/byte_batch_rate.py --merge notes.json > profiles/byte_batch.json"""
import argparse, hashlib, json, os, re, statistics, subprocess, sys, time

NQS, ROUNDS, ROWS = (4, 8, 32, 128, 1000), 9, 1 << 22
CALLS = {4: 40, 8: 40, 32: 20, 128: 10, 1000: 3}
SETTINGS = {"scan": 0, "batched": 1}   # byte_batch_min
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def resources():
    src = os.path.join(HERE, "semtools_amd", "csrc", "batch_byte.hip")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "-Xclang", "-target-feature", "-Xclang",
                        "-packed-fp32-ops", "-x", "hip", "--offload-device-only", "-c", src, "-o", "/dev/null",
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            t = re.search(r"batch_byte_kernelILb([01])E", m.group(1))
            name = f"batch_byte_kernel<filtered={t.group(1)}>" if t else "batch_byte_split_kernel"
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+(?:\[[^\]]+\])?):\s+(\d+)", line)
        if m and name:
            out[name][m.group(1).strip()] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--merge")
    a = ap.parse_args()
    if a.resources:
        print(json.dumps({"kernel_resources": resources(), "dynamic_lds_bytes_per_block": 128 * 784 + 8 * 4608 + 128 * 12 + 16}, indent=1))
        return
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    import semtools_amd as smt
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(17)
    ctx = smt.Context(0)
    x = torch.randint(-127, 128, (ROWS, 256), device=dev, generator=g, dtype=torch.int8)
    q = torch.randn(max(NQS), 256, device=dev, generator=g)
    torch.cuda.synchronize()
    c = smt.Corpus(ctx, device_ptr=x.data_ptr(), rows=ROWS, dtype=np.int8)
    out_r = torch.empty((max(NQS), 10), dtype=torch.int64, device=dev)
    out_d = torch.empty((max(NQS), 10), dtype=torch.float64, device=dev)
    st = torch.zeros(max(NQS), dtype=torch.int32, device=dev)

    def use(name):
        ctx.set_tuning("byte_batch_min", SETTINGS[name])

    def call(nq, n):
        for _ in range(n):
            c.search_topk_device(q.data_ptr(), nq, 10, 0, out_r.data_ptr(), out_d.data_ptr(), st.data_ptr())
        ctx.synchronize()

    ms = {name: {nq: [] for nq in NQS} for name in SETTINGS}
    for r in range(ROUNDS):
        for name in (list(SETTINGS) if r % 2 == 0 else list(SETTINGS)[::-1]):
            use(name)
            for nq in NQS:
                call(nq, 1)
                t0 = time.perf_counter(); call(nq, CALLS[nq]); ms[name][nq].append((time.perf_counter() - t0) / CALLS[nq] * 1e3)
    digest, unproved, kern = {}, {}, {}
    for name in SETTINGS:
        use(name)
        for nq in NQS:
            call(nq, 1)
            digest[name, nq] = hashlib.sha1(out_r[:nq].cpu().numpy().tobytes() + out_d[:nq].cpu().numpy().tobytes()).hexdigest()
            unproved[name, nq] = int((st[:nq] != 0).sum())
            if name != "scan":
                ctx.prof_enable(True); ctx.prof_reset(); call(nq, 3)
                kern[name, nq] = ctx.prof_read("batch_byte"); ctx.prof_enable(False)
    cells = {}
    for nq in NQS:
        row = {}
        for name in SETTINGS:
            v = ms[name][nq]
            med = statistics.median(v)
            row[name] = {"ms_per_call_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                         "queries_per_s": round(nq / med * 1e3, 1), "not_proved": unproved[name, nq]}
            if name != "scan":
                n, k_ms = kern[name, nq]
                row[name]["batch_byte_launches"] = n
                row[name]["batch_byte_tb_per_s"] = round((ROWS * 256) / (k_ms / n) / 1e9, 3) if n else None
                row[name]["batch_byte_g_rows_per_s"] = round(ROWS / (k_ms / n) / 1e6, 2) if n else None
                row[name]["faster_than_scan_beyond_spreads"] = (row["scan"]["ms_per_call_median"] - med >
                                                                 max(v) - min(v) + row["scan"]["ms_max"] - row["scan"]["ms_min"])
                row[name]["speedup_over_scan"] = round(row["scan"]["ms_per_call_median"] / med, 2)
        row["same_answers"] = len({digest[name, nq] for name in SETTINGS}) == 1
        assert row["same_answers"], (nq, {name: digest[name, nq] for name in SETTINGS})
        cells[str(nq)] = row
    border = next((nq for nq in NQS if all(cells[str(m)]["batched"]["faster_than_scan_beyond_spreads"] for m in NQS if m >= nq)), None)
    prof = {"what": "device form, top_k 10, 1 GiB of byte rows (4 Mi rows); ms per call by host clock around synchronised calls; scan = "
                    "byte_batch_min 0 (passes of four, the parent commit's route), batched = batch_byte_kernel at every nq; "
                    "batch_byte_tb_per_s / g_rows_per_s = row bytes / rows of a pass over the kernel's time by HIP events; not_proved = "
                    "statuses other than PROVED among the nq answers",
            "rounds": ROUNDS, "calls_per_round": CALLS, "smallest_nq_faster_from_there_on": border, "cells": cells}
    if a.merge:
        prof.update(json.load(open(a.merge)))
    print(json.dumps(prof, indent=1))


if __name__ == "__main__":
    main()
