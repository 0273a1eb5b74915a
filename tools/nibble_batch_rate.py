"""Batched nibble route (batch_nibble.hip) against the scan passes of four it replaces: 1 GiB of nibble rows (8 Mi rows of 256 int4),
top_k 10, the device form (smt_search_topk_device_ex) with nq = 4 .. 1000 queries, host clock around calls that end in a
synchronise.  One process, two settings of the same context taking turns round by round (nine rounds, the order alternating), so
both see the same drift of the machine: "scan" (nibble_batch_min = 0: exactly what the parent commit runs) and "batched" (the route
forced on at every nq).  Per cell: median and spread of ms per call, queries/s, whether the settings answered with the same bytes
(asserted), and -- from a profiled pass of its own -- the row rate of batch_nibble_kernel alone.  Then one full pass (128 queries)
against the BYTE route over the same number of rows (2 GiB of byte rows), alternating in the same way: the MFMA work per row is
equal, what differs is the unpack and the transpose.  --resources prints the build's register / LDS / scratch report of the unit
(no GPU needed); --merge FILE adds a JSON object (that report, what the list tests printed) to the profile.
python tools/nibble_batch_rate.py --merge notes.json > profiles/nibble_batch.json"""
import argparse, hashlib, json, os, re, statistics, subprocess, sys, time

NQS, ROUNDS, ROWS = (4, 5, 6, 8, 16, 32, 128, 1000), 9, 1 << 23
CALLS = {4: 40, 5: 40, 6: 40, 8: 40, 16: 30, 32: 20, 128: 10, 1000: 3}
SETTINGS = {"scan": 0, "batched": 1}   # nibble_batch_min
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def resources():
    src = os.path.join(HERE, "semtools_amd", "csrc", "batch_nibble.hip")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "-Xclang", "-target-feature", "-Xclang",
                        "-packed-fp32-ops", "-x", "hip", "--offload-device-only", "-c", src, "-o", "/dev/null",
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            t = re.search(r"batch_nibble_kernelILb([01])E", m.group(1))
            name = f"batch_nibble_kernel<filtered={t.group(1)}>" if t else "batch_nibble_split_kernel"
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+(?:\[[^\]]+\])?):\s+(\d+)", line)
        if m and name:
            out[name][m.group(1).strip()] = int(m.group(2))
    return out


def spread(v):
    return {"ms_per_call_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


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
    from semtools_amd import _lib as L
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(17)
    ctx = smt.Context(0)
    x = torch.randint(0, 256, (ROWS, 128), device=dev, generator=g, dtype=torch.uint8)   # every byte a pair of nibbles in [-8, 7]
    q = torch.randn(max(NQS), 256, device=dev, generator=g)
    torch.cuda.synchronize()
    c = smt.Corpus(ctx, device_ptr=x.data_ptr(), rows=ROWS, dtype=L.ROWS_I4)
    out_r = torch.empty((max(NQS), 10), dtype=torch.int64, device=dev)
    out_d = torch.empty((max(NQS), 10), dtype=torch.float64, device=dev)
    st = torch.zeros(max(NQS), dtype=torch.int32, device=dev)

    def use(name):
        ctx.set_tuning("nibble_batch_min", SETTINGS[name])

    def call(corpus, nq, n):
        for _ in range(n):
            corpus.search_topk_device(q.data_ptr(), nq, 10, 0, out_r.data_ptr(), out_d.data_ptr(), st.data_ptr())
        ctx.synchronize()

    ms = {name: {nq: [] for nq in NQS} for name in SETTINGS}
    for r in range(ROUNDS):
        for name in (list(SETTINGS) if r % 2 == 0 else list(SETTINGS)[::-1]):
            use(name)
            for nq in NQS:
                call(c, nq, 1)
                t0 = time.perf_counter(); call(c, nq, CALLS[nq]); ms[name][nq].append((time.perf_counter() - t0) / CALLS[nq] * 1e3)
    digest, unproved, kern = {}, {}, {}
    for name in SETTINGS:
        use(name)
        for nq in NQS:
            call(c, nq, 1)
            digest[name, nq] = hashlib.sha1(out_r[:nq].cpu().numpy().tobytes() + out_d[:nq].cpu().numpy().tobytes()).hexdigest()
            unproved[name, nq] = int((st[:nq] != 0).sum())
            if name != "scan":
                ctx.prof_enable(True); ctx.prof_reset(); call(c, nq, 3)
                kern[name, nq] = ctx.prof_read("batch_nibble"); ctx.prof_enable(False)
    cells = {}
    for nq in NQS:
        row = {}
        for name in SETTINGS:
            v = ms[name][nq]
            med = statistics.median(v)
            row[name] = dict(spread(v), queries_per_s=round(nq / med * 1e3, 1), not_proved=unproved[name, nq])
            if name != "scan":
                n, k_ms = kern[name, nq]
                row[name]["batch_nibble_launches"] = n
                row[name]["batch_nibble_tb_per_s"] = round((ROWS * 128) / (k_ms / n) / 1e9, 3) if n else None
                row[name]["batch_nibble_g_rows_per_s"] = round(ROWS / (k_ms / n) / 1e6, 2) if n else None
                row[name]["faster_than_scan_beyond_spreads"] = (row["scan"]["ms_per_call_median"] - med >
                                                                 max(v) - min(v) + row["scan"]["ms_max"] - row["scan"]["ms_min"])
                row[name]["speedup_over_scan"] = round(row["scan"]["ms_per_call_median"] / med, 2)
        row["same_answers"] = len({digest[name, nq] for name in SETTINGS}) == 1
        assert row["same_answers"], (nq, {name: digest[name, nq] for name in SETTINGS})
        cells[str(nq)] = row
    border = next((nq for nq in NQS if all(cells[str(m)]["batched"]["faster_than_scan_beyond_spreads"] for m in NQS if m >= nq)), None)

    # one full pass against the byte route over the same number of rows
    use("batched")
    xb = torch.randint(-127, 128, (ROWS, 256), device=dev, generator=g, dtype=torch.int8)
    torch.cuda.synchronize()
    cb = smt.Corpus(ctx, device_ptr=xb.data_ptr(), rows=ROWS, dtype=np.int8)
    ctx.set_tuning("byte_batch_min", 1)
    pair = {"nibble": c, "byte": cb}
    full = {name: [] for name in pair}
    for r in range(ROUNDS):
        for name in (list(pair) if r % 2 == 0 else list(pair)[::-1]):
            call(pair[name], 128, 1)
            t0 = time.perf_counter(); call(pair[name], 128, 10); full[name].append((time.perf_counter() - t0) / 10 * 1e3)
    full_pass = {name: spread(v) for name, v in full.items()}
    for name, prof_name in (("nibble", "batch_nibble"), ("byte", "batch_byte")):
        ctx.prof_enable(True); ctx.prof_reset(); call(pair[name], 128, 3)
        n, k_ms = ctx.prof_read(prof_name); ctx.prof_enable(False)
        full_pass[name]["kernel_ms"] = round(k_ms / n, 4)
    full_pass["nibble_over_byte"] = round(full_pass["nibble"]["ms_per_call_median"] / full_pass["byte"]["ms_per_call_median"], 3)

    prof = {"what": "device form, top_k 10, 1 GiB of nibble rows (8 Mi rows); ms per call by host clock around synchronised calls; scan = "
                    "nibble_batch_min 0 (passes of four, the parent commit's route), batched = batch_nibble_kernel at every nq; "
                    "batch_nibble_tb_per_s / g_rows_per_s = row bytes / rows of a pass over the kernel's time by HIP events; not_proved = "
                    "statuses other than PROVED among the nq answers; full_pass_against_byte_route = 128 queries over 8 Mi nibble rows "
                    "(1 GiB) and over 8 Mi byte rows (2 GiB), both batched, alternating, kernel_ms by HIP events",
            "rounds": ROUNDS, "calls_per_round": CALLS, "smallest_nq_faster_from_there_on": border, "cells": cells,
            "full_pass_against_byte_route": full_pass}
    if a.merge:
        prof.update(json.load(open(a.merge)))
    print(json.dumps(prof, indent=1))


if __name__ == "__main__":
    main()
