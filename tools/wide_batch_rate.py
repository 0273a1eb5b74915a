"""Batched wide route (batch_slab.hip) against a build of the PARENT commit: 1 GiB of rows at D = 512, 768, 1024, top_k 10, the device
form (smt_search_topk_device_ex) with nq = 4 .. 1000 queries, host clock around calls that end in a synchronise.  Two worker
processes, one per build, stay alive and take turns round by round (nine rounds), so both see the same drift of the machine; the new
build runs its batched route at every nq (slab_batch_min = 1).  Per cell: median and spread of ms per call for both builds, queries/s,
whether the answers of the two builds are the same bytes, and -- from a profiled pass of its own -- the byte rate of batch_slab_kernel
alone.  python tools/wide_batch_rate.py --parent <checkout of the parent commit, built> > profiles/wide_batch.json"""
import argparse, hashlib, json, os, statistics, subprocess, sys

DIMS, NQS, ROUNDS = (512, 768, 1024), (4, 8, 16, 32, 64, 256, 1000), 9
CALLS = {4: 20, 8: 20, 16: 20, 32: 20, 64: 10, 256: 4, 1000: 2}


def worker(root, batched):
    sys.path.insert(0, root)
    import torch
    import semtools_amd as smt
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(17)
    ctx = smt.Context(0)
    if batched:
        ctx.set_tuning("slab_batch_min", 1)
    cases = {}
    for D in DIMS:
        rows = (1 << 30) // (4 * D)
        x = torch.randn(rows, D, device=dev, generator=g)
        q = torch.randn(max(NQS), D, device=dev, generator=g)
        torch.cuda.synchronize()
        cases[D] = (x, q, rows, smt.Corpus(ctx, device_ptr=x.data_ptr(), rows=rows, dim=D))
    out_r = torch.empty((max(NQS), 10), dtype=torch.int64, device=dev)
    out_d = torch.empty((max(NQS), 10), dtype=torch.float64, device=dev)
    st = torch.zeros(max(NQS), dtype=torch.int32, device=dev)
    import time

    def call(D, nq, n):
        x, q, rows, c = cases[D]
        for _ in range(n):
            c.search_topk_device(q.data_ptr(), nq, 10, 0, out_r.data_ptr(), out_d.data_ptr(), st.data_ptr())
        ctx.synchronize()

    for line in sys.stdin:
        cmd = line.strip()
        res = {}
        for D in DIMS:
            for nq in NQS:
                call(D, nq, 1)
                if cmd == "round":
                    t0 = time.perf_counter(); call(D, nq, CALLS[nq]); res[f"{D}/{nq}"] = (time.perf_counter() - t0) / CALLS[nq] * 1e3
                elif cmd == "check":
                    res[f"{D}/{nq}"] = hashlib.sha1(out_r[:nq].cpu().numpy().tobytes() + out_d[:nq].cpu().numpy().tobytes()).hexdigest()
                elif cmd == "kernel":
                    ctx.prof_enable(True); ctx.prof_reset(); call(D, nq, 3)
                    n, ms = ctx.prof_read("batch_slab"); ctx.prof_enable(False)
                    res[f"{D}/{nq}"] = [n, ms]
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--worker", nargs=2)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], a.worker[1] == "1")
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    procs = {name: subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", root, flag], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
             for name, root, flag in (("new", here, "1"), ("parent", os.path.abspath(a.parent), "0"))}

    def ask(name, cmd):
        p = procs[name]
        p.stdin.write(cmd + "\n"); p.stdin.flush()
        line = p.stdout.readline()
        assert line, f"the {name} worker ended"
        return json.loads(line)

    ms = {name: {} for name in procs}
    for r in range(ROUNDS):
        for name in (("new", "parent") if r % 2 == 0 else ("parent", "new")):
            for cell, v in ask(name, "round").items():
                ms[name].setdefault(cell, []).append(v)
    hn, hp = ask("new", "check"), ask("parent", "check")
    kern = ask("new", "kernel")
    for p in procs.values():
        p.stdin.close(); p.wait()
    cells, border = {}, None
    for cell in ms["new"]:
        D, nq = map(int, cell.split("/"))
        row = {}
        for name in procs:
            v = ms[name][cell]
            med = statistics.median(v)
            row[name] = {"ms_per_call_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "queries_per_s": round(nq / med * 1e3, 1)}
        row["new_faster_beyond_spreads"] = row["parent"]["ms_per_call_median"] - row["new"]["ms_per_call_median"] > sum(row[n]["ms_max"] - row[n]["ms_min"] for n in procs)
        row["speedup"] = round(row["parent"]["ms_per_call_median"] / row["new"]["ms_per_call_median"], 2)
        row["same_answers"] = hn[cell] == hp[cell]
        n, k_ms = kern[cell]
        row["batch_slab_launches"] = n
        row["batch_slab_tb_per_s"] = round((1 << 30) / (k_ms / n) / 1e9, 3) if n else None
        cells[cell] = row
    for nq in NQS:
        if all(cells[f"{D}/{m}"]["new_faster_beyond_spreads"] for D in DIMS for m in NQS if m >= nq):
            border = nq
            break
    print(json.dumps({"what": "device form, top_k 10, 1 GiB of rows per width; ms per call by host clock around synchronised calls; "
                              "new = batched route at every nq (slab_batch_min 1), parent = build of the parent commit; "
                              "batch_slab_tb_per_s = row bytes of a pass over the kernel's time by HIP events",
                      "rounds": ROUNDS, "calls_per_round": CALLS, "smallest_nq_faster_at_all_widths": border, "cells": cells}, indent=1))


if __name__ == "__main__":
    main()
