"""Static instruction counts of a kernel's biggest loop, from a device assembly listing (hipcc with the flags of csrc/build.sh plus
--offload-device-only -S).  Counts the blocks that belong to the loop itself (depth 1), not its inner loops -- in scan_pair_kernel
those are the insert loops, which run for a few chunks in a thousand -- so the figures are "per row-loop iteration, no candidate":
vector, scalar, LDS and memory instructions, s_nop, waits, branches, exec-mask regions, and how many LDS reads have a full
lgkmcnt(0) wait directly behind them.  Both sides of a branch inside the loop are counted: an upper bound of one pass.
python tools/loop_inst_count.py listing.s scan_pair_kernelILb1 [out.json]"""
import json
import re
import sys


def count(path, symbol):
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*%s\w*:" % re.escape(symbol), l))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    body = lines[start:end]
    # blocks: a label or a "; %bb.N:" comment starts one; its comment names the loop it is in
    blocks, cur = [], {"header": None, "depth": 0, "insts": []}
    for l in body:
        m = re.match(r"^(\.LBB\w+:|; %bb\.\d+:)\s*(;.*)?$", l)
        if m:
            blocks.append(cur)
            c = m.group(2) or ""
            own = re.search(r"=>\s*This (?:Inner )?Loop Header: Depth=(\d+)", c)
            inl = re.search(r"in Loop: Header=(\w+) Depth=(\d+)", c)
            if own:
                cur = {"header": m.group(1).strip(".:"), "depth": int(own.group(1)), "insts": []}
            elif inl:
                cur = {"header": inl.group(1), "depth": int(inl.group(2)), "insts": []}
            else:
                cur = {"header": None, "depth": 0, "insts": []}
            continue
        t = l.strip()
        if t and not t.startswith((";", ".")):
            cur["insts"].append(t.split()[0] + " " + " ".join(t.split()[1:]))
    blocks.append(cur)
    loops = {}
    for b in blocks:
        if b["depth"] == 1:
            loops.setdefault(b["header"].replace("LBB", "BB"), []).extend(b["insts"])
    insts = max(loops.values(), key=len)
    out = dict.fromkeys(["vector", "scalar", "s_nop", "waitcnt", "branch", "lds", "vmem", "saveexec", "lds_read_then_full_wait"], 0)
    for i, t in enumerate(insts):
        op = t.split()[0]
        if op == "s_nop":
            out["s_nop"] += 1
        elif op == "s_waitcnt":
            out["waitcnt"] += 1
            if "lgkmcnt(0)" in t and i and insts[i - 1].startswith("ds_read"):
                out["lds_read_then_full_wait"] += 1
        elif op.startswith(("s_cbranch", "s_branch")):
            out["branch"] += 1
        elif op.startswith("s_"):
            out["scalar"] += 1
            out["saveexec"] += "saveexec" in op
        elif op.startswith("ds_"):
            out["lds"] += 1
        elif op.startswith(("global_", "flat_", "scratch_", "buffer_")):
            out["vmem"] += 1
        elif op.startswith("v_"):
            out["vector"] += 1
    out["all"] = len(insts)
    return out


if __name__ == "__main__":
    res = count(sys.argv[1], sys.argv[2])
    text = json.dumps(res, indent=1)
    if len(sys.argv) > 3:
        open(sys.argv[3], "w").write(text + "\n")
    print(text)
