"""The vector-instruction mix of a kernel's biggest loop, from a device assembly listing (hipcc with the flags of csrc/build.sh plus
--offload-device-only -S).  Like tools/loop_inst_count.py it takes the blocks of the loop itself (depth 1) and leaves out its inner
loops -- in the one-query scans those are the insert loops, which run for a few chunks in a thousand -- and counts both sides of a
branch inside the loop: an upper bound of one pass.  Here the vector instructions are counted by class, opcode by opcode; s_nop is
shown beside them (it is not a vector instruction, but it holds the issue slot of its wave).
python tools/loop_mix.py listing.s scan_deep_kernelILb1 [chunks per iteration] [out.json]"""
import json
import re
import sys

CLASSES = (                                                        # first match wins
    ("dpp_add", lambda op, t: op.startswith(("v_add_f32", "v_add_u32")) and ("quad_perm" in t or "row_" in t)),
    ("fma_mul", lambda op, t: op.startswith(("v_fma", "v_mul_f32", "v_pk_fma", "v_pk_mul"))),
    ("cndmask", lambda op, t: op.startswith("v_cndmask")),
    ("cmp", lambda op, t: op.startswith("v_cmp")),
    ("mov", lambda op, t: op.startswith(("v_mov", "v_accvgpr"))),
    ("swap", lambda op, t: op.startswith("v_swap")),
    ("lane_swap", lambda op, t: op.startswith("v_permlane")),
    ("rsq", lambda op, t: op.startswith("v_rsq")),
    ("add", lambda op, t: op.startswith(("v_add", "v_sub"))),
    ("readlane", lambda op, t: op.startswith(("v_readlane", "v_readfirstlane", "v_writelane"))),
)


def loop_insts(path, symbol):
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*%s\w*:" % re.escape(symbol), l))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    loops, header, depth = {}, None, 0
    for l in lines[start:end]:
        m = re.match(r"^(\.LBB\w+:|; %bb\.\d+:)\s*(;.*)?$", l)
        if m:
            c = m.group(2) or ""
            own = re.search(r"=>\s*This (?:Inner )?Loop Header: Depth=(\d+)", c)
            inl = re.search(r"in Loop: Header=(\w+) Depth=(\d+)", c)
            if own:
                header, depth = m.group(1).strip(".:").replace("LBB", "BB"), int(own.group(1))
            elif inl:
                header, depth = inl.group(1), int(inl.group(2))
            else:
                header, depth = None, 0
            continue
        t = l.strip()
        if depth == 1 and t and not t.startswith((";", ".")):
            loops.setdefault(header, []).append(t)
    return max(loops.values(), key=len)


def mix(path, symbol):
    out = {name: 0 for name, _ in CLASSES}
    out.update(other_valu=0, valu=0, s_nop=0)
    other = {}
    for t in loop_insts(path, symbol):
        op = t.split()[0]
        if op == "s_nop":
            out["s_nop"] += 1
        if not op.startswith("v_"):
            continue
        out["valu"] += 1
        for name, test in CLASSES:
            if test(op, t):
                out[name] += 1
                break
        else:
            out["other_valu"] += 1
            other[op] = other.get(op, 0) + 1
    out["other_valu_opcodes"] = other
    return out


if __name__ == "__main__":
    res = mix(sys.argv[1], sys.argv[2])
    chunks = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    if chunks > 1:
        res["per_chunk"] = {k: v / chunks for k, v in res.items() if isinstance(v, int)}
    text = json.dumps(res, indent=1)
    if len(sys.argv) > 4:
        open(sys.argv[4], "w").write(text + "\n")
    print(text)
