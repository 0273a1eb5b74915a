"""Which kernels differ between two builds, from device assembly listings (hipcc with the flags of csrc/build.sh plus
--offload-device-only -S, one .s per unit, any unit names: a kernel is found by its symbol wherever it lives).  For every kernel
symbol two things are compared: the text from its label to its end-of-function label, and its .amdhsa_kernel block.  Local labels
carry the number of the function inside its unit (.LBB<n>_, .Lfunc_end<n>, .Ltmp<n>), which changes when a kernel moves: they are
renumbered; comments are dropped.
python tools/asm_diff.py dir_a dir_b [symbol-substring ...]   -> prints the symbols compared and those that differ; exit 1 if any

--mnemonics (anywhere among the arguments): for the kernels whose text differs, is the difference in front of the row loop?  The
first token of each normalised line -- the opcode; every block label counts as the same token -- is compared instead of the line,
so that other register numbers and block numbers do not count.  Every hunk's line range (normalised lines of the kernel, from 1) is printed beside the line of the header of the
kernel's biggest depth-1 loop, found from the compiler's loop comments as tools/loop_mix.py finds it.  Exit 0 only if every
.amdhsa_kernel block is identical and every hunk ends before that header, in both listings."""
import difflib
import glob
import os
import re
import sys


def _norm(lines):
    """-> (normalised lines, for each of them its index in `lines`)"""
    out, at, tmp = [], [], {}
    for i, l in enumerate(lines):
        l = l.split(";", 1)[0].rstrip()
        if not l.strip():
            continue
        l = re.sub(r"\.LBB\d+_", ".LBB_", l)
        l = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", l)
        l = re.sub(r"\.Ltmp\d+", lambda m: ".Ltmp%d" % tmp.setdefault(m.group(0), len(tmp)), l)
        out.append(l)
        at.append(i)
    return out, at


def _loop_header(lines, at):
    """Normalised line number (from 1) of the header label of the biggest depth-1 loop -- most instructions in its own blocks, inner
    loops left out, as tools/loop_mix.py counts -- or None if the kernel has no loop."""
    size, where, header, depth = {}, {}, None, 0
    for i, l in enumerate(lines):
        m = re.match(r"^(\.LBB\w+:|; %bb\.\d+:)\s*(;.*)?$", l)
        if m:
            c = m.group(2) or ""
            own = re.search(r"=>\s*This (?:Inner )?Loop Header: Depth=(\d+)", c)
            inl = re.search(r"in Loop: Header=(\w+) Depth=(\d+)", c)
            if own:
                header, depth = m.group(1).strip(".:").replace("LBB", "BB"), int(own.group(1))
                if depth == 1:
                    where[header] = i
            elif inl:
                header, depth = inl.group(1), int(inl.group(2))
            else:
                header, depth = None, 0
            continue
        t = l.strip()
        if depth == 1 and t and not t.startswith((";", ".")):
            size[header] = size.get(header, 0) + 1
    if not size:
        return None
    return at.index(where[max(size, key=size.get)]) + 1


def kernels(directory):
    """symbol -> (normalised body, normalised .amdhsa_kernel block, line of the row loop's header in the body)"""
    found = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        lines = open(path).read().split("\n")
        label = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"^([A-Za-z_][\w$.]*):", l))}
        i = 0
        while i < len(lines):
            m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", lines[i])
            if not m:
                i += 1
                continue
            sym = m.group(1)
            j = next(k for k in range(i, len(lines)) if lines[k].strip() == ".end_amdhsa_kernel")
            start = label[sym]
            end = next(k for k in range(start, len(lines)) if re.match(r"^\.Lfunc_end\d+:", lines[k]))
            assert sym not in found, "kernel %s is defined twice in %s" % (sym, directory)
            body, at = _norm(lines[start:end + 1])
            found[sym] = (body, _norm(lines[i:j + 1])[0], _loop_header(lines[start:end + 1], at))
            i = j + 1
    return found


def _hunks(a, b):
    """Opcode-sequence hunks: ((first, last) in a, (first, last) in b), lines from 1; an empty side is (line before, that line)."""
    def tok(l):   # (a block label's number shifts with every block in front of it: all labels are one token)
        t = l.split()[0]
        return ".LBB:" if t.startswith(".LBB_") else t
    ta, tb = [tok(l) for l in a], [tok(l) for l in b]
    sm = difflib.SequenceMatcher(None, ta, tb, autojunk=False)
    return [((i1 + 1, i2), (j1 + 1, j2)) for op, i1, i2, j1, j2 in sm.get_opcodes() if op != "equal"]


def main(argv):
    mnemonics = "--mnemonics" in argv
    argv = [x for x in argv if x != "--mnemonics"]
    a, b = kernels(argv[1]), kernels(argv[2])
    want = argv[3:]
    syms = sorted(s for s in set(a) | set(b) if not want or any(w in s for w in want))
    bad = []
    for s in syms:
        if s not in a or s not in b:
            bad.append((s, "only in " + (argv[1] if s in a else argv[2])))
        elif a[s][0] != b[s][0]:
            bad.append((s, "code differs (%d / %d lines)" % (len(a[s][0]), len(b[s][0]))))
        elif a[s][1] != b[s][1]:
            bad.append((s, "kernel descriptor differs"))
    print("%d kernel symbols compared" % len(syms))
    for s in syms:
        print("  " + s)
    print("%d differ" % len(bad))
    for s, why in bad:
        print("  %s: %s" % (s, why))
    if not mnemonics:
        return 1 if bad else 0
    failed = 0
    for s, why in bad:
        if not why.startswith("code differs"):
            failed += 1
            continue
        hunks = _hunks(a[s][0], b[s][0])
        ha, hb = a[s][2], b[s][2]
        same_desc = a[s][1] == b[s][1]
        early = ha is not None and hb is not None and all(x[1] < ha and y[1] < hb for x, y in hunks)
        print("%s\n  descriptor %s; %d opcode hunks; row loop header at line %s / %s" %
              (s, "identical" if same_desc else "DIFFERS", len(hunks), ha, hb))
        for x, y in hunks:
            print("    lines %d-%d / %d-%d" % (x[0], x[1], y[0], y[1]))
        ok = same_desc and early
        print("  %s" % ("ok: every hunk ends before the row loop" if ok else "FAIL"))
        failed += 0 if ok else 1
    print("%d fail the --mnemonics bar" % failed)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
