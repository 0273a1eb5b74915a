"""Which kernels differ between two builds, from device assembly listings (hipcc with the flags of csrc/build.sh plus
--offload-device-only -S, one .s per unit, any unit names: a kernel is found by its symbol wherever it lives).  For every kernel
symbol two things are compared: the text from its label to its end-of-function label, and its .amdhsa_kernel block.  Local labels
carry the number of the function inside its unit (.LBB<n>_, .Lfunc_end<n>, .Ltmp<n>), which changes when a kernel moves: they are
renumbered; comments are dropped.
python tools/asm_diff.py dir_a dir_b [symbol-substring ...]   -> prints the symbols compared and those that differ; exit 1 if any"""
import glob
import os
import re
import sys


def _norm(lines):
    out, tmp = [], {}
    for l in lines:
        l = l.split(";", 1)[0].rstrip()
        if not l.strip():
            continue
        l = re.sub(r"\.LBB\d+_", ".LBB_", l)
        l = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", l)
        l = re.sub(r"\.Ltmp\d+", lambda m: ".Ltmp%d" % tmp.setdefault(m.group(0), len(tmp)), l)
        out.append(l)
    return out


def kernels(directory):
    """symbol -> (normalised body, normalised .amdhsa_kernel block)"""
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
            found[sym] = (_norm(lines[start:end + 1]), _norm(lines[i:j + 1]))
            i = j + 1
    return found


def main(argv):
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
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
