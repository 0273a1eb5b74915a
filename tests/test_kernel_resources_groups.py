"""Resources of the group-capable one-query scan (tuning key scan_pair, up to four calls per corpus pass), checked at build time like
tests/test_kernel_resources_pairing.py, which pins its registers (<= 64 VGPRs, no spill).

Here: no scratch at all; its LDS -- static plus the dynamic size the launcher asks for -- small enough that two scan blocks of
neighbouring streams share a CU with one select (160 KiB per CU, 84 KiB of them the select's at the headline's k = 10); and every
scan_topk_kernel instantiation has the registers it had before this kernel came (SMT_REDUCE_CHUNK4 carried a query accessor for
it for a while -- LDS images instead of registers; it reads q[n] directly again)."""
import os
import re

import pytest

from tests.test_kernel_resources import ROOT, _usage

CU_LDS = 160 * 1024
SELECT_LDS = 84 * 1024
# VGPRs of scan_topk_kernel<NQ, U, NT, FILTERED, STEAL> in a build of the parent commit (NT = 1 and NT = 0 agree everywhere)
PARENT_VGPRS = {
    (4, 4, 1, 0): 84, (4, 4, 0, 1): 80, (4, 4, 0, 0): 80, (4, 8, 0, 0): 109,
    (2, 4, 1, 0): 66, (2, 4, 0, 1): 64, (2, 4, 0, 0): 62, (2, 8, 0, 0): 92,
    (1, 4, 1, 0): 57, (1, 4, 0, 1): 55, (1, 4, 0, 0): 52, (1, 2, 0, 0): 34, (1, 8, 0, 0): 96,
}


def _pair_smem_bytes(threads):
    """pair_smem_bytes(threads) of scan_group.h, evaluated from its source text."""
    src = open(os.path.join(ROOT, "semtools_amd", "csrc", "scan_group.h")).read()
    group_max = int(re.search(r"constexpr int GROUP_MAX = (\d+);", src).group(1))
    body = re.search(r"static inline size_t pair_smem_bytes\(int threads\)\s*\{\s*return ([^;]+);", src).group(1)
    expr = body.replace("(size_t)", "").replace("sizeof(key_t64)", "8").replace("GROUP_MAX", str(group_max)).replace("/", "//")
    assert re.fullmatch(r"[\d\s+*/()a-z]+", expr), expr
    return group_max, int(eval(expr, {"__builtins__": {}}, {"threads": threads}))


@pytest.mark.timeout(900)
def test_group_capable_scan_has_no_scratch_fits_its_lds_and_leaves_the_plain_scans_alone():
    u = {**_usage("scan_pair.hip"), **_usage("scan_topk.hip")}    # (the grouped kernel's unit and the plain scans')
    pair = {k: v for k, v in u.items() if "scan_pair_kernel" in k}
    assert len(pair) == 2, list(u)
    group_max, _ = _pair_smem_bytes(512)
    assert group_max == 4
    for k, v in pair.items():
        assert v.get("ScratchSize [bytes/lane]", 0) == 0, (k, v)
        for threads in (512, 1024):                                # the default block and the largest
            lds = v.get("LDS Size [bytes/block]", 0) + _pair_smem_bytes(threads)[1]
            print(k, "threads", threads, "LDS", lds, "VGPRs", v["VGPRs"])
            assert lds <= (CU_LDS - SELECT_LDS) // 2, (k, threads, lds)
    scans = {k: v for k, v in u.items() if "scan_topk_kernel" in k}
    seen = set()
    for k, v in scans.items():
        m = re.search(r"scan_topk_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])ELb([01])E", k)
        assert m, k
        key = (int(m.group(1)), int(m.group(2)), int(m.group(4)), int(m.group(5)))
        assert v["VGPRs"] == PARENT_VGPRS[key], (k, v["VGPRs"], PARENT_VGPRS[key])
        seen.add(key)
    assert seen == set(PARENT_VGPRS), sorted(set(PARENT_VGPRS) - seen)
    assert len(scans) == 2 * len(PARENT_VGPRS), list(scans)
