"""Resources of the eight-call one-query scan (scan_wide_kernel, tuning key scan_take), checked at build time like
tests/test_kernel_resources_groups.py: it runs where scan_pair_kernel runs, two scan blocks of neighbouring streams on a CU beside
one select -- 2 x 64 + 4 x 96 = 512 VGPRs per SIMD, and (160 KiB - 84 KiB of the select at the headline's k = 10) / 2 of LDS per
block.  One register more and the select waits for scan blocks to leave."""
import os
import re

import pytest

from tests.test_kernel_resources import ROOT, _usage
from tests.test_kernel_resources_groups import CU_LDS, SELECT_LDS


def _wide_smem_bytes(threads):
    """wide_smem_bytes(threads) of scan_group.h, evaluated from its source text."""
    src = open(os.path.join(ROOT, "semtools_amd", "csrc", "scan_group.h")).read()
    wide_max = int(re.search(r"constexpr int WIDE_MAX = (\d+);", src).group(1))
    body = re.search(r"static inline size_t wide_smem_bytes\(int threads\)\s*\{\s*return ([^;]+);", src).group(1)
    expr = body.replace("(size_t)", "").replace("sizeof(key_t64)", "8").replace("WIDE_MAX", str(wide_max)).replace("/", "//")
    assert re.fullmatch(r"[\d\s+*/()a-z]+", expr), expr
    return wide_max, int(eval(expr, {"__builtins__": {}}, {"threads": threads}))


@pytest.mark.timeout(900)
def test_wide_scan_fits_beside_the_select_without_spill_or_scratch():
    u = _usage("scan_wide.hip")
    wide = {k: v for k, v in u.items() if "scan_wide_kernel" in k}
    assert len(wide) == 2, list(u)                                 # temporal and non-temporal row loads
    wide_max, dynamic = _wide_smem_bytes(512)                      # (the launcher runs it in blocks of at most 512 threads)
    assert wide_max == 8
    for k, v in wide.items():
        assert "scan_pair_kernel" not in k and "scan_topk_kernel" not in k, k   # (the tests that count those by name)
        assert v["VGPRs"] <= 64 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v.get("ScratchSize [bytes/lane]", 0) == 0, (k, v)
        lds = v.get("LDS Size [bytes/block]", 0) + dynamic
        print(k, "threads 512 LDS", lds, "VGPRs", v["VGPRs"])
        assert lds <= (CU_LDS - SELECT_LDS) // 2, (k, lds)
