"""Resources of the sixteen-call one-query scan (scan_deep_kernel, tuning key scan_deep), checked at build time like
tests/test_kernel_resources_wide.py: it runs where scan_wide_kernel runs, two scan blocks of neighbouring streams on a CU beside one
select -- 2 x 64 + 4 x 96 = 512 VGPRs per SIMD, and (160 KiB - 84 KiB of the select at the headline's k = 10) / 2 of LDS per block."""
import os
import re

import pytest

from tests.test_kernel_resources import ROOT, _usage
from tests.test_kernel_resources_groups import CU_LDS, SELECT_LDS


def _deep_smem_bytes(threads):
    """deep_smem_bytes(threads) of scan_group.h, evaluated from its source text."""
    src = open(os.path.join(ROOT, "semtools_amd", "csrc", "scan_group.h")).read()
    deep_max = int(re.search(r"constexpr int DEEP_MAX = (\d+);", src).group(1))
    body = re.search(r"static inline size_t deep_smem_bytes\(int threads\)\s*\{\s*return ([^;]+);", src).group(1)
    expr = body.replace("(size_t)", "").replace("sizeof(key_t64)", "8").replace("DEEP_MAX", str(deep_max)).replace("/", "//")
    assert re.fullmatch(r"[\d\s+*/()a-z]+", expr), expr
    return deep_max, int(eval(expr, {"__builtins__": {}}, {"threads": threads}))


@pytest.mark.timeout(900)
def test_deep_scan_fits_beside_the_select_without_spill_or_scratch():
    u = _usage("scan_deep.hip")
    deep = {k: v for k, v in u.items() if "scan_deep_kernel" in k}
    assert len(deep) == 2, list(u)                                 # temporal and non-temporal row loads
    deep_max, dynamic = _deep_smem_bytes(512)                      # (the launcher runs it in blocks of at most 512 threads)
    assert deep_max == 16
    # sixteen lists of 32 keys, sixteen records, sixteen locks, sixteen 1 KiB images, the control words: about 21 KiB at any block size
    assert dynamic == _deep_smem_bytes(64)[1] and 16 * (256 + 16 + 4 + 1024) <= dynamic <= 21 * 1024, dynamic
    for k, v in deep.items():
        for other in ("scan_wide_kernel", "scan_pair_kernel", "scan_topk_kernel"):   # (the tests that count those by name)
            assert other not in k, k
        assert v["VGPRs"] <= 64 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v.get("ScratchSize [bytes/lane]", 0) == 0, (k, v)
        lds = v.get("LDS Size [bytes/block]", 0) + dynamic
        print(k, "threads 512 LDS", lds, "VGPRs", v["VGPRs"])
        assert lds <= (CU_LDS - SELECT_LDS) // 2, (k, lds)
        assert 2 * lds + SELECT_LDS <= CU_LDS, (k, lds)            # two scan blocks and the select
