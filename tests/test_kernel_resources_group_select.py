"""Resources of the one-launch-per-pass select (group_select_kernel<8>, tuning key select_group), checked at build time like
tests/test_kernel_resources.py: its blocks run where final_select_kernel<8>'s ran, beside two scan blocks on a CU, so it keeps that
kernel's budget -- <= 96 VGPRs, nothing spilled, no scratch -- and asks for the same dynamic LDS: both launches size it with
final_smem_bytes(k'), and neither kernel has static LDS beside it."""
import os
import re

import pytest

from tests.test_kernel_resources import ROOT, _usage


@pytest.mark.timeout(900)
def test_group_select_keeps_the_budget_of_the_select_it_replaces():
    u = _usage("select.hip")
    group = {k: v for k, v in u.items() if "group_select_kernel" in k}
    assert len(group) == 1 and "group_select_kernelILi8E" in next(iter(group)), list(u)
    own = [v for k, v in u.items() if "final_select_kernelILi8ELb0" in k]
    assert len(own) == 1, list(u)
    g = next(iter(group.values()))
    print("group_select_kernel<8>", g, "final_select_kernel<8>", own[0])
    assert g["VGPRs"] <= 96 and g["VGPRs Spill"] == 0 and g["SGPRs Spill"] == 0, g
    assert g.get("ScratchSize [bytes/lane]", 0) == 0, g
    assert g.get("LDS Size [bytes/block]", 0) == own[0].get("LDS Size [bytes/block]", 0) == 0, (g, own[0])   # static LDS: none in either
    # ... and the dynamic size is one expression for both launch sites
    src = open(os.path.join(ROOT, "semtools_amd", "csrc", "select.hip")).read()
    launches = re.findall(r"hipLaunchKernelGGL\((SELECT_KERNELS\[[^,]+|group_select_kernel<8>), dim3\([^)]*\), dim3\(SEL_THREADS\),\s*([^,]+),", src)
    assert len(launches) == 2 and {smem.strip() for _, smem in launches} == {"final_smem_bytes(a.kp)"}, launches
