"""Resource budgets of the grouped large-k collect (topk_large.hip), checked at build time (no GPU): each of its six instantiations must
neither spill nor use scratch, stay within 128 VGPRs, and fit 160 KiB of LDS with 16 waves x G x 64 keys and the chunk counter."""
import pytest

from tests.test_kernel_resources import _usage


@pytest.mark.timeout(900)
def test_grouped_collect_kernels_do_not_spill_and_fit_the_lds():
    u = _usage("topk_large.hip")
    for g in (2, 3, 4):
        for filtered in (0, 1):
            name = f"largek_collect_group_kernelILi{g}ELb{filtered}E"
            (v,) = [v for k, v in u.items() if name in k]
            assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (name, v)
            assert v["VGPRs"] <= 128, (name, v)
            assert v["LDS Size [bytes/block]"] + 16 * g * 64 * 8 + 16 <= 160 * 1024, (name, v)
