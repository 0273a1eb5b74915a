"""Resource budgets of the large-k route's kernels (topk_large.hip), checked at build time (no GPU: hipcc cross-compiles and reports).

No kernel may spill or use scratch, and the finish kernel's static LDS plus its largest dynamic candidate block (16 Ki keys) must fit
the 160 KiB of a gfx950 CU."""
import pytest

from tests.test_kernel_resources import _usage

KERNELS = ("largek_sample_kernel", "largek_tau_kernel", "largek_collect_kernelILb0", "largek_collect_kernelILb1", "largek_finish_kernel")


@pytest.mark.timeout(900)
def test_largek_kernels_do_not_spill_and_fit_the_lds():
    u = _usage("topk_large.hip")
    for name in KERNELS:
        hits = [v for k, v in u.items() if name in k]
        assert len(hits) == 1, (name, list(u))
        v = hits[0]
        assert v["VGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (name, v)
        assert v["VGPRs"] <= 128, (name, v)
        extra = 16384 * 8 if "finish" in name else 16 * 256 * 8 + 16 if "collect" in name else 0
        assert v["LDS Size [bytes/block]"] + extra <= 160 * 1024, (name, v)
