"""Register budget of the pair-capable one-query scan (tuning key scan_pair), checked at build time like tests/test_kernel_resources.py.

scan_pair_kernel holds the two-query row loop and runs where the one-query kernel ran: two of its blocks share a CU with the
select of the neighbouring call, 2 x 64 + 4 x 96 = 512 VGPRs per SIMD.  One register more and the select waits for scan blocks to
leave, which costs a third of the step time with every parity test green."""
import pytest

from tests.test_kernel_resources import _usage


@pytest.mark.timeout(900)
def test_pair_capable_scan_fits_beside_the_select_and_does_not_spill():
    u = _usage("scan_pair.hip")
    pair = {k: v for k, v in u.items() if "scan_pair_kernel" in k}
    assert len(pair) == 2, list(u)                                 # temporal and non-temporal row loads
    for k, v in pair.items():
        assert v["VGPRs"] <= 64 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v.get("ScratchSize [bytes/lane]", 0) == 0, (k, v)
    sel = [v for k, v in _usage("select.hip").items() if "final_select_kernelILi8ELb0" in k]
    assert len(sel) == 1 and sel[0]["VGPRs"] <= 96, sel
