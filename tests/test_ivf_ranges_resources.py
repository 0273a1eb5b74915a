"""Resource budget of the search inside ranges (ivfpq_search.hip), checked at build time (no GPU: hipcc cross-compiles and reports).

The mask kernel and the four RANGED instantiations of ivf_adc_kernel must not spill and must not cost their unfiltered twins'
occupancy: same LDS, and a VGPR count inside the twin's allocation step (8 registers per lane; waves per SIMD = min(8, 512 // alloc)).
The four unfiltered instantiations -- the ones every search without ranges and the bench run -- must be what they were before the
ranged ones existed."""
import pytest

from tests.test_kernel_resources import _usage

# ivf_adc_kernel<THREADS, KIND> of commit 1c7a3332ac89c97db7f7be91ccc852c6d3ce3d19 (the parent of the ranged search), cross-compiled
# with the flags of _usage: (VGPRs, TotalSGPRs, LDS bytes per block, scratch bytes per lane)
PARENT = {(512, 1): (76, 106, 4096, 0), (256, 1): (67, 106, 2048, 0), (512, 0): (93, 81, 36864, 0), (256, 0): (93, 81, 34816, 0)}


def _waves(vgprs):
    alloc = -(-vgprs // 8) * 8
    return min(8, 512 // alloc)


@pytest.fixture(scope="module")
def usage():
    return _usage("ivfpq_search.hip")


def _adc(usage, threads, kind, ranged):
    hits = [v for k, v in usage.items() if f"ivf_adc_kernelILi{threads}ELi{kind}ELb{int(ranged)}EE" in k]
    assert len(hits) == 1, list(usage)
    return hits[0]


@pytest.mark.timeout(900)
def test_mask_kernel_and_ranged_scans_do_not_spill(usage):
    mask = [v for k, v in usage.items() if "ivf_range_mask_kernel" in k]
    assert len(mask) == 1, list(usage)
    for v in mask + [_adc(usage, t, k, True) for t, k in PARENT]:
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, v


@pytest.mark.timeout(900)
@pytest.mark.parametrize("threads,kind", sorted(PARENT))
def test_ranged_scan_keeps_the_occupancy_step_of_its_twin(usage, threads, kind):
    twin, ranged = _adc(usage, threads, kind, False), _adc(usage, threads, kind, True)
    print(f"<{threads}, {kind}>: twin {twin['VGPRs']} VGPRs, ranged {ranged['VGPRs']}")
    assert ranged["LDS Size [bytes/block]"] == twin["LDS Size [bytes/block]"], (twin, ranged)
    assert ranged["VGPRs"] <= -(-twin["VGPRs"] // 8) * 8, (twin, ranged)       # not above the twin's step boundary
    assert _waves(ranged["VGPRs"]) == _waves(twin["VGPRs"]), (twin, ranged)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("threads,kind", sorted(PARENT))
def test_unfiltered_scan_is_what_it_was(usage, threads, kind):
    v = _adc(usage, threads, kind, False)
    got = (v["VGPRs"], v["TotalSGPRs"], v["LDS Size [bytes/block]"], v["ScratchSize [bytes/lane]"])
    assert got == PARENT[(threads, kind)], (got, PARENT[(threads, kind)])
    assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, v
