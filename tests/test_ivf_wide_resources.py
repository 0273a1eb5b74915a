"""Resource budget of the wide IVF searches (ivfpq_search.hip), checked at build time (no GPU: hipcc cross-compiles and reports).

The eight instantiations of ivf_adc_pool_kernel and the pool's finish kernel must not spill; a pool instantiation shares stage 1
with its ivf_adc_kernel twin and must not cost its occupancy: no more LDS, and a VGPR count inside the twin's allocation step
(8 registers per lane; waves per SIMD = min(8, 512 // alloc))."""
import pytest

from tests.test_kernel_resources import _usage

INSTANCES = [(t, k, r) for t in (256, 512) for k in (0, 1) for r in (False, True)]


def _waves(vgprs):
    alloc = -(-vgprs // 8) * 8
    return min(8, 512 // alloc)


@pytest.fixture(scope="module")
def usage():
    return _usage("ivfpq_search.hip")


def _kernel(usage, name, threads, kind, ranged):
    hits = [v for k, v in usage.items() if f"{name}ILi{threads}ELi{kind}ELb{int(ranged)}EE" in k]
    assert len(hits) == 1, list(usage)
    return hits[0]


@pytest.mark.timeout(900)
def test_pool_scans_and_the_finish_do_not_spill(usage):
    finish = [v for k, v in usage.items() if "ivf_pool_finish_kernel" in k]
    assert len(finish) == 1, list(usage)
    for v in finish + [_kernel(usage, "ivf_adc_pool_kernel", t, k, r) for t, k, r in INSTANCES]:
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, v
    assert finish[0]["LDS Size [bytes/block]"] <= 64 * 1024, finish[0]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("threads,kind,ranged", INSTANCES)
def test_pool_scan_keeps_the_lds_and_the_occupancy_step_of_its_twin(usage, threads, kind, ranged):
    twin, pool = _kernel(usage, "ivf_adc_kernel", threads, kind, ranged), _kernel(usage, "ivf_adc_pool_kernel", threads, kind, ranged)
    print(f"<{threads}, {kind}, {ranged}>: twin {twin['VGPRs']} VGPRs, pool {pool['VGPRs']}")
    assert pool["LDS Size [bytes/block]"] <= twin["LDS Size [bytes/block]"], (twin, pool)
    assert _waves(pool["VGPRs"]) == _waves(twin["VGPRs"]), (twin, pool)
