"""Resource budget of the compaction kernel (compact.hip), checked at build time (no GPU: hipcc cross-compiles and reports).

The move must not take occupancy from anything else: no spill, no scratch, no LDS, and at most 64 VGPRs (8 waves per SIMD).  If a
deeper unroll ever needs more registers, the unroll comes down, not this cap."""
import pytest

from tests.test_kernel_resources import _usage

KERNELS = ("compact_gather_kernel",)


@pytest.mark.timeout(900)
def test_compact_kernels_do_not_spill_use_no_lds_and_stay_within_64_vgprs():
    u = _usage("compact.hip")
    assert len(u) == len(KERNELS), list(u)             # every kernel of the file is named here
    for name in KERNELS:
        hits = [v for k, v in u.items() if name in k]
        assert len(hits) == 1, (name, list(u))
        v = hits[0]
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
        assert v["ScratchSize [bytes/lane]"] == 0, (name, v)
        assert v["LDS Size [bytes/block]"] == 0, (name, v)
        assert v["VGPRs"] <= 64, (name, v)
