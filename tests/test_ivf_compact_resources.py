"""Resource budget of the kernels that carry an IVF index through a compaction (ivfpq_compact.hip), checked at build time (no GPU:
hipcc cross-compiles and reports).

They hold nothing that needs many registers: no spill, no scratch, at most 64 VGPRs (8 waves per SIMD).  If an unroll ever needs
more, the unroll comes down, not this cap.  LDS is allowed and recorded here, bytes per block:
  ivf_compact_mark_kernel     24592  (1024 staged ranges = 16 KiB, their prefixes = 8 KiB, 4 wave counts)
  ivf_compact_scan_kernel        64  (16 wave totals)
  ivf_compact_offsets_kernel      0
  ivf_compact_move_kernel         0  (the source of a wave's e-th kept entry comes from the ballot word in registers)"""
import pytest

from tests.test_kernel_resources import _usage

LDS = {"ivf_compact_mark_kernel": 24592, "ivf_compact_scan_kernel": 64, "ivf_compact_offsets_kernel": 0, "ivf_compact_move_kernel": 0}


@pytest.mark.timeout(900)
def test_index_compaction_kernels_do_not_spill_and_stay_within_64_vgprs():
    u = _usage("ivfpq_compact.hip")
    assert len(u) == len(LDS), list(u)                 # every kernel of the file is named here
    for name, lds in LDS.items():
        hits = [v for k, v in u.items() if name in k]
        assert len(hits) == 1, (name, list(u))
        v = hits[0]
        print(name, v)
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
        assert v["ScratchSize [bytes/lane]"] == 0, (name, v)
        assert v["VGPRs"] <= 64, (name, v)
        assert v["LDS Size [bytes/block]"] == lds, (name, v)
