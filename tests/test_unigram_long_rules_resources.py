"""Resource budgets of the long-piece kernel under the space rules (unigram_long_rules_kernels.hip), checked at build time (no GPU:
hipcc cross-compiles and reports): the file holds exactly the two forms of ug_long_rules_kernel, and both must show no spilled
VGPR, no scratch, and a lattice of SMT_UG_MAX_LONG nodes with its normalised buffer inside the 64 KiB of LDS a block may ask for --
the skip over an absorbed run needs no LDS of its own, so the bound is ug_long_kernel's (tests/test_unigram_long_resources.py)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def usage():
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "-x", "hip", "--offload-device-only",
                        "-c", os.path.join(ROOT, "semtools_amd", "csrc", "unigram_long_rules_kernels.hip"), "-o", "/dev/null",
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+(?:\[[^\]]+\])?):\s+(\d+)", line)
        if m and name:
            out[name][m.group(1).strip()] = int(m.group(2))
    return out


def test_both_forms_of_the_kernel_are_reported(usage):
    assert len(usage) == 2, sorted(usage)                # a kernel added to the file joins this test
    assert sum("ug_long_rules_kernelILb0" in k for k in usage) == 1 and sum("ug_long_rules_kernelILb1" in k for k in usage) == 1, sorted(usage)


def test_no_spills_no_scratch_and_the_lattice_fits_a_block(usage):
    for k, v in usage.items():
        print(k, v)
        assert v["VGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert 14 * 2048 < v["LDS Size [bytes/block]"] <= 65536, (k, v)     # 14 bytes per node, 2048 nodes, and the normalised buffer
