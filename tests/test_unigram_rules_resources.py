"""Register and LDS budgets of the Unigram device tokenizer's pass 1 under the space rules (unigram_rules_kernels.hip), checked at build
time (no GPU: hipcc cross-compiles and reports): both kernels of the file -- the ASCII scan and the UTF-8 scan, each with its LDS
lattice -- must show no spilled VGPR and no scratch, and the lattice must fit a block many times over, within the bound
tests/test_unigram_resources.py and tests/test_unigram_utf8_resources.py hold the kernels without the rules to."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["ug_scan_rules_kernel", "ug_scan_utf8_rules_kernel"]


@pytest.fixture(scope="module")
def usage():
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "-x", "hip", "--offload-device-only",
                        "-c", os.path.join(ROOT, "semtools_amd", "csrc", "unigram_rules_kernels.hip"), "-o", "/dev/null",
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


def test_every_kernel_of_the_file_is_reported(usage):
    for k in KERNELS:
        assert any(k in name for name in usage), (k, sorted(usage))
    assert len(usage) == len(KERNELS), sorted(usage)     # a kernel added to the file joins this list


def test_no_kernel_spills_or_uses_scratch(usage):
    for k, v in usage.items():
        print(k, v)
        assert v["VGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)


def test_the_lattice_fits_a_block_many_times_over(usage):
    for k, v in usage.items():
        assert 0 < v["LDS Size [bytes/block]"] <= 8192, (k, v)     # 14 bytes per node, 256 + SMT_UG_MAX_WORD nodes, the ASCII tables
