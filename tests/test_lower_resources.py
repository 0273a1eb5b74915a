"""The lower-casing kernels (lower_kernels.hip) keep everything in registers and LDS, checked at build time (no GPU: hipcc
cross-compiles and reports): no scratch and no spill -- the output code points of a character are three scalars, not an indexed
array -- and the LDS image of the tables leaves room for eight blocks on a CU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _usage(src):
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "-x", "hip", "--offload-device-only",
                        "-c", os.path.join(ROOT, "semtools_amd", "csrc", src), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
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


@pytest.mark.timeout(900)
def test_the_lower_kernels_have_no_scratch():
    u = _usage("lower_kernels.hip")
    kernels = {k: v for k, v in u.items() if "lower_flag_kernel" in k or "lower_pass_kernel" in k}
    assert len(kernels) == 3, list(u)                    # the flag pass, the counting pass, the writing pass
    for k, v in kernels.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v["VGPRs"] <= 64, (k, v)                  # 8 waves per SIMD
        assert v["LDS Size [bytes/block]"] <= 16 * 1024, (k, v)
