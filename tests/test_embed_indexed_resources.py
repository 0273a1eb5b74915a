"""Register budgets of K1's indexed kernels (embed_kernels.hip), checked at build time (no GPU: hipcc cross-compiles and reports).

embed_indexed_kernel<T, PF> -- the gather through the token array {row, weight} of a vocabulary-quantised model -- shares its body
with embed_kernel and runs at four waves per SIMD like it (__launch_bounds__(256, 4)): every instantiation -- f32, half and int8
tables, ids and token entries prefetched or not -- must stay within 128 VGPRs without spilling and without scratch."""
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


@pytest.fixture(scope="module")
def kernels():
    u = _usage("embed_kernels.hip")
    # Itanium mangling of embed_indexed_kernel<T, PF>: T = f (float), DF16_ (_Float16), a (signed char); PF = Lb1 / Lb0
    found = {}
    for k, v in u.items():
        m = re.search(r"embed_indexed_kernelI(f|DF16_|a)Lb([01])E", k)
        if m:
            found[({"f": "f32", "DF16_": "f16", "a": "i8"}[m.group(1)], m.group(2) == "1")] = v
    return found, u


def test_all_six_indexed_instantiations_and_the_pack_kernel_exist(kernels):
    found, everything = kernels
    assert sorted(found) == sorted((t, pf) for t in ("f32", "f16", "i8") for pf in (False, True)), sorted(found)
    assert any("embed_pack_tokens_kernel" in k for k in everything)


def test_no_indexed_instantiation_spills_or_leaves_four_waves_per_simd(kernels):
    for k, v in kernels[0].items():
        print(k, v)
        assert v["VGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["VGPRs"] <= 128, (k, v)
