"""tools/micro/shared_list: the insert routine of scan_wide_kernel's block lists (csrc/shared_list.h) alone.  Eight waves push a fixed
stream of 4096 keys with many equal distances into one list through one lock; the list must end as the sorted k' smallest keys for
k' = 1, 9, 18 and 32, the threshold as the k'-th key, the lock free and the error word 0."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eight_waves_one_list():
    exe = os.path.join(ROOT, "tools", "micro", "shared_list")
    if not os.path.exists(exe):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                               exe + ".hip", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "PASS shared_list" in r.stdout, r.stdout + r.stderr
    for kp in (1, 9, 18, 32):
        assert "kp %d: ok" % kp in r.stdout, r.stdout
