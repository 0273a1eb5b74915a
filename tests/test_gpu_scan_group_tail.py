"""The chunk loop of scan_pair_kernel after its cuts: ONE tail for the four query trees (tree g's total comes out in row g of the
wave, where lane 16 g + j reads it), the row loop unrolled by two (the two row buffers swap names, no register copy), and one
wave-uniform base address per full chunk (only the chunk that crosses the end of the corpus clamps its rows).  None of that may move
a rounding or a row: every series here is compared byte for byte (rows, f64 distances, status words) with its scan_pair = 0 run,
which the one-query kernel serves.

The corpora give a wave an odd and an even number of chunks (both halves of the unrolled loop end it), a last chunk of 1, 2 and 3
rows (the clamped path) and of 4 (4096: the full-chunk path up to the last row); scan_pair = 1, 2, 3 make passes that serve exactly
2, 3 and 4 calls (trees 2 and 3 absent, tree 3 absent, all there); k = 56 fills the 64-key lists.  Set up like
tests/test_gpu_scan_group_loop.py: the series runner of tests/test_gpu_scan_pairing.py, scan_pair_wait_us = 2000."""
import os
import subprocess

import pytest

from tests.test_gpu_scan_pairing import _same, _series

pytestmark = pytest.mark.gpu

CALLS = 24
ROWS = (1, 2, 3, 4, 5, 7, 33, 4095, 4096, 4099)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Setup:
    pass


@pytest.fixture(scope="module")
def S():
    import torch
    import semtools_amd as smt

    s = _Setup()
    s.torch = torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(61)
    s.x = torch.randn(max(ROWS), 256, device=dev, generator=g)
    s.x /= s.x.norm(dim=1, keepdim=True)
    s.qs = torch.randn(64, 256, device=dev, generator=g)
    s.qs /= s.qs.norm(dim=1, keepdim=True)
    s.q_adv = None
    torch.cuda.synchronize()
    # (a context whose stream cannot pair at all is given up for one on the next stream: tests/test_gpu_scan_groups.py says why)
    for attempt in range(6):
        s.stream = torch.cuda.Stream(dev)
        s.ctx = smt.Context(0, stream=s.stream.cuda_stream)
        s.corpora = {n: smt.Corpus(s.ctx, device_ptr=s.x.data_ptr(), rows=n) for n in ROWS + (1000,)}
        s.ctx.set_tuning("async_select", 1)
        if _series(s, (1000,), 8, (10,), 1)[1][0] > 0 or attempt == 5:
            break
        for c in s.corpora.values():
            c.close()
        s.ctx.close()
    s.want = {}
    s.seen = {}                                                    # scan_pair -> launches that served 1, 2, 3, 4 calls, summed
    yield s
    for c in s.corpora.values():
        c.close()
    s.ctx.close()


def _alone(s, rows, k):
    """The scan_pair = 0 answers of a series, computed once."""
    if (rows, k) not in s.want:
        got, counts = _series(s, (rows,), CALLS, (k,), pair=0)
        assert counts == (0, 0, 0), counts
        s.want[(rows, k)] = got
    return s.want[(rows, k)]


@pytest.mark.parametrize("pair", [1, 2, 3])
@pytest.mark.parametrize("k", [1, 10, 56])
@pytest.mark.parametrize("rows", ROWS)
def test_groups_of_two_three_and_four_equal_the_lone_scan(S, rows, k, pair):
    want = _alone(S, rows, k)
    before = S.ctx.scan_groups()
    got, counts = _series(S, (rows,), CALLS, (k,), pair=pair)
    by_size = tuple(int(b - a) for a, b in zip(before, S.ctx.scan_groups()))
    print("rows", rows, "k", k, "scan_pair", pair, "launches by calls served", by_size)
    _same(got, want)
    assert sum((n + 1) * v for n, v in enumerate(by_size)) == CALLS, (by_size, counts)
    assert all(v == 0 for v in by_size[pair + 1:]), by_size        # no group larger than scan_pair + 1
    S.seen[pair] = tuple(a + b for a, b in zip(S.seen.get(pair, (0, 0, 0, 0)), by_size))


def test_every_group_size_was_seen(S):
    """Passes that served exactly 2, 3 and 4 calls occurred in the series above (smt_debug_scan_groups): scan_pair = n makes groups
    of n + 1 where the host is far enough ahead, which scan_pair_wait_us = 2000 sees to."""
    for pair in (1, 2, 3):
        if pair not in S.seen:                                     # (run alone: one series per group limit)
            before = S.ctx.scan_groups()
            _series(S, (4099,), CALLS, (10,), pair=pair)
            S.seen[pair] = tuple(int(b - a) for a, b in zip(before, S.ctx.scan_groups()))
        print("scan_pair", pair, "launches by calls served", S.seen[pair])
        assert S.seen[pair][pair] > 0, (pair, S.seen[pair])


def test_merged_tail_equals_the_lone_tree_bit_for_bit():
    """tools/micro/wave_sum4_group_tail: heads, row steps and the merged tail against wave_sum4 on 64 rounds of inputs whose sums
    depend on the order of the additions -- <c, c> in every lane, query tree g in every lane of row g; also for a group of two."""
    exe = os.path.join(ROOT, "tools", "micro", "wave_sum4_group_tail")
    if not os.path.exists(exe):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                               exe + ".hip", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS wave_sum4_group_tail" in r.stdout, r.stdout + r.stderr
