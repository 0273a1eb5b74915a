"""scan_deep_kernel permutes a chunk's four rows by lane (register k of lane l holds row k ^ (l & 3)) and runs the heads of its
seventeen reduction trees without selects (csrc/device_utils.h: swizzle_rows4, wave_sum4_swizzled_head).  No sum may change a bit and
no lane may be paired with another row: the micro tool compares the trees with wave_sum4 on-device, and every series here is compared
byte for byte (rows, f64 distances, status words) with its scan_deep = 0 run, which the one-query kernel serves, at the smallest
shapes where a permutation can go wrong -- ragged last chunks (the clamped copies of the last row), the winner in each position of
a chunk, near-ties in every place of a group.  Passes that served sixteen calls must occur (all four phases of the chunk).

Set up like tests/test_gpu_scan_deep.py, whose series runner and accounting are used as they are."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_nearties import adversarial_corpus
from tests.test_gpu_scan_deep import _accounted, _same, _series, _sixteen_per_group

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = 64                                                         # 32 per stream: two full groups of sixteen
DEEP = 15
RAGGED = (2, 3, 4, 5, 6, 7, 4 * 64 + 1, 4 * 64 + 2, 4 * 64 + 3)   # one chunk, two chunks, and a ragged chunk behind a full turn of 64 chunks
ADV = {(seed, n): dict(n=n, n_better=5, n_cluster=24 if n < 100 else 40, seed=seed) for seed in (55, 56) for n in (33, 1000)}


class _Setup:
    pass


@pytest.fixture(scope="module")
def H():
    import torch
    import semtools_amd as smt

    s = _Setup()
    s.torch = torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(77)

    def unit(t):
        return t / t.norm(dim=-1, keepdim=True)

    s.x = unit(torch.randn(1000, 256, device=dev, generator=g))
    s.qs = unit(torch.randn(64, 256, device=dev, generator=g))
    # ragged chunks: the LAST row of each corpus is u, and the sixteen queries lie around u
    u = unit(torch.randn(256, device=dev, generator=g))
    s.q_last = unit(u + 0.3 * unit(torch.randn(16, 256, device=dev, generator=g))).contiguous()
    s.tensors = {}
    for n in RAGGED:
        t = s.x[:n].clone()
        t[n - 1] = u
        s.tensors[("ragged", n)] = t
    # row positions: 64 rows, sixteen chunks; query g's winner (the query itself) at position (g + shift) % 4 of chunk g
    s.q_pos = s.qs[32:48].contiguous()
    for shift in range(4):
        t = s.x[100:164].clone()
        for q in range(16):
            t[4 * q + (q + shift) % 4] = s.q_pos[q]
        s.tensors[("pos", shift)] = t
    s.adv = {key: adversarial_corpus(**kw) for key, kw in ADV.items()}
    torch.cuda.synchronize()
    # (why a context that cannot take anything along is given up for one on the next stream: tests/test_gpu_scan_groups.py)
    for attempt in range(6):
        s.stream = torch.cuda.Stream(dev)
        s.ctx = smt.Context(0, stream=s.stream.cuda_stream)
        s.corpora = {1000: smt.Corpus(s.ctx, device_ptr=s.x.data_ptr(), rows=1000)}
        s.ctx.set_tuning("async_select", 1)
        if _series(s, (1000,), 8, (10,), DEEP)[2][0] > 0 or attempt == 5:
            break
        for c in s.corpora.values():
            c.close()
        s.ctx.close()
    for key, t in s.tensors.items():
        s.corpora[key] = smt.Corpus(s.ctx, device_ptr=t.data_ptr(), rows=t.shape[0])
    for key, (_, emb, _) in s.adv.items():
        c = smt.Corpus(s.ctx)
        c.append(emb)
        s.corpora[("adv",) + key] = c
    s.ctx.set_tuning("async_select", 1)
    yield s
    for c in s.corpora.values():
        c.close()
    s.ctx.close()


def _both(s, name, k, queries, want_check=None, tries=6):
    """The scan_deep = 0 series once, then up to `tries` series at scan_deep = 15, each compared and accounted for; returns the
    reference and how many launches served sixteen calls."""
    want, deep0, counts0, wide0 = _series(s, (name,), CALLS, (k,), 0, qsel=_sixteen_per_group, queries=queries)
    assert counts0 == (0, 0, 0) and deep0 == (0,) * 16 and wide0 == (0,) * 8, (counts0, deep0, wide0)
    if want_check:
        want_check(want)
    sixteen = 0
    for _ in range(tries):
        got, deep, counts, wide = _series(s, (name,), CALLS, (k,), DEEP, qsel=_sixteen_per_group, queries=queries)
        _same(got, want)
        _accounted(deep, counts, wide, CALLS)
        sixteen += deep[15]
        if sixteen:
            break
    return want, sixteen


def test_permuted_heads_equal_the_lone_tree_bit_for_bit():
    """tools/micro/wave_sum4_swizzled: the rows permuted in place, the products on the permuted registers, the heads without selects,
    the row steps and both tails against wave_sum4 on 64 rounds of inputs whose sums depend on the order of the additions (with
    signed zeros, denormals and one huge element per row among them)."""
    exe = os.path.join(ROOT, "tools", "micro", "wave_sum4_swizzled")
    if not os.path.exists(exe):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                               exe + ".hip", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS wave_sum4_swizzled" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("waves", [1, 8])
@pytest.mark.parametrize("rows", RAGGED)
def test_ragged_last_chunk(H, rows, waves):
    """The last chunk holds 1, 2 or 3 rows and clamped copies of the last one, which is every query's best match: it must be listed
    once, under its own number, whichever register the permutation put the copies in."""
    H.ctx.set_tuning("scan_blocks", 1)
    H.ctx.set_tuning("scan_threads", 64 * waves)
    try:
        sixteen = 0
        for k in (1, 10):
            def check(want, k=k):
                n_out = min(k, rows)
                for i in range(CALLS):
                    got = want[0][i, :n_out].tolist()
                    assert got[0] == rows - 1 and len(set(got)) == n_out and all(0 <= r < rows for r in got), (i, got)
            sixteen += _both(H, ("ragged", rows), k, H.q_last, check)[1]
        assert sixteen > 0                                         # a pass went through all four phases
    finally:
        H.ctx.set_tuning("scan_blocks", 0)
        H.ctx.set_tuning("scan_threads", 512)


@pytest.mark.parametrize("shift", range(4))
def test_winner_in_every_position_of_a_chunk(H, shift):
    """Query g's winner is row (g + shift) % 4 of chunk g: a lane that tested another row of the chunk than the one it reports returns
    another row number."""
    def check(want):
        for i in range(CALLS):
            q = _sixteen_per_group(i)
            assert want[0][i, 0] == 4 * q + (q + shift) % 4, (i, want[0][i])
    assert _both(H, ("pos", shift), 1, H.q_pos, check)[1] > 0


@pytest.mark.parametrize("key", sorted(ADV))
def test_near_ties_in_every_place_of_a_group(H, key):
    """Near-ties around the 10th place in 33 and in 1000 rows, the query in each of the sixteen places of a group in turn: which of
    them the f32 scan nominates decides the verdict, so the status words must be equal too."""
    q_adv = H.torch.from_numpy(H.adv[key][0]).to(H.qs.device)
    sixteen, words = 0, set()
    for place in range(16):
        qs = H.qs[16:32].clone()
        qs[place] = q_adv
        want, n = _both(H, ("adv",) + key, 10, qs, tries=1 if sixteen else 6)
        words |= set(np.unique(want[2][[i for i in range(CALLS) if _sixteen_per_group(i) == place]]).tolist())
        sixteen += n
    print("near-ties", key, "status words of the query:", sorted(words))
    assert sixteen > 0
