"""scan_deep_kernel folds the sixteen queries x four rows of a chunk into ONE register, one (row, query) pair per lane
(csrc/device_utils.h, the folded lane map: lane l = 16 R + 4 i + j tests row j ^ (i odd ? 3 : 0) against query 4 R + ((4 - i) & 3)),
and runs one distance, one compare and one ballot per chunk.  No sum may change a bit, no lane may be paired with another row, query,
record or <c, c>, and the lists must not care in which order candidates are offered: the micro tool compares every stage of the trees
with wave_sum4 on-device, and every series here is compared byte for byte (rows, f64 distances, status words) with its scan_deep = 0
run, which the one-query kernel serves, at the smallest shapes where the new map can go wrong.  Passes of sixteen must occur.

Set up like tests/test_gpu_scan_deep.py, whose series runner and accounting are used as they are."""
import os
import subprocess

import pytest

from tests.test_gpu_nearties import adversarial_corpus
from tests.test_gpu_scan_deep import _accounted, _same, _series, _sixteen_per_group

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = 64                                                         # 32 per stream: two full groups of sixteen
DEEP = 15
RAGGED = (1, 2, 3, 4, 5, 6, 7, 4 * 64 + 1, 4 * 64 + 2, 4 * 64 + 3)   # one chunk, two chunks, and a ragged chunk behind a full turn of 64 chunks
ADV = {(seed, n): dict(n=n, n_better=5, n_cluster=24 if n < 100 else 40, seed=seed) for seed in (55, 56) for n in (33, 1000)}
N_STEEP = 4096
CC_CHUNK = 5                                                       # the chunk of the 64-row corpora that holds the special row


class _Setup:
    pass


@pytest.fixture(scope="module")
def F():
    import torch
    import semtools_amd as smt

    s = _Setup()
    s.torch = torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(83)

    def unit(t):
        return t / t.norm(dim=-1, keepdim=True)

    s.x = unit(torch.randn(2000, 256, device=dev, generator=g))
    s.qs = unit(torch.randn(64, 256, device=dev, generator=g))
    s.tensors = {("x", 0): s.x[:1000], ("x", 1): s.x[1000:]}
    # ragged chunks: the LAST row of each corpus is u, and the sixteen queries lie around u
    u = unit(torch.randn(256, device=dev, generator=g))
    s.q_last = unit(u + 0.3 * unit(torch.randn(16, 256, device=dev, generator=g))).contiguous()
    for n in RAGGED:
        t = s.x[:n].clone()
        t[n - 1] = u
        s.tensors[("ragged", n)] = t
    # lane <-> (query, row): 64 rows, sixteen chunks; query g's winner (the query itself) at position (g + shift) % 4 of chunk g
    s.q_pos = s.qs[32:48].contiguous()
    s.q_pos_reversed = s.q_pos.flip(0).contiguous()
    for shift in range(4):
        t = s.x[100:164].clone()
        for q in range(16):
            t[4 * q + (q + shift) % 4] = s.q_pos[q]
        s.tensors[("pos", shift)] = t
    # <c, c> per lane: 64 rows that point AWAY from the queries (distances about 1.6), and at position pos of one chunk
    #   zero: the zero row, at distance 1 every nonzero query's best match and at distance 0 the zero query's (a lane that took
    #         another row's <c, c> for it, or its <c, c> for another row, moves a row across that gap);
    #   dup:  a copy of row 2, every query's best match by construction (u itself): equal keys but for the row number;
    #   norm: every row scaled by 1, 30, 900 or 27000 by its position in the chunk, rotated chunk by chunk -- the cosine distance
    #         does not change, what the kernel computes with another row's <c, c> is off by a factor of 30 at the least
    s.q_cc = s.q_last
    away = (-unit(u + 0.5 * unit(torch.randn(64, 256, device=dev, generator=g)))).contiguous()
    scale = torch.tensor([1.0, 30.0, 900.0, 27000.0], device=dev)
    for pos in range(4):
        t = away.clone()
        t[4 * CC_CHUNK + pos] = 0.0
        s.tensors[("zero", pos)] = t
        t = away.clone()
        t[2] = u
        t[4 * CC_CHUNK + pos] = u
        s.tensors[("dup", pos)] = t
        t = s.x[300:364].clone()
        for r in range(64):
            t[r] *= scale[(r + r // 4 + pos) % 4]
        s.tensors[("norm", pos)] = t
    # insert order: distances that fall strictly with the row number, and the mirror image (tests/test_gpu_scan_deep.py)
    basis = torch.linalg.qr(torch.randn(256, 18, device=dev, generator=g, dtype=torch.float64))[0].T
    theta = torch.linspace(1.5, 0.1, N_STEEP, device=dev, dtype=torch.float64)
    s.tensors["steep"] = (torch.cos(theta)[:, None] * basis[0] + torch.sin(theta)[:, None] * basis[1]).float().contiguous()
    s.tensors["mirror"] = s.tensors["steep"].flip(0).contiguous()
    s.qsteep = (basis[0] + 0.2 * basis[2:18]).float().contiguous()
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
    s.ref = {}
    s.blocks_waves = (0, 8)
    yield s
    for c in s.corpora.values():
        c.close()
    s.ctx.close()


def _want(s, names, ks, queries, qsel=_sixteen_per_group, want_check=None):
    """The scan_deep = 0 answers of a series at the current block settings: computed once, checked once, never changed."""
    key = (names, ks, queries.data_ptr(), qsel, s.blocks_waves)
    if key not in s.ref:
        want, deep0, counts0, wide0 = _series(s, names, CALLS, ks, 0, qsel=qsel, queries=queries)
        assert counts0 == (0, 0, 0) and deep0 == (0,) * 16 and wide0 == (0,) * 8, (counts0, deep0, wide0)
        if want_check:
            want_check(want)
        s.ref[key] = want
    return s.ref[key]


def _both(s, name, k, queries, want_check=None, tries=6, take=DEEP, qsel=_sixteen_per_group, most=None, names=None):
    """The scan_deep = 0 series over corpus `name` (or the corpora `names` in turn), then up to `tries` series at scan_deep = take, each
    compared and accounted for; returns the reference and how many launches served `most` calls (take + 1 unless given)."""
    names = names or (name,)
    most = take + 1 if most is None else most
    want = _want(s, names, (k,), queries, qsel, want_check)
    full = 0
    for _ in range(tries):
        got, deep, counts, wide = _series(s, names, CALLS, (k,), take, qsel=qsel, queries=queries)
        _same(got, want)
        _accounted(deep, counts, wide, CALLS, take=most - 1)
        full += deep[most - 1]
        if full:
            break
    return want, full


def _blocks(s, blocks, waves):
    s.blocks_waves = (blocks, waves)
    s.ctx.set_tuning("scan_blocks", blocks)
    s.ctx.set_tuning("scan_threads", 64 * waves)


def test_folded_trees_equal_the_lone_tree_bit_for_bit():
    """tools/micro/wave_sum4_folded: the rows permuted by m(l), the query images read from the slots they were written to, V, W, X and the
    final register of sixteen trees and the <c, c> column against wave_sum4 and its stages, all 64 lanes, on 64 rounds of inputs whose sums
    depend on the order of the additions (signed zeros, denormals and one huge element per row among them), for passes of one to
    four phases through the progressive tail; each of the 64 (query, row) pairs is held by one lane."""
    exe = os.path.join(ROOT, "tools", "micro", "wave_sum4_folded")
    if not os.path.exists(exe):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                               exe + ".hip", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS wave_sum4_folded" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("shift", range(4))
def test_every_lane_reports_its_own_row_and_query(F, shift, reverse):
    """Query g's winner is row (g + shift) % 4 of chunk g, shift 0 .. 3: all 64 (query, row) pairs.  A lane that tested another row than
    the one it reports returns another row number, a lane that read another query's record or offered to another query's list
    loses the winner; the same with the sixteen queries in the opposite order (every query in the mirrored place of the group)."""
    def check(want):
        for i in range(CALLS):
            q = 15 - _sixteen_per_group(i) if reverse else _sixteen_per_group(i)
            assert want[0][i, 0] == 4 * q + (q + shift) % 4, (i, want[0][i])
    assert _both(F, ("pos", shift), 1, F.q_pos_reversed if reverse else F.q_pos, check)[1] > 0


@pytest.mark.parametrize("waves", [1, 8])
@pytest.mark.parametrize("rows", RAGGED)
def test_ragged_last_chunk_with_reversed_rows(F, rows, waves):
    """The last chunk holds 1, 2 or 3 rows and clamped copies of the last one, which is every query's best match; the odd quads of
    a wave hold the rows of a chunk in reverse, so the lanes that are off differ from quad to quad.  The last row must be listed
    once, under its own number, and no row twice."""
    _blocks(F, 1, waves)
    try:
        sixteen = 0
        for k in (1, 10):
            def check(want, k=k):
                n_out = min(k, rows)
                for i in range(CALLS):
                    got = want[0][i, :n_out].tolist()
                    assert got[0] == rows - 1 and len(set(got)) == n_out and all(0 <= r < rows for r in got), (i, got)
            sixteen += _both(F, ("ragged", rows), k, F.q_last, check)[1]
        assert sixteen > 0                                         # a pass went through all four phases
    finally:
        _blocks(F, 0, 8)


@pytest.mark.parametrize("pos", range(4))
def test_zero_row_in_every_position_of_a_chunk(F, pos):
    """Every lane computes its distance with the <c, c> of ITS row: the zero row is every query's best match at distance 1 (the other
    rows point away), the ten answers behind it are decided by the other rows' own norms."""
    def check(want):
        assert (want[0][:, 0] == 4 * CC_CHUNK + pos).all() and (want[1][:, 0] == 1.0).all(), want[0][:, 0]
    assert _both(F, ("zero", pos), 10, F.q_cc, check)[1] > 0


@pytest.mark.parametrize("pos", range(4))
def test_duplicate_of_the_winner_in_every_position_of_a_chunk(F, pos):
    def check(want):
        assert want[0][:, :2].tolist() == [[2, 4 * CC_CHUNK + pos]] * CALLS, want[0][:, :2]   # equal keys: in row order
    assert _both(F, ("dup", pos), 10, F.q_cc, check)[1] > 0


@pytest.mark.parametrize("pos", range(4))
def test_rows_of_very_different_norms(F, pos):
    assert _both(F, ("norm", pos), 10, F.qs[16:32].contiguous())[1] > 0


def test_zero_query_in_every_place_of_a_group(F):
    """The zero rules go through the one distance of the chunk: against the zero query the zero row is at distance 0 and every other
    row at 1, in whichever lane the query sits."""
    sixteen = 0
    for place in range(16):
        qs = F.q_cc.clone()
        qs[place] = 0.0
        F.keep = getattr(F, "keep", []) + [qs]                    # (the references are keyed by the queries' address)

        def check(want, place=place):
            for i in range(CALLS):
                if _sixteen_per_group(i) == place:
                    assert want[0][i, 0] == 4 * CC_CHUNK + 1 and want[1][i, 0] == 0.0 and (want[1][i, 1:10] == 1.0).all(), (i, want[1][i])
        sixteen += _both(F, ("zero", 1), 10, qs, check, tries=1 if sixteen else 6)[1]
    assert sixteen > 0


@pytest.mark.parametrize("take", range(8, 16))
def test_limits_eight_to_fifteen(F, take):
    """A pass of 9 .. 16 calls: phases 2 and 3 on or off, the last phase that is on with one to four queries."""
    full = _both(F, 1000, 10, F.qs[:16].contiguous(), take=take)[1]
    print("limit", take, "launches that served", take + 1, ":", full)
    assert full > 0 or take < DEEP


@pytest.mark.parametrize("size", range(1, 17))
def test_groups_that_end_early_at_every_size(F, size):
    """Runs of `size` calls per stream in front of one corpus, then as many in front of another with the same number of rows: passes
    of at most `size` calls, the queries behind the last one absent -- their images are whatever the block's memory holds, their
    lanes are off and must never insert."""
    names = (("x", 0),) * (2 * size) + (("x", 1),) * (2 * size)
    want, full = _both(F, None, 10, F.qs[:16].contiguous(), most=size, names=names)
    print("runs of", size, ": launches that served", size, ":", full)
    assert full > 0


@pytest.mark.parametrize("key", sorted(ADV))
def test_near_ties_in_every_place_of_full_and_partial_passes(F, key):
    """Near-ties around the 10th place in 33 and in 1000 rows, the query in each of the sixteen places of a group in turn, in passes of
    sixteen and in passes cut at a limit of 8 .. 15: which of them the f32 scan nominates decides the verdict, so the status words
    must be equal too."""
    q_adv = F.torch.from_numpy(F.adv[key][0]).to(F.qs.device)
    sixteen = 0
    for place in range(16):
        qs = F.qs[16:32].clone()
        qs[place] = q_adv
        F.keep = getattr(F, "keep", []) + [qs]
        sixteen += _both(F, ("adv",) + key, 10, qs, tries=1 if sixteen else 6)[1]
        _both(F, ("adv",) + key, 10, qs, tries=1, take=8 + place % 8)
    assert sixteen > 0


@pytest.mark.parametrize("k", [10, 24])
@pytest.mark.parametrize("waves", [1, 4, 8])
@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("name", ["steep", "mirror"])
def test_every_row_inserts_in_every_list_in_the_new_order(F, name, blocks, waves, k):
    """steep: every row a block reduces is its best so far and goes to the head of all sixteen lists, now offered in the order of
    the folded map's lanes and not query by query; mirror: the lists fill once.  Lists of 18 and of 32 keys."""
    _blocks(F, blocks, waves)
    try:
        expect = list(range(N_STEEP - 1, N_STEEP - 1 - k, -1)) if name == "steep" else list(range(k))

        def check(want):
            for i in range(CALLS):
                assert want[0][i, :k].tolist() == expect, i
        assert _both(F, name, k, F.qsteep, check)[1] > 0             # (all sixteen places at once)
    finally:
        _blocks(F, 0, 8)
