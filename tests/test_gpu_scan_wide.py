"""scan_take = 4 .. 7: a queued one-query scan takes up to seven later calls of its stream (steps i + 2 .. i + 14) along in one corpus
pass (scan_wide_kernel), and their own scans end at once.  Every series is compared byte for byte (rows, f64 distances, status words)
with its scan_take = 0 run, and the eight-entry histogram of smt_debug_scan_groups_wide must account for every call with nothing
above the limit.

Set up like tests/test_gpu_scan_groups.py: a context of its own on a fresh torch stream (given up for the next one if nothing can be
taken along on it at all), scan_pair_wait_us = 2000, so that corpora which scan faster than the host issues calls still group."""
import pytest

from tests.test_gpu_nearties import adversarial_corpus
from tests.test_gpu_scan_pairing import _same

pytestmark = pytest.mark.gpu

ROWS = (1, 5, 1000, 65_537, 300_001)   # one ragged chunk, two chunks, one block, several blocks, every CU busy for many rounds
CALLS = 48
ADV_SEEDS = (55, 56)
N_STEEP = 4096


class _Setup:
    pass


def _series(s, names, n, ks, take, wait_us=2000, qsel=None, queries=None, fresh_query=False):
    """n back-to-back calls over the corpora `names` in turn, k from `ks` in turn, at scan_take = `take`: (rows, dists, status) as
    numpy arrays, the launches of the series by calls served (eight entries) and its (paired, alone, absorbed)."""
    torch, ctx, stream = s.torch, s.ctx, s.stream
    qs = s.qs if queries is None else queries
    ctx.set_tuning("scan_take", take)
    ctx.set_tuning("scan_pair_wait_us", wait_us if take else 0)
    kmax = max(ks)
    dev = qs.device
    with torch.cuda.stream(stream):
        rows = torch.full((n, kmax), -7, dtype=torch.int64, device=dev)
        dist = torch.full((n, kmax), -7.0, dtype=torch.float64, device=dev)
        status = torch.full((n,), 7, dtype=torch.int32, device=dev)
        qbuf = torch.zeros((n, 256), dtype=torch.float32, device=dev)
        if fresh_query:
            big_in = torch.ones(64 << 20, dtype=torch.float32, device=dev)
            big_out = torch.empty_like(big_in)
    stream.synchronize()
    before, before_sizes = ctx.scan_pairs(), ctx.scan_groups_wide()
    try:
        for i in range(n):
            q = qs[qsel(i) if qsel else i % len(qs)]
            if fresh_query:
                # written by a torch op on the context's stream right before the call: such a call must not be taken along
                with torch.cuda.stream(stream):
                    torch.mul(big_in, 1.0, out=big_out)
                    torch.mul(q, 1.0, out=qbuf[i])
                q = qbuf[i]
            s.corpora[names[i % len(names)]].search_topk_device(q.data_ptr(), 1, ks[i % len(ks)], 0, rows[i].data_ptr(),
                                                                dist[i].data_ptr(), out_status_ptr=status[i:].data_ptr())
        ctx.synchronize()
        counts = tuple(int(b - a) for a, b in zip(before, ctx.scan_pairs()))
        by_size = tuple(int(b - a) for a, b in zip(before_sizes, ctx.scan_groups_wide()))
    finally:
        ctx.set_tuning("scan_take", 0)
        ctx.set_tuning("scan_pair_wait_us", 0)
    print("scan_take=%d %s n=%d ks=%s: by calls served %s (paired, alone, absorbed) %s" % (take, names, n, ks, by_size, counts))
    return (rows.cpu().numpy(), dist.cpu().numpy(), status.cpu().numpy()), by_size, counts


@pytest.fixture(scope="module")
def S():
    import torch
    import semtools_amd as smt

    s = _Setup()
    s.torch = torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(59)
    s.x = torch.randn(ROWS[-1], 256, device=dev, generator=g)
    s.x /= s.x.norm(dim=1, keepdim=True)
    s.xdup = s.x[:65_537].clone()
    s.xdup[100:200] = s.xdup[0:100]                                # exact duplicate rows: equal keys but for the row number
    s.xdup[40_000:40_100] = s.xdup[0:100]
    s.qs = torch.randn(64, 256, device=dev, generator=g)
    s.qs /= s.qs.norm(dim=1, keepdim=True)
    s.qs[0] = 0.0                                                  # a zero query
    s.qs[2] = s.xdup[7]                                            # a query that IS a duplicated row
    # a corpus whose distance to each of eight queries falls strictly with the row number: rows in the plane (u, w) at angles that
    # fall from 1.5 to 0.1 (cosines 3e-5 apart at the least, f32 resolves 6e-8), queries u + 0.2 z_g with z_g orthogonal to the plane
    basis = torch.linalg.qr(torch.randn(256, 10, device=dev, generator=g, dtype=torch.float64))[0].T
    theta = torch.linspace(1.5, 0.1, N_STEEP, device=dev, dtype=torch.float64)
    s.xsteep = (torch.cos(theta)[:, None] * basis[0] + torch.sin(theta)[:, None] * basis[1]).float().contiguous()
    s.qsteep = (basis[0] + 0.2 * basis[2:10]).float().contiguous()
    s.adv = {seed: adversarial_corpus(seed=seed) for seed in ADV_SEEDS}   # 40 near-ties around the 10th place
    torch.cuda.synchronize()
    # (why a context that cannot take anything along is given up for one on the next stream: tests/test_gpu_scan_groups.py)
    for attempt in range(6):
        s.stream = torch.cuda.Stream(dev)
        s.ctx = smt.Context(0, stream=s.stream.cuda_stream)
        s.corpora = {n: smt.Corpus(s.ctx, device_ptr=s.x.data_ptr(), rows=n) for n in ROWS}
        s.ctx.set_tuning("async_select", 1)
        if _series(s, (1000,), 8, (10,), 1)[2][0] > 0 or attempt == 5:   # (the last one stays: the tests then say what is wrong)
            break
        for c in s.corpora.values():
            c.close()
        s.ctx.close()
    s.corpora["other"] = smt.Corpus(s.ctx, device_ptr=s.x[5_000:].data_ptr(), rows=65_537)   # other rows, same count
    s.corpora["dup"] = smt.Corpus(s.ctx, device_ptr=s.xdup.data_ptr(), rows=65_537)
    s.corpora["steep"] = smt.Corpus(s.ctx, device_ptr=s.xsteep.data_ptr(), rows=N_STEEP)
    for seed in ADV_SEEDS:
        c = smt.Corpus(s.ctx)
        c.append(s.adv[seed][1])
        s.corpora[("adv", seed)] = c
    s.ctx.set_tuning("async_select", 1)
    s.ref = {}
    yield s
    for c in s.corpora.values():
        c.close()
    s.ctx.close()


def _want(s, key, *args, **kw):
    """The scan_take = 0 answers of a series, computed once and never changed."""
    if key not in s.ref:
        got, by_size, counts = _series(s, *args, take=0, **kw)
        assert counts == (0, 0, 0) and by_size == (0,) * 8, (counts, by_size)
        s.ref[key] = got
    return s.ref[key]


def _accounted(by_size, counts, calls, take=7):
    paired, alone, absorbed = counts
    assert sum((n + 1) * v for n, v in enumerate(by_size)) == calls, (by_size, calls)
    assert all(v == 0 for v in by_size[take + 1:]), (by_size, take)
    assert paired + alone + absorbed == calls and paired <= absorbed <= 7 * paired, (counts, calls)
    assert by_size[0] == alone and sum(by_size[1:]) == paired, (by_size, counts)


@pytest.mark.parametrize("k", [1, 10, 24])
@pytest.mark.parametrize("rows", ROWS)
def test_uniform_series(S, rows, k):
    want = _want(S, ("uniform", rows, k), (rows,), CALLS, (k,))
    if rows >= 1000:
        assert (want[2][1:] == 0).all()                            # (call 0 carries the zero query)
    got, by_size, counts = _series(S, (rows,), CALLS, (k,), 7)
    _same(got, want)
    _accounted(by_size, counts, CALLS)
    assert counts[0] > 0, counts


def test_list_width_boundary(S):
    """k = 24 keeps 32 candidates per list, the widest the half-wave lists hold; k = 25 keeps 33 and runs the four-call kernel."""
    more = 0
    for _ in range(6):
        for k in (24, 25):
            want = _want(S, ("uniform", 65_537, k), (65_537,), CALLS, (k,))
            got, by_size, counts = _series(S, (65_537,), CALLS, (k,), 7)
            _same(got, want)
            _accounted(by_size, counts, CALLS, take=7 if k == 24 else 3)
            assert counts[0] > 0, counts
            if k == 24:
                more += sum(by_size[4:])
        if more:
            break
    assert more > 0


@pytest.mark.parametrize("take", [4, 5, 6, 7])
def test_group_sizes(S, take):
    """Whether a later call may be taken also depends on a host-side query of the caller's stream, which races with the GPU: counted
    over up to six series, every one of them checked."""
    want = _want(S, ("uniform", 65_537, 10), (65_537,), CALLS, (10,))
    full = 0
    for _ in range(6):
        got, by_size, counts = _series(S, (65_537,), CALLS, (10,), take)
        _same(got, want)
        _accounted(by_size, counts, CALLS, take=take)
        full += by_size[take]
        if full:
            break
    assert full > 0


def _eight_per_group(i):
    return (i // 2) % 8                                            # steps i, i + 2, ... i + 14 carry eight different queries


@pytest.mark.parametrize("seed", ADV_SEEDS)
def test_near_ties_in_every_position_of_a_group(S, seed):
    """40 near-ties around the 10th place: which of them the f32 scan nominates decides the rows of an UNCERTAIN answer, so one
    rounding that differs from the one-query kernel's shows as a byte that differs.  The query goes through the eight places of the
    series' period in turn: whichever call leads, it sits in every row of the wave and in both phases."""
    q_adv = S.torch.from_numpy(S.adv[seed][0]).to(S.qs.device)
    name = ("adv", seed)
    alone = _want(S, ("adv alone", seed), (name,), 8, (10,), queries=q_adv[None])
    print("seed", seed, "status words of the query alone:", sorted(set(alone[2].tolist())))
    if seed == 55:
        assert (alone[2] == 1).all()                               # SMT_STATUS_UNCERTAIN (tests/test_gpu_scan_group_loop.py)
    more = 0
    for place in range(8):
        qs = S.qs[8:16].clone()
        qs[place] = q_adv
        want = _want(S, ("adv", seed, place), (name,), CALLS, (10,), qsel=_eight_per_group, queries=qs)
        got, by_size, counts = _series(S, (name,), CALLS, (10,), 7, qsel=_eight_per_group, queries=qs)
        _same(got, want)
        _accounted(by_size, counts, CALLS)
        for i in range(CALLS):
            if _eight_per_group(i) == place:                       # ... and the query's answer is that of the query alone
                assert all(x[i].tobytes() == y[0].tobytes() for x, y in zip(got, alone)), (place, i)
        more += sum(by_size[4:])
    assert more > 0


@pytest.mark.parametrize("k", [24, 1])
def test_every_row_inserts_in_all_eight_lists(S, k):
    """Distances that fall with the row number: every row a wave reduces is its best so far and goes to the head of its list, so
    every insert shifts across lanes 31 | 32 of the register pair and moves the threshold at lane kp - 1 of its half."""
    queries = S.qsteep
    want = _want(S, ("steep", k), ("steep",), CALLS, (k,), qsel=_eight_per_group, queries=queries)
    expect = list(range(N_STEEP - 1, N_STEEP - 1 - k, -1))
    for i in range(CALLS):
        assert want[0][i, :k].tolist() == expect, i
    more = 0
    for _ in range(6):
        got, by_size, counts = _series(S, ("steep",), CALLS, (k,), 7, qsel=_eight_per_group, queries=queries)
        _same(got, want)
        _accounted(by_size, counts, CALLS)
        more += by_size[7]
        if more:
            break
    assert more > 0                                                # (all eight places at once)


def test_zero_query_and_exact_duplicate_rows(S):
    def qsel(i):
        return (i // 3) % 8                                        # the zero query three times, then the duplicated row's three times ...
    want = _want(S, ("dup",), ("dup",), CALLS, (10,), qsel=qsel)
    assert want[0][6, :3].tolist() == [7, 107, 40_007]             # the three copies, in row order
    got, by_size, counts = _series(S, ("dup",), CALLS, (10,), 7, qsel=qsel)
    _same(got, want)
    _accounted(by_size, counts, CALLS)
    assert counts[0] > 0, counts


def test_two_corpora_in_turn(S):
    names = (65_537, "other")                                      # steps i + 2, i + 4, ... are in front of the same corpus
    want = _want(S, ("two",), names, CALLS, (10,))
    got, by_size, counts = _series(S, names, CALLS, (10,), 7)
    _same(got, want)
    _accounted(by_size, counts, CALLS)
    assert counts[0] > 0, counts


def test_three_corpora_in_turn_never_group(S):
    names = (65_537, "other", "dup")                               # step i + 2 is in front of another corpus (by address)
    want = _want(S, ("three",), names, CALLS, (10,))
    got, by_size, counts = _series(S, names, CALLS, (10,), 7)
    _same(got, want)
    _accounted(by_size, counts, CALLS)
    assert by_size == (CALLS,) + (0,) * 7, by_size


def test_a_group_ends_where_the_corpus_changes(S):
    names = (65_537,) * 8 + ("other",) * 8                         # equal row counts, other rows: runs of four calls on each stream
    want = _want(S, ("runs",), names, CALLS, (10,))
    got, by_size, counts = _series(S, names, CALLS, (10,), 7)
    _same(got, want)
    _accounted(by_size, counts, CALLS, take=3)
    assert counts[0] > 0, counts


def test_cut_descriptor_ring(S):
    """200 calls with no wait and no synchronise before the end, the descriptor ring cut to 64 slots: a descriptor rewritten before
    the scan that would read it starts fails the step check, which only ends that group early.  (A wait that ran out would come
    back as an error from the synchronise.)"""
    want = _want(S, ("ring",), (300_001,), 200, (10,), wait_us=0)
    S.ctx.set_tuning("scan_pair_ring", 64)
    try:
        got, by_size, counts = _series(S, (300_001,), 200, (10,), 7, wait_us=0)
    finally:
        S.ctx.set_tuning("scan_pair_ring", 4096)
    _same(got, want)
    _accounted(by_size, counts, 200)


def test_query_written_on_the_stream_right_before_the_call(S):
    want = _want(S, ("uniform", 65_537, 10), (65_537,), CALLS, (10,))
    got, by_size, counts = _series(S, (65_537,), CALLS, (10,), 7, fresh_query=True)
    _same(got, want)
    _accounted(by_size, counts, CALLS)
    assert by_size == (CALLS,) + (0,) * 7, by_size


def test_decoy_rows_on_both_sides_of_a_grouped_series(S):
    """Layout A of tests/decoys.py, as tests/test_gpu_scan_groups_decoys.py runs it: an adopted corpus with rows that would rank first
    for every query in the 64 rows before and behind it.  Every returned id must be allowed, every proved answer the oracle's."""
    from tests import decoys as D
    from tests.test_gpu_decoys import Adopted, _check_series
    from tests.test_gpu_decoys import _series as decoy_series

    torch, ctx, stream = S.torch, S.ctx, S.stream
    n, k, calls = 4097, 10, 32
    qs = D.queries()
    a = Adopted(ctx, n, "finite")
    try:
        qd = torch.from_numpy(qs[:5]).to("cuda:0")
        torch.cuda.synchronize()
        want = a.ref.topk(qs[:5], k)
        more = 0
        try:
            ctx.set_tuning("scan_take", 7)
            ctx.set_tuning("scan_pair_wait_us", 2000)
            ctl_st = decoy_series(torch, ctx, stream, a.ctl, qd, calls, k)[2]
            for s in range(6):
                before = ctx.scan_groups_wide()
                rows, dist, st, counts = decoy_series(torch, ctx, stream, a.c, qd, calls, k)
                by_size = tuple(int(y - x) for x, y in zip(before, ctx.scan_groups_wide()))
                _accounted(by_size, counts, calls)
                _check_series(lambda i: (a.ref, want), rows, dist, st, ctl_st, k, ("A-wide", n, s))
                more += sum(by_size[4:])
                if more:
                    break
        finally:
            ctx.set_tuning("scan_take", 0)
            ctx.set_tuning("scan_pair_wait_us", 0)
        assert more > 0                                            # (some pass served more than four calls)
    finally:
        a.close()
