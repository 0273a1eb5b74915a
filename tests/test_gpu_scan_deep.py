"""scan_deep = 8 .. 15: a queued one-query scan takes up to fifteen later calls of its stream (steps i + 2 .. i + 30) along in one
corpus pass (scan_deep_kernel), and their own scans end at once.  Every series is compared byte for byte (rows, f64 distances, status
words) with its scan_deep = 0 run at the same settings, and the sixteen-entry histogram of smt_debug_scan_groups_deep must account for
every call with nothing above the limit.

Set up like tests/test_gpu_scan_wide.py: a context of its own on a fresh torch stream (given up for the next one if nothing can be
taken along on it at all), scan_pair_wait_us = 2000, so that corpora which scan faster than the host issues calls still group.  No
test lets that wait, or a list's lock, run out: a wait that ran out would come back as an error from the synchronise."""
import pytest

from tests.test_gpu_nearties import adversarial_corpus
from tests.test_gpu_scan_pairing import _same

pytestmark = pytest.mark.gpu

ROWS = (1, 5, 31, 33, 1000, 65_537)   # one ragged chunk, two chunks, eight chunks but one, eight and a ragged one, one block, several blocks
CALLS = 64                            # 32 per stream: two full groups of sixteen
ADV_SEEDS = (55, 56)
N_STEEP = 4096
DEEP = 15


class _Setup:
    pass


def _series(s, names, n, ks, take, wait_us=2000, qsel=None, queries=None, fresh_query=False, key="scan_deep", stall=0):
    """n back-to-back calls over the corpora `names` in turn, k from `ks` in turn, at `key` = `take`: (rows, dists, status) as numpy
    arrays, the launches of the sixteen-call kernel by calls served (sixteen entries), the series' (paired, alone, absorbed) and the
    eight-entry histogram of the other kernels."""
    torch, ctx, stream = s.torch, s.ctx, s.stream
    qs = s.qs if queries is None else queries
    ctx.set_tuning(key, take)
    ctx.set_tuning("scan_pair_wait_us", wait_us if take else 0)
    kmax = max(ks)
    dev = qs.device
    with torch.cuda.stream(stream):
        rows = torch.full((n, kmax), -7, dtype=torch.int64, device=dev)
        dist = torch.full((n, kmax), -7.0, dtype=torch.float64, device=dev)
        status = torch.full((n,), 7, dtype=torch.int32, device=dev)
        qbuf = torch.zeros((n, 256), dtype=torch.float32, device=dev)
        if fresh_query or stall:
            big_in = torch.ones(64 << 20, dtype=torch.float32, device=dev)
            big_out = torch.empty_like(big_in)
    stream.synchronize()
    before, before_deep, before_wide = ctx.scan_pairs(), ctx.scan_groups_deep(), ctx.scan_groups_wide()
    try:
        with torch.cuda.stream(stream):
            for _ in range(stall):                                 # the GPU is busy while the host runs ahead
                torch.mul(big_in, 1.0, out=big_out)
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
        deep = tuple(int(b - a) for a, b in zip(before_deep, ctx.scan_groups_deep()))
        wide = tuple(int(b - a) for a, b in zip(before_wide, ctx.scan_groups_wide()))
    finally:
        ctx.set_tuning(key, 0)
        ctx.set_tuning("scan_pair_wait_us", 0)
    print("%s=%d %s n=%d ks=%s: deep launches by calls served %s (paired, alone, absorbed) %s others %s"
          % (key, take, names, n, ks, deep, counts, wide))
    return (rows.cpu().numpy(), dist.cpu().numpy(), status.cpu().numpy()), deep, counts, wide


@pytest.fixture(scope="module")
def S():
    import torch
    import semtools_amd as smt

    s = _Setup()
    s.torch = torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(61)
    s.x = torch.randn(ROWS[-1] + 5_000, 256, device=dev, generator=g)
    s.x /= s.x.norm(dim=1, keepdim=True)
    s.xdup = s.x[:65_537].clone()
    s.xdup[100:200] = s.xdup[0:100]                                # exact duplicate rows: equal keys but for the row number
    s.xdup[40_000:40_100] = s.xdup[0:100]
    s.qs = torch.randn(64, 256, device=dev, generator=g)
    s.qs /= s.qs.norm(dim=1, keepdim=True)
    s.qs[0] = 0.0                                                  # a zero query
    s.qs[2] = s.xdup[7]                                            # a query that IS a duplicated row
    # a corpus whose distance to each of sixteen queries falls strictly with the row number: rows in the plane (u, w) at angles that
    # fall from 1.5 to 0.1 (cosines 3e-5 apart at the least, f32 resolves 6e-8), queries u + 0.2 z_g with z_g orthogonal to the plane;
    # and its mirror image, whose distances rise with the row number
    basis = torch.linalg.qr(torch.randn(256, 18, device=dev, generator=g, dtype=torch.float64))[0].T
    theta = torch.linspace(1.5, 0.1, N_STEEP, device=dev, dtype=torch.float64)
    s.xsteep = (torch.cos(theta)[:, None] * basis[0] + torch.sin(theta)[:, None] * basis[1]).float().contiguous()
    s.xmirror = s.xsteep.flip(0).contiguous()
    s.qsteep = (basis[0] + 0.2 * basis[2:18]).float().contiguous()
    s.adv = {seed: adversarial_corpus(seed=seed) for seed in ADV_SEEDS}   # 40 near-ties around the 10th place
    torch.cuda.synchronize()
    # (why a context that cannot take anything along is given up for one on the next stream: tests/test_gpu_scan_groups.py)
    for attempt in range(6):
        s.stream = torch.cuda.Stream(dev)
        s.ctx = smt.Context(0, stream=s.stream.cuda_stream)
        s.corpora = {n: smt.Corpus(s.ctx, device_ptr=s.x.data_ptr(), rows=n) for n in ROWS}
        s.ctx.set_tuning("async_select", 1)
        if _series(s, (1000,), 8, (10,), DEEP)[2][0] > 0 or attempt == 5:   # (the last one stays: the tests then say what is wrong)
            break
        for c in s.corpora.values():
            c.close()
        s.ctx.close()
    s.corpora["other"] = smt.Corpus(s.ctx, device_ptr=s.x[5_000:].data_ptr(), rows=65_537)   # other rows, same count
    s.corpora["dup"] = smt.Corpus(s.ctx, device_ptr=s.xdup.data_ptr(), rows=65_537)
    s.corpora["steep"] = smt.Corpus(s.ctx, device_ptr=s.xsteep.data_ptr(), rows=N_STEEP)
    s.corpora["mirror"] = smt.Corpus(s.ctx, device_ptr=s.xmirror.data_ptr(), rows=N_STEEP)
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
    """The scan_deep = 0 answers of a series, computed once and never changed."""
    if key not in s.ref:
        got, deep, counts, wide = _series(s, *args, take=0, **kw)
        assert counts == (0, 0, 0) and deep == (0,) * 16 and wide == (0,) * 8, (counts, deep, wide)
        s.ref[key] = got
    return s.ref[key]


def _accounted(deep, counts, wide, calls, take=DEEP):
    """Every call is served by a launch of the sixteen-call kernel or ran the plain kernel alone (`alone` counts both, deep[0] the
    former); no pass serves more than take + 1 calls; the other kernels' histogram sees nothing but the calls that ran alone."""
    paired, alone, absorbed = counts
    assert sum((n + 1) * v for n, v in enumerate(deep)) + (alone - deep[0]) == calls, (deep, counts, calls)
    assert alone >= deep[0] and all(v == 0 for v in deep[take + 1:]), (deep, take)
    assert paired + alone + absorbed == calls and paired <= absorbed <= 15 * paired, (counts, calls)
    assert sum(deep[1:]) == paired, (deep, counts)
    assert wide == (alone,) + (0,) * 7, (wide, counts)


@pytest.mark.parametrize("k", [1, 10, 24])
@pytest.mark.parametrize("rows", ROWS)
def test_uniform_series(S, rows, k):
    want = _want(S, ("uniform", rows, k), (rows,), CALLS, (k,))
    if rows >= 1000:
        assert (want[2][1:] == 0).all()                            # (call 0 carries the zero query)
    got, deep, counts, wide = _series(S, (rows,), CALLS, (k,), DEEP)
    _same(got, want)
    _accounted(deep, counts, wide, CALLS)
    assert counts[0] > 0, counts


@pytest.mark.parametrize("take", range(8, 16))
def test_group_sizes(S, take):
    """Whether a later call may be taken also depends on a host-side query of the caller's stream, which races with the GPU: counted
    over up to six series, every one of them checked."""
    want = _want(S, ("uniform", 65_537, 10), (65_537,), CALLS, (10,))
    full = 0
    for _ in range(6 if take == DEEP else 1):
        got, deep, counts, wide = _series(S, (65_537,), CALLS, (10,), take)
        _same(got, want)
        _accounted(deep, counts, wide, CALLS, take=take)
        assert counts[0] > 0, counts
        full += deep[take]
        if full:
            break
    print("limit", take, "launches that served", take + 1, ":", full)
    assert full > 0 or take < DEEP                                 # at the limit of fifteen: a launch that served sixteen


def _sixteen_per_group(i):
    return (i // 2) % 16                                           # steps i, i + 2, ... i + 30 carry sixteen different queries


@pytest.mark.parametrize("seed", ADV_SEEDS)
def test_near_ties_in_every_position_of_a_group(S, seed):
    """40 near-ties around the 10th place: which of them the f32 scan nominates decides the rows of an UNCERTAIN answer, so one
    rounding that differs from the one-query kernel's shows as a byte that differs.  The query goes through the sixteen places of the
    series' period in turn: whichever call leads, it sits in every row of the wave and in all four phases."""
    q_adv = S.torch.from_numpy(S.adv[seed][0]).to(S.qs.device)
    name = ("adv", seed)
    alone = _want(S, ("adv alone", seed), (name,), 8, (10,), queries=q_adv[None])
    print("seed", seed, "status words of the query alone:", sorted(set(alone[2].tolist())))
    if seed == 55:
        assert (alone[2] == 1).all()                               # SMT_STATUS_UNCERTAIN (tests/test_gpu_scan_group_loop.py)
    more = 0
    for place in range(16):
        qs = S.qs[16:32].clone()
        qs[place] = q_adv
        want = _want(S, ("adv", seed, place), (name,), CALLS, (10,), qsel=_sixteen_per_group, queries=qs)
        got, deep, counts, wide = _series(S, (name,), CALLS, (10,), DEEP, qsel=_sixteen_per_group, queries=qs)
        _same(got, want)
        _accounted(deep, counts, wide, CALLS)
        for i in range(CALLS):
            if _sixteen_per_group(i) == place:                     # ... and the query's answer is that of the query alone
                assert all(x[i].tobytes() == y[0].tobytes() for x, y in zip(got, alone)), (place, i)
        more += sum(deep[8:])
    assert more > 0                                                # (some pass went into phases 2 and 3)


def test_zero_query_in_every_position_of_a_group(S):
    more = 0
    for place in range(16):
        qs = S.qs[16:32].clone()
        qs[place] = 0.0
        want = _want(S, ("zero", place), (1000,), CALLS, (10,), qsel=_sixteen_per_group, queries=qs)
        got, deep, counts, wide = _series(S, (1000,), CALLS, (10,), DEEP, qsel=_sixteen_per_group, queries=qs)
        _same(got, want)
        _accounted(deep, counts, wide, CALLS)
        more += sum(deep[8:])
    assert more > 0


@pytest.mark.parametrize("waves", [1, 4, 8])
@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("name", ["steep", "mirror"])
def test_every_row_inserts_in_all_sixteen_lists(S, name, blocks, waves):
    """steep: distances that fall with the row number, so every row a block reduces is its best so far and goes to the head of all
    sixteen lists -- the waves of a block meet at every lock, chunk after chunk.  mirror: distances that rise, so the lists fill once
    and every later row fails at the threshold.  One and two blocks of one, four and eight waves."""
    k = 24
    S.ctx.set_tuning("scan_blocks", blocks)
    S.ctx.set_tuning("scan_threads", 64 * waves)
    try:
        want = _want(S, (name, blocks, waves), (name,), CALLS, (k,), qsel=_sixteen_per_group, queries=S.qsteep)
        expect = list(range(N_STEEP - 1, N_STEEP - 1 - k, -1)) if name == "steep" else list(range(k))
        for i in range(CALLS):
            assert want[0][i, :k].tolist() == expect, i
        more = 0
        for _ in range(6):
            got, deep, counts, wide = _series(S, (name,), CALLS, (k,), DEEP, qsel=_sixteen_per_group, queries=S.qsteep)
            _same(got, want)
            _accounted(deep, counts, wide, CALLS)
            more += deep[15]
            if more:
                break
        assert more > 0                                            # (all sixteen places at once)
    finally:
        S.ctx.set_tuning("scan_blocks", 0)
        S.ctx.set_tuning("scan_threads", 512)


def test_exact_duplicate_rows(S):
    def qsel(i):
        return (i // 3) % 16                                       # the zero query three times, then the next one three times ...
    want = _want(S, ("dup",), ("dup",), CALLS, (10,), qsel=qsel)
    assert want[0][6, :3].tolist() == [7, 107, 40_007]             # the three copies (ties at the threshold but for the row), in row order
    got, deep, counts, wide = _series(S, ("dup",), CALLS, (10,), DEEP, qsel=qsel)
    _same(got, want)
    _accounted(deep, counts, wide, CALLS)
    assert counts[0] > 0, counts


def test_two_corpora_in_turn(S):
    names = (65_537, "other")                                      # steps i + 2, i + 4, ... are in front of the same corpus
    want = _want(S, ("two",), names, CALLS, (10,))
    got, deep, counts, wide = _series(S, names, CALLS, (10,), DEEP)
    _same(got, want)
    _accounted(deep, counts, wide, CALLS)
    assert counts[0] > 0, counts


def test_three_corpora_in_turn_never_group(S):
    names = (65_537, "other", "dup")                               # step i + 2 is in front of another corpus (by address)
    want = _want(S, ("three",), names, CALLS, (10,))
    got, deep, counts, wide = _series(S, names, CALLS, (10,), DEEP)
    _same(got, want)
    _accounted(deep, counts, wide, CALLS)
    assert counts == (0, CALLS, 0), counts


def test_a_group_ends_where_the_corpus_changes(S):
    names = (65_537,) * 12 + ("other",) * 12                       # equal row counts, other rows: runs of six calls on each stream
    want = _want(S, ("runs",), names, CALLS, (10,))
    got, deep, counts, wide = _series(S, names, CALLS, (10,), DEEP)
    _same(got, want)
    _accounted(deep, counts, wide, CALLS, take=5)
    assert counts[0] > 0, counts


def test_a_group_ends_where_k_changes(S):
    ks = (10,) * 10 + (24,) * 10                                   # lists of 18 and of 32 candidates: runs of five calls on each stream
    want = _want(S, ("ks",), (65_537,), CALLS, ks)
    got, deep, counts, wide = _series(S, (65_537,), CALLS, ks, DEEP)
    _same(got, want)
    _accounted(deep, counts, wide, CALLS, take=4)
    assert counts[0] > 0, counts


def test_cut_descriptor_ring_with_the_host_far_ahead(S):
    """200 calls with no wait and no synchronise before the end, behind 4 ms of other work on the context's stream, the descriptor ring
    cut to 64 slots: the host is more than 64 calls ahead when the first scans start, and a descriptor rewritten before the scan that
    would read it starts fails the step check, which only ends that group early."""
    want = _want(S, ("ring",), (65_537,), 200, (10,), wait_us=0)
    S.ctx.set_tuning("scan_pair_ring", 64)
    try:
        got, deep, counts, wide = _series(S, (65_537,), 200, (10,), DEEP, wait_us=0, stall=40)
    finally:
        S.ctx.set_tuning("scan_pair_ring", 4096)
    _same(got, want)
    _accounted(deep, counts, wide, 200)


def test_query_written_on_the_stream_right_before_the_call(S):
    want = _want(S, ("uniform", 65_537, 10), (65_537,), CALLS, (10,))
    got, deep, counts, wide = _series(S, (65_537,), CALLS, (10,), DEEP, fresh_query=True)
    _same(got, want)
    _accounted(deep, counts, wide, CALLS)
    assert counts == (0, CALLS, 0), counts


def test_scan_take_runs_the_eight_call_kernel_as_before(S):
    want = _want(S, ("uniform", 65_537, 10), (65_537,), CALLS, (10,))
    got, deep, counts, wide = _series(S, (65_537,), CALLS, (10,), 7, key="scan_take")
    _same(got, want)
    assert deep == (0,) * 16, deep
    paired, alone, absorbed = counts
    assert sum((n + 1) * v for n, v in enumerate(wide)) == CALLS, wide
    assert wide[0] == alone and sum(wide[1:]) == paired and paired <= absorbed <= 7 * paired and paired > 0, (wide, counts)
