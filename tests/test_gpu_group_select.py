"""select_group = 1: a launch of the sixteen-call scan is followed by ONE select launch (group_select_kernel) that serves every call of
its pass -- block 0 the launch's own, block g the g-th call taken along, from the parameters the deciding wave copied into the record.
Every series is compared byte for byte with its select_group = 0 run at the same inputs and settings: rows, f64 distances, status
words, the guard words around every output list, and smt_ctx_uncertain_count.  The histogram of smt_debug_select_groups must agree
with the scan's own counters: one select launch that served n calls per scan launch that served n, one that served none per absorbed
scan.

Set up like tests/test_gpu_scan_deep.py: a context of its own on a fresh torch stream (given up for the next one if nothing can be
taken along on it at all), scan_pair_wait_us = 2000 so that corpora which scan faster than the host issues calls still group.  No test
lets that wait, or a list's lock, run out."""
import pytest

from tests.test_gpu_nearties import adversarial_corpus
from tests.test_gpu_scan_pairing import _same

pytestmark = pytest.mark.gpu

ROWS = (1, 5, 33, 1000, 65_537)
CALLS = 64                             # 32 per stream: two full groups of sixteen
DEEP = 15
GUARD = 2                              # words in front of and behind every output list that no launch may touch
ADV_SEED = 55                          # its query's answer is UNCERTAIN: the sticky counter moves


class _Setup:
    pass


def _series(s, names, n, ks, group, take=DEEP, key="scan_deep", wait_us=2000, qsel=None, queries=None, lead=0, ring=4096):
    """n back-to-back calls over the corpora `names` in turn, k from `ks` in turn, at select_group = `group`.  Call i has its own
    row_base (1000 i + 3), its own output lists with GUARD words around them, and goes through the plain entry (no status pointer)
    when i % 3 == 1.  Returns (rows, dists, status, uncertain count) with the guards in place, the select launches by calls served
    (seventeen entries), the scan launches of the sixteen-call kernel by calls served, (paired, alone, absorbed) and the other
    kernels' histogram.  lead: that many calls over the 8 M-row corpus come first (answers into buffers of their own): the internal
    streams are busy for milliseconds while the caller's stream stays empty, so the host runs far ahead of calls that can be taken."""
    torch, ctx, stream = s.torch, s.ctx, s.stream
    qs = s.qs if queries is None else queries
    ctx.set_tuning("select_group", group)
    ctx.set_tuning(key, take)
    ctx.set_tuning("scan_pair_wait_us", wait_us if take else 0)
    ctx.set_tuning("scan_pair_ring", ring)
    kmax = max(ks)
    dev = qs.device
    with torch.cuda.stream(stream):
        rows = torch.full((n, kmax + 2 * GUARD), -7, dtype=torch.int64, device=dev)
        dist = torch.full((n, kmax + 2 * GUARD), -7.0, dtype=torch.float64, device=dev)
        status = torch.full((n,), 7, dtype=torch.int32, device=dev)
        lead_rows = torch.full((max(lead, 1), kmax), -7, dtype=torch.int64, device=dev)
        lead_dist = torch.full((max(lead, 1), kmax), -7.0, dtype=torch.float64, device=dev)
        lead_status = torch.full((max(lead, 1),), 7, dtype=torch.int32, device=dev)
    stream.synchronize()
    ctx.uncertain_count(reset=True)
    before = ctx.select_groups(), ctx.scan_groups_deep(), ctx.scan_pairs(), ctx.scan_groups_wide()
    try:
        for i in range(lead):
            s.corpora["big"].search_topk_device(qs[i % len(qs)].data_ptr(), 1, kmax, 0, lead_rows[i].data_ptr(), lead_dist[i].data_ptr(),
                                                out_status_ptr=lead_status[i:].data_ptr())
        for i in range(n):
            q = qs[qsel(i) if qsel else i % len(qs)]
            s.corpora[names[i % len(names)]].search_topk_device(
                q.data_ptr(), 1, ks[i % len(ks)], 1000 * i + 3, rows[i, GUARD:].data_ptr(), dist[i, GUARD:].data_ptr(),
                out_status_ptr=None if i % 3 == 1 else status[i:].data_ptr())
        ctx.synchronize()
        after = ctx.select_groups(), ctx.scan_groups_deep(), ctx.scan_pairs(), ctx.scan_groups_wide()
        sel, deep, counts, wide = (tuple(int(b - a) for a, b in zip(x, y)) for x, y in zip(before, after))
        uncertain = ctx.uncertain_count(reset=True)
    finally:
        ctx.set_tuning(key, 0)
        ctx.set_tuning("scan_pair_wait_us", 0)
        ctx.set_tuning("scan_pair_ring", 4096)
        ctx.set_tuning("select_group", 1)
    print("select_group=%d %s=%d %s n=%d ks=%s: select launches by calls served %s scans %s (paired, alone, absorbed) %s uncertain %d"
          % (group, key, take, names, n, ks, sel, deep, counts, uncertain))
    rows, dist, status = rows.cpu().numpy(), dist.cpu().numpy(), status.cpu().numpy()
    for i in range(n):                                             # what must not be touched
        k = ks[i % len(ks)]
        assert (rows[i, :GUARD] == -7).all() and (rows[i, GUARD + k:] == -7).all(), i
        assert (dist[i, :GUARD] == -7.0).all() and (dist[i, GUARD + k:] == -7.0).all(), i
        assert (rows[i, GUARD:GUARD + k] != -7).all(), i           # ... and every call has its answer
        assert (status[i] == 7) == (i % 3 == 1), (i, status[i])
    return (rows, dist, status, uncertain), sel, deep, counts, wide


@pytest.fixture(scope="module")
def S():
    import torch
    import semtools_amd as smt

    s = _Setup()
    s.torch = torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(67)
    s.x = torch.randn(ROWS[-1] + 5_000, 256, device=dev, generator=g)
    s.x /= s.x.norm(dim=1, keepdim=True)
    s.qs = torch.randn(64, 256, device=dev, generator=g)
    s.qs /= s.qs.norm(dim=1, keepdim=True)
    s.qs[0] = 0.0                                                  # a zero query
    s.adv = adversarial_corpus(seed=ADV_SEED)                      # 40 near-ties around the 10th place
    torch.cuda.synchronize()
    # (why a context that cannot take anything along is given up for one on the next stream: tests/test_gpu_scan_groups.py)
    for attempt in range(6):
        s.stream = torch.cuda.Stream(dev)
        s.ctx = smt.Context(0, stream=s.stream.cuda_stream)
        s.corpora = {n: smt.Corpus(s.ctx, device_ptr=s.x.data_ptr(), rows=n) for n in ROWS}
        s.ctx.set_tuning("async_select", 1)
        if _series(s, (1000,), 8, (10,), 1)[3][0] > 0 or attempt == 5:   # (the last one stays: the tests then say what is wrong)
            break
        for c in s.corpora.values():
            c.close()
        s.ctx.close()
    s.corpora["other"] = smt.Corpus(s.ctx, device_ptr=s.x[5_000:].data_ptr(), rows=65_537)   # other rows, same count
    c = smt.Corpus(s.ctx)
    c.append(s.adv[1])
    s.corpora["adv"] = c
    s.xbig = s.x[:65_536].repeat(128, 1)                           # 8 Mi rows, 8 GiB: a pass takes milliseconds
    s.corpora["big"] = smt.Corpus(s.ctx, device_ptr=s.xbig.data_ptr(), rows=s.xbig.shape[0])
    s.ctx.set_tuning("async_select", 1)
    s.ref = {}
    yield s
    for c in s.corpora.values():
        c.close()
    s.ctx.close()


def _want(s, name, *args, **kw):
    """The select_group = 0 answers of a series, computed once and never changed."""
    if name not in s.ref:
        got, sel, deep, counts, wide = _series(s, *args, group=0, **kw)
        assert sel == (0,) * 17, sel                               # no launch of the group select
        s.ref[name] = got
    return s.ref[name]


def _equal(got, want):
    _same(got, want)
    assert got[3] == want[3], (got[3], want[3])                    # smt_ctx_uncertain_count


def _accounted(sel, deep, counts, calls, most=16):
    """One select launch that served n calls behind every scan launch that served n, one that served none behind every absorbed scan;
    the calls that ran the plain kernel alone kept their own select."""
    paired, alone, absorbed = counts
    assert sel[1:] == deep, (sel, deep)
    assert sel[0] == absorbed, (sel, counts)
    assert sum(n * v for n, v in enumerate(sel)) + (alone - deep[0]) == calls, (sel, counts, calls)
    assert all(v == 0 for v in sel[most + 1:]), (sel, most)


@pytest.mark.parametrize("k", [1, 10, 24])
@pytest.mark.parametrize("rows", ROWS)
def test_uniform_series(S, rows, k):
    want = _want(S, ("uniform", rows, k), (rows,), CALLS, (k,))
    got, sel, deep, counts, wide = _series(S, (rows,), CALLS, (k,), 1)
    _equal(got, want)
    _accounted(sel, deep, counts, CALLS)
    assert counts[0] > 0, counts


def test_a_select_launch_serves_more_than_one_call(S):
    """The route: whether a later call may be taken depends on a host-side query of the caller's stream, which races with the GPU, so
    up to six series are counted, every one of them checked."""
    want = _want(S, ("uniform", 65_537, 10), (65_537,), CALLS, (10,))
    many = full = 0
    for _ in range(6):
        got, sel, deep, counts, wide = _series(S, (65_537,), CALLS, (10,), 1)
        _equal(got, want)
        _accounted(sel, deep, counts, CALLS)
        many += sum(sel[2:])
        full += sel[16]
        if full:
            break
    assert many > 0 and full > 0, (many, full)                     # ... and one that served sixteen


@pytest.mark.parametrize("size", range(1, 17))
def test_groups_of_every_size(S, size):
    """Runs of 2 x size calls over one corpus, then as many over other rows of the same count: every stream sees runs of `size` calls,
    and a group ends where the corpus changes, so no select launch serves more than `size` calls."""
    names = (65_537,) * (2 * size) + ("other",) * (2 * size)
    n = max(CALLS, 4 * size)
    want = _want(S, ("runs", size), names, n, (10,))
    got, sel, deep, counts, wide = _series(S, names, n, (10,), 1)
    _equal(got, want)
    _accounted(sel, deep, counts, n, most=size)
    if size == 1:
        assert counts == (0, n, 0) and sum(sel[2:]) == 0, (counts, sel)


def test_limits_below_sixteen(S):
    for take in range(8, 15):
        want = _want(S, ("limit", take), (65_537,), CALLS, (10,), take=take)
        got, sel, deep, counts, wide = _series(S, (65_537,), CALLS, (10,), 1, take=take)
        _equal(got, want)
        _accounted(sel, deep, counts, CALLS, most=take + 1)


def _sixteen_per_group(i):
    return (i // 2) % 16                                           # steps i, i + 2, ... i + 30 carry sixteen different queries


def test_near_ties_in_every_position_of_a_group(S):
    """40 near-ties around the 10th place: an UNCERTAIN answer's rows, its status word and the sticky counter all come from the
    member's select, wherever in the group it runs."""
    q_adv = S.torch.from_numpy(S.adv[0]).to(S.qs.device)
    more = 0
    for place in range(16):
        qs = S.qs[16:32].clone()
        qs[place] = q_adv
        want = _want(S, ("adv", place), ("adv",), CALLS, (10,), qsel=_sixteen_per_group, queries=qs)
        assert want[3] >= CALLS // 16, want[3]                     # the adversarial query's four calls at the least
        got, sel, deep, counts, wide = _series(S, ("adv",), CALLS, (10,), 1, qsel=_sixteen_per_group, queries=qs)
        _equal(got, want)
        _accounted(sel, deep, counts, CALLS)
        more += sum(sel[2:])
    assert more > 0


def test_zero_query_in_every_position_of_a_group(S):
    more = 0
    for place in range(16):
        qs = S.qs[16:32].clone()
        qs[place] = 0.0
        want = _want(S, ("zero", place), (1000,), CALLS, (10,), qsel=_sixteen_per_group, queries=qs)
        got, sel, deep, counts, wide = _series(S, (1000,), CALLS, (10,), 1, qsel=_sixteen_per_group, queries=qs)
        _equal(got, want)
        _accounted(sel, deep, counts, CALLS)
        more += sum(sel[2:])
    assert more > 0


def test_a_group_ends_where_k_changes(S):
    ks = (10,) * 10 + (24,) * 10                                   # lists of 18 and of 32 candidates: runs of five calls on each stream
    want = _want(S, ("ks",), (65_537,), CALLS, ks)
    got, sel, deep, counts, wide = _series(S, (65_537,), CALLS, ks, 1)
    _equal(got, want)
    _accounted(sel, deep, counts, CALLS, most=5)


def test_cut_descriptor_ring_with_the_host_far_ahead(S):
    """200 calls with no wait and no synchronise before the end, behind eight calls over an 8 M-row corpus, both descriptor rings cut
    to 64 slots: the host is more than 64 calls ahead when the first of the 200 scans starts and has rewritten slots that a leader
    would read.  A rewritten slot fails the step check and ends the group; the select parameters of a call that was taken were copied
    at the decision and are never read from a slot afterwards.  Every answer equals the reference run with the full ring."""
    want = _want(S, ("ring",), (65_537,), 200, (10,), wait_us=0, lead=8)
    got, sel, deep, counts, wide = _series(S, (65_537,), 200, (10,), 1, wait_us=0, lead=8, ring=64)
    _equal(got, want)
    _accounted(sel, deep, counts, 208)


@pytest.mark.parametrize("key,take", [("scan_take", 7), ("scan_pair", 3)])
def test_the_older_kernels_keep_their_own_selects(S, key, take):
    want = _want(S, ("older", key), (65_537,), CALLS, (10,), take=take, key=key)
    got, sel, deep, counts, wide = _series(S, (65_537,), CALLS, (10,), 1, take=take, key=key)
    _equal(got, want)
    assert sel == (0,) * 17 and deep == (0,) * 16, (sel, deep)
    assert counts[0] > 0, counts
