"""scan_pair = 2 / 3: a queued one-query scan takes up to three later calls of its stream (steps i + 2, i + 4, i + 6) along in one
corpus pass, and their own scans end at once.  Every series is compared byte for byte (rows, f64 distances, status words) with its
scan_pair = 0 run, and the device counters must account for every call, by launch (smt_debug_scan_pairs) and by the number of calls
a launch served (smt_debug_scan_groups).

Set up like tests/test_gpu_scan_pairing.py (whose series runner this file uses): a context of its own on a torch stream, and
scan_pair_wait_us = 2000, so that corpora which scan faster than the host issues calls still group."""
import pytest

from tests.test_gpu_scan_pairing import _same, _series

pytestmark = pytest.mark.gpu

ROWS = (1, 5, 1000, 65_537, 300_001)   # one ragged chunk, two chunks, one block, several blocks, every CU busy for many rounds
CALLS = 24


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
    g.manual_seed(53)
    s.x = torch.randn(ROWS[-1], 256, device=dev, generator=g)
    s.x /= s.x.norm(dim=1, keepdim=True)
    s.xdup = s.x[:65_537].clone()
    s.xdup[100:200] = s.xdup[0:100]                                # exact duplicate rows: equal keys but for the row number
    s.xdup[40_000:40_100] = s.xdup[0:100]
    s.qs = torch.randn(64, 256, device=dev, generator=g)
    s.qs /= s.qs.norm(dim=1, keepdim=True)
    s.qs[0] = 0.0                                                  # a zero query
    s.qs[2] = s.xdup[7]                                            # a query that IS a duplicated row
    s.q_adv = None
    torch.cuda.synchronize()
    # Whether a later call can be taken also hangs on the hardware queue the caller's stream shares with the library's internal
    # streams: behind one of them its event markers wait for the very scan that is waiting for the later call, the stream never
    # reads as empty and NOTHING is ever taken, pairs included.  Which queue a torch stream gets depends on how many the process made
    # before, so a context that cannot pair at all is given up for one on the next stream.
    for attempt in range(6):
        s.stream = torch.cuda.Stream(dev)
        s.ctx = smt.Context(0, stream=s.stream.cuda_stream)
        s.corpora = {n: smt.Corpus(s.ctx, device_ptr=s.x.data_ptr(), rows=n) for n in ROWS}
        s.ctx.set_tuning("async_select", 1)
        if _series(s, (1000,), 8, (10,), 1)[1][0] > 0 or attempt == 5:   # (the last one stays: the tests then say what is wrong)
            break
        for c in s.corpora.values():
            c.close()
        s.ctx.close()
    s.corpora["other"] = smt.Corpus(s.ctx, device_ptr=s.x[5_000:].data_ptr(), rows=65_537)   # other rows, same count
    s.corpora["dup"] = smt.Corpus(s.ctx, device_ptr=s.xdup.data_ptr(), rows=65_537)
    s.ctx.set_tuning("async_select", 1)
    s.ref = {}
    yield s
    for c in s.corpora.values():
        c.close()
    s.ctx.close()


def _grouped(s, *args, pair=3, **kw):
    """A series at scan_pair = `pair`: (answers, (paired, alone, absorbed), by_size)."""
    before = s.ctx.scan_groups()
    got, counts = _series(s, *args, pair=pair, **kw)
    by_size = tuple(int(b - a) for a, b in zip(before, s.ctx.scan_groups()))
    print("  by_size", by_size)
    return got, counts, by_size


def _want(s, key, *args, **kw):
    """The scan_pair = 0 answers of a series, computed once and never changed."""
    if key not in s.ref:
        got, counts = _series(s, *args, pair=0, **kw)
        assert counts == (0, 0, 0), counts
        s.ref[key] = got
    return s.ref[key]


def _accounted(counts, by_size, calls):
    paired, alone, absorbed = counts
    assert paired + alone + absorbed == calls, (counts, calls)
    assert paired <= absorbed <= 3 * paired, counts
    assert sum(by_size) == paired + alone, (by_size, counts)
    assert by_size[0] == alone and sum(by_size[1:]) == paired, (by_size, counts)
    assert sum((n + 1) * v for n, v in enumerate(by_size)) == calls, (by_size, calls)


@pytest.mark.parametrize("k", [1, 10, 56])
@pytest.mark.parametrize("rows", ROWS)
def test_uniform_series(S, rows, k):
    want = _want(S, ("uniform", rows, k), (rows,), CALLS, (k,))
    if rows >= 1000:
        assert (want[2][1:] == 0).all()                            # (call 0 carries the zero query)
    got, counts, by_size = _grouped(S, (rows,), CALLS, (k,))
    _same(got, want)
    _accounted(counts, by_size, CALLS)
    assert counts[0] > 0, counts


def test_some_launch_serves_four_calls(S):
    """Whether a later call may be taken also depends on a host-side query of the caller's stream, which races with the GPU: counted
    over several series, every one of them checked."""
    want = _want(S, ("uniform", 65_537, 10), (65_537,), CALLS, (10,))
    full = 0
    for _ in range(6):
        got, counts, by_size = _grouped(S, (65_537,), CALLS, (10,))
        _same(got, want)
        _accounted(counts, by_size, CALLS)
        full += by_size[3]
    assert full > 0


@pytest.mark.parametrize("pair,never", [(1, (2, 3)), (2, (3,))])
def test_smaller_limits(S, pair, never):
    """scan_pair = 1 is the pair mode (2 x paired + alone == calls, absorbed == paired); scan_pair = 2 never serves four."""
    want = _want(S, ("uniform", 65_537, 10), (65_537,), CALLS, (10,))
    seen = [0, 0, 0, 0]
    for _ in range(3):
        got, counts, by_size = _grouped(S, (65_537,), CALLS, (10,), pair=pair)
        _same(got, want)
        _accounted(counts, by_size, CALLS)
        if pair == 1:
            assert 2 * counts[0] + counts[1] == CALLS and counts[2] == counts[0], counts
        seen = [a + b for a, b in zip(seen, by_size)]
    assert all(seen[n] == 0 for n in never) and seen[pair] > 0, seen


def test_zero_query_and_exact_duplicate_rows(S):
    def qsel(i):
        return (i // 3) % 8                                        # the zero query three times, then the duplicated row's three times ...
    want = _want(S, ("dup",), ("dup",), CALLS, (10,), qsel=qsel)
    assert want[0][6, :3].tolist() == [7, 107, 40_007]             # the three copies, in row order
    got, counts, by_size = _grouped(S, ("dup",), CALLS, (10,), qsel=qsel)
    _same(got, want)
    _accounted(counts, by_size, CALLS)
    assert counts[0] > 0, counts


def test_two_corpora_in_turn(S):
    names = (65_537, "other")                                      # steps i + 2, i + 4, i + 6 are in front of the same corpus
    want = _want(S, ("two",), names, CALLS, (10,))
    got, counts, by_size = _grouped(S, names, CALLS, (10,))
    _same(got, want)
    _accounted(counts, by_size, CALLS)
    assert counts[0] > 0, counts


def test_three_corpora_in_turn_never_group(S):
    names = (65_537, "other", "dup")                               # step i + 2 is in front of another corpus (by address)
    want = _want(S, ("three",), names, CALLS, (10,))
    got, counts, by_size = _grouped(S, names, CALLS, (10,))
    _same(got, want)
    _accounted(counts, by_size, CALLS)
    assert by_size == (CALLS, 0, 0, 0), by_size


@pytest.mark.parametrize("ks,largest", [((10, 3), 4), ((10, 10, 3, 3), 1), ((10, 10, 10, 10, 3, 3, 3, 3), 2)])
def test_alternating_k_ends_a_group(S, ks, largest):
    """The lists of a group have one size (k'), and the group is a prefix: equal k two calls apart groups, unequal k does not, and
    with k changing every four calls step i + 4 always differs from step i or from step i + 2 -- no launch serves more than two."""
    want = _want(S, ("ks", ks), (65_537,), CALLS, ks)
    got, counts, by_size = _grouped(S, (65_537,), CALLS, ks)
    _same(got, want)
    _accounted(counts, by_size, CALLS)
    assert all(v == 0 for v in by_size[largest:]), by_size
    assert (counts[0] > 0) == (largest > 1), counts


@pytest.mark.parametrize("what", ["host_at", "largek_at"])
def test_other_calls_in_the_middle_of_a_series(S, what):
    """A host-form search (drains the pipeline) and a k = 100 call (another route, on the context's stream) at call 13 of 24."""
    kw = {what: 13}
    want = _want(S, ("mid", what), (65_537,), CALLS, (10,), **kw)
    got, counts, by_size = _grouped(S, (65_537,), CALLS, (10,), **kw)
    _same(got, want)
    if what == "host_at":
        assert got[3][0].tolist() == want[3][0].tolist() and got[3][1].tobytes() == want[3][1].tobytes()
    _accounted(counts, by_size, CALLS - (1 if what == "largek_at" else 0))   # (calls that went through the group-capable scan)
    assert counts[0] > 0, counts


def test_profiled_launches_and_their_successors_run_alone(S):
    """prof_every = 8: launches 0, 8, 16 are bracketed by events and 1, 9, 17 follow one; none of the six leads or is taken."""
    want = _want(S, ("uniform", 65_537, 10), (65_537,), CALLS, (10,))
    S.ctx.prof_enable(True)
    S.ctx.set_tuning("prof_every", 8)
    S.ctx.prof_reset()
    try:
        got, counts, by_size = _grouped(S, (65_537,), CALLS, (10,))
        timed = S.ctx.prof_read("scan")[0]
    finally:
        S.ctx.set_tuning("prof_every", 1)
        S.ctx.prof_enable(False)
    _same(got, want)
    _accounted(counts, by_size, CALLS)
    assert timed == CALLS // 8 and counts[1] >= 2 * timed, (timed, counts)
    assert counts[0] > 0 and by_size[3] == 0, (counts, by_size)    # (steps i + 2 .. i + 6 of any leader include a launch that runs alone)


def test_cut_descriptor_ring(S):
    """200 calls with no wait and no synchronise before the end, the descriptor ring cut to 64 slots: a descriptor rewritten before
    the scan that would read it starts fails the step check, which only ends that group early."""
    want = _want(S, ("ring",), (300_001,), 200, (10,), wait_us=0)
    S.ctx.set_tuning("scan_pair_ring", 64)
    try:
        got, counts, by_size = _grouped(S, (300_001,), 200, (10,), wait_us=0)
    finally:
        S.ctx.set_tuning("scan_pair_ring", 4096)
    _same(got, want)
    _accounted(counts, by_size, 200)
