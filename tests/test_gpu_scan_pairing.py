"""scan_pair: queued one-query scans of the scan_overlap pipeline share a corpus pass -- the scan of call i takes the query of call
i + 2 along and call i + 2's own scan ends at once.  Every case is compared byte for byte (rows, distances, status words) with
scan_pair = 0, and the device counters must account for every call: 2 x paired + alone == calls, absorbed == paired.

The small corpora scan in a few microseconds, faster than the host issues calls, so those series set scan_pair_wait_us = 2000: the
deciding block then waits for the later call's descriptor and pairing does not depend on timing.  The 1 M-row series run as shipped
(no wait): there the GPU is behind the host, which is the case the feature is for."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_BIG = 1_000_000
N_A, N_B = 4_099, 70_001          # not multiples of the 4-row chunk; one block / more than one block per launch


class _Setup:
    pass


@pytest.fixture(scope="module")
def S():
    import torch
    import semtools_amd as smt
    from tests.test_gpu_nearties import adversarial_corpus

    s = _Setup()
    s.torch = torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(47)
    s.x = torch.randn(N_BIG, 256, device=dev, generator=g)
    s.x /= s.x.norm(dim=1, keepdim=True)
    s.qs = torch.randn(64, 256, device=dev, generator=g)
    s.qs /= s.qs.norm(dim=1, keepdim=True)
    s.qs[0] = 0.0                                                  # a zero query
    q_adv, emb_adv, _ = adversarial_corpus(seed=55)                # 40 near-ties around the 10th place: k = 10 is UNCERTAIN
    s.q_adv = torch.from_numpy(q_adv).to(dev)
    torch.cuda.synchronize()
    s.stream = torch.cuda.Stream(dev)
    s.ctx = smt.Context(0, stream=s.stream.cuda_stream)
    s.corpora = {
        "a": smt.Corpus(s.ctx, device_ptr=s.x.data_ptr(), rows=N_A),
        "b": smt.Corpus(s.ctx, device_ptr=s.x.data_ptr(), rows=N_B),
        "c": smt.Corpus(s.ctx, device_ptr=s.x[5_000:].data_ptr(), rows=N_B),   # other rows, same count
        "big": smt.Corpus(s.ctx, device_ptr=s.x.data_ptr(), rows=N_BIG),
    }
    adv = smt.Corpus(s.ctx)
    adv.append(emb_adv)
    s.corpora["adv"] = adv
    s.ctx.set_tuning("async_select", 1)
    s.ref = {}
    yield s
    for c in s.corpora.values():
        c.close()
    s.ctx.close()


def _series(s, names, n, ks, pair, wait_us=2000, row_bases=(0,), qsel=None, adv_query=False, fresh_query=False, host_at=None,
            largek_at=None, off_at=None, wait="ctx"):
    """n back-to-back calls over the corpora `names` in turn, k from `ks` in turn; returns (rows, dists, status, host answer) as
    numpy arrays and the (paired, alone, absorbed) counted during the series."""
    torch, ctx, stream = s.torch, s.ctx, s.stream
    ctx.set_tuning("scan_pair", pair)
    ctx.set_tuning("scan_pair_wait_us", wait_us if pair else 0)
    kmax = max(max(ks), 100 if largek_at is not None else 0)
    dev = s.qs.device
    with torch.cuda.stream(stream):
        rows = torch.full((n, kmax), -7, dtype=torch.int64, device=dev)
        dist = torch.full((n, kmax), -7.0, dtype=torch.float64, device=dev)
        status = torch.full((n,), 7, dtype=torch.int32, device=dev)
        qbuf = torch.zeros((n, 256), dtype=torch.float32, device=dev)
        if fresh_query:
            big_in = torch.ones(64 << 20, dtype=torch.float32, device=dev)
            big_out = torch.empty_like(big_in)
    stream.synchronize()
    before = ctx.scan_pairs()
    host = None
    try:
        for i in range(n):
            k = 100 if i == largek_at else ks[i % len(ks)]
            q = s.q_adv if adv_query else s.qs[qsel(i) if qsel else i % 64]
            if fresh_query:
                # written by a torch op on the context's stream right before the call: such a call must not be taken along
                with torch.cuda.stream(stream):
                    torch.mul(big_in, 1.0, out=big_out)
                    torch.mul(q, 1.0, out=qbuf[i])
                q = qbuf[i]
            if i == off_at:
                ctx.set_tuning("scan_pair", 0)
            s.corpora[names[i % len(names)]].search_topk_device(q.data_ptr(), 1, k, row_bases[i % len(row_bases)], rows[i].data_ptr(),
                                                                dist[i].data_ptr(), out_status_ptr=status[i:].data_ptr())
            if i == host_at:
                host = s.corpora[names[0]].search(s.qs[1].cpu().numpy(), top_k=10)[0]
        if wait == "ctx":
            ctx.synchronize()
        else:
            torch.cuda.synchronize()
        after = ctx.scan_pairs()
    finally:
        ctx.set_tuning("scan_pair", 0)
        ctx.set_tuning("scan_pair_wait_us", 0)
    counts = tuple(int(b - a) for a, b in zip(before, after))
    print("scan_pair=%d %s n=%d ks=%s: paired %d alone %d absorbed %d" % ((pair, names, n, ks) + counts))
    return (rows.cpu().numpy(), dist.cpu().numpy(), status.cpu().numpy(), host), counts


def _want(s, key, *args, **kw):
    """The scan_pair = 0 answers of a series, computed once."""
    if key not in s.ref:
        got, counts = _series(s, *args, pair=0, **kw)
        assert counts == (0, 0, 0), counts
        s.ref[key] = got
    return s.ref[key]


def _same(a, b):
    for x, y in zip(a[:3], b[:3]):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def _accounted(counts, calls, can_pair=True):
    paired, alone, absorbed = counts
    assert 2 * paired + alone == calls and absorbed == paired, (counts, calls)
    assert (paired > 0) == can_pair, counts


@pytest.mark.parametrize("names", [("a",), ("b",), ("a", "b"), ("b", "c")])
@pytest.mark.parametrize("k", [1, 10, 56])
def test_series_over_one_and_two_corpora(S, names, k):
    want = _want(S, ("const", names, k), names, 120, (k,))
    assert (want[2][np.arange(120) % 64 != 0] == 0).all()          # (calls 0 and 64 carry the zero query)
    got, counts = _series(S, names, 120, (k,), 1)
    _same(got, want)
    _accounted(counts, 120)


def test_three_corpora_in_turn_never_pair(S):
    names = ("a", "b", "c")                                        # call i + 2 is in front of another corpus, by row count or by address
    want = _want(S, ("three",), names, 120, (10,))
    got, counts = _series(S, names, 120, (10,), 1)
    _same(got, want)
    _accounted(counts, 120, can_pair=False)


@pytest.mark.parametrize("ks,can_pair", [((10, 3), True), ((10, 10, 3, 3), False)])
def test_alternating_k(S, ks, can_pair):
    """The lists of a pair have one size: equal k two calls apart pairs, unequal k does not."""
    want = _want(S, ("ks", ks), ("b",), 120, ks)
    got, counts = _series(S, ("b",), 120, ks, 1)
    _same(got, want)
    _accounted(counts, 120, can_pair)


def test_row_base_differs_per_call(S):
    bases = (0, 1_000, 5_000_000_000)                              # the select's business: such calls still pair
    want = _want(S, ("bases",), ("b",), 120, (10,), row_bases=bases)
    assert want[0][1, 0] >= 1_000 and want[0][2, 0] >= 5_000_000_000
    got, counts = _series(S, ("b",), 120, (10,), 1, row_bases=bases)
    _same(got, want)
    _accounted(counts, 120)


def test_zero_query_and_one_query_twice_in_a_pair(S):
    def qsel(i):
        return (i // 4) % 64                                       # calls i and i + 2 carry the same query; the first four the zero query
    want = _want(S, ("qsel",), ("b",), 120, (10,), qsel=qsel)
    got, counts = _series(S, ("b",), 120, (10,), 1, qsel=qsel)
    _same(got, want)
    _accounted(counts, 120)
    assert got[0][0].tolist() == got[0][2].tolist() and got[1][0].tobytes() == got[1][2].tobytes()


def test_uncertain_verdict_is_the_same_paired_and_alone(S):
    want = _want(S, ("adv",), ("adv",), 40, (10,), adv_query=True)
    assert (want[2] == 1).all()                                    # SMT_STATUS_UNCERTAIN: no certificate through 40 near-ties
    S.ctx.uncertain_count()
    got, counts = _series(S, ("adv",), 40, (10,), 1, adv_query=True)
    _same(got, want)
    _accounted(counts, 40)
    assert S.ctx.uncertain_count() == 40


@pytest.mark.parametrize("every,can_pair", [(4, False), (8, True)])
def test_profiled_launches_and_their_successors_run_alone(S, every, can_pair):
    """prof_every = 4: launches 0, 4, 8 ... are bracketed by events, 1, 5, 9 ... follow one, and a launch two steps in front of either
    finds no partner: nothing pairs.  prof_every = 8 leaves two launches in eight that can take a partner."""
    want = _want(S, ("const", ("b",), 10), ("b",), 120, (10,))
    S.ctx.prof_enable(True)
    S.ctx.set_tuning("prof_every", every)
    S.ctx.prof_reset()
    try:
        got, counts = _series(S, ("b",), 120, (10,), 1)
        timed = S.ctx.prof_read("scan")[0]
    finally:
        S.ctx.set_tuning("prof_every", 1)
        S.ctx.prof_enable(False)
    _same(got, want)
    _accounted(counts, 120, can_pair)
    assert timed == 120 // every
    assert counts[1] >= 2 * timed                                  # the timed launches and their successors


def test_query_written_on_the_stream_right_before_the_call(S):
    want = _want(S, ("const", ("b",), 10), ("b",), 120, (10,))
    got, counts = _series(S, ("b",), 120, (10,), 1, fresh_query=True)
    _same(got, want)
    _accounted(counts, 120, can_pair=False)


@pytest.mark.parametrize("what", ["host_at", "largek_at", "off_at"])
def test_other_calls_in_the_middle_of_a_series(S, what):
    """A host-form search (drains the pipeline), a k = 100 call (the sampled-threshold route on the context's stream) and scan_pair
    switched off, each at call 61 of 120."""
    kw = {what: 61}
    want = _want(S, ("mid", what), ("b",), 120, (10,), **kw)
    got, counts = _series(S, ("b",), 120, (10,), 1, **kw)
    _same(got, want)
    if what == "host_at":
        assert got[3][0].tolist() == want[3][0].tolist() and got[3][1].tobytes() == want[3][1].tobytes()
    paired, alone, absorbed = counts
    assert paired > 0 and absorbed == paired
    assert 2 * paired + alone == {"host_at": 120, "largek_at": 119, "off_at": 61}[what]   # (calls that went through the paired-mode scan)


def test_odd_series_ending_in_torch_synchronize(S):
    want = _want(S, ("odd",), ("b",), 121, (10,), wait="torch")
    got, counts = _series(S, ("b",), 121, (10,), 1, wait="torch")
    _same(got, want)
    _accounted(counts, 121)


@pytest.mark.parametrize("ring", [4096, 64])
def test_big_corpus_as_shipped_and_ring_reuse(S, ring):
    """200 calls over 1 M rows with no wait and no synchronise before the end, so the host runs far more than 70 calls ahead of the
    GPU.  With the ring cut to 64 slots (scan_pair_ring) descriptors are rewritten before the scan that would read them starts:
    that scan fails the step check and runs alone."""
    want = _want(S, ("big",), ("big",), 200, (10,), wait_us=0)
    assert (want[2][np.arange(200) % 64 != 0] == 0).all()
    S.ctx.set_tuning("scan_pair_ring", ring)
    try:
        got, counts = _series(S, ("big",), 200, (10,), 1, wait_us=0)
    finally:
        S.ctx.set_tuning("scan_pair_ring", 4096)
    _same(got, want)
    paired, alone, absorbed = counts
    assert 2 * paired + alone == 200 and absorbed == paired, counts
    assert paired > 0, counts
