"""GPU: top-k for 57 <= k <= 1024 through the sampled-threshold route (topk_large.hip).

The device form answers these k without a host synchronisation; every list it marks PROVED is the oracle's exact answer (same rows,
same f64 bits).  smt_search takes the same route and re-answers a query it cannot prove by the all-keys path, so its answers are
byte-equal to the all-keys path's (tuning key largek_sampled = 0) and to the oracle's."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import synth

pytestmark = pytest.mark.gpu

N = 200_000
KS = [57, 64, 100, 512, 1024]
NQS = [1, 3, 4, 5, 37]


def _oracle(emb, q, k):
    res = orc.search_documents(emb, [len(emb)], q, n_lines=0, top_k=k, accurate=True)
    return [r["match_line"] for r in res], np.array([r["distance"] for r in res])


@pytest.fixture(scope="module")
def dev_ctx():
    import torch
    import semtools_amd as smt

    ctx = smt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def big(dev_ctx):
    import torch
    import semtools_amd as smt

    emb = synth.unit_rows(N, seed=41)
    x = torch.from_numpy(emb).to("cuda:0")
    c = smt.Corpus(dev_ctx, device_ptr=x.data_ptr(), rows=N)
    qs = synth.unit_query(42, nq=max(NQS))
    ref = [_oracle(emb, q, max(KS)) for q in qs]
    yield emb, x, c, qs, ref
    c.close()


def _device(c, qs, k, row_base=0):
    import torch

    qd = torch.from_numpy(np.ascontiguousarray(qs)).to("cuda:0")
    nq = qd.shape[0]
    rows = torch.empty((nq, k), dtype=torch.int64, device="cuda:0")
    dist = torch.empty((nq, k), dtype=torch.float64, device="cuda:0")
    st = torch.empty(nq, dtype=torch.int32, device="cuda:0")
    c.search_topk_device(qd.data_ptr(), nq, k, row_base, rows.data_ptr(), dist.data_ptr(), st.data_ptr())
    torch.cuda.synchronize()
    return rows.cpu().numpy().view(np.uint64), dist.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("k", KS)
def test_device_form_proved_lists_equal_the_oracle(big, k):
    emb, _, c, qs, ref = big
    proved = total = 0
    for nq in NQS:
        rows, dist, st = _device(c, qs[:nq], k)
        for i in range(nq):
            total += 1
            if st[i] != 0:
                assert st[i] in (1, 2), st[i]
                continue
            proved += 1
            orows, odist = ref[i]
            assert rows[i].tolist() == orows[:k], (k, nq, i)
            assert np.array_equal(dist[i], odist[:k]), (k, nq, i)
    assert proved >= 0.95 * total, (proved, total)


def test_route_is_the_sampled_one(big, dev_ctx):
    _, _, c, qs, _ = big
    dev_ctx.prof_enable(True)
    dev_ctx.prof_reset()
    try:
        _device(c, qs[:1], 100)
        n_collect, _ = dev_ctx.prof_read("largek_collect")
        n_tau, _ = dev_ctx.prof_read("largek_tau")
        n_finish, _ = dev_ctx.prof_read("largek_finish")
        n_scan, _ = dev_ctx.prof_read("scan")
    finally:
        dev_ctx.prof_enable(False)
    assert n_collect >= 1 and n_tau >= 1 and n_finish >= 1
    assert n_scan == 0


def test_k_above_1024_refused_and_k_56_unchanged(big):
    from semtools_amd._lib import SmtError

    _, _, c, qs, ref = big
    with pytest.raises(SmtError):
        _device(c, qs[:1], 1025)
    rows, dist, st = _device(c, qs[:1], 56)
    assert st[0] == 0 and rows[0].tolist() == ref[0][0][:56]


def test_k_larger_than_the_corpus_comes_back_padded(dev_ctx):
    import torch
    import semtools_amd as smt

    emb = synth.unit_rows(700, seed=5)
    x = torch.from_numpy(emb).to("cuda:0")
    c = smt.Corpus(dev_ctx, device_ptr=x.data_ptr(), rows=700)
    q = synth.unit_query(6)
    rows, dist, st = _device(c, q, 1000, row_base=10)
    orows, odist = _oracle(emb, q[0], 1000)
    assert st[0] == 0
    assert (rows[0][:700] - 10).tolist() == orows and np.array_equal(dist[0][:700], odist)
    assert (rows[0][700:] == np.uint64(2**64 - 1)).all() and np.isinf(dist[0][700:]).all()
    hr, hd = c.search(q, top_k=1000)[0]
    assert hr.tolist() == orows and np.array_equal(hd, odist)
    c.close()


def test_nan_query_is_invalid(big, dev_ctx):
    _, _, c, qs, ref = big
    q = qs[:3].copy()
    q[1, 7] = np.nan
    dev_ctx.uncertain_count(reset=True)
    rows, dist, st = _device(c, q, 100)
    assert st[1] == 3
    assert dev_ctx.uncertain_count(reset=True) >= 1
    for i in (0, 2):
        if st[i] == 0:
            assert rows[i].tolist() == ref[i][0][:100]


def test_pipelined_calls_equal_single_calls(big):
    import torch

    _, _, c, qs, _ = big
    qd = torch.from_numpy(np.ascontiguousarray(qs)).to("cuda:0")
    n_calls, k = 50, 100
    rows = torch.empty((n_calls, k), dtype=torch.int64, device="cuda:0")
    dist = torch.empty((n_calls, k), dtype=torch.float64, device="cuda:0")
    st = torch.empty(n_calls, dtype=torch.int32, device="cuda:0")
    for i in range(n_calls):
        j = i % qd.shape[0]
        c.search_topk_device(qd[j].data_ptr(), 1, k, 0, rows[i].data_ptr(), dist[i].data_ptr(), st[i:].data_ptr())
    torch.cuda.synchronize()
    for i in range(0, n_calls, 7):
        r1, d1, s1 = _device(c, qs[i % qd.shape[0]][None], k)
        assert rows[i].cpu().numpy().view(np.uint64).tolist() == r1[0].tolist()
        assert np.array_equal(dist[i].cpu().numpy(), d1[0]) and int(st[i]) == int(s1[0])


def test_tie_cluster_across_the_kth_place(dev_ctx):
    """3000 identical rows straddle the 100th place: no list may be PROVED wrongly, and smt_search still equals the oracle."""
    import torch
    import semtools_amd as smt

    emb = synth.unit_rows(N, seed=43)
    q = synth.unit_query(44)
    orows, _ = _oracle(emb, q[0], 60)
    dup = emb[orows[-1]].copy()
    rng = np.random.default_rng(45)
    emb[rng.choice(N, size=3000, replace=False)] = dup
    x = torch.from_numpy(emb).to("cuda:0")
    c = smt.Corpus(dev_ctx, device_ptr=x.data_ptr(), rows=N)
    k = 100
    orows, odist = _oracle(emb, q[0], k)
    rows, dist, st = _device(c, q, k)
    assert st[0] != 0          # identical rows across the k-th place: no certificate can hold
    hr, hd = c.search(q, top_k=k)[0]
    assert hr.tolist() == orows and np.array_equal(hd, odist)
    c.close()


def _both(ctx, c, qs, **kw):
    ctx.set_tuning("largek_sampled", 0)
    try:
        old = c.search(qs, **kw)
    finally:
        ctx.set_tuning("largek_sampled", 1)
    new = c.search(qs, **kw)
    for (r0, d0), (r1, d1) in zip(old, new):
        assert r0.tolist() == r1.tolist() and d0.tobytes() == d1.tobytes()
    return new


@pytest.mark.parametrize("k", [57, 100, 1000])
def test_host_form_documents_mode(big, dev_ctx, k):
    _, _, c, qs, ref = big
    new = _both(dev_ctx, c, qs[:5], top_k=k)
    for i, (r, d) in enumerate(new):
        assert r.tolist() == ref[i][0][:k] and np.array_equal(d, ref[i][1][:k])


@pytest.mark.parametrize("k", [57, 100, 1000])
def test_host_form_workspace_ranges_threshold(big, dev_ctx, k):
    from semtools_amd import _lib as L

    emb, _, c, qs, _ = big
    ranges = [(0, 30_000), (50_000, 51_000), (90_000, 160_000), (199_000, 200_000)]
    sub = np.concatenate([np.arange(b, e) for b, e in ranges])
    new = _both(dev_ctx, c, qs[:4], top_k=k, mode=L.MODE_WORKSPACE, ranges=ranges, max_distance=0.93)
    thr = float(np.float32(1.0) - np.float32(0.93))   # the score threshold as the library forms it (store.rs:502-503)
    for i, (r, d) in enumerate(new):
        # every row of the subset, ordered (distance, row): the subset is ascending, so its index order is row order
        res = orc.search_documents(emb[sub], [len(sub)], qs[i], n_lines=0, top_k=len(sub), accurate=True)
        hits = [(int(sub[h["match_line"]]), h["distance"]) for h in res if (1.0 - h["distance"]) > thr][:k]
        assert r.tolist() == [j for j, _ in hits] and np.array_equal(d, np.array([v for _, v in hits]))


@pytest.mark.parametrize("prepack", [False, True])
def test_host_form_batch_of_64(dev_ctx, prepack):
    import torch
    import semtools_amd as smt

    n = 300_000
    emb = synth.unit_rows(n, seed=47)
    c = smt.Corpus(dev_ctx)
    c.append(emb)
    if prepack:
        c.prepack(True)
    qs = synth.unit_query(48, nq=64)
    for k in (57, 100, 1000):
        new = _both(dev_ctx, c, qs, top_k=k)
        for i in (0, 31, 63):
            orows, odist = _oracle(emb, qs[i], k)
            assert new[i][0].tolist() == orows and np.array_equal(new[i][1], odist)
    c.close()


def test_k3_sweep_route_for_batches(big, dev_ctx):
    """Five or more unfiltered queries collect in one sweep of the batched kernel (prof name gemm_thr), not a pass per query."""
    _, _, c, qs, ref = big
    dev_ctx.prof_enable(True)
    dev_ctx.prof_reset()
    try:
        rows, dist, st = _device(c, qs[:8], 100)
        n_thr, _ = dev_ctx.prof_read("gemm_thr")
        n_collect, _ = dev_ctx.prof_read("largek_collect")
    finally:
        dev_ctx.prof_enable(False)
    assert n_thr == 1 and n_collect == 0
    assert (st == 0).sum() >= 7
    for i in range(8):
        if st[i] == 0:
            assert rows[i].tolist() == ref[i][0][:100] and np.array_equal(dist[i], ref[i][1][:100])


@pytest.mark.parametrize("transport", ["peer", "copy"])
def test_sharded_device_form_equals_single_corpus(big, transport):
    import torch
    import semtools_amd as smt

    emb, _, c, qs, ref = big
    g = smt.Group.logical(0, 3)
    try:
        g.set_transport(transport)
        sc = smt.ShardedCorpus(g, rows=emb)
        for k in (100, 1024):
            for nq in (2, 5):
                qd = torch.from_numpy(np.ascontiguousarray(qs[:nq])).cuda()
                out = torch.zeros((nq, 2, k), dtype=torch.int64, device="cuda")
                st = torch.full((nq,), 7, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                sc.search_topk_device([qd.data_ptr()] * 3, nq, k, [out.data_ptr(), 0, 0], [st.data_ptr(), 0, 0])
                g.synchronize()
                m, s_ = out.cpu().numpy(), st.cpu().numpy()
                assert (s_ == 0).sum() >= nq - 1, s_
                for i in range(nq):
                    if s_[i] != 0:
                        continue
                    assert np.ascontiguousarray(m[i, 0]).view(np.uint64).tolist() == ref[i][0][:k], (transport, k, nq, i)
                    assert np.array_equal(np.ascontiguousarray(m[i, 1]).view(np.float64), ref[i][1][:k])
        sc.close()
    finally:
        g.close()


def test_sharded_device_form_refuses_more_than_8192_candidates(big):
    import torch
    import semtools_amd as smt
    from semtools_amd._lib import SmtError

    emb, _, _, qs, _ = big
    g = smt.Group.logical(0, 9)
    try:
        sc = smt.ShardedCorpus(g, rows=emb[:90_000])
        qd = torch.from_numpy(np.ascontiguousarray(qs[:1])).cuda()
        out = torch.zeros((1, 2, 1000), dtype=torch.int64, device="cuda")
        with pytest.raises(SmtError):
            sc.search_topk_device([qd.data_ptr()] * 9, 1, 1000, [out.data_ptr()] + [0] * 8)   # 9 x 1000 > 8192
        # 9 x 900 = 8100 candidates are accepted: the in-place merge on its 128 KiB LDS branch.  Its answer is read: where every shard
        # proved its list (combined status 0) it is the oracle's over the 90 000 rows
        out900 = torch.full((1, 2, 900), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        st = torch.full((1,), 7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        sc.search_topk_device([qd.data_ptr()] * 9, 1, 900, [out900.data_ptr()] + [0] * 8, [st.data_ptr()] + [0] * 8)
        g.synchronize()
        m, s_ = out900.cpu().numpy(), st.cpu().numpy()
        print("combined status of the 9 x 900 call", s_.tolist())
        assert s_[0] in (0, 1, 2), s_
        if s_[0] == 0:
            orows, odist = _oracle(emb[:90_000], qs[0], 900)
            assert np.ascontiguousarray(m[0, 0]).view(np.uint64).tolist() == orows
            assert np.array_equal(np.ascontiguousarray(m[0, 1]).view(np.float64), odist)
        sc.close()
    finally:
        g.close()
