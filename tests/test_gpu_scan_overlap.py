"""scan_overlap (default 1): one-query device searches in the async pipeline run scan + select of call i on internal stream i & 1,
consecutive scans overlapping behind a start gate.  Every case is compared byte for byte with scan_overlap = 0 (the aux-stream pipeline)."""
import pytest

pytestmark = pytest.mark.gpu

N_BIG = 1_000_000
SIZES = (N_BIG, 300_000, 5_000, 1_000)


@pytest.fixture(scope="module")
def setup():
    import torch
    import semtools_amd as smt

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(31)
    x = torch.randn(N_BIG, 256, device=dev, generator=g)
    x /= x.norm(dim=1, keepdim=True)
    qs = torch.randn(64, 256, device=dev, generator=g)
    qs /= qs.norm(dim=1, keepdim=True)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(dev)
    ctx = smt.Context(0, stream=stream.cuda_stream)
    corpora = [smt.Corpus(ctx, device_ptr=x.data_ptr(), rows=n) for n in SIZES]
    ctx.set_tuning("async_select", 1)
    yield torch, ctx, stream, corpora, qs
    for c in corpora:
        c.close()
    ctx.close()


def _series(torch, ctx, stream, corpora, qs, n, ks, overlap, wait="ctx", fresh_query=False, host_at=None, off_at=None, on_aux=False):
    """n back-to-back calls alternating the corpora and the k in `ks`; returns (rows, dists, status) as numpy arrays.
    on_aux: the answers returned are COPIES made on the context's aux stream right behind each call (no sync in between)."""
    ctx.set_tuning("scan_overlap", overlap)
    kmax = max(ks)
    dev = qs.device
    with torch.cuda.stream(stream):
        rows = torch.full((n, kmax), -7, dtype=torch.int64, device=dev)
        dist = torch.full((n, kmax), -7.0, dtype=torch.float64, device=dev)
        status = torch.full((n,), 7, dtype=torch.int32, device=dev)
        qbuf = torch.zeros((n, 256), dtype=torch.float32, device=dev)
        if fresh_query:
            # ~0.5 GB of traffic in front of every query write: a scan that did not wait for the stream would read a zero query
            big_in = torch.ones(64 << 20, dtype=torch.float32, device=dev)
            big_out = torch.empty_like(big_in)
    aux = None
    if on_aux:
        aux = torch.cuda.ExternalStream(ctx.aux_stream(), device=dev)
        with torch.cuda.stream(aux):
            rows2, dist2, status2 = torch.empty_like(rows), torch.empty_like(dist), torch.empty_like(status)
    stream.synchronize()
    host = None
    for i in range(n):
        k = ks[i % len(ks)]
        q = qs[i % 64]
        if fresh_query:
            # the query is written by a torch op on the context's stream right before the call, no host sync in between
            with torch.cuda.stream(stream):
                torch.mul(big_in, 1.0, out=big_out)
                torch.mul(q, 1.0, out=qbuf[i])
            q = qbuf[i]
        if off_at is not None and i == off_at:
            ctx.set_tuning("scan_overlap", 0)
        corpora[i % len(corpora)].search_topk_device(q.data_ptr(), 1, k, 0, rows[i].data_ptr(), dist[i].data_ptr(),
                                                     out_status_ptr=status[i:].data_ptr())
        if aux is not None:
            if k > 56:
                # not an async select: the sampled-threshold route runs on the context's stream, which is what orders work behind it
                aux.wait_stream(stream)
            with torch.cuda.stream(aux):
                rows2[i].copy_(rows[i])
                dist2[i].copy_(dist[i])
                status2[i].copy_(status[i])
        if host_at is not None and i == host_at:
            host = corpora[0].search(qs[0].cpu().numpy(), top_k=10)[0]
    if wait == "ctx":
        ctx.synchronize()
    else:
        torch.cuda.synchronize()
    if aux is not None:
        rows, dist, status = rows2, dist2, status2
    return rows.cpu().numpy(), dist.cpu().numpy(), status.cpu().numpy(), host


def _same(a, b):
    for x, y in zip(a[:3], b[:3]):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("ks", [(10,), (10, 3), (56, 1, 10)])
def test_overlap_series_equals_aux_pipeline(setup, ks):
    torch, ctx, stream, corpora, qs = setup
    want = _series(torch, ctx, stream, corpora, qs, 240, ks, 0)
    assert (want[2] == 0).all()
    for rep in range(2):
        got = _series(torch, ctx, stream, corpora, qs, 240, ks, 1)
        _same(got, want)


@pytest.mark.parametrize("on_aux", [False, True])
@pytest.mark.parametrize("ks", [(10, 100), (56, 57, 1, 1024, 10)])
def test_large_k_calls_inside_the_overlapped_series(setup, ks, on_aux):
    """k > 56 takes the sampled-threshold route on the context's stream (bind_device(ctx, true)) between one-query calls whose scan
    and select run on the two internal streams: rows, distances and status words are the bytes of scan_overlap = 0.  on_aux: the
    answers are copied on the aux stream right behind each call; behind a large-k call that stream first waits for the context's."""
    torch, ctx, stream, corpora, qs = setup
    want = _series(torch, ctx, stream, corpora, qs, 240, ks, 0, on_aux=on_aux)
    assert set(want[2].tolist()) <= {0, 1, 2}
    small = [i for i in range(240) if ks[i % len(ks)] <= 56]
    assert (want[2][small] == 0).all()
    large = [i for i in range(240) if ks[i % len(ks)] > 56]
    assert (want[2][large] == 0).sum() >= 0.95 * len(large)        # and the large-k calls did prove their lists
    assert (want[2][large] != 2).all()                             # (an overflowed buffer keeps keys in the order of its atomics)
    for i in large:                                                # a written list, padded behind min(k, n)
        k = ks[i % len(ks)]
        n = SIZES[i % len(SIZES)]
        assert (want[0][i, :min(k, n)] >= 0).all() and (want[0][i, min(k, n):k] == -1).all() and (want[0][i, k:] == -7).all()
    for rep in range(2):
        got = _series(torch, ctx, stream, corpora, qs, 240, ks, 1, on_aux=on_aux)
        _same(got, want)


@pytest.mark.parametrize("gate", [0, 50, 100])
def test_gate_setting_changes_no_answer(setup, gate):
    torch, ctx, stream, corpora, qs = setup
    want = _series(torch, ctx, stream, corpora, qs, 200, (10,), 0)
    ctx.set_tuning("scan_gate_pct", gate)
    try:
        got = _series(torch, ctx, stream, corpora, qs, 200, (10,), 1)
    finally:
        ctx.set_tuning("scan_gate_pct", 50)
    _same(got, want)


def test_query_written_on_the_stream_right_before_the_call(setup):
    torch, ctx, stream, corpora, qs = setup
    want = _series(torch, ctx, stream, corpora, qs, 200, (10, 3), 0)
    got = _series(torch, ctx, stream, corpora, qs, 200, (10, 3), 1, fresh_query=True)
    _same(got, want)


def test_results_after_torch_synchronize(setup):
    torch, ctx, stream, corpora, qs = setup
    want = _series(torch, ctx, stream, corpora, qs, 200, (10,), 0)
    got = _series(torch, ctx, stream, corpora, qs, 200, (10,), 1, wait="torch")
    _same(got, want)


def test_host_search_mid_series_drains(setup):
    torch, ctx, stream, corpora, qs = setup
    want = _series(torch, ctx, stream, corpora, qs, 200, (10,), 0, host_at=101)
    got = _series(torch, ctx, stream, corpora, qs, 200, (10,), 1, host_at=101)
    _same(got, want)
    assert got[3][0].tolist() == want[3][0].tolist() and got[3][1].tobytes() == want[3][1].tobytes()
    assert got[3][0].tolist() == want[0][0, :10].tolist()      # call 0: corpus 0 (1 M rows), query 0, k = 10


def test_mode_switched_off_mid_series(setup):
    torch, ctx, stream, corpora, qs = setup
    want = _series(torch, ctx, stream, corpora, qs, 200, (10, 3), 0)
    got = _series(torch, ctx, stream, corpora, qs, 200, (10, 3), 1, off_at=117)
    _same(got, want)
    # ... and back on, then the plain in-order path
    got = _series(torch, ctx, stream, corpora, qs, 200, (10, 3), 1)
    _same(got, want)
    ctx.set_tuning("async_select", 0)
    try:
        got = _series(torch, ctx, stream, corpora, qs, 200, (10, 3), 1)
    finally:
        ctx.set_tuning("async_select", 1)
    _same(got, want)


def test_work_chained_on_the_aux_stream_sees_the_answers(setup):
    """smt_ctx_aux_stream's contract: work a host enqueues on the aux stream after a call runs behind that call's select -- also when
    the select ran on a scan stream (scan_overlap)."""
    torch, ctx, stream, corpora, qs = setup
    want = _series(torch, ctx, stream, corpora, qs, 200, (10, 3), 0, on_aux=True)
    assert (want[2] == 0).all()
    got = _series(torch, ctx, stream, corpora, qs, 200, (10, 3), 1, on_aux=True)
    _same(got, want)
