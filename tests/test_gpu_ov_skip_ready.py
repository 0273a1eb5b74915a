"""ov_skip_ready = 1: a pipeline call made while the caller's stream is empty records no ready event on that stream and puts no wait
in front of its scan; a call made while work is still queued there is ordered behind it as before.  Answers are compared byte for
byte with ov_skip_ready = 0, and smt_debug_ov_ready counts the ready events that were recorded."""
import pytest

from tests.test_gpu_scan_pairing import _same

pytestmark = pytest.mark.gpu

ROWS = 65_537
CALLS = 64


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
    g.manual_seed(71)
    s.x = torch.randn(ROWS, 256, device=dev, generator=g)
    s.x /= s.x.norm(dim=1, keepdim=True)
    s.qs = torch.randn(16, 256, device=dev, generator=g)
    s.qs /= s.qs.norm(dim=1, keepdim=True)
    torch.cuda.synchronize()
    s.stream = torch.cuda.Stream(dev)
    s.ctx = smt.Context(0, stream=s.stream.cuda_stream)
    s.corpus = smt.Corpus(s.ctx, device_ptr=s.x.data_ptr(), rows=ROWS)
    s.ctx.set_tuning("async_select", 1)
    yield s
    s.corpus.close()
    s.ctx.close()


def _series(s, skip, n=CALLS, k=10, fresh=()):
    """n back-to-back calls at ov_skip_ready = `skip`; the calls named in `fresh` read their query from a buffer that a torch op on the
    caller's stream fills right before the call, behind ~2 ms of other work on that stream.  Returns (rows, dists, status) and the
    ready events recorded by the calls in `fresh` and by the others."""
    torch, ctx, stream = s.torch, s.ctx, s.stream
    dev = s.qs.device
    ctx.set_tuning("ov_skip_ready", skip)
    with torch.cuda.stream(stream):
        rows = torch.full((n, k), -7, dtype=torch.int64, device=dev)
        dist = torch.full((n, k), -7.0, dtype=torch.float64, device=dev)
        status = torch.full((n,), 7, dtype=torch.int32, device=dev)
        qbuf = s.qs[5].repeat(n, 1).contiguous()                   # another query than the one the op writes
        big_in = torch.ones(64 << 20, dtype=torch.float32, device=dev)
        big_out = torch.empty_like(big_in)
    stream.synchronize()
    rec_fresh = rec_other = 0
    try:
        for i in range(n):
            q = s.qs[i % len(s.qs)]
            if i in fresh:
                with torch.cuda.stream(stream):
                    for _ in range(20):
                        torch.mul(big_in, 1.0, out=big_out)
                    torch.mul(q, 1.0, out=qbuf[i])
                q = qbuf[i]
            before = ctx.ov_ready_records()
            s.corpus.search_topk_device(q.data_ptr(), 1, k, 0, rows[i].data_ptr(), dist[i].data_ptr(), out_status_ptr=status[i:].data_ptr())
            if i in fresh:
                rec_fresh += ctx.ov_ready_records() - before
            else:
                rec_other += ctx.ov_ready_records() - before
            if i in fresh:
                stream.synchronize()                               # (the next calls find the caller's stream empty again)
        ctx.synchronize()
    finally:
        ctx.set_tuning("ov_skip_ready", 1)
    print("ov_skip_ready=%d fresh=%s: ready events of the fresh calls %d, of the others %d" % (skip, sorted(fresh), rec_fresh, rec_other))
    return (rows.cpu().numpy(), dist.cpu().numpy(), status.cpu().numpy()), rec_fresh, rec_other


def test_answers_equal_and_no_event_on_an_empty_stream(S):
    want, _, rec_other = _series(S, 0)
    assert rec_other == CALLS                                      # as before: one ready event per call
    assert (want[2] == 0).all()
    got, _, rec_other = _series(S, 1)
    _same(got, want)
    assert rec_other == 0, rec_other                               # nothing was queued on the caller's stream at any call


def test_a_query_still_being_written_on_the_callers_stream_is_waited_for(S):
    fresh = (3, 20, 41)
    want, _, _ = _series(S, 0)                                     # every query read from where it lies: the answers of the queries themselves
    for skip in (0, 1):
        got, rec_fresh, rec_other = _series(S, skip, fresh=fresh)
        _same(got, want)                                           # ... not those of what the buffer held before the op ran
        assert rec_fresh == len(fresh), (skip, rec_fresh)          # the ready event's path was taken
        assert rec_other == (0 if skip else CALLS - len(fresh)), (skip, rec_other)
