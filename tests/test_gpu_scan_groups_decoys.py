"""GPU: grouped one-query scans (scan_pair = 3) may not look outside the rows they were given either.  One decoy series of
tests/decoys.py through grouped calls: layout A, the adopted corpus with rows that would rank first for every query in the 64 rows
before and behind it.  Every returned id must be allowed and every proved answer bit-equal to the oracle's over the allowed rows
(the checks of tests/test_gpu_decoys.py, whose helpers this file uses)."""
import pytest

from tests import decoys as D
from tests.test_gpu_decoys import Adopted, _check_series, _series, qs, tuned  # noqa: F401  (qs: a fixture)

pytestmark = pytest.mark.gpu

N = 4097                                                           # several blocks, a ragged last chunk
assert N in D.SIZES_A


@pytest.fixture(scope="module")
def piped():
    """A context of its own on a torch stream with the async select pipeline on, as in tests/test_gpu_decoys.py -- on a stream where
    queued calls can be taken along at all (tests/test_gpu_scan_groups.py says why some cannot)."""
    import torch
    import semtools_amd as smt

    x = torch.zeros(1000, 256, device="cuda:0")
    x[:, 0] = 1.0
    torch.cuda.synchronize()
    for attempt in range(6):
        stream = torch.cuda.Stream(torch.device("cuda:0"))
        ctx = smt.Context(0, stream=stream.cuda_stream)
        ctx.set_tuning("async_select", 1)
        probe = smt.Corpus(ctx, device_ptr=x.data_ptr(), rows=1000)
        with tuned(ctx, scan_overlap=1, scan_pair=1, scan_pair_wait_us=2000):
            paired = _series(torch, ctx, stream, probe, x[:1], 8, 10)[3][0]
        probe.close()
        if paired > 0 or attempt == 5:                             # (the last one stays: the test then says what is wrong)
            break
        ctx.close()
    yield torch, ctx, stream
    ctx.set_tuning("async_select", 0)
    ctx.close()


def test_a_grouped_series_of_one_query_calls(piped, qs):
    torch, ctx, stream = piped
    k, calls, series = 10, 16, 6
    a = Adopted(ctx, N, "finite")
    try:
        qd = torch.from_numpy(qs[:5]).to("cuda:0")
        torch.cuda.synchronize()
        want = a.ref.topk(qs[:5], k)
        paired = alone = absorbed = 0
        full = 0
        with tuned(ctx, scan_overlap=1, scan_pair=3, scan_pair_wait_us=2000):
            ctl_st = _series(torch, ctx, stream, a.ctl, qd, calls, k)[2]
            for s in range(series):
                before = ctx.scan_groups()
                rows, dist, st, counts = _series(torch, ctx, stream, a.c, qd, calls, k)
                by_size = [int(y - x) for x, y in zip(before, ctx.scan_groups())]
                paired, alone, absorbed = paired + counts[0], alone + counts[1], absorbed + counts[2]
                full += by_size[3]
                assert sum((n + 1) * v for n, v in enumerate(by_size)) == calls, by_size
                _check_series(lambda i: (a.ref, want), rows, dist, st, ctl_st, k, ("A-groups", N, s))
        assert paired + alone + absorbed == series * calls and paired <= absorbed <= 3 * paired, (paired, alone, absorbed)
        assert full > 0, (paired, alone, absorbed)                 # (some pass served four calls, decoys on both sides of its rows)
    finally:
        a.close()
