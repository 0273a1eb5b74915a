"""Byte rows, batched route (batch_byte.hip): the block lists of batch_byte_kernel and the answers of calls of byte_batch_min queries
and more against NumPy in float64 over the STORED integers.

Largest |nominated - f64| seen by the list tests on an MI355X: profiles/byte_batch.json ("max_nomination_error")."""
import numpy as np
import pytest

import semtools_amd as smt
from semtools_amd import _lib as L
from tests.test_gpu_byte_rows import adopted, byte_corpus, extreme_rows, quant
from tests.test_gpu_wide_batch import RANGES, check_lists
from tests.test_gpu_wide_rows import PAD, ref_dist, ref_topk, search_ex

pytestmark = pytest.mark.gpu
F32 = np.float32
BOUND = 1.2 * (2.0 ** -19 + 1e-6)   # f32_err_batch_byte (byte_rows.h)
BATCH_MIN = 8                       # set explicitly: no case depends on the measured default ...
DEFAULT_MIN = 4                     # ... of tuning key byte_batch_min (common.h), which the session's context gets back


@pytest.fixture
def ctx(gpu_ctx):
    gpu_ctx.set_tuning("byte_batch_min", BATCH_MIN)
    try:
        yield gpu_ctx
    finally:
        gpu_ctx.set_tuning("byte_batch_min", DEFAULT_MIN)
        gpu_ctx.set_tuning("scan_blocks", 0)


def calls(ctx, fn):
    """fn() with profiling on: (its result, batch_byte launches, scan_byte launches)"""
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        out = fn()
        return out, ctx.prof_read("batch_byte")[0], ctx.prof_read("scan_byte")[0]
    finally:
        ctx.prof_enable(False)


def special_queries(Q, neg_row):
    Q[2] = 0
    Q[3] = 0; Q[3, 77] = -3.0                                   # one-hot: the top digit reaches 64
    Q[4] = 0.25                                                 # all equal: 2^22 / 16 = 2^18, both lower digits zero
    Q[5] = np.where(np.arange(256) == 9, 1.0, 1e-7 * Q[5])      # components near 1e-7 beside a large one: top digits zero
    Q[6] = neg_row
    return Q


@pytest.mark.parametrize("blocks,top_k", [(1, 56), (2, 1)])     # k' = 64 and 9
@pytest.mark.parametrize("n", [1, 31, 33, 577])
def test_block_lists_against_f64(ctx, n, blocks, top_k):
    rng = np.random.default_rng(7 * 256 + n)
    X = rng.standard_normal((n, 256)).astype(F32)
    Q = rng.standard_normal((33, 256)).astype(F32)
    Q[0] = X[0] + 0.05 * Q[0]
    special_queries(Q, np.full(256, 128.0, F32))
    if n >= 31:
        X[5] = 0
        X[20] = X[3]
        X[n - 1] = X[3]
        X[min(31, n - 1)] = X[3]                                # a tile's last row
    if n >= 577:
        X[300:303] = X[3]
        X[544] = 0
    Xs = quant(X).astype(F32)
    ctx.set_tuning("scan_blocks", blocks)
    c = byte_corpus(ctx, X)
    got = [(Xs, nq, c.debug_batch_byte_lists(Q[:nq], top_k)) for nq in (1, 33)]
    c.close()
    q8 = np.resize(extreme_rows(), (n, 256))                    # the same shape adopted, with the extreme rows (-128s) from 31 rows on
    a, _t = adopted(ctx, q8)
    got += [(q8.astype(F32), 33, a.debug_batch_byte_lists(Q, top_k))]
    a.close()
    nb = min(blocks, (n + 255) // 256)
    worst = max(check_lists(keys, rows, Q[:nq], nb, min(64, top_k + 8), BOUND) for rows, nq, keys in got)
    print(f"max nomination error n={n} blocks={blocks}: {worst:.3e} (bound {BOUND:.3e})")


@pytest.mark.parametrize("ranged", [False, True])
@pytest.mark.parametrize("k", [1, 56])
@pytest.mark.parametrize("shape", [(4099, 8), (577, 33), (577, 129), (63, 8)])   # 129 queries: a pass and more
def test_answers_equal_f64_reference(ctx, shape, k, ranged):
    n, nq = shape
    rng = np.random.default_rng(256 + n)
    X = rng.standard_normal((n, 256)).astype(F32)
    Q = rng.standard_normal((nq, 256)).astype(F32)
    Xs = quant(X).astype(F32)
    ranges = [(min(b, n), min(e, n)) for b, e in RANGES] if ranged else None
    allowed = np.concatenate([np.arange(b, e) for b, e in ranges]) if ranged else np.arange(n)
    refs = []
    for q in Q:
        d = ref_dist(q, Xs[allowed])
        order = np.lexsort((allowed, d))
        s = d[order]
        kp = min(64, k + 8)
        if len(s) > kp:   # the precondition: no query needs the fallback (the k-th and k'-th distances lie two bounds apart)
            assert s[kp - 1] - s[min(k, len(s)) - 1] > 2 * BOUND
        refs.append((allowed[order[:k]].astype(np.uint64), s[:k]))
    c = byte_corpus(ctx, X)
    ctx.uncertain_count(reset=True)
    res, n_batch, _ = calls(ctx, lambda: c.search(Q, top_k=k, ranges=ranges))
    assert n_batch > 0 and ctx.uncertain_count(reset=True) == 0
    for (rows, dd), (rr, rd) in zip(res, refs):
        assert np.array_equal(rows, rr) and np.array_equal(dd.view(np.uint64), rd.view(np.uint64))
    if not ranged:
        (rows, dd, st), n_batch, _ = calls(ctx, lambda: search_ex(ctx, c, Q, k, 1000))
        assert n_batch > 0 and (st == L.STATUS_PROVED).all()
        for qi, (rr, rd) in enumerate(refs):
            m = len(rr)
            assert np.array_equal(rows[qi, :m], rr + np.uint64(1000)) and np.array_equal(dd[qi, :m].view(np.uint64), rd.view(np.uint64))
            assert (rows[qi, m:] == PAD).all() and np.isinf(dd[qi, m:]).all()
    c.close()


def test_near_ties(ctx):
    rng = np.random.default_rng(5)                          # the corpus of test_gpu_byte_rows.py::test_equal_rows_past_the_guard_band
    X = rng.standard_normal((580, 256)).astype(F32)
    where = rng.permutation(580)[:80]
    X[where] = X[0] * F32(2.0) ** rng.integers(-3, 4, (80, 1)).astype(F32)   # 80 rows of one direction: equal stored bytes
    Xs = quant(X).astype(F32)
    assert (Xs[where] == Xs[0]).all()
    q = X[0]
    c = byte_corpus(ctx, X)
    rr, rd = ref_topk(q, Xs, 10)
    res, n_batch, n_scan = calls(ctx, lambda: c.search(np.tile(q, (8, 1)), top_k=10))
    assert n_batch > 0 and n_scan == 0                      # the scan's bound is the wider one: nothing runs again through it
    for rows, dist in res:
        assert np.array_equal(rows, rr) and np.array_equal(dist, rd)
    ctx.uncertain_count(reset=True)
    _, _, st = search_ex(ctx, c, np.tile(q, (8, 1)), 10, 0)
    assert int((st != L.STATUS_PROVED).sum()) == ctx.uncertain_count(reset=True)
    c.close()


def test_the_border(ctx):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((577, 256)).astype(F32)
    Q = rng.standard_normal((BATCH_MIN, 256)).astype(F32)
    c = byte_corpus(ctx, X)
    assert calls(ctx, lambda: c.search(Q[:BATCH_MIN - 1], top_k=3))[1:] == (0, 2)   # passes of four
    assert calls(ctx, lambda: c.search(Q, top_k=3))[1:] == (1, 0)
    ctx.set_tuning("byte_batch_min", 0)
    assert calls(ctx, lambda: c.search(Q, top_k=3))[1:] == (0, 2)
    ctx.set_tuning("byte_batch_min", BATCH_MIN)
    c.close()
    for kw in ({"dtype": np.float16}, {}):   # half corpora and f32 corpora never take it
        f = smt.Corpus(ctx, **kw)
        f.append(X)
        assert calls(ctx, lambda: f.search(Q, top_k=3))[1] == 0
        f.close()
