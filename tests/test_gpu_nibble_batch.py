"""Nibble rows, batched route (batch_nibble.hip): the block lists of batch_nibble_kernel and the answers of calls of nibble_batch_min
queries and more against NumPy in float64 over the STORED integers.

Largest |nominated - f64| seen by the list tests on an MI355X: profiles/nibble_batch.json ("max_nomination_error")."""
import numpy as np
import pytest

import semtools_amd as smt
from semtools_amd import _lib as L
from tests.test_gpu_nibble_rows import adopted, extreme_rows, nibble_corpus, quant
from tests.test_gpu_wide_batch import RANGES, check_lists
from tests.test_gpu_wide_rows import PAD, ref_dist, ref_topk, search_ex

pytestmark = pytest.mark.gpu
F32 = np.float32
BOUND = 1.2 * (2.0 ** -19 + 1e-6)   # f32_err_batch_nibble (nibble_rows.h)
BATCH_MIN = 8                       # set explicitly: no case depends on the measured default ...
DEFAULT_MIN = 4                     # ... of tuning key nibble_batch_min (common.h), which the session's context gets back


@pytest.fixture
def ctx(gpu_ctx):
    gpu_ctx.set_tuning("nibble_batch_min", BATCH_MIN)
    try:
        yield gpu_ctx
    finally:
        gpu_ctx.set_tuning("nibble_batch_min", DEFAULT_MIN)
        gpu_ctx.set_tuning("scan_blocks", 0)


def calls(ctx, fn):
    """fn() with profiling on: (its result, batch_nibble launches, scan_nibble launches)"""
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        out = fn()
        return out, ctx.prof_read("batch_nibble")[0], ctx.prof_read("scan_nibble")[0]
    finally:
        ctx.prof_enable(False)


@pytest.mark.parametrize("blocks,top_k", [(1, 56), (2, 1)])     # k' = 64 and 9
@pytest.mark.parametrize("n", [1, 7, 9, 31, 33, 577])           # either side of a load (8 rows) and of a tile (32); many tiles, ragged
def test_block_lists_against_f64(ctx, n, blocks, top_k):
    rng = np.random.default_rng(4 * 256 + n)
    X = rng.standard_normal((n, 256)).astype(F32)
    Q = rng.standard_normal((33, 256)).astype(F32)
    Q[0] = X[0] + 0.05 * Q[0]
    Q[2] = 0
    Q[3] = 0; Q[3, 77] = -3.0                                   # one-hot: the top digit reaches 64
    Q[4] = 0.25                                                 # all equal: 2^22 / 16 = 2^18, both lower digits zero
    Q[5] = np.where(np.arange(256) == 9, 1.0, 1e-7 * Q[5])      # components near 1e-7 beside a large one: top digits zero
    Q[6] = 8.0                                                  # against the adopted row of -8s: every product at its extreme
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
    c = nibble_corpus(ctx, X)
    got = [(Xs, nq, c.debug_batch_nibble_lists(Q[:nq], top_k)) for nq in (1, 33)]
    c.close()
    q4 = np.resize(extreme_rows(), (n, 256))                    # the same shape adopted, with the extreme rows (-8s)
    a, _t = adopted(ctx, q4)
    got += [(q4.astype(F32), 33, a.debug_batch_nibble_lists(Q, top_k))]
    a.close()
    nb = min(blocks, (n + 255) // 256)
    worst = max(check_lists(keys, rows, Q[:nq], nb, min(64, top_k + 8), BOUND) for rows, nq, keys in got)
    print(f"max nomination error n={n} blocks={blocks}: {worst:.3e} (bound {BOUND:.3e})")


def test_the_order_of_the_nibbles(ctx):
    """row r = 7 e_r (the last: -8 e_255) against 256 one-hot queries: any disagreement between the rows' unpack order and the query
    image -- odd or even nibble, the end of a dword, of a unit, of a row -- sends some query to another row"""
    q4 = (7 * np.eye(256)).astype(np.int8)
    q4[255, 255] = -8
    Q = np.eye(256, dtype=F32)
    Q[255, 255] = -1
    c, _t = adopted(ctx, q4)
    (rows, dist, st), n_batch, n_scan = calls(ctx, lambda: search_ex(ctx, c, Q, 1, 0))
    assert (n_batch, n_scan) == (2, 0)
    assert np.array_equal(rows[:, 0], np.arange(256, dtype=np.uint64)) and (dist == 0.0).all() and (st == L.STATUS_PROVED).all()
    c.close()


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
    c = nibble_corpus(ctx, X)
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
    rng = np.random.default_rng(5)
    X = rng.standard_normal((580, 256)).astype(F32)
    where = rng.permutation(580)[:80]
    X[where] = X[0] * F32(2.0) ** rng.integers(-3, 4, (80, 1)).astype(F32)   # 80 rows of one direction: equal stored nibbles
    Xs = quant(X).astype(F32)
    assert (Xs[where] == Xs[0]).all()
    q = X[0]
    c = nibble_corpus(ctx, X)
    rr, rd = ref_topk(q, Xs, 10)
    res, n_batch, n_scan = calls(ctx, lambda: c.search(np.tile(q, (8, 1)), top_k=10))
    assert n_batch > 0 and n_scan == 0                      # the scan's bound is no tighter: nothing runs again through it
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
    c = nibble_corpus(ctx, X)
    assert calls(ctx, lambda: c.search(Q[:BATCH_MIN - 1], top_k=3))[1:] == (0, 2)   # passes of four
    assert calls(ctx, lambda: c.search(Q, top_k=3))[1:] == (1, 0)
    ctx.set_tuning("nibble_batch_min", 0)
    assert calls(ctx, lambda: c.search(Q, top_k=3))[1:] == (0, 2)
    ctx.set_tuning("nibble_batch_min", BATCH_MIN)
    c.close()
    for kw in ({"dtype": np.int8}, {"dtype": np.float16}, {}):   # byte, half and f32 corpora never take it
        f = smt.Corpus(ctx, **kw)
        f.append(X)
        assert calls(ctx, lambda: f.search(Q, top_k=3))[1] == 0
        f.close()
