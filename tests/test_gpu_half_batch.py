"""Half rows, batched route (batch_half.hip): the block lists of batch_half_kernel and the answers of calls of half_batch_min queries
and more against NumPy in float64 over the STORED values, X.astype(float16).astype(float32).

Largest |nominated - f64| seen by the list tests on an MI355X, per kind of row: profiles/half_batch.json ("max_nomination_error")."""
import numpy as np
import pytest

import semtools_amd as smt
from semtools_amd import _lib as L
from tests.nominate_ref import worst_case_rows_bf16x3
from tests.test_gpu_wide_batch import RANGES, check_lists
from tests.test_gpu_wide_rows import PAD, ref_dist, ref_topk, search_ex

pytestmark = pytest.mark.gpu
F16, F32 = np.float16, np.float32
BOUND = 1.2 * (33 * 2.0 ** -22 + 1e-6)   # f32_err_batch_half (half_rows.h)
BATCH_MIN = 8                            # set explicitly: no case depends on the measured default ...
DEFAULT_MIN = 4                          # ... of tuning key half_batch_min (common.h), which the session's context gets back


@pytest.fixture
def ctx(gpu_ctx):
    gpu_ctx.set_tuning("half_batch_min", BATCH_MIN)
    try:
        yield gpu_ctx
    finally:
        gpu_ctx.set_tuning("half_batch_min", DEFAULT_MIN)
        gpu_ctx.set_tuning("scan_blocks", 0)


def half_corpus(ctx, X):
    c = smt.Corpus(ctx, dtype=F16)
    c.append(X)
    return c


def calls(ctx, fn):
    """fn() with profiling on: (its result, batch_half launches, scan_half launches)"""
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        out = fn()
        return out, ctx.prof_read("batch_half")[0], ctx.prof_read("scan_half")[0]
    finally:
        ctx.prof_enable(False)


@pytest.mark.parametrize("blocks,top_k", [(1, 56), (2, 1)])     # k' = 64 and 9
@pytest.mark.parametrize("n", [1, 31, 33, 577])
def test_block_lists_against_f64(ctx, n, blocks, top_k):
    rng = np.random.default_rng(7 * 256 + n)
    X = rng.standard_normal((n, 256)).astype(F32)
    Q = rng.standard_normal((33, 256)).astype(F32)
    Q[0] = X[0] + 0.05 * Q[0]
    Q[2] = 0
    if n >= 31:
        X[2] = rng.uniform(-1, 1, 256).astype(F32) * F32(2.0 ** -15)   # stored as subnormal halves only (half_case)
        X[5] = 0
        X[7] /= np.linalg.norm(X[7])
        X[7, :8] = rng.uniform(-1, 1, 8).astype(F32) * F32(2.0 ** -15)   # a unit row with eight subnormal components
        X[9] *= F32(500.0) / np.abs(X[9]).max() * F32(2.0 ** 7)          # the largest component: 64000
        X[20] = X[3]
        X[n - 1] = X[3]
        X[min(31, n - 1)] = X[3]                                         # a tile's last row
    if n >= 577:
        X[300:303] = X[3]
        X[544] = 0
    Xs = X.astype(F16).astype(F32)
    assert np.isfinite(Xs).all()
    if n >= 31:
        assert 0 < np.abs(Xs[2]).max() < 2.0 ** -14 and 0 < np.abs(Xs[7, :8]).max() < 2.0 ** -14 and np.abs(Xs[9]).max() > 60000
        Q[3] = Xs[2] * F32(2.0 ** 15) + F32(0.01) * Q[3]
        Q[4] = Xs[9] + Q[4]
        Q[5] = Xs[7] + F32(0.01) * Q[5]
    c = half_corpus(ctx, X)
    ctx.set_tuning("scan_blocks", blocks)
    got = [(nq, c.debug_batch_half_lists(Q[:nq], top_k)) for nq in (1, 33)]
    c.close()
    nb = min(blocks, (n + 255) // 256)
    worst = max(check_lists(keys, Xs, Q[:nq], nb, min(64, top_k + 8), BOUND) for nq, keys in got)
    print(f"max nomination error n={n} blocks={blocks}: {worst:.3e} (bound {BOUND:.3e})")
    if n >= 31:   # the subnormal row against its own query, alone: what the MFMA did with subnormal inputs
        keys = got[1][1][3]
        d32 = (keys[keys & np.uint64(0xFFFFFFFF) == 2] >> np.uint64(32)).astype(np.uint32).view(F32)
        print(f"subnormal row: nominated {d32}, exact {ref_dist(Q[3], Xs[2:3])[0]:.3e}")


@pytest.mark.parametrize("direct", [0, 1])   # both row paths of the kernel (tuning key half_batch_direct)
def test_worst_case_rows(ctx, direct):
    X = worst_case_rows_bf16x3(np.random.default_rng(11 * 256), 33).astype(F32)
    Xs = X.astype(F16).astype(F32)
    c = half_corpus(ctx, X)
    ctx.set_tuning("scan_blocks", 1)
    ctx.set_tuning("half_batch_direct", direct)
    try:
        keys = c.debug_batch_half_lists(Xs, 56)
        ctx.set_tuning("scan_blocks", 0)
        res = c.search(Xs, top_k=3)
    finally:
        ctx.set_tuning("half_batch_direct", 0)
    worst = check_lists(keys, Xs, Xs, 1, 64, BOUND)
    print(f"worst-case rows: {worst:.3e} (bound {BOUND:.3e})")
    for q, (rows, dist) in zip(Xs, res):
        rr, rd = ref_topk(q, Xs, 3)
        assert np.array_equal(rows, rr) and np.array_equal(dist.view(np.uint64), rd.view(np.uint64))
    c.close()


@pytest.mark.parametrize("ranged", [False, True])
@pytest.mark.parametrize("k", [1, 56])
@pytest.mark.parametrize("shape", [(4099, 8), (577, 33), (577, 129), (63, 8)])   # 129 queries: a pass and more
def test_answers_equal_f64_reference(ctx, shape, k, ranged):
    n, nq = shape
    rng = np.random.default_rng(256 + n)
    X = rng.standard_normal((n, 256)).astype(F32)
    Q = rng.standard_normal((nq, 256)).astype(F32)
    Xs = X.astype(F16).astype(F32)
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
    c = half_corpus(ctx, X)
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


def test_near_ties_rerun_through_the_scan(ctx):
    rng = np.random.default_rng(5)                          # the corpus of test_gpu_half_rows.py::test_near_ties_past_the_guard_band
    X = rng.standard_normal((580, 256)).astype(F32)
    b = (X[0] / np.linalg.norm(X[0])).astype(F16)
    for i, r in enumerate(rng.permutation(580)[:80]):       # 80 rows, one step of the half grid of one component apart
        X[r] = b
        X[r, 3 * i] = np.nextafter(b[3 * i], F16(np.inf))
    Xs = X.astype(F16).astype(F32)
    q = b.astype(F32)
    c = half_corpus(ctx, X)
    rr, rd = ref_topk(q, Xs, 10)
    res, n_batch, n_scan = calls(ctx, lambda: c.search(np.tile(q, (8, 1)), top_k=10))
    assert n_batch > 0 and n_scan > 0                       # unproved by the batched route: run again through the scan
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
    c = half_corpus(ctx, X)
    assert calls(ctx, lambda: c.search(Q[:BATCH_MIN - 1], top_k=3))[1:] == (0, 2)   # passes of four
    assert calls(ctx, lambda: c.search(Q, top_k=3))[1:] == (1, 0)
    ctx.set_tuning("half_batch_min", 0)
    assert calls(ctx, lambda: c.search(Q, top_k=3))[1:] == (0, 2)
    ctx.set_tuning("half_batch_min", BATCH_MIN)
    c.close()
    for D in (256, 512):   # f32 rows never take it
        f = smt.Corpus(ctx, dim=D)
        f.append(rng.standard_normal((577, D)).astype(F32))
        assert calls(ctx, lambda: f.search(rng.standard_normal((BATCH_MIN, D)).astype(F32), top_k=3))[1] == 0
        f.close()
