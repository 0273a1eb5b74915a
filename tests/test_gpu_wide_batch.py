"""Wide rows, batched route (batch_slab.hip): the block lists of batch_slab_kernel and the answers of calls of slab_batch_min queries
and more against the float64 reference of test_gpu_wide_rows.py.

Largest |nominated - f64| seen by the list tests on an MI355X: see profiles/wide_batch.json ("max_nomination_error")."""
import numpy as np
import pytest

import semtools_amd as smt
from semtools_amd import _lib as L
from tests.nominate_ref import worst_case_rows_bf16x3
from tests.test_gpu_wide_rows import DIMS, PAD, ref_dist, ref_topk, search_ex

pytestmark = pytest.mark.gpu
KEY_PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
GUARD = np.uint64(0x5A5A5A5A5A5A5A5A)
BATCH_MIN = 8                                   # the default of tuning key slab_batch_min
RANGES = [(3, 3), (5, 6), (10, 1027), (2000, 2000), (3001, 3004)]   # of test_ranges_and_workspace_mode


def bound(D):   # f32_err_batch_slab (wide_rows.h)
    return 1.2 * (3 * 2.0 ** -16 + 48 * (D // 256) * 2.0 ** -22 + 1e-6)


def qb(D):
    return 64 if D == 512 else 32


def check_lists(keys, X, Q, blocks, kp, err):
    """every property of the block lists [nq + 1][blocks][k'] against float64; returns the largest nomination error"""
    nq, n = len(Q), len(X)
    assert keys.shape == (nq + 1, blocks, kp) and (keys[nq] == GUARD).all()
    owner = (np.arange(n) // 32) % (blocks * 8) // 8          # tiles are dealt to the launch's waves round robin, 8 waves a block
    worst = 0.0
    for qi in range(nq):
        d64 = ref_dist(Q[qi], X)
        seen = []
        for b in range(blocks):
            lst = keys[qi, b]
            m = int((lst != KEY_PAD).sum())
            assert (lst[m:] == KEY_PAD).all() and (lst[1:m] > lst[:m - 1]).all(), (qi, b)
            rows = (lst[:m] & np.uint64(0xFFFFFFFF)).astype(np.int64)
            d32 = (lst[:m] >> np.uint64(32)).astype(np.uint32).view(np.float32).astype(np.float64)
            assert len(set(rows.tolist())) == m and (owner[rows] == b).all(), (qi, b)
            e = np.abs(d32 - d64[rows]).max() if m else 0.0
            worst = max(worst, float(e))
            assert e <= err, (qi, b, e)
            mine = np.flatnonzero(owner == b)
            must = mine if m < kp else mine[d64[mine] < d32[-1] - err]   # a short list holds every row of its block
            assert set(must.tolist()) <= set(rows.tolist()), (qi, b)
            seen += rows.tolist()
        assert len(seen) == len(set(seen)), qi
    return worst


@pytest.mark.parametrize("blocks,top_k", [(1, 56), (2, 1)])     # k' = 64 and 9
@pytest.mark.parametrize("n", [1, 31, 33, 577])
@pytest.mark.parametrize("D", DIMS)
def test_block_lists_against_f64(gpu_ctx, D, n, blocks, top_k):
    rng = np.random.default_rng(7 * D + n)
    X = rng.standard_normal((n, D)).astype(np.float32)
    Q = rng.standard_normal((33, D)).astype(np.float32)
    Q[0] = X[0] + 0.05 * Q[0]
    Q[2] = 0
    if n >= 31:
        X[5] = 0
        X[20] = X[3]
        X[n - 1] = X[3]
    if n >= 577:
        X[300:303] = X[3]
        X[544] = 0
    c = smt.Corpus(gpu_ctx, dim=D)
    c.append(X)
    gpu_ctx.set_tuning("scan_blocks", blocks)
    try:
        got = [(nq, c.debug_batch_slab_lists(Q[:nq], top_k)) for nq in (1, 33)]
    finally:
        gpu_ctx.set_tuning("scan_blocks", 0)
        c.close()
    nb = min(blocks, (n + 255) // 256)
    worst = max(check_lists(keys, X, Q[:nq], nb, min(64, top_k + 8), bound(D)) for nq, keys in got)
    print(f"max nomination error D={D} n={n} blocks={blocks}: {worst:.3e} (bound {bound(D):.3e})")


def batch_calls(ctx, fn):
    """fn() with profiling on: (its result, batch_slab launches, scan_slab launches)"""
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        out = fn()
        return out, ctx.prof_read("batch_slab")[0], ctx.prof_read("scan_slab")[0]
    finally:
        ctx.prof_enable(False)


@pytest.mark.parametrize("ranged", [False, True])
@pytest.mark.parametrize("k", [1, 56])
@pytest.mark.parametrize("shape", [(4099, 8), (577, 33), (577, 0), (63, 8)])   # nq 0: a pass and one query, QB + 1
@pytest.mark.parametrize("D", DIMS)
def test_answers_equal_f64_reference(gpu_ctx, D, shape, k, ranged):
    n, nq = shape[0], shape[1] or qb(D) + 1
    rng = np.random.default_rng(D + n)
    X = rng.standard_normal((n, D)).astype(np.float32)
    Q = rng.standard_normal((nq, D)).astype(np.float32)
    ranges = [(min(b, n), min(e, n)) for b, e in RANGES] if ranged else None
    allowed = np.concatenate([np.arange(b, e) for b, e in ranges]) if ranged else np.arange(n)
    dist = [ref_dist(q, X[allowed]) for q in Q]
    refs = []
    for d in dist:
        order = np.lexsort((allowed, d))
        s = d[order]
        kp = min(64, k + 8)
        if len(s) > kp:   # the precondition: no query needs the fallback (the k-th and k'-th distances lie two bounds apart)
            assert s[kp - 1] - s[min(k, len(s)) - 1] > 2 * bound(D)
        refs.append((allowed[order[:k]].astype(np.uint64), s[:k]))
    c = smt.Corpus(gpu_ctx, dim=D)
    c.append(X)
    gpu_ctx.uncertain_count(reset=True)
    res, n_batch, _ = batch_calls(gpu_ctx, lambda: c.search(Q, top_k=k, ranges=ranges))
    assert n_batch > 0 and gpu_ctx.uncertain_count(reset=True) == 0
    for (rows, dd), (rr, rd) in zip(res, refs):
        assert np.array_equal(rows, rr) and np.array_equal(dd.view(np.uint64), rd.view(np.uint64))
    if not ranged:
        (rows, dd, st), n_batch, _ = batch_calls(gpu_ctx, lambda: search_ex(gpu_ctx, c, Q, k, 1000))
        assert n_batch > 0 and (st == L.STATUS_PROVED).all()
        for qi, (rr, rd) in enumerate(refs):
            m = len(rr)
            assert np.array_equal(rows[qi, :m], rr + np.uint64(1000)) and np.array_equal(dd[qi, :m].view(np.uint64), rd.view(np.uint64))
            assert (rows[qi, m:] == PAD).all() and np.isinf(dd[qi, m:]).all()
    c.close()


@pytest.mark.parametrize("D", DIMS)
def test_near_ties_rerun_through_the_scan(gpu_ctx, D):
    rng = np.random.default_rng(5 * D)                      # the corpus of test_near_ties_past_the_guard_band
    X = rng.standard_normal((580, D)).astype(np.float32)
    b = X[0] / np.linalg.norm(X[0])
    for i, r in enumerate(rng.permutation(580)[:80]):       # 80 rows, one ulp of one component apart
        X[r] = b
        X[r, 3 * i] = np.nextafter(b[3 * i], np.float32(np.inf))
    Q = np.tile(b, (8, 1))
    c = smt.Corpus(gpu_ctx, dim=D)
    c.append(X)
    rr, rd = ref_topk(b, X, 10)
    res, n_batch, n_scan = batch_calls(gpu_ctx, lambda: c.search(Q, top_k=10))
    assert n_batch > 0 and n_scan > 0                       # unproved by the batched route: run again through the scan
    for rows, dist in res:
        assert np.array_equal(rows, rr) and np.array_equal(dist, rd)
    gpu_ctx.uncertain_count(reset=True)
    _, _, st = search_ex(gpu_ctx, c, Q, 10, 0)
    assert int((st != L.STATUS_PROVED).sum()) == gpu_ctx.uncertain_count(reset=True)
    c.close()


@pytest.mark.parametrize("D", DIMS)
def test_worst_case_rows(gpu_ctx, D):
    S, n = D // 256, 33
    rng = np.random.default_rng(11 * D)
    X = (np.concatenate([worst_case_rows_bf16x3(rng, n) for _ in range(S)], axis=1) / np.sqrt(S)).astype(np.float32)
    c = smt.Corpus(gpu_ctx, dim=D)
    c.append(X)
    gpu_ctx.set_tuning("scan_blocks", 1)
    try:
        keys = c.debug_batch_slab_lists(X, 56)
    finally:
        gpu_ctx.set_tuning("scan_blocks", 0)
    worst = check_lists(keys, X, X, 1, 64, bound(D))
    print(f"worst-case rows D={D}: {worst:.3e} (bound {bound(D):.3e})")
    for q, (rows, dist) in zip(X, c.search(X, top_k=3)):
        rr, rd = ref_topk(q, X, 3)
        assert np.array_equal(rows, rr) and np.array_equal(dist.view(np.uint64), rd.view(np.uint64))
    c.close()


def test_below_the_border_nothing_changes(gpu_ctx):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((577, 512)).astype(np.float32)
    Q = rng.standard_normal((BATCH_MIN, 512)).astype(np.float32)
    c = smt.Corpus(gpu_ctx, dim=512)
    c.append(X)
    assert batch_calls(gpu_ctx, lambda: c.search(Q[:BATCH_MIN - 1], top_k=3))[1:] == (0, 2)   # passes of four
    assert batch_calls(gpu_ctx, lambda: c.search(Q, top_k=3))[1:] == (1, 0)
    gpu_ctx.set_tuning("slab_batch_min", 0)
    try:
        assert batch_calls(gpu_ctx, lambda: c.search(Q, top_k=3))[1:] == (0, 2)
    finally:
        gpu_ctx.set_tuning("slab_batch_min", BATCH_MIN)
        c.close()
