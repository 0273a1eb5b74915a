"""Half rows (SMT_ROWS_F16: 256 binary16 values a row): store, embed and exact search against NumPy in float64 over the STORED
values, X.astype(float16).astype(float32).  Reference distance, reference top-k and the device-form call are the wide rows' test's."""
import functools

import numpy as np
import pytest

import semtools_amd as smt
from semtools_amd import _lib as L
from oracle import oracle_np
from tests.test_gpu_wide_rows import PAD, corpus_of, ref_dist, ref_topk, search_ex

pytestmark = pytest.mark.gpu
F16, F32 = np.float16, np.float32
F32_ERR_HALF = 4 * 20 / 2 ** 24   # half_rows.h


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def half_case(n):
    """corpus_of(256, n) -- duplicates, zero rows, a zero query -- with row 2 stored as subnormal halves only and query 2 next to it;
    returns (rows as given, rows as stored, queries)"""
    X, Q = (a.copy() for a in corpus_of(256, n))
    if n >= 3:
        X[2] = np.random.default_rng(n).uniform(-1, 1, 256).astype(F32) * F32(2.0 ** -15)
        Q[2] = X[2].astype(F16).astype(F32) * F32(2.0 ** 15) + F32(0.01) * Q[2]
    Xs = X.astype(F16).astype(F32)
    assert n < 3 or (np.abs(Xs[2]).max() < 2.0 ** -14 and np.abs(Xs[2]).max() > 0)
    return X, Xs, Q


def half_corpus(ctx, X):
    c = smt.Corpus(ctx, dtype=F16)
    c.append(X)
    return c


def test_store_bit_for_bit(gpu_ctx):
    import torch
    rng = np.random.default_rng(1)
    X = (rng.standard_normal((37, 256)) * 10.0 ** rng.integers(-8, 3, (37, 1))).astype(F32)   # down to rows that round to zeros
    X[5] = 0
    X[5, :8] = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65504, 65519.99, 2.0 ** -24, 1.5 * 2.0 ** -25, 2.0 ** -25, -0.0]
    ref = X.astype(F16)
    assert ref[5, :8].view(np.uint16).tolist() == [0x3C00, 0x3C02, 0x7BFF, 0x7BFF, 1, 1, 0, 0x8000]
    c = half_corpus(gpu_ctx, X)
    assert c.dtype == F16 and c.dim == 256 and np.array_equal(bits(c.read_rows(0, 37)), bits(ref))
    bad = X[:3].copy()
    bad[1, 7] = 65520
    for call in (lambda: c.append(bad), lambda: c.write_rows(4, bad)):
        with pytest.raises(L.SmtError) as e:
            call()
        assert e.value.code == L.SMT_E_INVALID and c.rows == 37 and np.array_equal(bits(c.read_rows(0, 37)), bits(ref))
    c.write_rows(3, X[10:12])
    c.truncate(20)
    assert c.append(X[30:33]) == 20 and c.rows == 23
    want = np.concatenate([ref[:3], ref[10:12], ref[5:20], ref[30:33]])
    assert np.array_equal(bits(c.read_rows(0, 23)), bits(want))
    t = torch.from_numpy(ref).cuda()
    d = smt.Corpus(gpu_ctx, device_ptr=t.data_ptr(), rows=37, dtype=F16)
    assert d.dtype == F16 and np.array_equal(bits(d.read_rows(0, 37)), bits(ref))
    t[3, 3] = float("inf")
    with pytest.raises(L.SmtError) as e:
        smt.Corpus(gpu_ctx, device_ptr=t.data_ptr(), rows=37, dtype=F16)
    assert e.value.code == L.SMT_E_INVALID
    c.close(); d.close()


@pytest.mark.parametrize("dtype", [F32, F16, np.int8])
def test_embed_into_a_half_corpus(gpu_ctx, dtype):
    rng = np.random.default_rng(256)   # (the inputs of test_gpu_wide_rows.py::test_embed_bit_for_bit at D = 256)
    V, max_tokens = 300, 20
    table = rng.integers(-127, 128, (V, 256)).astype(np.int8) if dtype == np.int8 else rng.standard_normal((V, 256)).astype(dtype)
    lens = [0, 1, 2, 17, max_tokens + 3, 5, 0, 17]
    lines = [rng.integers(0, V, n) for n in lens]
    lines[3][4] = V + 7
    ids = np.concatenate(lines).astype(np.uint32)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    ref = np.stack([oracle_np.pool_ids(table, l, True, max_tokens) for l in lines])
    m = smt.Model(gpu_ctx, table, normalize=True)
    c = half_corpus(gpu_ctx, ref[:1])
    emb, first = m.embed(ids, offsets, max_tokens=max_tokens, append_to=c)
    assert first == 1 and c.rows == 9 and np.array_equal(bits(emb), bits(ref))
    assert np.array_equal(bits(c.read_rows(1, 8)), bits(F16(ref)))
    c.close(); m.close()


def check_search(gpu_ctx, n, nq, k):
    X, Xs, Q = half_case(n)
    Q = Q[:nq]
    c = half_corpus(gpu_ctx, X)
    refs = [ref_topk(q, Xs, k) for q in Q]
    for (rows, dist), (rr, rd) in zip(c.search(Q, top_k=k), refs):
        assert len(rows) == min(k, n) and np.array_equal(rows, rr) and np.array_equal(dist.view(np.uint64), rd.view(np.uint64))
    base = 1000
    rows, dist, st = search_ex(gpu_ctx, c, Q, k, base)
    full = [ref_dist(q, Xs) for q in Q]
    for qi, (rr, rd) in enumerate(refs):
        m = int((rows[qi] != PAD).sum())
        assert (rows[qi, m:] == PAD).all() and np.isinf(dist[qi, m:]).all() and st[qi] in (L.STATUS_PROVED, L.STATUS_UNCERTAIN)
        if st[qi] == L.STATUS_PROVED:
            assert m == len(rr) and np.array_equal(rows[qi, :m], rr + np.uint64(base)) and np.array_equal(dist[qi, :m], rd)
        else:   # every returned pair is exact
            assert m == len(rr) and np.array_equal(dist[qi, :m], full[qi][(rows[qi, :m] - np.uint64(base)).astype(np.int64)])
    c.close()


@pytest.mark.parametrize("k", [1, 10, 56])
@pytest.mark.parametrize("nq", [1, 4, 5])
@pytest.mark.parametrize("n", [1, 2, 3, 9, 63, 4099])
def test_search_equals_f64_reference(gpu_ctx, n, nq, k):
    check_search(gpu_ctx, n, nq, k)


def test_search_with_two_blocks(gpu_ctx):
    gpu_ctx.set_tuning("scan_blocks", 2)   # waves take many steps each
    try:
        check_search(gpu_ctx, 4099, 5, 10)
    finally:
        gpu_ctx.set_tuning("scan_blocks", 0)


@pytest.mark.parametrize("k", [1, 10, 56])
def test_proved_where_it_must_be(gpu_ctx, k):
    rng = np.random.default_rng(4)
    u, v = rng.standard_normal((2, 256))
    u /= np.linalg.norm(u)
    v -= (v @ u) * u
    v /= np.linalg.norm(v)
    d = 2e-3 * (1 + rng.permutation(200))   # a staircase of distances, rows in no order
    X = ((1 - d)[:, None] * u + np.sqrt(1 - (1 - d) ** 2)[:, None] * v).astype(F32)
    q = u.astype(F32)
    Xs = X.astype(F16).astype(F32)
    assert np.diff(np.sort(ref_dist(q, Xs))).min() >= 1e-3 > 100 * 2 * F32_ERR_HALF
    c = half_corpus(gpu_ctx, X)
    gpu_ctx.uncertain_count(reset=True)
    rows, dist, st = search_ex(gpu_ctx, c, q[None], k, 0)
    rr, rd = ref_topk(q, Xs, k)
    assert st[0] == L.STATUS_PROVED and gpu_ctx.uncertain_count(reset=True) == 0
    assert np.array_equal(rows[0], rr) and np.array_equal(dist[0], rd)
    c.close()


def test_ranges_and_workspace_mode(gpu_ctx):
    X, _, Q = half_case(4099)
    X = X.copy()
    q = Q[1]
    X[9] = q   # the best row of the corpus, one row in front of a range
    Xs = X.astype(F16).astype(F32)
    c = half_corpus(gpu_ctx, X)
    ranges = [(3, 3), (5, 6), (10, 1027), (1501, 1510), (1600, 1607), (2000, 2000), (3001, 3004)]   # odd begins, odd ends
    allowed = np.concatenate([np.arange(b, e) for b, e in ranges])
    rr, rd = ref_topk(q, Xs, 10, allowed)
    rows, dist = c.search(q, top_k=10, ranges=ranges)[0]
    assert 9 not in rows.tolist() and np.array_equal(rows, rr) and np.array_equal(dist, rd)
    assert c.search(q, top_k=10)[0][0][0] == 9
    for nq in (4, 5):   # the four-slot kernel inside ranges
        for (rows, dist), qq in zip(c.search(Q[:nq], top_k=10, ranges=ranges), Q[:nq]):
            r2, d2 = ref_topk(qq, Xs, 10, allowed)
            assert np.array_equal(rows, r2) and np.array_equal(dist, d2)
    rows, dist = c.search(q, top_k=3, ranges=[(5, 6)], row_base=7)[0]
    assert rows.tolist() == [12] and dist.tolist() == [ref_dist(q, Xs[5:6])[0]]
    assert len(c.search(q, top_k=3, ranges=[(8, 8)])[0][0]) == 0
    md = float(rd[4] + rd[5]) / 2   # a max_distance that cuts the list mid-way (score > 1 - max_distance, the threshold an f32)
    keep = int(((1.0 - rd) > float(F32(1.0) - F32(md))).sum())
    assert 0 < keep < 10
    rows, dist = c.search(q, top_k=10, max_distance=md, mode=L.MODE_WORKSPACE, ranges=ranges)[0]
    assert np.array_equal(rows, rr[:keep]) and np.array_equal(dist, rd[:keep])
    assert len(c.search(q, top_k=0, mode=L.MODE_WORKSPACE, ranges=ranges)[0][0]) == 0
    zrows, zdist = c.search(np.zeros(256, F32), top_k=4, mode=L.MODE_WORKSPACE, ranges=ranges)[0]
    assert zrows.tolist() == [5, 10, 11, 12] and zdist.tolist() == [1.0] * 4
    c.close()


def test_near_ties_past_the_guard_band(gpu_ctx):
    rng = np.random.default_rng(5)
    X = rng.standard_normal((580, 256)).astype(F32)
    b = (X[0] / np.linalg.norm(X[0])).astype(F16)
    where = rng.permutation(580)[:80]
    for i, r in enumerate(where):   # 80 rows, one step of the half grid of one component apart
        X[r] = b
        X[r, 3 * i] = np.nextafter(b[3 * i], F16(np.inf))
    Xs = X.astype(F16).astype(F32)
    assert np.array_equal(Xs[where], X[where])
    q = b.astype(F32)
    c = half_corpus(gpu_ctx, X)
    rr, rd = ref_topk(q, Xs, 10)
    rows, dist = c.search(q, top_k=10)[0]
    assert np.array_equal(rows, rr) and np.array_equal(dist, rd)
    gpu_ctx.uncertain_count(reset=True)
    _, _, st = search_ex(gpu_ctx, c, q[None], 10, 0)
    assert (st[0] != L.STATUS_PROVED) == (gpu_ctx.uncertain_count(reset=True) == 1)
    c.close()


def test_refusals(gpu_ctx, tmp_path):
    X, Xs, Q = half_case(63)
    c = half_corpus(gpu_ctx, X)
    f = smt.Corpus(gpu_ctx)
    f.append(X)
    before = f.search(Q[0], top_k=5)[0]
    refused = [lambda: c.search(Q[0], top_k=3, max_distance=0.5), lambda: c.search(Q[0], top_k=57),
               lambda: search_ex(gpu_ctx, c, Q[:1], 57, 0), lambda: c.prepack(), lambda: c.compact([(0, 2)]),
               lambda: c.save(tmp_path / "a.smt"), lambda: c.append_to_file(tmp_path / "a.smt", 0),
               lambda: smt.IvfPq(c, nlist=32), lambda: smt.IvfPq.load(c, tmp_path / "none.ivf"),
               lambda: c.debug_scan_lists(Q[:1], 3), lambda: c.image_tile(0), lambda: smt.Corpus(gpu_ctx, dim=512, dtype=F16)]
    for call in refused:
        with pytest.raises(L.SmtError) as e:
            call()
        assert e.value.code == L.SMT_E_UNSUPPORTED and "half rows" in str(e.value), str(e.value)
    assert not (tmp_path / "a.smt").exists()
    with pytest.raises(L.SmtError) as e:
        smt.Corpus(gpu_ctx, dtype=7)
    assert e.value.code == L.SMT_E_INVALID
    rr, rd = ref_topk(Q[0], Xs, 5)
    rows, dist = c.search(Q[0], top_k=5)[0]
    assert np.array_equal(rows, rr) and np.array_equal(dist, rd) and c.rows == 63
    after = f.search(Q[0], top_k=5)[0]
    assert f.dtype == F32 and np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    c.close(); f.close()
