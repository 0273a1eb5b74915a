"""Byte rows (SMT_ROWS_I8: 256 signed bytes a row): store, embed and exact search against NumPy in float64 over the STORED integers,
quant(X).astype(float32).  Reference distance, reference top-k and the device-form call are the wide rows' test's.
The largest |d32 - d64| of the scan's keys is not collected: no hook exposes them; f32_err_byte is DERIVED (byte_rows.h)."""
import functools

import numpy as np
import pytest

import semtools_amd as smt
from semtools_amd import _lib as L
from oracle import oracle_np
from tests.test_gpu_wide_rows import PAD, corpus_of, ref_dist, ref_topk, search_ex

pytestmark = pytest.mark.gpu
I8, F32 = np.int8, np.float32
F32_ERR_BYTE = 4 * 28 / 2 ** 24   # byte_rows.h


def quant(X):
    """the rounding rule of include/semtools_hip.h ("BYTE ROWS"), every array float32"""
    X = np.asarray(X, F32)
    amax = np.abs(X).max(1, keepdims=True)
    with np.errstate(divide="ignore"):
        s = np.where(amax > 0, F32(127) / amax, F32(0))
    return np.rint(X * s).astype(I8)


@functools.lru_cache(maxsize=None)
def byte_case(n):
    """corpus_of(256, n) -- duplicates, zero rows, a zero query; returns (rows as given, rows as stored, queries)"""
    X, Q = corpus_of(256, n)
    return X, quant(X).astype(F32), Q


def byte_corpus(ctx, X):
    c = smt.Corpus(ctx, dtype=I8)
    c.append(X)
    return c


def adopted(ctx, q8):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(q8)).cuda()
    return smt.Corpus(ctx, device_ptr=t.data_ptr(), rows=len(q8), dtype=I8), t


def extreme_rows():
    rng = np.random.default_rng(3)
    q8 = rng.integers(-128, 128, (21, 256)).astype(I8)
    q8[4] = -128
    q8[9] = np.where(np.arange(256) % 2 == 0, -128, 127)
    return q8


def test_store_bit_for_bit(gpu_ctx):
    rng = np.random.default_rng(1)
    X = (rng.standard_normal((37, 256)) * 10.0 ** rng.integers(-8, 3, (37, 1))).astype(F32)
    X[5:8] = 0                 # a zero row, a row with one component, a row with amax = 127 (s = 1) and ties
    X[6, 17] = -3.5
    X[7, :6] = [127, 0.5, 1.5, 2.5, -0.5, -2.5]
    ref = quant(X)
    assert not ref[5].any() and ref[6, 17] == -127 and ref[7, :6].tolist() == [127, 0, 2, 2, 0, -2] and ref.min() > -128
    c = byte_corpus(gpu_ctx, X)
    row_bytes = L.C.c_uint64()
    L.check(L.lib().smt_corpus_info(c._h, None, None, L.C.byref(row_bytes)))
    assert row_bytes.value == 256 and c.dtype == I8 and c.dim == 256 and np.array_equal(c.read_rows(0, 37), ref.astype(F32))
    bad = X[:3].copy()
    bad[1, 7] = np.nan
    for call in (lambda: c.append(bad), lambda: c.write_rows(4, bad)):
        with pytest.raises(L.SmtError) as e:
            call()
        assert e.value.code == L.SMT_E_INVALID and c.rows == 37 and np.array_equal(c.read_rows(0, 37), ref.astype(F32))
    c.write_rows(3, X[10:12])
    c.truncate(20)
    assert c.append(X[30:33] * F32(2.0 ** -9)) == 20 and c.rows == 23   # (a power of two changes no stored byte)
    want = np.concatenate([ref[:3], ref[10:12], ref[5:20], ref[30:33]])
    assert np.array_equal(c.read_rows(0, 23), want.astype(F32))
    d, _t = adopted(gpu_ctx, q8 := extreme_rows())
    assert d.dtype == I8 and np.array_equal(d.read_rows(0, 21), q8.astype(F32))
    c.close(); d.close()


@pytest.mark.parametrize("dtype", [F32, np.float16, I8])
def test_embed_into_a_byte_corpus(gpu_ctx, dtype):
    rng = np.random.default_rng(256)   # (the inputs of test_gpu_half_rows.py::test_embed_into_a_half_corpus)
    V, max_tokens = 300, 20
    table = rng.integers(-127, 128, (V, 256)).astype(I8) if dtype == I8 else rng.standard_normal((V, 256)).astype(dtype)
    lens = [0, 1, 2, 17, max_tokens + 3, 5, 0, 17]
    lines = [rng.integers(0, V, n) for n in lens]
    lines[3][4] = V + 7
    ids = np.concatenate(lines).astype(np.uint32)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    ref = np.stack([oracle_np.pool_ids(table, l, True, max_tokens) for l in lines])
    m = smt.Model(gpu_ctx, table, normalize=True)
    c = byte_corpus(gpu_ctx, ref[:1])
    emb, first = m.embed(ids, offsets, max_tokens=max_tokens, append_to=c)
    assert first == 1 and c.rows == 9 and np.array_equal(emb.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(c.read_rows(1, 8), quant(ref).astype(F32))
    c.close(); m.close()


def check_search(gpu_ctx, c, Xs, Q, k):
    n = len(Xs)
    refs = [ref_topk(q, Xs, k) for q in Q]
    for (rows, dist), (rr, rd) in zip(c.search(Q, top_k=k), refs):
        assert len(rows) == min(k, n) and np.array_equal(rows, rr) and np.array_equal(dist.view(np.uint64), rd.view(np.uint64))
    base = 1000
    rows, dist, st = search_ex(gpu_ctx, c, Q, k, base)
    for qi, (rr, rd) in enumerate(refs):
        m = int((rows[qi] != PAD).sum())
        assert (rows[qi, m:] == PAD).all() and np.isinf(dist[qi, m:]).all() and st[qi] in (L.STATUS_PROVED, L.STATUS_UNCERTAIN)
        if st[qi] == L.STATUS_PROVED:
            assert m == len(rr) and np.array_equal(rows[qi, :m], rr + np.uint64(base)) and np.array_equal(dist[qi, :m], rd)
        else:   # every returned pair is exact
            assert m == len(rr) and np.array_equal(dist[qi, :m], ref_dist(Q[qi], Xs)[(rows[qi, :m] - np.uint64(base)).astype(np.int64)])


# one step is 16 rows, one block of eight waves 128, 4099 several blocks; nq 5 is a full pass plus one
@pytest.mark.parametrize("n,nq,k", [(1, 1, 1), (3, 2, 10), (4, 1, 10), (5, 4, 1), (15, 5, 10), (16, 1, 56), (17, 4, 10), (127, 2, 56),
                                    (128, 5, 1), (129, 1, 10), (4099, 5, 10), (4099, 1, 56), (4099, 4, 56)])
def test_search_equals_f64_reference(gpu_ctx, n, nq, k):
    X, Xs, Q = byte_case(n)
    check_search(gpu_ctx, byte_corpus(gpu_ctx, X), Xs, Q[:nq], k)


def test_search_with_two_blocks(gpu_ctx):
    gpu_ctx.set_tuning("scan_blocks", 2)   # waves take many steps each: the prefetched step
    try:
        X, Xs, Q = byte_case(4099)
        c = byte_corpus(gpu_ctx, X)
        check_search(gpu_ctx, c, Xs, Q, 10)
        ranges = [(1, 1500), (1601, 4099)]
        for (rows, dist), q in zip(c.search(Q, top_k=10, ranges=ranges), Q):
            rr, rd = ref_topk(q, Xs, 10, np.concatenate([np.arange(b, e) for b, e in ranges]))
            assert np.array_equal(rows, rr) and np.array_equal(dist, rd)
        c.close()
    finally:
        gpu_ctx.set_tuning("scan_blocks", 0)


def test_search_adopted_extremes(gpu_ctx):
    q8 = extreme_rows()   # -128 everywhere, -128 / 127 alternating: signs and the exact |c|^2
    Q = np.stack([-np.ones(256), q8[9], q8[4] + 0.3 * q8[2], q8[0], np.ones(256)]).astype(F32)
    c, _t = adopted(gpu_ctx, q8)
    assert [int(r[0]) for r, _ in c.search(Q[:2], top_k=1)] == [4, 9]
    check_search(gpu_ctx, c, q8.astype(F32), Q, 10)
    c.close()


@pytest.mark.parametrize("k", [1, 10, 56])
def test_proved_where_it_must_be(gpu_ctx, k):
    rng = np.random.default_rng(4)
    u, v = rng.standard_normal((2, 256))
    u /= np.linalg.norm(u)
    v = (v - (v @ u) * u) / np.linalg.norm(v - (v @ u) * u)
    d = 2e-3 * (1 + rng.permutation(200))   # a staircase of distances, rows in no order
    X = ((1 - d)[:, None] * u + np.sqrt(1 - (1 - d) ** 2)[:, None] * v).astype(F32)
    q = u.astype(F32)
    Xs = quant(X).astype(F32)
    assert np.diff(np.sort(ref_dist(q, Xs))).min() >= 1e-3 > 50 * 2 * F32_ERR_BYTE   # (the stored rows keep the stairs apart)
    c = byte_corpus(gpu_ctx, X)
    gpu_ctx.uncertain_count(reset=True)
    rows, dist, st = search_ex(gpu_ctx, c, q[None], k, 0)
    rr, rd = ref_topk(q, Xs, k)
    assert st[0] == L.STATUS_PROVED and gpu_ctx.uncertain_count(reset=True) == 0
    assert np.array_equal(rows[0], rr) and np.array_equal(dist[0], rd)
    c.close()


@pytest.mark.parametrize("begin,length", [(1, 1), (2, 4), (3, 9), (5, 5), (1, 8)])
def test_ranges_begin_anywhere(gpu_ctx, begin, length):
    X, _, Q = byte_case(129)
    X = X.copy()
    Q = (Q[0] + F32(0.05) * Q).astype(F32)            # five queries around one direction (the fourth is that direction) ...
    X[begin - 1] = X[begin + length] = Q[3]           # ... whose best rows sit directly outside both ends
    Xs = quant(X).astype(F32)
    c = byte_corpus(gpu_ctx, X)
    ranges = [(begin, begin + length), (40 + begin, 47), (100, 100), (126, 129)]
    allowed = np.concatenate([np.arange(b, e) for b, e in ranges])
    assert {int(c.search(q, top_k=1)[0][0][0]) for q in Q} == {begin - 1}
    for nq in (1, 5):
        for (rows, dist), q in zip(c.search(Q[:nq], top_k=10, ranges=ranges), Q):
            rr, rd = ref_topk(q, Xs, 10, allowed)
            assert np.array_equal(rows, rr) and np.array_equal(dist, rd)
    rows, dist = c.search(Q[1], top_k=3, ranges=[(begin, begin + 1)], row_base=7)[0]
    assert rows.tolist() == [begin + 7] and dist.tolist() == [ref_dist(Q[1], Xs[begin:begin + 1])[0]]
    c.close()


def test_workspace_mode(gpu_ctx):
    X, Xs, Q = byte_case(4099)
    c = byte_corpus(gpu_ctx, X)
    ranges = [(3, 3), (5, 6), (10, 1027), (1501, 1510), (3001, 3004)]
    rr, rd = ref_topk(Q[1], Xs, 10, np.concatenate([np.arange(b, e) for b, e in ranges]))
    md = float(rd[4] + rd[5]) / 2   # a max_distance that cuts the list mid-way (score > 1 - max_distance, the threshold an f32)
    keep = int(((1.0 - rd) > float(F32(1.0) - F32(md))).sum())
    assert 0 < keep < 10
    rows, dist = c.search(Q[1], top_k=10, max_distance=md, mode=L.MODE_WORKSPACE, ranges=ranges)[0]
    assert np.array_equal(rows, rr[:keep]) and np.array_equal(dist, rd[:keep])
    assert len(c.search(Q[1], top_k=0, mode=L.MODE_WORKSPACE, ranges=ranges)[0][0]) == 0
    zrows, zdist = c.search(np.zeros(256, F32), top_k=4, mode=L.MODE_WORKSPACE, ranges=ranges)[0]
    assert zrows.tolist() == [5, 10, 11, 12] and zdist.tolist() == [1.0] * 4
    c.close()


def test_equal_rows_past_the_guard_band(gpu_ctx):
    rng = np.random.default_rng(5)
    X = rng.standard_normal((580, 256)).astype(F32)
    where = rng.permutation(580)[:80]
    X[where] = X[0] * F32(2.0) ** rng.integers(-3, 4, (80, 1)).astype(F32)   # 80 rows of one direction: equal stored bytes
    Xs = quant(X).astype(F32)
    assert (Xs[where] == Xs[0]).all()
    q = X[0]
    c = byte_corpus(gpu_ctx, X)
    rr, rd = ref_topk(q, Xs, 10)
    rows, dist = c.search(q, top_k=10)[0]
    assert np.array_equal(rows, rr) and np.array_equal(dist, rd)
    gpu_ctx.uncertain_count(reset=True)
    rows, dist, st = search_ex(gpu_ctx, c, q[None], 10, 0)
    assert (st[0] != L.STATUS_PROVED) == (gpu_ctx.uncertain_count(reset=True) == 1)
    assert np.array_equal(dist[0], ref_dist(q, Xs)[rows[0].astype(np.int64)])
    c.close()


def test_refusals(gpu_ctx, tmp_path):
    X, Xs, Q = byte_case(127)
    c = byte_corpus(gpu_ctx, X)
    f = smt.Corpus(gpu_ctx)
    f.append(X)
    before = f.search(Q[0], top_k=5)[0]
    refused = [lambda: c.search(Q[0], top_k=3, max_distance=0.5), lambda: c.search(Q[0], top_k=57),
               lambda: search_ex(gpu_ctx, c, Q[:1], 57, 0), lambda: c.prepack(), lambda: c.image_tile(0), lambda: c.compact([(0, 2)]),
               lambda: c.save(tmp_path / "a.smt"), lambda: c.append_to_file(tmp_path / "a.smt", 0),
               lambda: smt.IvfPq(c, nlist=32), lambda: smt.IvfPq.load(c, tmp_path / "none.ivf"),
               lambda: c.debug_scan_lists(Q[:1], 3), lambda: c.debug_batched_scores(Q[:1]), lambda: c.debug_nominations(Q[:1]),
               lambda: c.debug_bootstrap_minima(Q[:1]), lambda: c.debug_batch_slab_lists(Q[:1], 3), lambda: c.debug_batch_half_lists(Q[:1], 3),
               lambda: smt.Corpus(gpu_ctx, dim=512, dtype=I8)]
    for call in refused:
        with pytest.raises(L.SmtError) as e:
            call()
        assert e.value.code == L.SMT_E_UNSUPPORTED and "byte rows" in str(e.value), str(e.value)
    assert not (tmp_path / "a.smt").exists()
    with pytest.raises(L.SmtError) as e:
        smt.Corpus(gpu_ctx, dtype=7)
    assert e.value.code == L.SMT_E_INVALID
    rr, rd = ref_topk(Q[0], Xs, 5)
    rows, dist = c.search(Q[0], top_k=5)[0]
    assert np.array_equal(rows, rr) and np.array_equal(dist, rd) and c.rows == 127
    after = f.search(Q[0], top_k=5)[0]
    assert f.dtype == F32 and np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    c.close(); f.close()
