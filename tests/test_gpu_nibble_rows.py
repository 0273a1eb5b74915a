"""Nibble rows (SMT_ROWS_I4: 256 signed 4-bit integers a row, 128 B): store, embed and exact search against NumPy in float64 over
the STORED integers, quant(X).astype(float32).  Reference distance, reference top-k and the device-form call are the wide rows'
test's.  The largest |d32 - d64| of the scan's keys is not collected: no hook exposes them; f32_err_nibble is DERIVED (nibble_rows.h)."""
import functools

import numpy as np
import pytest

import semtools_amd as smt
from semtools_amd import _lib as L
from oracle import oracle_np
from tests.test_gpu_wide_rows import PAD, corpus_of, ref_dist, ref_topk, search_ex

pytestmark = pytest.mark.gpu
I8, F32 = np.int8, np.float32
F32_ERR_NIBBLE = 1.2 * (2.0 ** -19 + 1e-6)   # nibble_rows.h


def quant(X):
    """the rounding rule of include/semtools_hip.h ("NIBBLE ROWS"), every array float32"""
    X = np.asarray(X, F32)
    amax = np.abs(X).max(1, keepdims=True)
    with np.errstate(divide="ignore"):
        s = np.where(amax > 0, F32(7) / amax, F32(0))
    return np.rint(X * s).astype(I8)


def pack(q):
    return ((q[:, 0::2] & 15) | ((q[:, 1::2] & 15) << 4)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def nibble_case(n):
    """corpus_of(256, n) -- duplicates, zero rows, a zero query; returns (rows as given, rows as stored, queries)"""
    X, Q = corpus_of(256, n)
    return X, quant(X).astype(F32), Q


def nibble_corpus(ctx, X):
    c = smt.Corpus(ctx, dtype="int4")
    c.append(X)
    return c


def adopted(ctx, q4):
    import torch
    t = torch.from_numpy(pack(q4)).cuda()
    return smt.Corpus(ctx, device_ptr=t.data_ptr(), rows=len(q4), dtype=L.ROWS_I4), t


def extreme_rows():
    q4 = np.random.default_rng(3).integers(-8, 8, (14, 256)).astype(I8)
    q4[0], q4[1], q4[2:7] = -8, 7, 0
    q4[2, 0], q4[3, 0], q4[4, 255], q4[5, 31], q4[6, 32] = 7, -8, -8, 7, 1   # single-axis rows: ends of a row, of a lane, of a dword
    return q4


def test_store_bit_for_bit(gpu_ctx):
    rng = np.random.default_rng(1)
    X = (rng.standard_normal((37, 256)) * 10.0 ** rng.integers(-8, 3, (37, 1))).astype(F32)
    X[5:8] = 0                 # a zero row, a row whose only (largest) component is negative, a row with amax = 7 (s = 1) and ties
    X[6, 17] = -3.5
    X[7, :6] = [7, 0.5, 1.5, 2.5, -0.5, -2.5]
    ref = quant(X)
    assert not ref[5].any() and ref[6, 17] == -7 and ref[7, :6].tolist() == [7, 0, 2, 2, 0, -2] and ref.min() == -7 and ref.max() == 7
    c = nibble_corpus(gpu_ctx, X)
    row_bytes = L.C.c_uint64()
    L.check(L.lib().smt_corpus_info(c._h, None, None, L.C.byref(row_bytes)))
    assert row_bytes.value == 128 and c.dtype == "int4" and c.dim == 256 and np.array_equal(c.read_rows(0, 37), ref.astype(F32))
    bad = X[:3].copy()
    bad[1, 7] = np.nan
    for call in (lambda: c.append(bad), lambda: c.write_rows(4, bad)):
        with pytest.raises(L.SmtError) as e:
            call()
        assert e.value.code == L.SMT_E_INVALID and c.rows == 37 and np.array_equal(c.read_rows(0, 37), ref.astype(F32))
    c.write_rows(3, X[10:12])
    c.truncate(20)
    assert c.append(X[30:33] * F32(2.0 ** -9)) == 20 and c.rows == 23   # (a power of two changes no stored nibble)
    want = np.concatenate([ref[:3], ref[10:12], ref[5:20], ref[30:33]])
    assert np.array_equal(c.read_rows(0, 23), want.astype(F32))
    d, _t = adopted(gpu_ctx, q4 := extreme_rows())   # a packed uint8 tensor, -8 nibbles included
    assert d.dtype == "int4" and np.array_equal(d.read_rows(0, 14), q4.astype(F32)) and np.array_equal(d.read_rows(3, 2), q4[3:5].astype(F32))
    c.close(); d.close()


@pytest.mark.parametrize("dtype", [F32, np.float16, I8])
def test_embed_into_a_nibble_corpus(gpu_ctx, dtype):
    rng = np.random.default_rng(256)   # (the inputs of test_gpu_byte_rows.py::test_embed_into_a_byte_corpus)
    V, max_tokens = 300, 20
    table = rng.integers(-127, 128, (V, 256)).astype(I8) if dtype == I8 else rng.standard_normal((V, 256)).astype(dtype)
    lens = [0, 1, 2, 17, max_tokens + 3, 5, 0, 17]
    lines = [rng.integers(0, V, n) for n in lens]
    lines[3][4] = V + 7
    ids = np.concatenate(lines).astype(np.uint32)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    ref = np.stack([oracle_np.pool_ids(table, l, True, max_tokens) for l in lines])
    m = smt.Model(gpu_ctx, table, normalize=True)
    c = nibble_corpus(gpu_ctx, ref[:1])
    emb, first = m.embed(ids, offsets, max_tokens=max_tokens, append_to=c)
    assert first == 1 and c.rows == 9 and np.array_equal(emb.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(c.read_rows(1, 8), quant(ref).astype(F32))
    c.close(); m.close()


def check_search(gpu_ctx, c, Xs, Q, k, proved=False):
    n = len(Xs)
    refs = [ref_topk(q, Xs, k) for q in Q]
    for (rows, dist), (rr, rd) in zip(c.search(Q, top_k=k), refs):
        assert len(rows) == min(k, n) and np.array_equal(rows, rr) and np.array_equal(dist.view(np.uint64), rd.view(np.uint64))
    base = 1000
    rows, dist, st = search_ex(gpu_ctx, c, Q, k, base)
    for qi, (rr, rd) in enumerate(refs):
        m = int((rows[qi] != PAD).sum())
        assert (rows[qi, m:] == PAD).all() and np.isinf(dist[qi, m:]).all()
        assert st[qi] == L.STATUS_PROVED or (not proved and st[qi] == L.STATUS_UNCERTAIN)
        if st[qi] == L.STATUS_PROVED:
            assert m == len(rr) and np.array_equal(rows[qi, :m], rr + np.uint64(base)) and np.array_equal(dist[qi, :m], rd)
        else:   # every returned pair is exact
            assert m == len(rr) and np.array_equal(dist[qi, :m], ref_dist(Q[qi], Xs)[(rows[qi, :m] - np.uint64(base)).astype(np.int64)])


# one row; either side of a load (8 rows); either side of a step (32); many steps and blocks with a ragged end.  nq 5: a pass and one
@pytest.mark.parametrize("k", [1, 10, 56])
@pytest.mark.parametrize("nq", [1, 4, 5])
@pytest.mark.parametrize("n", [1, 7, 9, 31, 33, 4099])
def test_search_equals_f64_reference(gpu_ctx, n, nq, k):
    X, Xs, Q = nibble_case(n)
    c = nibble_corpus(gpu_ctx, X)
    check_search(gpu_ctx, c, Xs, Q[:nq], k)
    c.close()


def test_search_with_two_blocks(gpu_ctx):
    gpu_ctx.set_tuning("scan_blocks", 2)   # waves take many steps each: the prefetched step
    try:
        X, Xs, Q = nibble_case(4099)
        c = nibble_corpus(gpu_ctx, X)
        check_search(gpu_ctx, c, Xs, Q, 10)
        ranges = [(1, 1500), (1601, 4099)]
        for (rows, dist), q in zip(c.search(Q, top_k=10, ranges=ranges), Q):
            rr, rd = ref_topk(q, Xs, 10, np.concatenate([np.arange(b, e) for b, e in ranges]))
            assert np.array_equal(rows, rr) and np.array_equal(dist, rd)
        c.close()
    finally:
        gpu_ctx.set_tuning("scan_blocks", 0)


@pytest.mark.parametrize("begin,length", [(1, 1), (3, 4), (5, 9), (13, 5)])
def test_ranges_begin_anywhere(gpu_ctx, begin, length):
    X, _, Q = nibble_case(129)
    X = X.copy()
    Q = (Q[0] + F32(0.05) * Q).astype(F32)            # five queries around one direction (the fourth is that direction) ...
    X[begin - 1] = X[begin + length] = Q[3]           # ... whose best rows sit directly outside both ends
    Xs = quant(X).astype(F32)
    c = nibble_corpus(gpu_ctx, X)
    ranges = [(begin, begin + length), (40 + begin, 60), (100, 100), (126, 129)]   # (the last ends at the last row)
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
    X, Xs, Q = nibble_case(4099)
    c = nibble_corpus(gpu_ctx, X)
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


def test_integer_extremes(gpu_ctx):
    q4 = extreme_rows()   # 14 rows, fewer than k': every list is complete, hence PROVED whatever ties
    axis = np.zeros((2, 256), F32)
    axis[0, 0], axis[1, 255] = 1, -3   # n_i = +-2^22: the top digit's end
    Q = np.concatenate([axis, np.ones((1, 256), F32), -np.ones((1, 256), F32), q4[:1].astype(F32)])   # the last: <c, n> = 2^29 on row 0
    c, _t = adopted(gpu_ctx, q4)
    assert [int(r[0]) for r, _ in c.search(Q, top_k=1)] == [2, 4, 1, 0, 0]
    check_search(gpu_ctx, c, q4.astype(F32), Q, 10, proved=True)
    c.close()


@functools.lru_cache(maxsize=None)
def staircase():
    rng = np.random.default_rng(4)
    u = rng.standard_normal(256)
    X = (rng.uniform(0.05, 3.0, (4000, 1)) * u + rng.standard_normal((4000, 256))).astype(F32)   # a larger draw around one direction
    q = u.astype(F32)
    d = ref_dist(q, quant(X).astype(F32))
    keep, last = [], -1.0
    for i in np.argsort(d):   # a staircase of STORED distances at least 1e-3 apart
        if d[i] - last >= 1e-3 and len(keep) < 200:
            keep.append(i)
            last = d[i]
    X = X[rng.permutation(keep)]   # rows in no order
    Xs = quant(X).astype(F32)
    return X, Xs, q, np.sort(ref_dist(q, Xs))


@pytest.mark.parametrize("k", [1, 10, 56])
def test_proved_where_it_must_be(gpu_ctx, k):
    X, Xs, q, stairs = staircase()
    assert len(X) == 200 and np.diff(stairs).min() >= 1e-3 > 100 * 2 * F32_ERR_NIBBLE
    c = nibble_corpus(gpu_ctx, X)
    gpu_ctx.uncertain_count(reset=True)
    rows, dist, st = search_ex(gpu_ctx, c, q[None], k, 0)
    rr, rd = ref_topk(q, Xs, k)
    assert st[0] == L.STATUS_PROVED and gpu_ctx.uncertain_count(reset=True) == 0
    assert np.array_equal(rows[0], rr) and np.array_equal(dist[0], rd)
    c.close()


def test_refusals(gpu_ctx, tmp_path):
    X, Xs, Q = nibble_case(127)
    c = nibble_corpus(gpu_ctx, X)
    refused = [lambda: c.search(Q[0], top_k=3, max_distance=0.5), lambda: c.search(Q[0], top_k=57),
               lambda: search_ex(gpu_ctx, c, Q[:1], 57, 0), lambda: c.prepack(), lambda: c.image_tile(0), lambda: c.compact([(0, 2)]),
               lambda: c.save(tmp_path / "a.smt"), lambda: c.append_to_file(tmp_path / "a.smt", 0),
               lambda: smt.IvfPq(c, nlist=32), lambda: smt.IvfPq.load(c, tmp_path / "none.ivf"),
               lambda: c.debug_scan_lists(Q[:1], 3), lambda: c.debug_batched_scores(Q[:1]), lambda: c.debug_nominations(Q[:1]),
               lambda: c.debug_bootstrap_minima(Q[:1]), lambda: c.debug_batch_slab_lists(Q[:1], 3), lambda: c.debug_batch_half_lists(Q[:1], 3),
               lambda: c.debug_batch_byte_lists(Q[:1], 3), lambda: smt.Corpus(gpu_ctx, dim=512, dtype="int4")]
    for call in refused:
        with pytest.raises(L.SmtError) as e:
            call()
        assert e.value.code == L.SMT_E_UNSUPPORTED and "nibble rows" in str(e.value), str(e.value)
    assert not (tmp_path / "a.smt").exists()
    with pytest.raises(L.SmtError) as e:
        smt.Corpus(gpu_ctx, dtype=7)
    assert e.value.code == L.SMT_E_INVALID
    rr, rd = ref_topk(Q[0], Xs, 5)
    rows, dist = c.search(Q[0], top_k=5)[0]
    assert np.array_equal(rows, rr) and np.array_equal(dist, rd) and c.rows == 127 and np.array_equal(c.read_rows(0, 127), Xs)
    c.close()
