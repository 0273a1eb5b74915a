"""Narrow rows (64 dimensions): embed and exact search against NumPy in float64.  np.cumsum is the sequential sum the contract is
written in; oracle_np._finish gives the distance."""
import ctypes as C
import functools

import numpy as np
import pytest

import semtools_amd as smt
from semtools_amd import _lib as L
from oracle import oracle_np

pytestmark = pytest.mark.gpu
D = 64
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)


def ref_dist(q, X):
    q64, X64 = q.astype(np.float64), X.astype(np.float64)
    ab, b2 = np.cumsum(X64 * q64, axis=1)[:, -1], np.cumsum(X64 * X64, axis=1)[:, -1]
    a2 = np.cumsum(q64 * q64)[-1]
    return np.array([oracle_np._finish(float(ab[i]), float(a2), float(b2[i])) for i in range(len(X))])


def ref_topk(q, X, k, rows=None):
    rows = np.arange(len(X)) if rows is None else np.asarray(rows)
    d = ref_dist(q, X[rows])
    order = np.lexsort((rows, d))[:k]
    return rows[order].astype(np.uint64), d[order]


@functools.lru_cache(maxsize=None)
def corpus_of(n):
    """n rows with exact duplicates (ties by row) and zero rows where n allows, and five queries, the fourth all zero"""
    rng = np.random.default_rng(D + n)
    X = rng.standard_normal((n, D)).astype(np.float32)
    Q = rng.standard_normal((5, D)).astype(np.float32)
    Q[0] = X[0] + 0.05 * Q[0]
    Q[3] = 0
    if n >= 3:
        X[n // 2] = X[0]
        X[1] = 0
    if n >= 63:
        X[40:44] = X[7]
        X[50] = 0
    X.setflags(write=False)
    Q.setflags(write=False)
    return X, Q


def search_ex(ctx, c, Q, k, row_base):
    import torch
    q = torch.from_numpy(np.array(Q, dtype=np.float32)).cuda()
    rows = torch.zeros((len(Q), k), dtype=torch.int64, device="cuda")
    dist = torch.zeros((len(Q), k), dtype=torch.float64, device="cuda")
    st = torch.full((len(Q),), 9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    c.search_topk_device(q.data_ptr(), len(Q), k, row_base, rows.data_ptr(), dist.data_ptr(), st.data_ptr())
    ctx.synchronize()
    return rows.cpu().numpy().view(np.uint64), dist.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("dtype", [np.float32, np.float16, np.int8])
def test_embed_bit_for_bit(gpu_ctx, dtype, normalize):
    rng = np.random.default_rng(D)
    V, max_tokens = 300, 20
    table = rng.integers(-127, 128, (V, D)).astype(np.int8) if dtype == np.int8 else rng.standard_normal((V, D)).astype(dtype)
    lens = [0, 1, 2, 17, max_tokens + 3, 5, 0, 17, 3]   # nine lines: not a multiple of the four a wave holds
    lines = [rng.integers(0, V, n) for n in lens]
    lines[3][4] = V + 7   # an id outside the table adds nothing and still counts
    ids = np.concatenate(lines).astype(np.uint32)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    ref = np.stack([oracle_np.pool_ids(table, l, normalize, max_tokens) for l in lines])
    m = smt.Model(gpu_ctx, table, normalize=normalize)
    c = smt.Corpus(gpu_ctx, dim=D)
    emb, _ = m.embed(ids, offsets, max_tokens=max_tokens)
    assert emb.shape == (len(lens), D) and np.array_equal(emb.view(np.uint32), ref.view(np.uint32))
    _, first = m.embed(ids, offsets, max_tokens=max_tokens, append_to=c, want_host=False)
    assert first == 0 and np.array_equal(c.read_rows(0, len(lens)).view(np.uint32), ref.view(np.uint32))
    c.close(); m.close()


def test_identity_corpus(gpu_ctx):
    c = smt.Corpus(gpu_ctx, dim=D)
    c.append(np.eye(D, dtype=np.float32))
    js = [0, 3, 4, 15, 16, 63]   # the lane and DPP-row borders of the layout
    res = c.search(np.eye(D, dtype=np.float32)[js], top_k=3)
    for j, (rows, dist) in zip(js, res):
        others = [r for r in range(3) if r != j][:2]
        assert rows.tolist() == [j] + others and dist.tolist() == [0.0, 1.0, 1.0], (j, rows, dist)
    c.close()


@pytest.mark.parametrize("k", [1, 10, 56])
@pytest.mark.parametrize("nq", [1, 4, 5])
@pytest.mark.parametrize("n", [1, 3, 63, 4099])
def test_search_equals_f64_reference(gpu_ctx, n, nq, k):
    X, Q = corpus_of(n)
    Q = Q[:nq]
    c = smt.Corpus(gpu_ctx, dim=D)
    c.append(X)
    refs = [ref_topk(q, X, k) for q in Q]
    for (rows, dist), (rr, rd) in zip(c.search(Q, top_k=k), refs):
        assert len(rows) == min(k, n) and np.array_equal(rows, rr) and np.array_equal(dist.view(np.uint64), rd.view(np.uint64))
    base = 1000
    rows, dist, st = search_ex(gpu_ctx, c, Q, k, base)
    full = [ref_dist(q, X) for q in Q]
    for qi, (rr, rd) in enumerate(refs):
        m = int((rows[qi] != PAD).sum())
        assert (rows[qi, m:] == PAD).all() and np.isinf(dist[qi, m:]).all() and st[qi] in (L.STATUS_PROVED, L.STATUS_UNCERTAIN)
        if st[qi] == L.STATUS_PROVED:
            assert m == len(rr) and np.array_equal(rows[qi, :m], rr + np.uint64(base)) and np.array_equal(dist[qi, :m], rd)
        else:   # every returned pair is exact
            assert m == len(rr) and np.array_equal(dist[qi, :m], full[qi][(rows[qi, :m] - np.uint64(base)).astype(np.int64)])
    c.close()


def test_ranges_and_workspace_mode(gpu_ctx):
    X, Q = corpus_of(4099)
    X = X.copy()
    q = Q[1]
    X[9] = q   # the best row of the corpus, one row in front of a range
    c = smt.Corpus(gpu_ctx, dim=D)
    c.append(X)
    ranges = [(3, 3), (5, 6), (10, 1027), (2000, 2000), (3001, 3004)]   # starts that are no multiple of the four rows of a load
    allowed = np.concatenate([np.arange(b, e) for b, e in ranges])
    rr, rd = ref_topk(q, X, 10, allowed)
    rows, dist = c.search(q, top_k=10, ranges=ranges)[0]
    assert 9 not in rows.tolist() and np.array_equal(rows, rr) and np.array_equal(dist, rd)
    assert c.search(q, top_k=10)[0][0][0] == 9
    rows, dist = c.search(q, top_k=3, ranges=[(5, 6)], row_base=7)[0]
    assert rows.tolist() == [12] and dist.tolist() == [ref_dist(q, X[5:6])[0]]
    assert len(c.search(q, top_k=3, ranges=[(8, 8)])[0][0]) == 0
    # workspace mode: a max_distance that cuts the list mid-way (score > 1 - max_distance, the threshold an f32), and top_k = 0
    md = float(rd[4] + rd[5]) / 2
    keep = int(((1.0 - rd) > float(np.float32(1.0) - np.float32(md))).sum())
    assert 0 < keep < 10
    rows, dist = c.search(q, top_k=10, max_distance=md, mode=L.MODE_WORKSPACE, ranges=ranges)[0]
    assert np.array_equal(rows, rr[:keep]) and np.array_equal(dist, rd[:keep])
    assert len(c.search(q, top_k=0, mode=L.MODE_WORKSPACE, ranges=ranges)[0][0]) == 0
    zrows, zdist = c.search(np.zeros(D, np.float32), top_k=4, mode=L.MODE_WORKSPACE, ranges=ranges)[0]
    assert zrows.tolist() == [5, 10, 11, 12] and zdist.tolist() == [1.0] * 4
    c.close()


def test_near_ties_past_the_guard_band(gpu_ctx):
    rng = np.random.default_rng(5 * D)
    X = rng.standard_normal((580, D)).astype(np.float32)
    b = X[0] / np.linalg.norm(X[0])
    where = rng.permutation(580)[:80]
    for i, r in enumerate(where):   # 80 rows, one ulp of one component apart
        X[r] = b
        X[r, (3 * i) % D] = np.nextafter(b[(3 * i) % D], np.float32(np.inf))
    c = smt.Corpus(gpu_ctx, dim=D)
    c.append(X)
    rr, rd = ref_topk(b, X, 10)
    rows, dist = c.search(b, top_k=10)[0]
    assert np.array_equal(rows, rr) and np.array_equal(dist, rd)
    gpu_ctx.uncertain_count(reset=True)
    _, _, st = search_ex(gpu_ctx, c, b[None], 10, 0)
    assert (st[0] != L.STATUS_PROVED) == (gpu_ctx.uncertain_count(reset=True) == 1)
    c.close()


def test_refusals_and_files(gpu_ctx, tmp_path):
    lib, h = L.lib(), C.c_void_p()
    for dim in (128, 384):
        assert lib.smt_corpus_create(gpu_ctx._h, dim, 0, C.byref(h)) == L.SMT_E_UNSUPPORTED and b"256" in lib.smt_last_error()
    X, Q = corpus_of(63)
    c = smt.Corpus(gpu_ctx, dim=D)
    c.append(X)
    before = c.search(Q[:2], top_k=5)
    group = smt.Group.logical(0, 1)
    table = np.ones((4, D), np.float32)
    q256 = np.zeros((1, 256), np.float32)
    refused = [lambda: c.search(Q[0], top_k=3, max_distance=0.5), lambda: c.search(Q[0], top_k=57), lambda: c.prepack(), lambda: c.compact([(0, 2)]),
               lambda: smt.IvfPq(c, nlist=32), lambda: smt.IvfPq.load(c, tmp_path / "none.ivf"),
               lambda: smt.Model(gpu_ctx, table, mapping=[0, 1, 2, 3]), lambda: smt.Model(gpu_ctx, table, weights=np.ones(4, np.float32)),
               lambda: L.check(lib.smt_sharded_corpus_create(group._h, D, C.byref(h))),
               lambda: L.check(lib.smt_sharded_model_create(group._h, L.np_ptr(table), 4, D, 1, C.byref(h))),
               lambda: c.debug_batched_scores(q256), lambda: c.debug_nominations(q256), lambda: c.debug_bootstrap_minima(q256),
               lambda: c.debug_scan_lists(q256, 3), lambda: c.debug_select_lists(0, 1, 0, 1, 1, 1, 0, 0),
               lambda: c.debug_batch_slab_lists(Q[:1], 3), lambda: c.debug_batch_half_lists(Q[:1], 3),
               lambda: smt.Corpus(gpu_ctx, dim=D, dtype=np.float16), lambda: smt.Corpus(gpu_ctx, dim=D, dtype=np.int8)]
    for i, call in enumerate(refused):
        with pytest.raises(L.SmtError) as e:
            call()
        assert e.value.code == L.SMT_E_UNSUPPORTED and "64" in str(e.value), (i, str(e.value))
    group.close()
    after = c.search(Q[:2], top_k=5)
    assert c.rows == 63 and all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(before, after))
    # save, load and append_to_file round-trip a narrow corpus byte for byte
    p1, p2 = tmp_path / "a.smt", tmp_path / "b.smt"
    c.truncate(3)
    c.save(p1)
    d = smt.Corpus.load(gpu_ctx, p1)
    assert d.dim == D and np.array_equal(d.read_rows(0, 3).view(np.uint32), X[:3].view(np.uint32))
    more = corpus_of(4099)[0][:63]
    c.append(more)
    c.write_rows(1, more[:1])
    c.truncate(60)
    c.write_rows(1, X[1:2])
    c.append_to_file(p1, 3)
    c.save(p2)
    assert p1.read_bytes() == p2.read_bytes() and p1.read_bytes()[32:] == np.concatenate([X[:3], more])[:60].tobytes()
    c.close(); d.close()
