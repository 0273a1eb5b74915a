"""GPU: smt_ivfpq_compact -- the corpus is compacted in place and the IVF index follows it instead of being rebuilt
(ivfpq_compact.hip).  The index is saved before and after the call and both files are parsed (tests/ivf_ref.read_index): the second
must be tests/ivf_compact_ref.carry of the first, array by array and byte for byte -- no tolerances anywhere in this file.

6 007 rows in 32 lists: list borders and the last word of the alive bitmap are ragged, and every list holds at most 512 rows, so
that a search at rerank 512 re-scores every probed list entirely (include/semtools_hip.h, smt_ivfpq_search)."""
import numpy as np
import pytest

from tests import ivf_compact_ref as K
from tests import ivf_ref as R
from tests.test_gpu_compact import expected_moved, kept_index

pytestmark = pytest.mark.gpu

N, NLIST, SEED = 6007, 32, 77
KINDS = pytest.mark.parametrize("lpca", [False, True], ids=["pq", "lpca"])


@pytest.fixture(scope="module")
def emb():
    return R.iso_rows(N + 500, SEED)                       # the corpus is the first N rows; the rest is appended by some tests


def build(ctx, rows, lpca):
    import semtools_amd as smt

    c = smt.Corpus(ctx)
    c.append(rows)
    ix = smt.IvfPq(c, nlist=NLIST, train_iters=5, local_pca=lpca)
    assert ix.list_sizes().max() <= 512                    # the condition everything below rests on
    return c, ix


def saved(ix, path):
    ix.save(path)
    return path.read_bytes(), R.read_index(path)


def same_rows(c, want):
    return c.rows == len(want) and np.array_equal(c.read_rows(0, c.rows).view(np.uint32), want.view(np.uint32))


def complement(rows, n):
    keep, at = [], 0
    for r in sorted(int(r) for r in rows):
        if r > at:
            keep.append((at, r))
        at = r + 1
    return keep + ([(at, n)] if at < n else [])


def keep_list(case, f):
    if case == "wide":
        return [(0, 1000), (1500, 3000), (3001, 4097), (4160, N)]
    if case == "pairs_of_four":                           # 1 502 ranges: past the 1024 ranges the mark kernel stages in LDS
        return [(4 * i, 4 * i + 2) for i in range(1502)]
    if case == "empties_a_list":                          # the complement of the longest list's rows
        l = int(np.argmax(np.diff(f["offsets"].astype(np.int64))))
        return complement(f["ids"][int(f["offsets"][l]):int(f["offsets"][l + 1])], N)
    if case == "one_row":
        return [(3333, 3334)]
    raise KeyError(case)


@KINDS
@pytest.mark.parametrize("case", ["wide", "pairs_of_four", "empties_a_list", "one_row"])
def test_index_after_the_call_is_the_carried_index(gpu_ctx, emb, tmp_path, lpca, case):
    c, ix = build(gpu_ctx, emb[:N], lpca)
    _, f = saved(ix, tmp_path / "before.ivf")
    keep = keep_list(case, f)
    if case == "pairs_of_four":
        assert len(keep) > 1024
    idx = kept_index(keep, N)
    moved, dropped = ix.compact(keep)
    _, g = saved(ix, tmp_path / "after.ivf")
    want = K.carry(f, keep)
    assert K.same_index(want, g) == []
    assert g["n_rows"] == len(idx) == ix.info()["rows"] and dropped == N - len(idx)
    assert moved == expected_moved(idx)
    assert same_rows(c, emb[:N][idx])
    assert int(ix.list_sizes().max()) == int(np.diff(want["offsets"].astype(np.int64)).max())
    if case == "empties_a_list":
        assert int(ix.list_sizes().min()) == 0
    ix.close(); c.close()


@KINDS
def test_a_list_that_drops_nothing_is_a_no_op(gpu_ctx, emb, tmp_path, lpca):
    c, ix = build(gpu_ctx, emb[:N], lpca)
    before, _ = saved(ix, tmp_path / "before.ivf")
    stats = gpu_ctx.compact_stats()
    assert ix.compact([(0, 2000), (2000, 2000), (2000, N)]) == (0, 0)
    after = gpu_ctx.compact_stats()
    assert after.calls == stats.calls + 1 and after.rows_moved == stats.rows_moved
    assert saved(ix, tmp_path / "after.ivf")[0] == before
    assert same_rows(c, emb[:N])
    ix.close(); c.close()


@KINDS
@pytest.mark.parametrize("case", ["wide", "pairs_of_four"])
def test_same_answers_as_the_search_inside_the_keep_list(gpu_ctx, emb, tmp_path, lpca, case):
    """rerank 512 on lists of <= 512 rows: every probed list is re-scored entirely, and the probe sees only the centroids, which the
    call does not touch.  So the search inside ranges = keep BEFORE the call, its rows renamed, is the unfiltered search AFTER it."""
    c, ix = build(gpu_ctx, emb[:N], lpca)
    keep = keep_list(case, None)
    qs = R.iso_rows(16, SEED + 1)
    before = {p: ix.search(qs, top_k=10, nprobe=p, rerank=512, ranges=keep) for p in (4, 32)}
    ix.compact(keep)
    for nprobe, want in before.items():
        got = ix.search(qs, top_k=10, nprobe=nprobe, rerank=512)
        for qi, ((gr, gd), (wr, wd)) in enumerate(zip(got, want)):
            alive, new = K.remap(wr, keep)
            assert alive.all() and len(wr) == 10
            assert gr.tolist() == new.tolist(), (nprobe, qi)
            assert gd.tobytes() == wd.tobytes(), (nprobe, qi)
    ix.close(); c.close()


@KINDS
def test_partly_covered_corpus(gpu_ctx, emb, tmp_path, lpca):
    """500 rows appended to the corpus and not yet to the index: the call drops rows on both sides of row 6 007, the index covers
    the kept rows below it, and smt_ivfpq_append then takes in the kept rows above it."""
    c, ix = build(gpu_ctx, emb[:N], lpca)
    c.append(emb[N:])
    _, f = saved(ix, tmp_path / "before.ivf")
    keep = [(0, 5000), (5500, 6100), (6300, N + 500)]
    idx = kept_index(keep, N + 500)
    below = int((idx < N).sum())
    moved, dropped = ix.compact(keep)
    assert (moved, dropped) == (expected_moved(idx), N - below)
    assert same_rows(c, emb[idx])
    _, g = saved(ix, tmp_path / "carried.ivf")
    assert K.same_index(K.carry(f, keep), g) == [] and g["n_rows"] == below == ix.info()["rows"]
    assert ix.append() == len(idx) - below
    _, h = saved(ix, tmp_path / "appended.ivf")
    assert sorted(h["ids"].tolist()) == list(range(len(idx)))          # every row exactly once
    off = h["offsets"].astype(np.int64)
    for l in range(NLIST):
        assert (np.diff(h["ids"][off[l]:off[l + 1]].astype(np.int64)) > 0).all()
    # the carried entries kept their codes through the append
    _, pos_g = R.list_of_rows(g)
    _, pos_h = R.list_of_rows(h)
    assert np.array_equal(h["codes"][pos_h[:below]], g["codes"][pos_g])
    ix.close(); c.close()


@KINDS
def test_refused_lists_change_nothing(gpu_ctx, emb, tmp_path, lpca):
    import semtools_amd as smt
    from semtools_amd import _lib as L

    c, ix = build(gpu_ctx, emb[:N], lpca)
    c.append(emb[N:])
    before, _ = saved(ix, tmp_path / "before.ivf")
    for bad, code in (([(10, 20), (0, 5)], L.SMT_E_INVALID),                  # unsorted
                      ([(0, 10), (9, 20)], L.SMT_E_INVALID),                  # overlapping
                      ([(0, 10), (6000, N + 501)], L.SMT_E_INVALID),          # past the corpus
                      ([(N, N + 100), (N + 200, N + 500)], L.SMT_E_UNSUPPORTED),   # keeps no row the index covers
                      ([], L.SMT_E_UNSUPPORTED)):
        with pytest.raises(smt.SmtError) as e:
            ix.compact(bad)
        assert e.value.code == code, bad
        assert same_rows(c, emb)
        assert saved(ix, tmp_path / "after.ivf")[0] == before
    got = ix.search(emb[17], top_k=1, nprobe=NLIST, rerank=512)[0]
    assert got[0].tolist() == [17]                                            # and it still answers
    ix.close(); c.close()


def test_adopted_corpus_is_refused(gpu_ctx, emb, tmp_path):
    import torch
    import semtools_amd as smt
    from semtools_amd import _lib as L

    t = torch.from_numpy(emb[:N]).cuda()
    torch.cuda.synchronize()
    c = smt.Corpus(gpu_ctx, device_ptr=t.data_ptr(), rows=N)
    ix = smt.IvfPq(c, nlist=NLIST, train_iters=5)
    before, _ = saved(ix, tmp_path / "before.ivf")
    with pytest.raises(smt.SmtError) as e:
        ix.compact([(0, 1000), (2000, N)])
    assert e.value.code == L.SMT_E_UNSUPPORTED and c.rows == N
    assert saved(ix, tmp_path / "after.ivf")[0] == before
    assert np.array_equal(t.cpu().numpy().view(np.uint32), emb[:N].view(np.uint32))
    ix.close(); c.close()


@KINDS
def test_a_device_search_issued_before_the_call_holds_the_old_answer(gpu_ctx, emb, lpca):
    import torch

    c, ix = build(gpu_ctx, emb[:N], lpca)
    qs = R.iso_rows(16, SEED + 2)
    want = ix.search(qs, top_k=10, nprobe=8, rerank=512)
    qd = torch.from_numpy(qs).cuda()
    rows = torch.zeros((16, 10), dtype=torch.int64, device="cuda")
    dist = torch.zeros((16, 10), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ix.search_device(qd.data_ptr(), 16, 10, 8, 512, 0, rows.data_ptr(), dist.data_ptr())
    ix.compact(keep_list("pairs_of_four", None))           # frees the arrays the search reads: only behind the stream
    gpu_ctx.synchronize()
    r, d = rows.cpu().numpy().view(np.uint64), dist.cpu().numpy()
    for qi, (wr, wd) in enumerate(want):
        assert len(wr) == 10 and r[qi].tolist() == wr.tolist(), qi
        assert d[qi].tobytes() == wd.tobytes(), qi
    ix.close(); c.close()


def test_an_index_that_was_not_carried_still_refuses(gpu_ctx, emb):
    """Only the index the call is made on follows the rows: a second one on the same corpus is what any index is after
    smt_corpus_compact."""
    import semtools_amd as smt

    c, ix = build(gpu_ctx, emb[:N], False)
    other = smt.IvfPq(c, nlist=NLIST, train_iters=5)
    ix.compact([(0, 3000), (3100, N)])
    assert len(ix.search(emb[5], top_k=3, nprobe=4)[0][0]) == 3
    with pytest.raises(smt.SmtError, match="shrank"):
        other.search(emb[5], top_k=3, nprobe=4)
    other.close(); ix.close(); c.close()
