"""smt_corpus_compact: keep a sorted list of row ranges and close the gaps IN PLACE on the device (compact.hip).  The rows are
compared as bit patterns with numpy's concatenation of the kept slices; searches after a compaction are compared with a corpus
built fresh from the kept rows (rows ==, f64 distances array_equal)."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import synth

pytestmark = pytest.mark.gpu

N_MAX = 70_001           # crosses the default bounce capacity of 65 536 rows
N_OVERLAP = 1_000_000    # the row count tests/test_gpu_scan_overlap.py uses for the overlapped one-query route


@pytest.fixture(scope="module")
def x():
    rng = np.random.default_rng(5)
    return np.ascontiguousarray(rng.standard_normal((N_MAX, 256), dtype=np.float32))


@pytest.fixture
def ctx64(gpu_ctx):
    """the session's context with a 64-row bounce buffer: 5000 rows take about 80 steps"""
    gpu_ctx.set_tuning("compact_bounce_rows", 64)
    gpu_ctx.compact_stats(reset=True)
    yield gpu_ctx
    gpu_ctx.set_tuning("compact_bounce_rows", 65536)


def random_documents(n, seed):
    """"documents" of 1..40 rows covering [0, n), every one kept or dropped by a fair coin"""
    rng = np.random.default_rng(seed)
    keep, at = [], 0
    while at < n:
        ln = min(int(rng.integers(1, 41)), n - at)
        if rng.integers(0, 2):
            keep.append((at, at + ln))
        at += ln
    return keep


def keep_lists(n):
    return {
        "all": [(0, n)],
        "none": [],
        "all_but_row_0": [(1, n)],                              # delta = 1: every step bounced, each destination overlaps its sources
        "all_but_a_prefix_of_200": [(min(200, n), n)],          # delta >= B = 64: direct steps only
        "prefix_of_10_then_every_second": [(i, i + 1) for i in range(10, n, 2)],   # mixed
        "only_the_last_row": [(n - 1, n)],
        "random_documents": random_documents(n, 11),
        "empty_ranges_between": [(0, 0), (min(3, n), min(3, n)), (min(5, n), n), (n, n)],
    }


def kept_index(keep, n):
    return np.concatenate([np.arange(b, e, dtype=np.int64) for b, e in keep] + [np.zeros(0, np.int64)])


def expected_moved(idx):
    """the kept rows behind the first gap"""
    off = np.nonzero(idx != np.arange(len(idx)))[0]
    return int(len(idx) - off[0]) if len(off) else 0


def check_bytes(smt, ctx, x, n, keep):
    c = smt.Corpus(ctx)
    c.append(x[:n])
    before = ctx.compact_stats()
    moved = c.compact(keep)
    idx = kept_index(keep, n)
    assert c.rows == len(idx)
    got = c.read_rows(0, c.rows)
    assert np.array_equal(got.view(np.uint32), x[:n][idx].view(np.uint32))
    assert moved == expected_moved(idx)
    after = ctx.compact_stats()
    assert after.calls == before.calls + 1 and after.rows_moved == before.rows_moved + moved
    c.close()
    return moved


@pytest.mark.parametrize("n", [1, 33, 5000])
@pytest.mark.parametrize("case", list(keep_lists(1)))
def test_kept_rows_bit_for_bit(ctx64, x, n, case):
    import semtools_amd as smt

    moved = check_bytes(smt, ctx64, x, n, keep_lists(n)[case])
    if case in ("all", "none"):
        assert moved == 0


@pytest.mark.parametrize("case", ["all_but_row_0", "random_documents", "all_but_a_prefix_of_200"])
def test_default_bounce_across_its_border(gpu_ctx, x, case):
    """70 001 rows with the default 65 536-row bounce buffer: a bounced step of full capacity and a second, shorter one"""
    import semtools_amd as smt

    gpu_ctx.set_tuning("compact_bounce_rows", 65536)
    check_bytes(smt, gpu_ctx, x, N_MAX, keep_lists(N_MAX)[case])


def test_bounce_setting_is_clamped_to_its_floor(gpu_ctx, x):
    import semtools_amd as smt

    gpu_ctx.set_tuning("compact_bounce_rows", 1)     # floor 64
    try:
        check_bytes(smt, gpu_ctx, x, 1000, [(1, 1000)])
    finally:
        gpu_ctx.set_tuning("compact_bounce_rows", 65536)


def test_invalid_lists_leave_the_corpus_untouched(gpu_ctx, x):
    import semtools_amd as smt
    from semtools_amd import _lib as L

    n = 500
    c = smt.Corpus(gpu_ctx)
    c.append(x[:n])
    for bad in ([(10, 20), (0, 5)],          # unsorted
                [(0, 10), (9, 20)],          # overlapping
                [(0, 10), (490, n + 1)],     # end > rows
                [(7, 3)]):                   # begin > end
        with pytest.raises(smt.SmtError) as e:
            c.compact(bad)
        assert e.value.code == L.SMT_E_INVALID
        assert c.rows == n and np.array_equal(c.read_rows(0, n).view(np.uint32), x[:n].view(np.uint32))
    c.close()


def test_adopted_corpus_is_refused(gpu_ctx):
    import torch
    import semtools_amd as smt
    from semtools_amd import _lib as L

    t = torch.ones(100, 256, device="cuda")
    torch.cuda.synchronize()
    c = smt.Corpus(gpu_ctx, device_ptr=t.data_ptr(), rows=100)
    with pytest.raises(smt.SmtError) as e:
        c.compact([(50, 100)])
    assert e.value.code == L.SMT_E_UNSUPPORTED and c.rows == 100
    c.close()
    assert bool((t == 1).all())


def test_compact_stats_count_and_reset(gpu_ctx, x):
    import semtools_amd as smt

    gpu_ctx.compact_stats(reset=True)
    assert gpu_ctx.compact_stats() == (0, 0)
    c = smt.Corpus(gpu_ctx)
    c.append(x[:100])
    assert c.compact([(0, 40), (50, 100)]) == 50
    assert c.compact([(10, 90)]) == 80
    assert c.compact([(0, 80)]) == 0
    st = gpu_ctx.compact_stats(reset=True)
    assert st.calls == 3 and st.rows_moved == 130
    assert gpu_ctx.compact_stats() == (0, 0)
    c.close()


# ------------------------------------------------------------------ searches after a compaction

N_S = 5000


@pytest.fixture(scope="module")
def searched(gpu_ctx):
    """unit rows with planted duplicates (ties) and zero rows; the random-documents keep list; the fresh corpus of the kept rows"""
    import semtools_amd as smt

    emb = synth.unit_rows(N_S, seed=9)
    keep = random_documents(N_S, 23)
    kept = emb[kept_index(keep, N_S)]
    fresh = smt.Corpus(gpu_ctx)
    fresh.append(kept)
    yield emb, keep, kept, fresh
    fresh.close()


def same_answers(got, want):
    assert len(got) == len(want)
    for (gr, gd), (wr, wd) in zip(got, want):
        assert gr.tolist() == wr.tolist()
        assert np.array_equal(gd, wd)


@pytest.mark.parametrize("what", ["one_query", "three_queries", "top_100", "threshold", "workspace_threshold"])
def test_searches_equal_a_fresh_corpus(gpu_ctx, searched, what):
    import semtools_amd as smt
    from semtools_amd import _lib as L

    emb, keep, kept, fresh = searched
    c = smt.Corpus(gpu_ctx)
    c.append(emb)
    c.compact(keep)
    qs = synth.unit_query(3, nq=3)
    qs[1] = kept[len(kept) // 2]                      # a stored row: distance 0, and its planted duplicates tie
    kw = dict(one_query=dict(top_k=10), three_queries=dict(top_k=10), top_100=dict(top_k=100), threshold=dict(top_k=3, max_distance=0.9),
              workspace_threshold=dict(top_k=20, max_distance=0.95, mode=L.MODE_WORKSPACE))[what]
    q = qs[1:2] if what == "one_query" else qs
    same_answers(c.search(q, **kw), fresh.search(q, **kw))
    c.close()


def test_batch_re_packs_the_operand_image(gpu_ctx, searched):
    import semtools_amd as smt

    emb, keep, kept, fresh = searched
    c = smt.Corpus(gpu_ctx)
    c.append(emb)
    c.prepack(True)                                   # the image describes the rows as they are BEFORE the compaction
    qs = synth.unit_query(4, nq=16)
    qs[5] = kept[77]
    c.search(qs, top_k=10)
    size = c.image_bytes
    assert size > 0
    c.compact(keep)
    assert c.image_bytes == size                      # the allocation stays; tiles from the first moved row on are packed again
    same_answers(c.search(qs, top_k=10), fresh.search(qs, top_k=10))
    c.close()


def test_kept_range_set_survives(gpu_ctx, searched):
    import semtools_amd as smt

    emb, keep, kept, fresh = searched
    c = smt.Corpus(gpu_ctx)
    c.append(emb)
    ranges = [(b, b + 7) for b in range(3, len(kept) - 10, 50)]
    qs = synth.unit_query(6, nq=16)
    c.search(qs, top_k=5, ranges=ranges)
    c.search(qs, top_k=5, ranges=ranges)              # second sight: the list is kept on the device
    kept_sets, hits, builds = c.range_sets()
    assert kept_sets == 1 and builds == 1
    c.compact(keep)
    same_answers(c.search(qs, top_k=5, ranges=ranges), fresh.search(qs, top_k=5, ranges=ranges))
    kept_sets, hits_after, builds = c.range_sets()
    assert kept_sets == 1 and builds == 1 and hits_after > hits   # answered from the kept set: it depends on the ranges only
    c.close()


def test_append_after_compaction(gpu_ctx, searched):
    import semtools_amd as smt

    emb, keep, kept, fresh = searched
    c = smt.Corpus(gpu_ctx)
    c.append(emb)
    c.compact(keep)
    new = synth.unit_query(44, nq=40)
    assert c.append(new) == len(kept)
    assert c.rows == len(kept) + 40
    assert np.array_equal(c.read_rows(0, c.rows).view(np.uint32), np.concatenate([kept, new]).view(np.uint32))
    rows, dist = c.search(new[13], top_k=1)[0]
    assert rows.tolist() == [len(kept) + 13] and dist[0] < 1e-9
    c.close()


# ------------------------------------------------------------------ ordering against the one-query pipeline

def oracle_topk(emb, q, k):
    res = orc.search_documents(emb, [len(emb)], q, n_lines=0, top_k=k, accurate=True)
    return [r["match_line"] for r in res], [r["distance"] for r in res]


def test_ordered_between_overlapped_device_searches():
    """8 one-query device searches of the overlapped pipeline, the compaction, 8 more, ONE synchronisation: the first 8 answers
    are the old corpus's, the last 8 the new one's."""
    import torch
    import semtools_amd as smt

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(17)
    xt = torch.randn(N_OVERLAP, 256, device=dev, generator=g)
    xt /= xt.norm(dim=1, keepdim=True)
    qs = torch.randn(4, 256, device=dev, generator=g)
    qs /= qs.norm(dim=1, keepdim=True)
    emb = xt.cpu().numpy()
    del xt
    stream = torch.cuda.Stream(dev)
    ctx = smt.Context(0, stream=stream.cuda_stream)
    c = smt.Corpus(ctx)
    c.append(emb)
    ctx.set_tuning("async_select", 1)
    k = 10
    # drop 600 000 rows in front and every 7th document of 50 rows behind them: direct steps first, bounced ones after
    keep = [(b, min(b + 50, N_OVERLAP)) for i, b in enumerate(range(600_000, N_OVERLAP, 50)) if i % 7]
    with torch.cuda.stream(stream):
        rows = torch.full((16, k), -7, dtype=torch.int64, device=dev)
        dist = torch.full((16, k), -7.0, dtype=torch.float64, device=dev)
        status = torch.full((16,), 7, dtype=torch.int32, device=dev)
    stream.synchronize()
    for i in range(16):
        if i == 8:
            c.compact(keep)
        c.search_topk_device(qs[i % 4].data_ptr(), 1, k, 0, rows[i].data_ptr(), dist[i].data_ptr(), out_status_ptr=status[i:].data_ptr())
    ctx.synchronize()
    rows, dist, status = rows.cpu().numpy(), dist.cpu().numpy(), status.cpu().numpy()
    assert (status == 0).all(), status                # every answer PROVED
    new = emb[kept_index(keep, N_OVERLAP)]
    assert c.rows == len(new)
    qh = qs.cpu().numpy()
    for j in range(4):
        for base, mat in ((0, emb), (8, new)):
            wr, wd = oracle_topk(mat, qh[j], k)
            for i in (base + j, base + j + 4):
                assert rows[i].tolist() == wr, (i, rows[i], wr)
                assert np.allclose(dist[i], wd, rtol=0, atol=1e-12)
    c.close()
    ctx.close()


# ------------------------------------------------------------------ an index names rows by position

def test_ivf_index_after_compaction(gpu_ctx):
    import semtools_amd as smt

    n = 60_000
    xs = synth.clustered_rows_torch(n, 32, 8, 21, "cuda").cpu().numpy()
    c = smt.Corpus(gpu_ctx)
    c.append(xs)
    ix = smt.IvfPq(c, nlist=32, train_iters=5)
    q = xs[123]
    before = ix.search(q, top_k=5, nprobe=32)
    assert c.compact([(0, 1000), (1000, n)]) == 0     # keeps every row: nothing moves, the index stays valid
    after = ix.search(q, top_k=5, nprobe=32)
    same_answers(after, before)
    assert c.compact([(0, 1000), (1001, n)]) == n - 1001
    with pytest.raises(smt.SmtError, match="shrank"):
        ix.search(q, top_k=5, nprobe=32)
    ix.close()
    c.close()
