"""smt_sharded_corpus_compact: every shard keeps its part of a GLOBAL keep list and closes its own gaps; the piece list shrinks with
it.  Compared with a single-GPU corpus holding the same rows: bytes, searches (host form and device form, both transports), files."""
import numpy as np
import pytest

from tests import synth
from tests.test_gpu_compact import kept_index, random_documents, same_answers

pytestmark = pytest.mark.gpu

APPENDS = (700, 1300, 90, 900, 650)     # unequal; the 90 rows go to one shard (fewer than 64 per rank), the others are dealt over all
N = sum(APPENDS)


def build(smt, group, emb):
    sc = smt.ShardedCorpus(group, empty=True)
    at = 0
    for n in APPENDS:
        assert sc.append(emb[at:at + n]) == at
        at += n
    return sc


def piece_ranges(sc):
    out, at = [], 0
    for rows, rank in sc.layout():
        out.append((at, at + rows, rank))
        at += rows
    return out


def check_equal(smt, gpu_ctx, group, sc, want_rows, tmp_path, tag, tie_query=None):
    import torch

    n_ranks = group.info()["n_ranks"]
    assert sc.rows == len(want_rows)
    assert np.array_equal(sc.read_rows(0, sc.rows).view(np.uint32), want_rows.view(np.uint32))
    layout = sc.layout()
    assert sum(r for r, _ in layout) == sc.rows and all(r > 0 for r, _ in layout)
    assert int(sc.rank_rows().sum()) == sc.rows
    for (r0, k0), (r1, k1) in zip(layout, layout[1:]):
        assert k0 != k1                                # neighbours on one rank have merged
    single = smt.Corpus(gpu_ctx)
    single.append(want_rows)
    qs = synth.unit_query(12, nq=3)
    if tie_query is not None:
        qs[2] = tie_query
    k = 10
    want = single.search(qs, top_k=k)
    if tie_query is not None:
        assert want[2][1][0] == want[2][1][1]          # the tie pair leads the list, lower global row first
    same_answers(sc.search(qs, top_k=k), want)
    same_answers(sc.search(qs[1], top_k=3, max_distance=0.95), single.search(qs[1], top_k=3, max_distance=0.95))
    ranges = [(5, 40), (sc.rows // 2, sc.rows // 2 + 300)]
    same_answers(sc.search(qs, top_k=k, ranges=ranges), single.search(qs, top_k=k, ranges=ranges))
    qd = torch.from_numpy(qs).cuda()
    for transport in ("peer", "copy") if n_ranks > 1 else ("peer",):
        if n_ranks > 1:
            group.set_transport(transport)
        outs = [torch.full((3, 2, k), -1, dtype=torch.int64, device="cuda") for _ in range(n_ranks)]
        torch.cuda.synchronize()
        sc.search_topk_device([qd.data_ptr()] * n_ranks, 3, k, [o.data_ptr() for o in outs])
        group.synchronize()
        for o in outs:
            m = o.cpu().numpy()
            for i in range(3):
                assert np.ascontiguousarray(m[i, 0]).view(np.uint64).tolist() == want[i][0].tolist(), (transport, i)
                assert np.array_equal(np.ascontiguousarray(m[i, 1]).view(np.float64), want[i][1])
    a, b = tmp_path / f"sharded_{tag}.f32", tmp_path / f"single_{tag}.f32"
    sc.save(a)
    single.save(b)
    assert a.read_bytes() == b.read_bytes()
    single.close()


@pytest.mark.parametrize("n_ranks", [1, 3])
def test_sharded_compaction_equals_the_single_corpus(gpu_ctx, tmp_path, n_ranks):
    import semtools_amd as smt

    emb = synth.unit_rows(N, seed=14)
    keep = random_documents(N, 31)
    idx = kept_index(keep, N)
    # a tie pair that straddles two pieces: a kept row of the first append copied over a kept row of the fourth
    ta = int(idx[idx < APPENDS[0]][5])
    tb = int(idx[idx >= sum(APPENDS[:3])][5])
    emb[tb] = emb[ta]
    group = smt.Group.logical(0, n_ranks)
    sc = build(smt, group, emb)
    if n_ranks > 1:
        assert max(np.bincount([rank for _, rank in sc.layout()])) >= 3      # every rank holds several pieces
        pieces = piece_ranges(sc)
        assert [p for p in pieces if p[0] <= ta < p[1]] != [p for p in pieces if p[0] <= tb < p[1]]
    moved = sc.compact(keep)
    assert 0 < moved <= len(idx)
    kept = emb[idx]
    check_equal(smt, gpu_ctx, group, sc, kept, tmp_path, "first", tie_query=emb[ta])
    # a second append and a second compaction -- this one empties one whole piece
    more = synth.unit_rows(800, seed=15)
    assert sc.append(more) == len(kept)
    now = np.concatenate([kept, more])
    pieces = piece_ranges(sc)
    b, e, _ = pieces[1] if len(pieces) > 1 else (0, len(now) // 2, 0)      # (one shard holds one piece: its first half goes)
    keep2 = [r for r in [(0, b), (e, len(now))] if r[1] > r[0]]
    n_pieces = len(pieces)
    sc.compact(keep2)
    assert len(sc.layout()) < n_pieces or n_pieces == 1
    check_equal(smt, gpu_ctx, group, sc, now[kept_index(keep2, len(now))], tmp_path, "second")
    sc.close()
    group.close()


def test_invalid_global_list_is_refused(gpu_ctx):
    import semtools_amd as smt
    from semtools_amd import _lib as L

    emb = synth.unit_rows(N, seed=14)
    group = smt.Group.logical(0, 3)
    sc = build(smt, group, emb)
    layout = sc.layout()
    for bad in ([(10, 20), (0, 5)], [(0, 10), (9, 20)], [(0, N + 1)], [(7, 3)]):
        with pytest.raises(smt.SmtError) as e:
            sc.compact(bad)
        assert e.value.code == L.SMT_E_INVALID
    assert sc.layout() == layout and np.array_equal(sc.read_rows(0, N).view(np.uint32), emb.view(np.uint32))
    assert sc.compact([(0, N)]) == 0 and sc.layout() == layout          # keep-all: nothing moves, the pieces stay
    sc.close()
    group.close()
