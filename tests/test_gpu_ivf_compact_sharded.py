"""GPU: smt_sharded_ivfpq_compact on three logical shards -- a GLOBAL keep list that crosses piece borders; every shard's index must
be tests/ivf_compact_ref.carry of what it was under ITS part of the list, which the test cuts out of the piece layout as it is before
the call.  Byte for byte, and the searches before (inside the list) and after (unfiltered) must agree as in test_gpu_ivf_compact.py."""
import numpy as np
import pytest

from tests import ivf_compact_ref as K
from tests import ivf_ref as R
from tests.test_gpu_compact import kept_index, random_documents

pytestmark = pytest.mark.gpu

APPENDS = (2400, 1800, 90, 1717)        # 6 007 rows; the 90 go to one shard, the others are dealt over all three: several pieces per rank
N = sum(APPENDS)
NLIST, N_RANKS = 32, 3


def build(smt, group, emb):
    sc = smt.ShardedCorpus(group, empty=True)
    at = 0
    for n in APPENDS:
        assert sc.append(emb[at:at + n]) == at
        at += n
    return sc


def localize(layout, keep, rank):
    """The part of a global range list that lies on `rank`, in that rank's local rows (adjacent ranges merged)."""
    out, g, lb = [], 0, 0
    for rows, rk in layout:
        if rk == rank:
            for b, e in keep:
                lo, hi = max(b, g), min(e, g + rows)
                if hi > lo:
                    r = (lb + lo - g, lb + hi - g)
                    if out and out[-1][1] == r[0]:
                        out[-1] = (out[-1][0], r[1])
                    else:
                        out.append(r)
            lb += rows
        g += rows
    return out


def shard_files(six, path):
    six.save(path)
    parts = [path.parent / f"{path.name}.r{r}of{N_RANKS}" for r in range(N_RANKS)]
    return [p.read_bytes() for p in parts], [R.read_index(p) for p in parts]


@pytest.mark.parametrize("shared", [True, False], ids=["shared_centroids", "separate_centroids"])
def test_every_shard_carries_its_part(gpu_ctx, tmp_path, shared):
    import semtools_amd as smt

    emb = R.iso_rows(N, 78)
    group = smt.Group.logical(0, N_RANKS)
    sc = build(smt, group, emb)
    layout = sc.layout()
    assert max(np.bincount([rank for _, rank in layout])) >= 3          # every rank holds several pieces
    six = smt.ShardedIvfPq(sc, nlist=NLIST, train_iters=5, local_pca=True, shared_centroids=shared)
    for r in range(N_RANKS):
        assert six.shard_list_sizes(r, NLIST).max() <= 512
    _, before = shard_files(six, tmp_path / "before.ivf")
    if shared:
        assert all(f["centroids"].tobytes() == before[0]["centroids"].tobytes() for f in before)
    keep = random_documents(N, 41)                                      # "documents" of 1 .. 40 rows, kept or dropped by a fair coin
    borders = np.cumsum([rows for rows, _ in layout])[:-1]
    assert any(b < x < e for b, e in keep for x in borders)             # a kept range straddles a piece border
    idx = kept_index(keep, N)
    local = [localize(layout, keep, r) for r in range(N_RANKS)]
    assert sum(e - b for l in local for b, e in l) == len(idx)
    qs = R.iso_rows(16, 79)
    answers = {p: six.search(qs, top_k=10, nprobe=p, rerank=512, ranges=keep) for p in (4, 32)}
    moved, dropped = six.compact(keep)
    assert dropped == N - len(idx) and 0 < moved <= len(idx)
    assert sc.rows == len(idx) and np.array_equal(sc.read_rows(0, sc.rows).view(np.uint32), emb[idx].view(np.uint32))
    _, after = shard_files(six, tmp_path / "after.ivf")
    for r in range(N_RANKS):
        assert K.same_index(K.carry(before[r], local[r]), after[r]) == [], r
    assert six.info()["rows"] == len(idx)
    for nprobe, want in answers.items():
        got = six.search(qs, top_k=10, nprobe=nprobe, rerank=512)
        for qi, ((gr, gd), (wr, wd)) in enumerate(zip(got, want)):
            alive, new = K.remap(wr, keep)
            assert alive.all() and len(wr) == 10
            assert gr.tolist() == new.tolist(), (nprobe, qi)
            assert gd.tobytes() == wd.tobytes(), (nprobe, qi)
    six.close(); sc.close(); group.close()


def test_refusals_leave_every_shard_untouched(gpu_ctx, tmp_path):
    import semtools_amd as smt
    from semtools_amd import _lib as L

    emb = R.iso_rows(N, 78)
    group = smt.Group.logical(0, N_RANKS)
    sc = build(smt, group, emb)
    layout = sc.layout()
    six = smt.ShardedIvfPq(sc, nlist=NLIST, train_iters=5, local_pca=True, shared_centroids=True)
    before, _ = shard_files(six, tmp_path / "before.ivf")
    first_piece = (0, layout[0][0])                                     # rows of ONE rank only: the other shards' indexes would end empty
    for bad, code in (([(10, 20), (0, 5)], L.SMT_E_INVALID), ([(0, N + 1)], L.SMT_E_INVALID), ([first_piece], L.SMT_E_UNSUPPORTED)):
        with pytest.raises(smt.SmtError) as e:
            six.compact(bad)
        assert e.value.code == code, bad
        assert sc.layout() == layout and np.array_equal(sc.read_rows(0, N).view(np.uint32), emb.view(np.uint32))
        assert shard_files(six, tmp_path / "after.ivf")[0] == before
    assert six.compact([(0, 3000), (3000, N)]) == (0, 0)                # keep-all: nothing moves
    assert sc.layout() == layout and shard_files(six, tmp_path / "after.ivf")[0] == before
    six.close(); sc.close(); group.close()
