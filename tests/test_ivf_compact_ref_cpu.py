"""CPU: tests/ivf_compact_ref.carry -- the contract of smt_ivfpq_compact in NumPy -- on a hand-made index that went through the
file format (ivf_ref.write_index / read_index): 300 rows in 32 lists, one of them empty to begin with."""
import numpy as np
import pytest

from tests import ivf_compact_ref as K
from tests import ivf_ref as R

N, NLIST, EMPTY, VICTIM = 300, 32, 5, 7


@pytest.fixture(scope="module")
def index(tmp_path_factory):
    rng = np.random.default_rng(3)
    lists = [l for l in range(NLIST) if l != EMPTY]
    list_of = rng.choice(lists, N)
    list_of[:len(lists)] = lists                                       # every other list holds a row
    order = np.lexsort((np.arange(N), list_of))                        # list order, rows ascending inside a list
    ix = dict(nlist=NLIST, n_rows=N, kind=1,
              centroids=rng.standard_normal((NLIST, R.DIM)).astype("<f4"), cnorm_half=rng.random(NLIST).astype("<f4"),
              codebooks=rng.standard_normal((R.PQ_M, R.PQ_K, R.PQ_DSUB)).astype("<f4"),
              offsets=np.concatenate([[0], np.cumsum(np.bincount(list_of, minlength=NLIST))]).astype("<u8"),
              ids=order.astype("<u4"), codes=rng.integers(0, 256, (N, R.PQ_M)).astype("u1"),
              basis=rng.standard_normal((NLIST, R.LP_DIMS, R.DIM)).astype("<f4"), lscale=rng.random((NLIST, R.LP_DIMS)).astype("<f4"))
    path = tmp_path_factory.mktemp("ivf") / "hand.ivf"
    R.write_index(path, ix)
    f = R.read_index(path)
    assert not K.same_index(ix, f)
    assert f["offsets"][EMPTY] == f["offsets"][EMPTY + 1] and f["offsets"][VICTIM] < f["offsets"][VICTIM + 1]
    return f


def complement(rows, n):
    keep, at = [], 0
    for r in sorted(int(r) for r in rows):
        if r > at:
            keep.append((at, r))
        at = r + 1
    return keep + ([(at, n)] if at < n else [])


def keep_lists(f):
    victims = f["ids"][int(f["offsets"][VICTIM]):int(f["offsets"][VICTIM + 1])]
    return dict(empties_a_list=complement(victims, N), drops_nothing=[(0, 100), (100, 100), (100, N)], one_row=[(137, 138)],
                documents=[(3, 40), (41, 42), (100, 164), (200, 299)])


@pytest.mark.parametrize("case", ["empties_a_list", "drops_nothing", "one_row", "documents"])
def test_carry(index, case):
    f = index
    keep = keep_lists(f)[case]
    g = K.carry(f, keep)
    kept = np.concatenate([np.arange(b, e) for b, e in keep])           # kept[new row] = old row
    # the file's own invariants
    off = g["offsets"].astype(np.int64)
    assert g["n_rows"] == len(kept) == len(g["ids"]) == len(g["codes"]) and off[0] == 0 and off[-1] == g["n_rows"]
    assert (np.diff(off) >= 0).all()
    assert sorted(g["ids"].tolist()) == list(range(len(kept)))          # every kept row once, nothing else
    for l in range(NLIST):
        ids = g["ids"][off[l]:off[l + 1]].astype(np.int64)
        assert (np.diff(ids) > 0).all()                                 # ascending inside a list
        # the list holds exactly its old rows that were kept, and each kept row kept its code
        old = f["ids"][int(f["offsets"][l]):int(f["offsets"][l + 1])].astype(np.int64)
        assert kept[ids].tolist() == [r for r in old.tolist() if r in set(kept.tolist())]
    _, old_pos = R.list_of_rows(f)
    assert np.array_equal(g["codes"], f["codes"][old_pos[kept[g["ids"].astype(np.int64)]]])
    for name in ("centroids", "cnorm_half", "codebooks", "basis", "lscale"):
        assert g[name] is f[name]
    if case == "empties_a_list":
        assert off[VICTIM] == off[VICTIM + 1] and off[EMPTY] == off[EMPTY + 1] and g["n_rows"] < N
    if case == "drops_nothing":
        assert not K.same_index(f, g)
    if case == "one_row":
        assert g["n_rows"] == 1 and g["ids"].tolist() == [0] and np.diff(off).max() == 1
        assert np.array_equal(g["codes"][0], f["codes"][old_pos[137]])


def test_carried_index_goes_through_the_file_format(index, tmp_path):
    g = K.carry(index, keep_lists(index)["documents"])
    R.write_index(tmp_path / "carried.ivf", g)
    assert not K.same_index(g, R.read_index(tmp_path / "carried.ivf"))


def test_remap_is_the_prefix_map():
    alive, new = K.remap(np.arange(12), [(2, 4), (4, 4), (7, 10)])
    assert alive.tolist() == [False, False, True, True, False, False, False, True, True, True, False, False]
    assert new[alive].tolist() == [0, 1, 2, 3, 4]
