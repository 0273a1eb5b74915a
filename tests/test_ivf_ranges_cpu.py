"""CPU: the helpers of tests/ivf_ranges_ref.py against brute-force loops, on an index written in the file format by
ivf_ref.write_index; and the C ABI of the search inside ranges (three symbols, exported by the library and declared in the header)."""
import os
import re

import numpy as np
import pytest

from tests import ivf_ranges_ref as G
from tests import ivf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NLIST = 1000, 32
SYMBOLS = ("smt_ivfpq_search_ranges", "smt_ivfpq_search_ranges_device", "smt_sharded_ivfpq_search_ranges")


@pytest.fixture(scope="module")
def ix(tmp_path_factory):
    """A tiny index with real lists (rows in ascending order inside a list, as the build leaves them); the quantisers are zeros: no
    helper looks at them.  N is no multiple of 64: the last mask word is partial."""
    x = R.iso_rows(N, seed=11)
    cent = x[:: N // NLIST][:NLIST].copy()
    a = np.argmax(R.assign_scores(x, cent), axis=1)
    d = dict(nlist=NLIST, n_rows=N, kind=0, centroids=cent, cnorm_half=np.zeros(NLIST, np.float32),
             codebooks=np.zeros((R.PQ_M, R.PQ_K, R.PQ_DSUB), np.float32),
             offsets=np.concatenate([[0], np.cumsum(np.bincount(a, minlength=NLIST))]).astype(np.uint64),
             ids=np.argsort(a, kind="stable").astype(np.uint32), codes=np.zeros((N, R.PQ_M), np.uint8))
    path = tmp_path_factory.mktemp("ivf") / "ranges.ivf"
    R.write_index(path, d)
    return R.read_index(path)


def _sets(ix):
    big = int(np.argmax(np.diff(ix["offsets"].astype(np.int64))))
    size = int(ix["offsets"][big + 1] - ix["offsets"][big])
    return dict(alternate=G.alternate_blocks(N), scattered=G.scattered_rows(N), empties=G.with_empty_members(N),
                second=G.every_second_row(N), none=[(5, 5)], no_ranges=[], all=[(0, N)],
                border=G.borders_at(ix, big, 1, size - 1))


def _valid(ranges, n):
    prev = 0
    for b, e in ranges:
        assert prev <= b <= e <= n, (prev, b, e)
        prev = e


def test_builders_give_valid_range_sets(ix):
    for name, rs in _sets(ix).items():
        _valid(rs, N)
    assert len(G.scattered_rows(N)) == 40 and all(e == b + 1 for b, e in G.scattered_rows(N))
    assert G.alternate_blocks(250) == [(0, 100), (200, 250)]
    assert sum(b == e for b, e in G.with_empty_members(N)) >= 5 and sum(e > b for b, e in G.with_empty_members(N)) == 4
    assert len(G.every_second_row(N)) == N // 2


def test_in_ranges_against_a_loop(ix):
    rows = np.arange(N + 3)
    for name, rs in _sets(ix).items():
        want = [any(b <= r < e for b, e in rs) for r in rows]
        assert G.in_ranges(rows, rs).tolist() == want, name
    assert G.in_ranges(np.array([], dtype=np.int64), [(0, 5)]).shape == (0,)


def test_list_order_mask_against_a_loop(ix):
    for name, rs in _sets(ix).items():
        m = G.list_order_mask(ix, rs)
        assert m.dtype == np.dtype("<u8") and len(m) == (N + 63) // 64
        for p in range(len(m) * 64):
            want = p < N and any(b <= int(ix["ids"][p]) < e for b, e in rs)
            assert bool((int(m[p // 64]) >> (p % 64)) & 1) == want, (name, p)


def test_borders_at_cuts_exactly_those_positions(ix):
    off = ix["offsets"].astype(np.int64)
    for l in range(NLIST):
        size = int(off[l + 1] - off[l])
        ids = ix["ids"][off[l]:off[l + 1]].astype(np.int64)
        assert (np.diff(ids) > 0).all()
        for p0, p1 in ((0, 1), (0, size), (1, size - 1), (size - 1, size)):
            if not 0 <= p0 < p1 <= size:
                continue
            keep = G.in_ranges(ids, G.borders_at(ix, l, p0, p1))
            assert np.nonzero(keep)[0].tolist() == list(range(p0, p1)), (l, p0, p1)


def test_the_three_entry_points_are_exported_and_declared():
    from semtools_amd import _lib as L

    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "semtools_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), f"libsemtools_hip.so does not export {name}"
        assert name in L.EXPORTS
        assert re.search(r"^int %s\(" % name, header, re.M), f"include/semtools_hip.h does not declare {name}"
