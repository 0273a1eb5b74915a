"""The inputs of tests/test_gpu_decoys.py, checked in float64 with NumPy (no GPU): a decoy test proves something only if every finite
decoy would WIN wherever it leaked.  For every fixture the GPU tests use: each finite decoy is strictly nearer to every query than the
nearest allowed row and lies under every max_distance the tests pass, the oracle run on the whole buffer returns decoys only, and the
builders put allowed rows and decoys where they claim.  A fixture that fails here is changed, never the condition."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import decoys as D


@pytest.fixture(scope="module")
def qs():
    return D.queries()


def _conditions(buf, decoy_mask, qs, k=10):
    """The three conditions on a buffer whose rows `decoy_mask` marks as (finite) decoys."""
    dist = D.distances64(buf, qs)                                  # [rows, queries]
    dec, allowed = dist[decoy_mask], dist[~decoy_mask]
    assert np.isfinite(dec).all()
    assert (dec.max(axis=0) < allowed.min(axis=0)).all(), (dec.max(), allowed.min())
    assert dec.max() < min(D.MAX_DISTANCES)
    decoy_ids = set(np.flatnonzero(decoy_mask).tolist())
    kk = min(k, int(decoy_mask.sum()))
    for q in qs[::13]:
        res = orc.search_documents(buf, [len(buf)], q, n_lines=0, top_k=kk, accurate=True)
        assert len(res) == kk and all(r["match_line"] in decoy_ids for r in res)


def test_queries_sit_at_cosine_point_nine_from_the_centre(qs):
    c = D.centre().astype(np.float64)
    q = qs.astype(np.float64)
    assert len(qs) == D.NQ_MAX >= 130
    assert np.abs(np.linalg.norm(q, axis=1) - 1.0).max() < 1e-6 and abs(np.linalg.norm(c) - 1.0) < 1e-6
    assert np.abs(q @ c - D.COS_QC).max() < 1e-6
    assert len({x.tobytes() for x in qs}) == len(qs)               # distinct queries


def test_finite_decoys_are_exact_power_of_two_multiples_of_the_centre():
    c = D.centre()
    d = D.finite_decoys(12)
    for i, row in enumerate(d):
        j = D.SCALES[i % 5]
        assert np.array_equal(row, c * np.float32(2.0 ** j))
        assert np.array_equal(np.frexp(row)[0], np.frexp(c)[0])    # the same significands: only the exponent moved
    assert {D.SCALES[i % 5] for i in range(12)} == {-2, -1, 0, 1, 2}
    assert np.array_equal(D.finite_decoys(7, unit_only=True), np.repeat(c[None, :], 7, axis=0))
    nf = D.nonfinite_decoys(6)
    assert np.isnan(nf[0::2]).all() and np.isposinf(nf[1::2]).all()


@pytest.mark.parametrize("n", D.SIZES_A + (D.N_LARGEK,))
def test_layout_a(qs, n):
    buf, first = D.layout_a(n, seed=100 + n)
    assert first == D.G >= 64 and buf.shape == (n + 2 * D.G, 256)
    assert np.array_equal(buf[first:first + n], D.allowed_rows(n, 100 + n))
    mask = np.ones(len(buf), dtype=bool)
    mask[first:first + n] = False
    assert mask.sum() == 2 * D.G
    _conditions(buf, mask, qs)
    nf, _ = D.layout_a(n, seed=100 + n, flavour="nonfinite")
    assert np.array_equal(nf[first:first + n], buf[first:first + n])
    assert not np.isfinite(nf[mask]).any()
    assert np.isposinf(nf[first - 1]).all() and np.isposinf(nf[first + n]).all()      # an Inf row touches the corpus at either end
    if n >= 32:
        assert not buf[first + n // 3].any() and np.array_equal(buf[first + n - 2], buf[first + 1])   # a zero row and a duplicate


def test_range_lists_have_the_borders_the_kernels_care_about():
    n = D.N_B
    lists = D.range_lists(n)
    for name, ranges in lists.items():
        assert all(0 <= b <= e <= n for b, e in ranges), name
        assert all(ranges[i][1] <= ranges[i + 1][0] for i in range(len(ranges) - 1)), name     # sorted, disjoint
        assert ranges[0][0] == 0 and ranges[-1][1] == n, name
        assert any(b == e for b, e in ranges) and any(e - b == 1 for b, e in ranges), name      # empty ranges, single rows
        nonempty = [(b, e) for b, e in ranges if e > b]
        assert {b % 4 for b, _ in nonempty} == {e % 4 for _, e in nonempty} == set(range(4)), name
        # every range (but the one that ends at n) is followed by a decoy row: "one row too many" lands on a decoy
        mask = D.in_ranges(n, ranges)
        assert all(not mask[e] for _, e in nonempty if e < n), name
    dense = [(b, e) for b, e in lists["dense"] if e > b]
    assert {b % 32 for b, _ in dense} == {e % 32 for _, e in dense} == set(range(32))
    assert any(dense[i + 1][0] - dense[i][1] == 1 for i in range(len(dense) - 1))              # two ranges one decoy row apart
    # the tile table's density rule (common.h tiles_dense): tiles touched x 32 <= 4 x rows wanted -- and not for the sparse list
    for name, want in (("dense", True), ("sparse", False)):
        mask = D.in_ranges(n, lists[name])
        tiles = len({r // 32 for r in np.flatnonzero(mask)})
        assert (tiles * 32 <= 4 * int(mask.sum())) == want, name
    # three shards of ceil(n / 3) rows: a range crosses either border
    cut = -(-n // 3)
    for border in (cut, 2 * cut):
        assert any(b < border < e for b, e in dense), border


@pytest.mark.parametrize("name", ["dense", "sparse"])
@pytest.mark.parametrize("unit_only", [False, True])
def test_layout_b(qs, name, unit_only):
    n = D.N_B
    ranges = D.range_lists(n)[name]
    emb, elig = D.layout_b(n, ranges, seed=11, unit_only=unit_only)
    mask = D.in_ranges(n + D.G, ranges)
    assert emb.shape == (n + D.G, 256) and not mask[n:].any()                               # G guards behind the corpus
    assert np.array_equal(elig, np.flatnonzero(mask)) and 0 < len(elig) < n
    assert np.array_equal(emb[elig], D.allowed_rows(n, 11)[elig])
    c = D.centre()
    for r in np.flatnonzero(~mask):
        assert np.array_equal(np.frexp(emb[r])[0], np.frexp(c)[0])
    if unit_only:
        assert np.abs((emb.astype(np.float64) ** 2).sum(axis=1)[~mask] - 1.0).max() < 1e-3    # what smt_ivfpq_build accepts
    _conditions(emb, ~mask, qs)


@pytest.mark.parametrize("n", D.SIZES_C)
def test_layout_c(qs, n):
    rows = D.layout_c(n, seed=300 + n)
    assert rows.shape == (n + D.G, 256) and np.array_equal(rows[:n], D.allowed_rows(n, 300 + n))
    mask = np.arange(n + D.G) >= n
    _conditions(rows, mask, qs)
    # the allowed row planted before a compaction is the nearest allowed row of every query, and still farther than any decoy
    near = D.near_row()
    dn = D.distances64(near[None, :], qs)[0]
    assert (dn < D.distances64(rows[:n], qs).min(axis=0)).all() and (dn > D.distances64(rows[n:], qs).max(axis=0)).all()


def test_layout_shards(qs):
    sizes = (1301, 33, 1666)
    buf, first, rows = D.layout_shards(sizes, seed=21)
    assert first == [D.G, D.G + 1301 + D.G, D.G + 1301 + D.G + 33 + D.G] and len(buf) == sum(sizes) + 4 * D.G
    mask = np.ones(len(buf), dtype=bool)
    done = 0
    for f, s in zip(first, sizes):
        assert np.array_equal(buf[f:f + s], rows[done:done + s])
        mask[f:f + s] = False
        done += s
    assert mask.sum() == 4 * D.G
    _conditions(buf, mask, qs)


def test_expected_never_sees_a_decoy_and_maps_ids_back(qs):
    n = D.N_B
    ranges = D.range_lists(n)["dense"]
    emb, elig = D.layout_b(n, ranges, seed=11)
    allowed = set(elig.tolist())
    for rows, dist in D.expected(emb[elig], elig, qs[:3], 10):
        assert len(rows) == 10 and set(rows) <= allowed and (np.diff(dist) >= 0).all() and dist[0] > 0.5
    under = D.expected(emb[elig], elig, qs[:3], 3, max_distance=0.85)
    for (rows, dist), q in zip(under, qs[:3]):
        d = D.distances64(emb[elig], q)[:, 0]
        assert len(rows) == int((d < 0.85).sum()) and set(rows) <= allowed
    for rows, dist in D.expected_workspace(emb[elig], elig, qs[:3], 5, 0.85):
        assert len(rows) <= 5 and (dist < 0.85).all()
