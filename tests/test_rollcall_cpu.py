"""The inputs of tests/test_gpu_rollcall.py, checked in float64 with NumPy and against the oracle (no GPU), and the proof that the roll
call bites: a NumPy search that skips one kind of row fails it, while the random-corpus cases at k = 10 (the corpus, the range list
and the queries of tests/test_gpu_scan.py::test_many_small_ranges_all_paths) mostly do not notice.  A fixture that fails here is
changed, never the condition."""
import numpy as np
import pytest

from tests import decoys as D
from tests import rollcall as R
from tests import synth


# ---------------------------------------------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize("name", R.FIXTURES)
def test_fixture_conditions(name):
    fx = R.fixture(name)
    rc = fx.rc
    # every allowed row is in exactly one expected list, at the place its cosine says
    seen = np.concatenate(rc.lists)
    assert len(seen) == rc.n and np.array_equal(np.sort(seen), np.arange(rc.n))
    assert sum(size * len(js) for size, js in rc.by_size.items()) == rc.n and max(rc.by_size) <= rc.k
    assert rc.J == -(-rc.n // rc.k) <= R.J_MAX and len({q.tobytes() for q in rc.queries}) == len(rc.queries)
    norms = np.linalg.norm(rc.rows.astype(np.float64), axis=1)
    assert np.abs(norms - 1.0).max() < 1e-6
    # the buffer: the roll call's rows at the allowed ids, filler rows -- orthogonal to every query -- everywhere else
    if fx.ids is not None:
        assert np.array_equal(fx.buf[fx.ids], rc.rows) and len(fx.buf) == fx.total
        out = np.ones(fx.total, dtype=bool)
        out[fx.ids] = False
        assert out.any() and not fx.buf[out][:, :R.J_MAX].any()
        assert np.abs(np.linalg.norm(fx.buf[out].astype(np.float64), axis=1) - 1.0).max() < 1e-6
    # the oracle's accurate form over the allowed rows returns exactly those lists
    got = R.oracle_lists(rc, fx.ids)
    dist = D.distances64(rc.rows, rc.queries[:rc.J])                # [rows, queries]
    step = R.nominal_step(rc.k)
    for j in range(rc.J):
        rows, d = got[j]
        assert rows == fx.global_rows(j), (name, j)
        mine = rc.lists[j]
        d64 = dist[mine, j]
        assert np.abs(d64 - (1.0 - rc.cos[j])).max() < 1e-6, (name, j)
        assert np.abs(d - d64).max() < 1e-6, (name, j)
        if len(mine) > 1:
            # consecutive distances at least half a step apart, no two equal
            assert np.diff(d64).min() >= 0.5 * step, (name, j, np.diff(d64).min(), step)
            assert len(np.unique(d64)) == len(d64) and len(np.unique(d)) == len(d), (name, j)
        # the best unowned row is at least 0.3 behind the last place
        others = np.ones(rc.n, dtype=bool)
        others[mine] = False
        if others.any():
            assert dist[others, j].min() - d64.max() >= 0.3, (name, j, dist[others, j].min(), d64.max())


@pytest.mark.parametrize("name", R.SWEEP_FIXTURES)
def test_sweep_query_owns_every_row_in_row_order(name):
    """K4's query: the distances rise strictly with the row in steps of at most 5e-5, are distinct in f64, all under max_distance =
    0.9 by more than 0.02, and the oracle's threshold mode returns every allowed row in that order."""
    fx = R.fixture(name)
    rc = fx.rc
    assert rc.sweep and len(rc.queries) == rc.J + 1
    q = rc.queries[rc.J:]
    d = D.distances64(rc.rows, q)[:, 0]
    assert (np.diff(d) > 0).all() and np.diff(d).max() <= R.SWEEP_STEP_MAX * 1.001 and len(np.unique(d)) == rc.n
    assert np.diff(d).min() > 1e-6                                  # (f32 resolves 6e-8 here)
    assert d.max() < R.SWEEP_MAX_DISTANCE - 0.02 and d.min() > 0.7
    rows, od = D.expected(rc.rows, fx.ids, q, 1, max_distance=R.SWEEP_MAX_DISTANCE)[0]
    assert rows == (np.arange(rc.n) if fx.ids is None else fx.ids).tolist()
    assert len(np.unique(od)) == rc.n and (np.diff(od) > 0).all()
    # the ordinary queries at the same max_distance: their own set and nothing else
    for j in (0, rc.J - 1):
        rows, _ = D.expected(rc.rows, fx.ids, rc.queries[j:j + 1], 1, max_distance=R.SWEEP_MAX_DISTANCE)[0]
        assert rows == fx.global_rows(j)


def test_assignments_and_orders():
    owner, rank, J = R.assign(4097, 56, "strided")
    assert J == 74 and owner[:3].tolist() == [0, 1, 2] and rank[73:76].tolist() == [0, 1, 1]
    owner, rank, J = R.assign(4097, 56, "contiguous")
    assert J == 74 and owner[55:58].tolist() == [0, 1, 1] and rank[55:58].tolist() == [55, 0, 1] and (owner[-9:] == 73).all()
    assert np.allclose(R.ladder(56)[[0, -1]], [0.95, 0.40]) and np.allclose(R.ladder(1024)[[0, -1]], [0.95, 0.45])
    assert np.allclose(np.diff(R.ladder(56)), -0.01)
    # ascending: the first row of a set is its nearest; descending: its last; shuffled: neither order
    for order, first in (("ascending", 0), ("descending", 55)):
        rc = R.roll_call(4097, 56, "contiguous", order, seed=5)
        assert rc.lists[3][0] == 3 * 56 + first and rc.lists[3][-1] == 3 * 56 + 55 - first
    rc = R.roll_call(4097, 56, "contiguous", "shuffled", seed=5)
    assert sorted(rc.lists[3].tolist()) == list(range(168, 224)) and (np.diff(rc.lists[3]) < 0).any() and (np.diff(rc.lists[3]) > 0).any()
    assert {R.fixture(n).rc.order for n in R.FIXTURES} == set(R.ORDERS)
    assert {R.fixture(n).rc.assignment for n in R.FIXTURES} == set(R.ASSIGNMENTS)
    assert R.ends(4097, 192)[1][[0, -1]].tolist() == [3905, 4096] and len(R.ends(100, 192)) == 1


def test_layout_c_seams_and_shards():
    stages = R.stages_c()
    assert [s[1] for s in stages] == [R.N, R.N + 10, R.N + 5] == [R.fixture("C-" + s[0]).rc.n for s in stages]
    keep = stages[2][2]
    assert sum(e - b for b, e in keep) == R.N + 5 and all(b % 16 for b, _ in keep[1:]) and all(e % 16 for _, e in keep[:-1])
    assert sum(R.SHARDS) == R.N and len(set(R.SHARDS)) == 3 and 1 in R.SHARDS
    assert sum(R.SHARDS_LARGEK) == R.fixture("S-1024").rc.n > 3 * 5000
    assert R.N % 32 and R.N % 4 and R.N_I2 % 32 and 4001 // 32 == (R.N_I2 - 1) // 32 - 1   # the append crosses the old ragged tile


# ---------------------------------------------------------------------------------------------------------------- the range tables
@pytest.mark.parametrize("which", ["dense", "sparse"])
def test_range_tables_cover_the_allowed_set_exactly(which):
    """build_chunk_table_kernel's and build_tile_table_kernel's arithmetic (restated in tests/rollcall.py from range_tables.hip and
    search.cpp range_prefixes): the union of the descriptors is exactly the allowed set, no row and no tile twice."""
    ranges, ids = R.range_ids(which)
    rr, prefix, cp, tp = R.range_prefixes(ranges)
    assert prefix[-1] == len(ids) and all(e > b for b, e in rr) and len(rr) < len(ranges)
    chunks = R.chunk_table(ranges)
    assert len(chunks) == cp[-1] and all(1 <= cnt <= 4 for _, cnt in chunks)
    rows = np.concatenate([np.arange(r0, r0 + cnt) for r0, cnt in chunks])
    assert np.array_equal(rows, ids)                                # in order, each once
    assert any(cnt < 4 for _, cnt in chunks)
    tiles = R.tile_table(ranges)
    assert len(tiles) == tp[-1] and len({t for t, _ in tiles}) == len(tiles)
    assert [t for t, _ in tiles] == sorted(t for t, _ in tiles)
    rows = np.concatenate([32 * t + np.flatnonzero([(m >> b) & 1 for b in range(32)]) for t, m in tiles])
    assert np.array_equal(rows, ids) and all(m for _, m in tiles)
    assert len(tiles) == len({int(r) // 32 for r in ids})
    if which == "dense":
        assert len(_shared_tiles(ranges)) >= 3 and _bit31_of_shared_tiles(ranges, D.N_B)


# ---------------------------------------------------------------------------------------------------------------- the tests bite
def _shared_tiles(ranges):
    """tiles that two (non-empty) ranges touch"""
    seen, shared = set(), set()
    for b, e in ranges:
        if e > b:
            mine = set(range(b >> 5, ((e - 1) >> 5) + 1))
            shared |= mine & seen
            seen |= mine
    return shared


def _ragged_last_rows(ranges, n):
    if ranges is None:
        return {n - 1} if n % 4 else set()
    return {r0 + cnt - 1 for r0, cnt in R.chunk_table(ranges) if cnt < 4}


def _first_rows(ranges, n):
    return {0} if ranges is None else {b for b, e in ranges if e > b}


def _bit31_of_shared_tiles(ranges, n):
    mask = D.in_ranges(n, ranges)
    return {32 * t + 31 for t in _shared_tiles(ranges) if 32 * t + 31 < n and mask[32 * t + 31]}


def _after_seams(keep):
    at, out = 0, set()
    for b, e in keep[:-1]:
        at += e - b
        out.add(at)
    return out


def _last_rows_of_shards(sizes):
    return set((np.cumsum(sizes)[:-1] - 1).tolist())


def _roll_call_failures(fx, skip_of_query):
    """How many lists of the roll call a model search that skips skip_of_query(j) (global rows) gets wrong."""
    rc = fx.rc
    local = {int(g): i for i, g in enumerate(np.arange(rc.n) if fx.ids is None else fx.ids)}
    bad = 0
    for j in range(rc.J):
        skip = [local[g] for g in skip_of_query(j) if g in local]
        got = R.model_search(rc.rows, fx.ids, rc.queries[j], len(rc.lists[j]), skip)
        bad += got != fx.global_rows(j)
    return bad


_RANDOM = {}


def _random_cases():
    """The corpus, the range list and the seven queries of test_many_small_ranges_all_paths (k = 10)."""
    if not _RANDOM:
        emb = synth.unit_rows(20000, seed=3)
        rng = np.random.default_rng(21)
        ranges, pos = [], 0
        while pos < 19_000:
            length = int(rng.choice([1, 2, 3, 4, 5, 7, 8, 13, 64, 100]))
            ranges.append((pos, pos + length))
            pos += length + int(rng.choice([0, 1, 3, 50, 400]))
        _RANDOM.update(emb=emb, ranges=ranges, ids=np.concatenate([np.arange(b, e) for b, e in ranges]), qs=synth.unit_query(4, nq=7))
    return _RANDOM


def _random_failures(skip_of_query, filtered):
    """How many of the seven random queries at k = 10 notice the same broken search (over the range list, or over all 20 000 rows)."""
    r = _random_cases()
    ids = r["ids"] if filtered else np.arange(len(r["emb"]))
    rows = r["emb"][ids]
    local = {int(g): i for i, g in enumerate(ids)}
    bad = 0
    for j, q in enumerate(r["qs"]):
        skip = [local[g] for g in skip_of_query(j) if g in local]
        bad += R.model_search(rows, ids, q, 10, skip) != R.model_search(rows, ids, q, 10)
    return bad, len(r["qs"])


def _broken_searches():
    """(name, fixture, skip(query) on the fixture, skip(query) on the random cases, random cases filtered?)"""
    r = _random_cases()
    dense = R.range_ids("dense")[0]
    sparse = R.range_ids("sparse")[0]
    keep = R.stages_c()[2][2]
    group = lambda j, s=0: {4 * ((j + s) % 16) + ((j + s) % 16) % 4}   # the query in slot g never sees row 4 g + g mod 4
    every = lambda rows: (lambda j: rows)
    return [
        ("the last valid row of every ragged chunk (unfiltered)", "P-56-strided-shuffled", every(_ragged_last_rows(None, R.N)),
         every(_ragged_last_rows(None, 20000) | {19999}), False),
        ("the last valid row of every ragged chunk (sparse ranges)", "R-sparse-56", every(_ragged_last_rows(sparse, D.N_B)),
         every(_ragged_last_rows(r["ranges"], 20000)), True),
        ("the first row of every range", "R-dense-56", every(_first_rows(dense, D.N_B)), every(_first_rows(r["ranges"], 20000)), True),
        ("bit 31 of every tile mask shared by two ranges", "R-dense-56-strided", every(_bit31_of_shared_tiles(dense, D.N_B)),
         every(_bit31_of_shared_tiles(r["ranges"], 20000)), True),
        ("the row after every compaction seam", "C-compacted", every(_after_seams(keep)), every(_after_seams([(0, 9997), (9999, 10023), (10026, 20000)])), False),
        ("the last row of every shard but the last", "P-56-contiguous-shuffled", every(_last_rows_of_shards(R.SHARDS)),
         every(_last_rows_of_shards((6667, 6667, 6666))), False),
        ("one (query, row) pair of a 16-query group", "P-32-contiguous", group, group, False),
    ]


def test_skips_are_not_empty():
    for name, fixture, skip, skip_random, _ in _broken_searches():
        assert skip(1) and skip_random(1), name
        fx = R.fixture(fixture)
        allowed = set(range(fx.rc.n)) if fx.ids is None else set(fx.ids.tolist())
        assert skip(1) <= allowed, name                             # (every skipped row is a row the call was given)


@pytest.mark.parametrize("case", range(7))
def test_a_search_that_skips_rows_fails_the_roll_call(case, capsys):
    """Each broken search gets at least one list of the roll call wrong -- one list per skipped row, as every row is owed to exactly
    one query -- and the count of random-corpus cases that notice it is printed: the evidence for the gap."""
    name, fixture, skip, skip_random, filtered = _broken_searches()[case]
    fx = R.fixture(fixture)
    assert _roll_call_failures(fx, lambda j: set()) == 0            # (the unbroken model passes)
    bad = _roll_call_failures(fx, skip)
    if case < 6:
        skipped = set().union(*(skip(j) for j in range(fx.rc.J)))
        local = {int(g): i for i, g in enumerate(np.arange(fx.rc.n) if fx.ids is None else fx.ids)}
        owners = {int(fx.rc.owner[local[g]]) for g in skipped}
        assert bad == len(owners) > 0, (name, bad, len(owners))     # every skipped row is missed by the one query that owns it
    else:
        # the queries take the slots in turn, as the GPU series rotate them: series s puts query j into slot (j + s) mod 16.  Each of
        # the sixteen (slot, row) pairs is noticed in the one series that puts the row's owner into that slot
        bad = sum(_roll_call_failures(fx, lambda j, s=s: skip(j, s)) for s in range(16))
        assert bad == 16, (name, bad)
    rbad, rall = _random_failures(skip_random, filtered)
    with capsys.disabled():
        print("\nroll call: skipping %s fails %d of %d lists (%s); the random-corpus cases at k = 10 notice it in %d of %d queries"
              % (name, bad, fx.rc.J, fixture, rbad, rall))
    assert rbad < rall
