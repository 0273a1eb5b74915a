"""Roll-call rows: inputs for the tests that ask whether a search route looks at EVERY row it was given
(tests/test_rollcall_cpu.py checks the inputs and shows that the tests bite, tests/test_gpu_rollcall.py runs the routes).

The mirror image of tests/decoys.py.  Every allowed row is in the expected answer of exactly one query, at a known place.  The
queries are axis vectors, q_j = e_j for j < J <= 192; the last 64 dimensions are the filler subspace.  Allowed row r has one owner
query j and a rank m inside that query's set S_j:

    x_r = c e_j  +  sum over j' != j, j' < J of eps_{r,j'} e_{j'}  +  s_r f_r

with c = LADDER(k)[order[m]] (equal steps from 0.95 down to 0.40 for k <= 56, down to 0.45 above), eps seeded uniform in
[-0.01, 0.01] (the unowned rows lie spread around distance 1 as in a random corpus: exact ties at 1.0 would push the sampled
thresholds and K3's candidate buffers into their overflow fall-backs), f_r a seeded unit vector of the filler subspace and s_r what
makes x_r a unit row.  cos(x_r, q_j) = c to f32 rounding, so the answer of query j at top_k = |S_j| is S_j in the order of falling c;
every other row is about 0.4 behind the last place.  A dropped row shows as a stranger or as padding in the last place of one list;
a row read by the wrong lane, or credited to the wrong query, shows too.

Assignments of the allowed rows (i: index among them) to (owner, rank) -- J = ceil(n / k):
  strided     owner = i mod J, rank = i div J: consecutive rows belong to different queries;
  contiguous  owner = i div k, rank = i mod k: one query's winners are k consecutive rows (whole chunks, one wave's list, a block's).
Sets are not all of one size when k does not divide n (contiguous: a last, smaller set; strided: the first n mod J sets hold one row
more); a call batches only queries of sets of one size, with top_k = that size (RollCall.by_size).

Rows outside the allowed set (outside the ranges, beyond `rows`) are filler-only unit rows, orthogonal to every query: these tests are
about drops, leaks are the decoy tests' job.

The K4 fixtures add one more axis, e_J (sweep=True): every allowed row gets a component t_i on it that falls strictly with i in steps
of at most 5e-5 from 0.25 on, so that the query e_J at max_distance = 0.9 has to return every allowed row, in row order.

Nothing here needs a GPU; the builders return numpy arrays and the GPU tests upload them."""
import numpy as np

from tests import decoys as D

DIM = D.DIM
FILL = 64                       # the filler subspace: the last 64 dimensions
J_MAX = DIM - FILL              # 192 query axes at the most
C_HI = 0.95
EPS = 0.01
ASSIGNMENTS = ("strided", "contiguous")
ORDERS = ("ascending", "descending", "shuffled")
SWEEP_T0, SWEEP_SPAN, SWEEP_STEP_MAX = 0.25, 0.12, 5e-5
SWEEP_MAX_DISTANCE = 0.9
N = 4097                        # two blocks at scan_blocks = 2, a ragged chunk, a ragged tile
SHARDS = (1365, 1, 2731)        # layout S: three unequal shards of N rows
SHARDS_LARGEK = (5461, 5462, 5463)


def c_lo(k):
    return 0.40 if k <= 56 else 0.45


def ladder(k):
    """The k cosines of a set's places, falling in equal steps (k = 1: 0.95 alone)."""
    return np.linspace(C_HI, c_lo(k), k) if k > 1 else np.array([C_HI])


def nominal_step(k):
    return (C_HI - c_lo(k)) / (k - 1) if k > 1 else C_HI - c_lo(k)


def assign(n, k, assignment):
    """(owner, rank, J) of the n allowed rows."""
    J = -(-n // k)
    assert 1 <= J <= J_MAX, (n, k, J)
    i = np.arange(n, dtype=np.int64)
    if assignment == "strided":
        return i % J, i // J, J
    assert assignment == "contiguous", assignment
    return i // k, i % k, J


def place_order(size, order, seed):
    """rank (the order of the rows in memory) -> place on the ladder: which of a set's rows is nearest."""
    if order == "ascending":
        return np.arange(size)
    if order == "descending":
        return np.arange(size)[::-1].copy()
    assert order == "shuffled", order
    return np.random.default_rng(seed).permutation(size)


def filler_rows(m, seed):
    """m unit rows of the filler subspace: orthogonal to every query."""
    rng = np.random.default_rng(seed)
    out = np.zeros((m, DIM), dtype=np.float64)
    f = rng.standard_normal((m, FILL))
    out[:, J_MAX:] = f / np.linalg.norm(f, axis=1, keepdims=True)
    return np.ascontiguousarray(out, dtype=np.float32)


class RollCall:
    """n allowed rows with their owners: rows [n, 256] f32, queries [J (+ 1), 256] f32, lists[j] = the positions (among the allowed
    rows) of S_j in answer order, cos[j] = their intended cosines, by_size = {set size: [queries]}."""

    def __init__(self, n, k, assignment, order, seed, sweep=False):
        owner, rank, J = assign(n, k, assignment)
        assert J + (1 if sweep else 0) <= J_MAX
        self.n, self.k, self.J, self.assignment, self.order, self.seed, self.sweep = n, k, J, assignment, order, seed, sweep
        self.owner, self.rank = owner, rank
        sizes = np.bincount(owner, minlength=J)
        assert sizes.min() >= 1 and sizes.max() <= k
        rng = np.random.default_rng(seed)
        lad = ladder(k)
        place = np.empty(n, dtype=np.int64)
        for j in range(J):
            mine = np.flatnonzero(owner == j)
            assert np.array_equal(rank[mine], np.arange(len(mine)))
            place[mine] = place_order(len(mine), order, seed * 1000 + j)
        x = np.zeros((n, DIM), dtype=np.float64)
        x[:, :J] = rng.uniform(-EPS, EPS, size=(n, J))
        x[np.arange(n), owner] = lad[place]
        if sweep:
            step = min(SWEEP_STEP_MAX, SWEEP_SPAN / max(1, n - 1))
            x[:, J] = SWEEP_T0 - step * np.arange(n)
        f = rng.standard_normal((n, FILL))
        f /= np.linalg.norm(f, axis=1, keepdims=True)
        s2 = 1.0 - (x ** 2).sum(axis=1)
        assert s2.min() > 0.0, s2.min()
        x[:, J_MAX:] = np.sqrt(s2)[:, None] * f
        self.rows = np.ascontiguousarray(x, dtype=np.float32)
        self.place = place
        self.queries = np.zeros((J + (1 if sweep else 0), DIM), dtype=np.float32)
        self.queries[np.arange(len(self.queries)), np.arange(len(self.queries))] = 1.0
        self.lists, self.cos = [], []
        for j in range(J):
            mine = np.flatnonzero(owner == j)
            mine = mine[np.argsort(place[mine])]
            self.lists.append(mine)
            self.cos.append(lad[place[mine]])
        self.by_size = {}
        for j in range(J):
            self.by_size.setdefault(len(self.lists[j]), []).append(j)

    def calls(self, nq):
        """The roll call as (queries of one call, top_k): every query once, at most nq per call, equal set sizes only."""
        out = []
        for size in sorted(self.by_size, reverse=True):
            js = self.by_size[size]
            out += [(js[b:b + nq], size) for b in range(0, len(js), nq)]
        return out


def roll_call(n, k, assignment="strided", order="shuffled", seed=1, sweep=False):
    return RollCall(n, k, assignment, order, seed, sweep)


def embed(rc, total, ids, seed=90):
    """A buffer of `total` rows with the roll call's rows at `ids` and filler rows everywhere else."""
    ids = np.asarray(ids, dtype=np.int64)
    assert len(ids) == rc.n and len(np.unique(ids)) == rc.n and (ids < total).all()
    buf = filler_rows(total, seed)
    buf[ids] = rc.rows
    return np.ascontiguousarray(buf)


def ends(n, span):
    """The first and the last `span` rows of n (the two runs of a roll call whose J would pass 192): id arrays."""
    span = min(span, n)
    return [np.arange(0, span, dtype=np.int64)] + ([np.arange(n - span, n, dtype=np.int64)] if span < n else [])


def range_ids(name, n=D.N_B):
    """(ranges, ids of the allowed rows) of the decoy module's range lists."""
    ranges = D.range_lists(n)[name]
    return ranges, np.flatnonzero(D.in_ranges(n, ranges))


# ---------------------------------------------------------------------------------------------------------------- the fixtures
class Fixture:
    """One roll call in its buffer: rc, buf [total, 256] (filler rows outside `ids`), ids (None: the rows' own positions)."""

    def __init__(self, name, rc, total=None, ids=None):
        self.name, self.rc = name, rc
        self.ids = None if ids is None else np.asarray(ids, dtype=np.int64)
        self.total = rc.n if total is None else total
        self.buf = rc.rows if ids is None else embed(rc, self.total, self.ids)

    def global_rows(self, j):
        return expected_rows(self.rc, j, self.ids)


def _plain(n, k, assignment, order, seed, sweep=False):
    return lambda name: Fixture(name, roll_call(n, k, assignment, order, seed, sweep))


def _inside(total, ids, k, assignment, order, seed, sweep=False):
    return lambda name: Fixture(name, roll_call(len(ids), k, assignment, order, seed, sweep), total, ids)


def _ranged(which, k, assignment, order, seed, sweep=False):
    return lambda name: _inside(D.N_B, range_ids(which)[1], k, assignment, order, seed, sweep)(name)


N_I2 = 4051                     # layout I after a truncate to 4001 rows and an append of 50: the old ragged tile is rewritten
_BUILDERS = {
    # P / I / S: an owned corpus of N rows (I: with the fp16 image, S: cut into SHARDS)
    "P-56-strided-shuffled": _plain(N, 56, "strided", "shuffled", 11, sweep=True),
    "P-56-strided-descending": _plain(N, 56, "strided", "descending", 12),
    "P-56-contiguous-ascending": _plain(N, 56, "contiguous", "ascending", 13),
    "P-56-contiguous-shuffled": _plain(N, 56, "contiguous", "shuffled", 14),
    "P-1-first": _inside(N, ends(N, J_MAX)[0], 1, "strided", "ascending", 15),
    "P-1-last": _inside(N, ends(N, J_MAX)[1], 1, "strided", "ascending", 16),
    "P-2049-56": _plain(2049, 56, "strided", "shuffled", 17),
    "P-2049-56-contiguous": _plain(2049, 56, "contiguous", "descending", 18),
    "P-10-first": _inside(N, ends(N, 10 * J_MAX)[0], 10, "contiguous", "shuffled", 19),
    "P-10-last": _inside(N, ends(N, 10 * J_MAX)[1], 10, "strided", "shuffled", 20),
    "P-24-contiguous": _plain(N, 24, "contiguous", "shuffled", 28),
    "P-24-strided": _plain(N, 24, "strided", "descending", 29),
    "P-32-contiguous": _plain(N, 32, "contiguous", "descending", 21),
    "P-32-strided": _plain(N, 32, "strided", "shuffled", 22),
    "L-1024": _plain(D.N_LARGEK, 1024, "contiguous", "shuffled", 23),
    "L-1024-strided": _plain(D.N_LARGEK, 1024, "strided", "ascending", 24),
    "S-1024": _plain(sum(SHARDS_LARGEK), 1024, "contiguous", "shuffled", 25),
    "I-56-after-append": _plain(N_I2, 56, "contiguous", "shuffled", 26),
    "I-32-after-append": _plain(N_I2, 32, "strided", "shuffled", 27),
    # R: inside the decoy module's range lists over N_B rows
    "R-dense-56": _ranged("dense", 56, "contiguous", "shuffled", 31, sweep=True),
    "R-dense-56-strided": _ranged("dense", 56, "strided", "descending", 32),
    "R-dense-32": _ranged("dense", 32, "strided", "shuffled", 33),
    "R-dense-57": _ranged("dense", 57, "contiguous", "ascending", 34),
    "R-sparse-56": _ranged("sparse", 56, "strided", "shuffled", 35, sweep=True),
    "R-sparse-10": _ranged("sparse", 10, "contiguous", "shuffled", 36),
    # C: the rows present after each stage of layout C
    "C-truncated": _plain(N, 56, "contiguous", "shuffled", 41),
    "C-appended": _plain(N + 10, 56, "strided", "shuffled", 42),
    "C-compacted": _plain(N + 5, 56, "contiguous", "descending", 43),
}
FIXTURES = tuple(_BUILDERS)
SWEEP_FIXTURES = ("P-56-strided-shuffled", "R-dense-56", "R-sparse-56")     # the ones with K4's axis
_BUILT = {}


def fixture(name):
    """The fixture `name`, built once per process and never changed."""
    if name not in _BUILT:
        _BUILT[name] = _BUILDERS[name](name)
    return _BUILT[name]


# ---------------------------------------------------------------------------------------------------------------- layout C
def stages_c(n=N):
    """The stages of tests/test_gpu_decoys.py's layout C: truncate to n, append ten rows into the freed capacity, compact -- here with
    three kept ranges, so that neither end of a dropped run and no seam of the compacted corpus is a multiple of 16 (the compaction
    moves rows in 16-row runs).  [(stage, rows present, keep list or None)]"""
    h = n // 2
    keep = [(0, h - 3), (h - 1, h + 23), (h + 26, n + 10)]
    assert all(b % 16 and e % 16 for b, e in ((keep[0][1], keep[1][0]), (keep[1][1], keep[2][0])))
    assert all(s % 16 for s in (h - 3, h + 21)) and sum(e - b for b, e in keep) == n + 5
    return [("truncated", n, None), ("appended", n + 10, None), ("compacted", n + 5, keep)]


def before_compaction(final, keep, total, seed=91):
    """The content of `total` rows that compacts (keep list `keep`) to the rows `final`: filler rows in the dropped runs."""
    out = filler_rows(total, seed)
    at = 0
    for b, e in keep:
        out[b:e] = final[at:at + e - b]
        at += e - b
    assert at == len(final)
    return np.ascontiguousarray(out)


# ---------------------------------------------------------------------------------------------------------------- reference
def oracle_lists(rc, ids=None, js=None):
    """The oracle's accurate answers over the allowed rows for the queries js (default: all J) at top_k = |S_j|: [(rows, f64 dist)]."""
    js = range(rc.J) if js is None else js
    out = {}
    for size, members in rc.by_size.items():
        members = [j for j in members if j in set(js)]
        if members:
            for j, ans in zip(members, D.expected(rc.rows, ids, rc.queries[members], size)):
                out[j] = ans
    return [out[j] for j in js]


def expected_rows(rc, j, ids=None):
    rows = rc.lists[j]
    return (rows if ids is None else np.asarray(ids, dtype=np.int64)[rows]).tolist()


# ---------------------------------------------------------------------------------------------------------------- a model search
def model_search(rows, ids, q, k, skip=()):
    """A plain NumPy top-k over `rows` (f64 cosine distances, ties by row) that never looks at the positions in `skip`: the
    broken searches of tests/test_rollcall_cpu.py.  Returns the ids of the answer."""
    d = D.distances64(rows, q)[:, 0]
    if len(skip):
        d = d.copy()
        d[np.asarray(list(skip), dtype=np.int64)] = np.inf
    order = np.lexsort((np.arange(len(d)), d))[:k]
    order = order[np.isfinite(d[order])]
    return (order if ids is None else np.asarray(ids, dtype=np.int64)[order]).tolist()


# ---------------------------------------------------------------------------------------------------------------- range tables
def range_prefixes(ranges):
    """search.cpp range_prefixes over the non-empty ranges: (prefix, chunk_prefix, tile_prefix), each len + 1 words."""
    rr = [(b, e) for b, e in ranges if e > b]
    prefix, chunk, tile = [0], [0], [0]
    last_tile = None
    for b, e in rr:
        prefix.append(prefix[-1] + e - b)
        chunk.append(chunk[-1] + (e - b + 3) // 4)
        ft, lt = b >> 5, (e - 1) >> 5
        tile.append(tile[-1] + (lt - ft + 1) - (1 if ft == last_tile else 0))
        last_tile = lt
    return rr, prefix, chunk, tile


def chunk_table(ranges):
    """range_tables.hip build_chunk_table_kernel: [(row0, valid rows)] per 4-row chunk."""
    rr, _, cp, _ = range_prefixes(ranges)
    out = []
    for c in range(cp[-1]):
        lo, hi = 0, len(rr)
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if cp[mid] <= c:
                lo = mid
            else:
                hi = mid
        row0 = rr[lo][0] + (c - cp[lo]) * 4
        out.append((row0, min(rr[lo][1] - row0, 4)))
    return out


def tile_table(ranges):
    """range_tables.hip build_tile_table_kernel: [(tile, 32-bit row mask)] per aligned 32-row tile that holds a wanted row."""
    rr, _, _, tp = range_prefixes(ranges)
    out = []
    for v in range(tp[-1]):
        lo, hi = 0, len(rr)
        while lo < hi:
            mid = (lo + hi) >> 1
            if tp[mid + 1] > v:
                hi = mid
            else:
                lo = mid + 1
        i = lo
        first = rr[i][0] >> 5
        shared = i > 0 and ((rr[i - 1][1] - 1) >> 5) == first
        tile = first + (1 if shared else 0) + (v - tp[i])
        t0, t1 = tile << 5, (tile << 5) + 32
        mask, k = 0, i
        while k < len(rr) and rr[k][0] < t1:
            b, e = max(rr[k][0], t0), min(rr[k][1], t1)
            if e > b:
                mask |= ((1 << (e - b)) - 1) << (b - t0)
            k += 1
        out.append((tile, mask & 0xFFFFFFFF))
    return out
