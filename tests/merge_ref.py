"""A NumPy reference of the cross-shard top-k merge and of the status combine (csrc/merge.hip), and the constructed lists the merge
tests feed the kernels.  NumPy only: nothing here imports the library, and the merge is a plain lexsort that shares no code with
smt.merge_topk or tests/dist_protocol.py -- tests/test_merge_ref_cpu.py holds it against a brute-force rank count, the host merge
against it, and shows that the cases tell three subtly wrong merges from the right one.

Layouts: rows [n_lists][nq][k_in] uint64 and dist [n_lists][nq][k_in] float64 (the plain layout), or packed
[n_lists][nq][2][k] 64-bit words, rows then distance bits.  Padding is row UINT64_MAX; the distance beside it is +inf by convention
and is never looked at."""
import zlib

import numpy as np

PAD = np.uint64(0xFFFFFFFFFFFFFFFF)

# (n_lists, k_in, k_out, nq): the smallest shapes at which a loop or a branch of the kernels changes behaviour -- 256 threads per
# block, loops that stride by 256, the in-place kernel's LDS branch above 4096 candidates, 64 sources, 8192 candidates at most
SHAPES = [
    (1, 1, 1, 1), (1, 10, 10, 1), (3, 6, 6, 3), (3, 7, 7, 33), (5, 51, 51, 2), (4, 64, 64, 2), (1, 257, 257, 1), (64, 1, 10, 4),
    (64, 56, 56, 2), (8, 512, 512, 2), (17, 241, 241, 1), (8, 1024, 1024, 2), (64, 128, 128, 2), (4, 10, 3, 2), (4, 10, 40, 2),
    (4, 10, 64, 2), (2, 10, 300, 1), (8, 1024, 10, 1),
]


def merge_lists(rows, dist, k_out):
    """(rows [nq][k_out], dist [nq][k_out], counts [nq]): per query the k_out best of all lists' entries by (distance, row)
    ascending, entries whose row is UINT64_MAX dropped, the tail padded with UINT64_MAX / +inf."""
    rows = np.asarray(rows, dtype=np.uint64)
    dist = np.asarray(dist, dtype=np.float64)
    n_lists, nq, k_in = rows.shape
    out_r = np.full((nq, k_out), PAD, dtype=np.uint64)
    out_d = np.full((nq, k_out), np.inf, dtype=np.float64)
    counts = np.zeros(nq, dtype=np.uint64)
    for q in range(nq):
        r, d = rows[:, q, :].reshape(-1), dist[:, q, :].reshape(-1)
        keep = r != PAD
        r, d = r[keep], d[keep]
        order = np.lexsort((r, d))[:k_out]     # (last key is the primary one)
        out_r[q, :len(order)], out_d[q, :len(order)] = r[order], d[order]
        counts[q] = len(order)
    return out_r, out_d, counts


def combine_status(words):
    """words [n][nq] -> uint32 [nq]: the worst (largest) status word per query; n == 0 gives zeros."""
    words = np.asarray(words, dtype=np.uint64)
    if words.shape[0] == 0:
        return np.zeros(words.shape[1], dtype=np.uint32)
    return words.max(axis=0).astype(np.uint32)


def pack(rows, dist):
    """rows, dist [..., k] -> words [..., 2, k]: the rows, then the distances' bit patterns."""
    rows = np.asarray(rows, dtype=np.uint64)
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    return np.ascontiguousarray(np.stack([rows, dist.view(np.uint64)], axis=-2))


def unpack(words):
    """words [..., 2, k] -> (rows [..., k] uint64, dist [..., k] float64)."""
    words = np.asarray(words, dtype=np.uint64)
    return np.ascontiguousarray(words[..., 0, :]), np.ascontiguousarray(words[..., 1, :]).view(np.float64)


# ------------------------------------------------------------------------------------------------------------------- case contents
def _distinct_rows(rng, n):
    """n distinct random row numbers below UINT64_MAX, over the whole 64-bit range."""
    out = np.zeros(0, dtype=np.uint64)
    while len(out) < n:
        draw = rng.integers(0, 0xFFFFFFFFFFFFFFFF, size=2 * n + 8, dtype=np.uint64)   # (the high end is exclusive)
        out = np.unique(np.concatenate([out, draw]))
    return rng.permutation(out)[:n]


def _grid_rows(rng, n):
    """n distinct rows lo | hi << 32 off a grid of few low and few high words: many pairs differ in the high word only, many in
    the low word only, and the low words alone repeat."""
    n_hi = int(np.ceil(np.sqrt(n)))
    n_lo = -(-n // n_hi)
    lo = np.unique(np.concatenate([np.array([0, 1, 0xFFFFFFFF], dtype=np.uint64), rng.integers(0, 1 << 32, size=n_lo + 4, dtype=np.uint64)]))
    hi = np.unique(np.concatenate([np.array([0, 1, 0xFFFFFFFE], dtype=np.uint64), rng.integers(0, 0xFFFFFFFF, size=n_hi + 4, dtype=np.uint64)]))
    lo, hi = rng.permutation(lo)[:n_lo], rng.permutation(hi)[:n_hi]
    grid = (hi[:, None] << np.uint64(32) | lo[None, :]).reshape(-1)
    return rng.permutation(grid)[:n]


def _place(rows, dist, q, per_list, pad_dist=None):
    """Writes query q: per_list[l] = (rows, dist) of list l, put in (distance, row) order, the tail of the list left padded."""
    for l, (r, d) in enumerate(per_list):
        order = np.lexsort((r, d))
        rows[l, q, :len(r)], dist[l, q, :len(r)] = r[order], d[order]
        if pad_dist is not None:
            dist[l, q, len(r):] = pad_dist[l]


def _empty(n_lists, k_in, nq):
    return np.full((n_lists, nq, k_in), PAD, dtype=np.uint64), np.full((n_lists, nq, k_in), np.inf, dtype=np.float64)


def _deal(rng, n_lists, k_in, n):
    """n of the n_lists x k_in slots chosen at random: the list each of n entries goes to (no list gets more than k_in)."""
    return np.sort(rng.permutation(np.repeat(np.arange(n_lists), k_in))[:n])


def _dealt(rng, n_lists, k_in, k_out, nq):
    """One global list of distinct (distance, row) pairs dealt at random to the lists; query 0 fills every slot."""
    rows, dist = _empty(n_lists, k_in, nq)
    M = n_lists * k_in
    for q in range(nq):
        n = M if q == 0 else int(rng.integers((M + 1) // 2, M + 1))
        r = _distinct_rows(rng, n)
        d = rng.permutation(np.unique(rng.random(2 * n + 8) * 2.0))[:n]
        owner = _deal(rng, n_lists, k_in, n)
        _place(rows, dist, q, [(r[owner == l], d[owner == l]) for l in range(n_lists)])
    return rows, dist


def _ties(rng, n_lists, k_in, k_out, nq):
    """At most four distance values, one of them 0.0; rows off a grid that spans 2^32, the higher-numbered lists holding the lower
    rows; one group of equal distances straddles position k_out."""
    rows, dist = _empty(n_lists, k_in, nq)
    M = n_lists * k_in
    for q in range(nq):
        r = np.sort(_grid_rows(rng, M))
        values = np.concatenate([[0.0], np.sort(rng.random(3)) + 0.25])
        cuts = [c for c in rng.permutation(np.arange(1, M)).tolist() if c != k_out][:3]   # group borders, none at k_out
        bounds = np.array(sorted(cuts), dtype=np.int64)
        # the groups' sizes are fixed by the borders; which rows fall into which group is random
        group = np.searchsorted(bounds, np.arange(M), side="right")
        d = values[group][rng.permutation(M)]
        per_list = [(r[(n_lists - 1 - l) * k_in:(n_lists - l) * k_in], d[(n_lists - 1 - l) * k_in:(n_lists - l) * k_in]) for l in range(n_lists)]
        _place(rows, dist, q, per_list)
    return rows, dist


def _ragged(rng, n_lists, k_in, k_out, nq):
    """Lists of padding only, one list with a single entry, the others of any length; with two queries or more, every list of the
    last query is padding.  The odd-numbered lists carry 0.0 beside their padding rows: padding is known by the row alone."""
    rows, dist = _empty(n_lists, k_in, nq)
    pad_dist = [0.0 if l % 2 else np.inf for l in range(n_lists)]
    for q in range(nq):
        if nq >= 2 and q == nq - 1:
            _place(rows, dist, q, [(np.zeros(0, np.uint64), np.zeros(0))] * n_lists, pad_dist)
            continue
        lens = rng.integers(0, k_in + 1, size=n_lists)
        roles = rng.permutation(n_lists)
        lens[roles[0]] = 1                                   # the single entry
        lens[roles[1:1 + max(1, n_lists // 3)]] = 0          # padding only
        if q == 0:
            lens[roles[-1]] = k_in                           # ... and one full list
        n = int(lens.sum())
        r = _distinct_rows(rng, n)
        d = rng.permutation(np.unique(rng.random(2 * n + 8) * 2.0))[:n]
        off = np.concatenate([[0], np.cumsum(lens)])
        _place(rows, dist, q, [(r[off[l]:off[l + 1]], d[off[l]:off[l + 1]]) for l in range(n_lists)], pad_dist)
    return rows, dist


def _last_list_wins(rng, n_lists, k_in, k_out, nq):
    """Every entry of the last list is nearer than every entry of the others."""
    rows, dist = _empty(n_lists, k_in, nq)
    M = n_lists * k_in
    for q in range(nq):
        r = _distinct_rows(rng, M)
        d = rng.permutation(np.unique(rng.random(2 * M + 8)))[:M]
        per_list = []
        for l in range(n_lists):
            dl = d[l * k_in:(l + 1) * k_in]
            per_list.append((r[l * k_in:(l + 1) * k_in], dl * 0.5 if l == n_lists - 1 else 1.0 + dl))
        _place(rows, dist, q, per_list)
    return rows, dist


def _neighbours(rng, n_lists, k_in, k_out, nq):
    """Distances a few ulps apart -- half of them consecutive (np.nextafter), all of them one value once rounded to f32 -- under
    random rows, dealt at random."""
    rows, dist = _empty(n_lists, k_in, nq)
    M = n_lists * k_in
    for q in range(nq):
        base = np.float64(np.float32(0.25 + 0.5 * rng.random()))          # an f32 value: +2^24 ulps of f64 stay below half an f32 ulp
        steps = np.concatenate([np.arange(M // 2), M + rng.choice(1 << 24, size=M - M // 2, replace=False)]).astype(np.int64)
        d = (np.full(M, base).view(np.int64) + steps).view(np.float64)
        if M >= 2:
            assert d[1] == np.nextafter(d[0], np.inf) and (d.astype(np.float32) == np.float32(base)).all()
        d = rng.permutation(d)
        r = _distinct_rows(rng, M)
        owner = _deal(rng, n_lists, k_in, M)
        _place(rows, dist, q, [(r[owner == l], d[owner == l]) for l in range(n_lists)])
    return rows, dist


CONTENTS = [
    # (name, generator, least n_lists, least candidates)
    ("dealt", _dealt, 1, 1),
    ("ties", _ties, 1, 2),
    ("ragged", _ragged, 3, 3),
    ("last_list_wins", _last_list_wins, 2, 2),
    ("neighbours", _neighbours, 1, 2),
]


def case_names():
    """The names cases() yields, in its order, without building the lists."""
    return ["%s-%dx%d_to_%d_nq%d" % (name, n, k_in, k_out, nq) for (n, k_in, k_out, nq) in SHAPES
            for name, _, min_lists, min_m in CONTENTS if n >= min_lists and n * k_in >= min_m]


_CASES = {}


def case(name):
    """(rows, dist, k_out) of one named case; built once, from a seed that depends on the name alone.  Read-only arrays."""
    if name not in _CASES:
        content, shape = name.split("-")
        dims, nq = shape.split("_nq")
        lists, k_out = dims.split("_to_")
        n_lists, k_in = (int(v) for v in lists.split("x"))
        gen = {c[0]: c[1] for c in CONTENTS}[content]
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        rows, dist = gen(rng, n_lists, k_in, int(k_out), int(nq))
        rows.setflags(write=False)
        dist.setflags(write=False)
        _CASES[name] = (rows, dist, int(k_out))
    return _CASES[name]


def cases():
    """Yields (name, rows [n_lists][nq][k_in], dist [n_lists][nq][k_in], k_out) over SHAPES x CONTENTS.  Every query of a case has
    its own content; rows are distinct within a query (the kernels' precondition); every list is in (distance, row) order with
    its padding at the tail."""
    for name in case_names():
        yield (name,) + case(name)
