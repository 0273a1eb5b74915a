"""Decoy rows: inputs for the tests that ask whether a search route looks outside the rows it was given
(tests/test_decoys_cpu.py checks the inputs, tests/test_gpu_decoys.py runs the routes).

Every fixture draws its queries around ONE unit centre c: q_i = normalise(c + t u_i) with u_i a unit vector orthogonal to c and
t = tan(acos(0.9)), so cos(q_i, c) = 0.9.  The rows a call may see come from synth.unit_rows (duplicates and zero rows included):
the nearest of <= 20 k of them lies at a cosine distance of about 0.7 from any query.  A finite decoy is 2^j c (j cycling through
-2 .. 2: inside the numeric domain, a power-of-two scale changes no bit of the products): distance 0.1 to EVERY query.  One decoy
that a kernel lets through therefore ranks first for every query of the call, passes every threshold the tests use, and pulls
any sampled or tile-minimum threshold below every true row.  The non-finite flavour (NaN rows alternating with +Inf rows) shows a
kernel that masks by arithmetic instead of by selection; it is only used where the decoys lie OUTSIDE the corpus (layout A).

Layouts (G = 64 guard rows, at least every granule of the kernels: 4-row chunks, 16-row compaction runs, 32-row tiles):
  A  [G guards | n rows | G guards] in one buffer, the corpus is the adopted middle view;
  B  a corpus in which every row outside a range list is a decoy;
  C  n rows followed by G decoys, for an owned corpus that appends n + G rows and truncates to n.
Guards always lie in the same allocation as the rows: an over-read lands on a guard, never on unmapped memory.

Nothing here needs a GPU; the builders return numpy arrays and the GPU tests upload them."""
import math

import numpy as np

from oracle import oracle as orc
from tests import synth

G = 64
DIM = synth.DIM
COS_QC = 0.9
CENTRE_SEED = 7001
QUERY_SEED = 7002
NQ_MAX = 130
SCALES = (-2, -1, 0, 1, 2)

# the corpus sizes of layout A (every n, the K2 / K4 / K3 routes) and the size above the large-k shortcut border (16384 rows)
SIZES_A = (1, 3, 4, 5, 31, 32, 33, 63, 65, 127, 129, 2049, 4097)
N_LARGEK = 16385
SIZES_C = (33, 4097)
N_B = 5003                      # layout B: odd, its last chunk and its last tile are ragged
MAX_DISTANCES = (0.5, 0.85)     # every max_distance the GPU tests pass: all decoys lie under both, no allowed row under the first


def centre(seed=CENTRE_SEED):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal(DIM)
    c /= np.linalg.norm(c)
    return np.ascontiguousarray(c, dtype=np.float32)


def queries(nq=NQ_MAX, seed=QUERY_SEED, c=None):
    """nq unit queries with cos(q_i, c) = 0.9 (to f32 rounding)."""
    c64 = (centre() if c is None else c).astype(np.float64)
    c64 /= np.linalg.norm(c64)
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((nq, DIM))
    u -= (u @ c64)[:, None] * c64[None, :]
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    q = c64[None, :] + math.tan(math.acos(COS_QC)) * u
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.ascontiguousarray(q, dtype=np.float32)


def finite_decoys(m, c=None, unit_only=False, phase=0):
    """m rows 2^j c, j cycling through -2 .. 2 from `phase` on (unit_only: j = 0, for an index that refuses rows of other lengths)."""
    c = centre() if c is None else c
    j = np.zeros(m, dtype=np.int64) if unit_only else np.array([SCALES[(i + phase) % len(SCALES)] for i in range(m)], dtype=np.int64)
    return np.ascontiguousarray(np.ldexp(c[None, :].astype(np.float32), j[:, None]), dtype=np.float32)


def nonfinite_decoys(m):
    """m rows, all-NaN rows alternating with all-+Inf rows."""
    out = np.full((m, DIM), np.nan, dtype=np.float32)
    out[1::2] = np.inf
    return out


def near_row(c=None, seed=1, t=0.8):
    """An ALLOWED row nearer to every query than any random row (distance about 0.3 against 0.7), and farther than a decoy: the
    row whose stale copy a leak past a compacted corpus returns right behind the row itself."""
    c64 = (centre() if c is None else c).astype(np.float64)
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(DIM)
    u -= (u @ c64) * c64
    u /= np.linalg.norm(u)
    x = c64 + t * u
    return np.ascontiguousarray(x / np.linalg.norm(x), dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------- layouts
def allowed_rows(n, seed):
    """The rows of a fixture that a call may see: synth.unit_rows, with at least one zero row and one duplicate from 32 rows on."""
    x = synth.unit_rows(n, seed)
    if n >= 32:
        x[n // 3] = 0.0
        x[n - 2] = x[1]
    return x


def layout_a(n, seed, flavour="finite", c=None):
    """(buffer [G + n + G, 256], first allowed row = G).  flavour: "finite" or "nonfinite" guards."""
    buf = np.empty((G + n + G, DIM), dtype=np.float32)
    if flavour == "finite":
        buf[:G] = finite_decoys(G, c, phase=1)
        buf[G + n:] = finite_decoys(G, c, phase=3)
    else:
        buf[:G] = nonfinite_decoys(G)
        buf[G + n:] = nonfinite_decoys(G)[::-1]      # the row right behind the corpus is an Inf row, the one right before it too
    buf[G:G + n] = allowed_rows(n, seed)
    return buf, G


def in_ranges(n, ranges):
    mask = np.zeros(n, dtype=bool)
    for b, e in ranges:
        mask[b:e] = True
    return mask


def layout_b(n, ranges, seed, c=None, unit_only=False):
    """(buffer [n + G, 256], ids of the allowed rows): the corpus is the first n rows, every row of it outside `ranges` is a finite
    decoy, and so are the G rows behind it (append all, truncate to n: a range that ends at n has a guard behind it too)."""
    emb = np.concatenate([allowed_rows(n, seed), np.zeros((G, DIM), dtype=np.float32)])
    mask = in_ranges(n + G, ranges)
    out = np.flatnonzero(~mask)
    emb[out] = finite_decoys(len(out), c, unit_only=unit_only)
    return np.ascontiguousarray(emb), np.flatnonzero(mask)


def layout_c(n, seed, c=None):
    """[n + G, 256]: n allowed rows, then G finite decoys (append all, truncate to n)."""
    return np.ascontiguousarray(np.concatenate([allowed_rows(n, seed), finite_decoys(G, c, phase=2)]))


def layout_shards(sizes, seed, c=None):
    """(buffer, first row of every shard in the buffer): [G | shard 0 | G | shard 1 | G | ... | G], the shards' rows being
    consecutive pieces of allowed_rows(sum(sizes), seed)."""
    rows = allowed_rows(int(sum(sizes)), seed)
    parts, first, at, done = [finite_decoys(G, c)], [], G, 0
    for i, s in enumerate(sizes):
        first.append(at)
        parts += [rows[done:done + s], finite_decoys(G, c, phase=i + 1)]
        at += s + G
        done += s
    return np.ascontiguousarray(np.concatenate(parts)), first, rows


def dense_ranges(n=N_B):
    """Ranges for the tile table (they fill about half of nearly every 32-row tile, so tiles_dense holds): 32 ranges whose begins and
    ends take every residue mod 32 (and mod 4), the first one starting at row 0; then empty ranges, single rows, two single rows one
    decoy apart, and a range that ends at n."""
    out = []
    for i in range(40):
        b = 110 * i + i % 32                      # = 15 i (mod 32): every residue over 32 consecutive i
        out.append((b, b + 41 + (12 * i) % 32))   # end = 27 i + 9 (mod 32): every residue too
    t = out[-1][1] + 20
    out += [(t, t), (t + 1, t + 2), (t + 3, t + 4), (t + 5, t + 9), (t + 10, t + 10), (t + 37, t + 38), (t + 64, t + 96), (t + 97, t + 160)]
    out.append((n - 12, n))
    assert out[-2][1] < n - 12
    return out


def sparse_ranges(n=N_B):
    """Ranges for the chunk table only (far below the tile table's density): 1 .. 5 rows every 53 rows, begins and ends at every residue
    mod 4, with an empty range now and then; the first starts at row 0, the last ends at n."""
    out = []
    for i in range((n - 20) // 53):
        b = 53 * i
        out.append((b, b + 1 + i % 5))
        if i % 7 == 3:
            out.append((b + 9, b + 9))
    out.append((n - 3, n))
    return out


def range_lists(n=N_B):
    return dict(dense=dense_ranges(n), sparse=sparse_ranges(n))


# ---------------------------------------------------------------------------------------------------------------- reference
def expected(allowed, ids, qs, k, max_distance=None):
    """Per query (rows as a list, f64 distances): the oracle's accurate form over the ALLOWED rows only, ids mapped back through `ids`
    (None: the rows' own positions).  max_distance: every row under it (the oracle's threshold mode), k ignored."""
    allowed = np.ascontiguousarray(allowed, dtype=np.float32)
    out = []
    for q in np.ascontiguousarray(qs, dtype=np.float32).reshape(-1, DIM):
        res = orc.search_documents(allowed, [len(allowed)], q, n_lines=0, top_k=k, max_distance=max_distance, accurate=True)
        rows = np.array([r["match_line"] for r in res], dtype=np.int64)
        if ids is not None:
            rows = np.asarray(ids, dtype=np.int64)[rows]
        out.append((rows.tolist(), np.array([r["distance"] for r in res], dtype=np.float64)))
    return out


def expected_workspace(allowed, ids, qs, k, max_distance):
    """Store::search_line_embeddings' rule on top of `expected`: keep score = 1 - d > 1 - max_distance (the threshold in f32), best k."""
    thr = float(np.float32(1.0) - np.float32(max_distance))
    out = []
    for rows, dist in expected(allowed, ids, qs, k):
        keep = [j for j in range(len(rows)) if (1.0 - dist[j]) > thr]
        out.append(([rows[j] for j in keep], dist[keep]))
    return out


def control(ctx, allowed):
    """A fresh OWNED corpus that holds only the allowed rows: no decoy anywhere near it (G zero rows -- distance 1 to every query --
    are appended behind them and truncated away, so the memory behind the rows is the corpus' own and holds nothing that could
    win).  The caller runs the same call on it, for the status words a route without decoys gives, and closes it."""
    import semtools_amd as smt

    allowed = np.ascontiguousarray(allowed, dtype=np.float32)
    c = smt.Corpus(ctx)
    c.append(np.concatenate([allowed, np.zeros((G, DIM), dtype=np.float32)]))
    c.truncate(len(allowed))
    return c


def distances64(rows, qs):
    """float64 cosine distances [rows, queries] in NumPy (zero rows: 1), for the conditions on the inputs."""
    x = np.asarray(rows, dtype=np.float64)
    q = np.asarray(qs, dtype=np.float64).reshape(-1, DIM)
    nx = np.linalg.norm(x, axis=1)
    nq = np.linalg.norm(q, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        cos = (x @ q.T) / (nx[:, None] * nq[None, :])
    cos[nx == 0.0] = 0.0
    return 1.0 - cos
