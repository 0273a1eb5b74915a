"""A NumPy reference of the threshold search (K4, csrc/threshold.hip: every row with distance < max_distance, ordered by distance
and then by row), a model of how ONE wave collects its hits, and the constructed corpora the threshold tests search.  NumPy only:
nothing here imports the library.  tests/test_threshold_ref_cpu.py holds the reference against the C oracle, proves that every case
reaches the branch it was written for, and shows that six subtly wrong threshold searches each fail a named case;
tests/test_gpu_threshold.py runs the cases through Corpus.search.

The corpora.  A HIT row of a query q is normalize(q + t g), g a random unit vector (t = 0.9: distance about 0.19 .. 0.33), a MISS row
a random unit row (distance about 0.75 .. 1.25), every row scaled by a power of two in 2^-3 .. 2^3; max_distance is 0.6.  Every
builder asserts that no row of the corpus lies between HIT_BELOW and MISS_ABOVE for any query of the case: the empty band is a few
hundred times wider than the widest nomination band of the library (5.2e-4, the fp16 image), so the rows a kernel COLLECTS are the
rows the exact test keeps, and the hit counts the cases are named after are the counts the kernels see.  The border cases, whose
thresholds sit at distance 1, and the strictness cases, whose threshold IS a row's distance, say what they assert instead.

The one-wave model.  With scan_blocks = 1 and scan_threads = 64 the kernel is one wave that takes the chunks (4 rows; with ranges
every range is cut into chunks from its own first row, the last one short) in order: c(t) = t in csrc/chunk_deal.h.  A chunk's hits
go to a 256-entry buffer, which is flushed BEFORE a chunk that would not fit, and once at the end; a flush takes its slots from one
counter and stores the entries whose slot is below the capacity of the first pass (tuning key thr_hit_cap); a pass that counted
more hits than that runs again.  collect_one_wave() returns what such a pass stores and the sizes of its flushes."""
import zlib

import numpy as np

DIM = 256
CHUNK = 4                   # rows per chunk of the streaming kernels
HIT_BUF = 256               # entries of a wave's hit buffer
HOST_ORDER_MAX = 2048       # up to this many collected hits the host orders them, above it the device sorts
CAND_CAP = 2048             # candidate slots per query of the batched sweep
PREFILTER_GUARD = 8e-6      # the f32 prefilter of K4 is d32 < max_distance + 8e-6
MAX_DISTANCE = 0.6
HIT_BELOW, MISS_ABOVE = 0.40, 0.70
F = np.float32


# ------------------------------------------------------------------------------------------------------------------- the reference
def distances(emb, q):
    """oracle_np.cosine_accurate(q, row) for every row: the same f64 operations in the same order (np.add.accumulate adds one
    element after the other), vectorised over the rows."""
    a = np.asarray(q, dtype=np.float64).reshape(DIM)
    b = np.asarray(emb, dtype=np.float64).reshape(-1, DIM)
    if len(b) == 0:
        return np.zeros(0)
    ab = np.add.accumulate(a[None, :] * b, axis=1)[:, -1]
    a2 = np.add.accumulate(a * a)[-1]
    b2 = np.add.accumulate(b * b, axis=1)[:, -1]
    with np.errstate(divide="ignore", invalid="ignore"):
        d = 1.0 - ab * (1.0 / np.sqrt(a2)) * (1.0 / np.sqrt(b2))
    d = np.where(d > 0, d, 0.0)
    d[ab == 0] = 1.0
    if a2 == 0:
        d[b2 == 0] = 0.0
    return d


def distances_serial(emb, q):
    """oracle_np.cosine_serial(q, row) for every row (sums in f32, one element after the other), as float64."""
    a = np.asarray(q, dtype=F).reshape(DIM)
    b = np.asarray(emb, dtype=F).reshape(-1, DIM)
    ab = np.add.accumulate(a[None, :] * b, axis=1, dtype=F)[:, -1].astype(np.float64)
    a2 = float(np.add.accumulate(a * a, dtype=F)[-1])
    b2 = np.add.accumulate(b * b, axis=1, dtype=F)[:, -1].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = 1.0 - ab * (1.0 / np.sqrt(a2)) * (1.0 / np.sqrt(b2))
    d = np.where(d > 0, d, 0.0)
    d[ab == 0] = 1.0
    if a2 == 0:
        d[b2 == 0] = 0.0
    return d


def eligible(n, ranges):
    """The rows a call may return, ascending."""
    if ranges is None:
        return np.arange(n, dtype=np.int64)
    parts = [np.arange(b, e, dtype=np.int64) for b, e in ranges]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)


def answer(emb, q, max_distance, ranges=None, top_k=None):
    """(rows uint64, f64 distances): every eligible row with distance < max_distance, by (distance, row); with ranges the distances are
    computed over the gathered rows and the positions mapped back.  top_k: the first top_k of them (max_distance may be +inf)."""
    rows = eligible(len(emb), ranges)
    d = distances(np.asarray(emb)[rows], q)
    keep = d < max_distance
    rows, d = rows[keep], d[keep]
    order = np.lexsort((rows, d))[:top_k]
    return rows[order].astype(np.uint64), d[order]


# ------------------------------------------------------------------------------------------------------------ the one-wave model
def chunks_of(n, ranges=None):
    """[(first row, valid rows)] in the order one wave takes them."""
    out = []
    for b, e in ([(0, n)] if ranges is None else ranges):
        out += [(r, min(CHUNK, e - r)) for r in range(b, e, CHUNK)]
    return out


class Collected:
    def __init__(self):
        self.rows, self.count, self.flushes, self.fits = [], 0, [], []

    @property
    def sizes(self):
        return [size for _, size in self.flushes]


def collect_one_wave(passes, ranges=None, cap=None, wrong=None):
    """One pass of the one-wave kernel over rows whose prefilter verdicts are `passes`.  Returns .rows (what the pass stored, in slot
    order), .count (the hits it counted), .flushes [(first slot, size)] and .fits [(pending, arriving)] for every chunk that filled
    the buffer to exactly HIT_BUF without a flush.  wrong: one of the collect mistakes of WRONG."""
    passes = np.asarray(passes, dtype=bool)
    n, out, buf = len(passes), Collected(), []

    def flush(arriving=None):
        if not buf:
            return
        out.flushes.append((out.count, len(buf)))
        keep = buf[:HIT_BUF - arriving] if wrong == "flush-keeps-256-minus-cnt" and arriving is not None else buf
        out.rows += [r for i, r in enumerate(keep) if cap is None or out.count + i < cap]
        out.count += len(buf)
        del buf[:]

    for row0, valid in chunks_of(n, ranges):
        width = min(CHUNK, n - row0) if wrong == "short-chunk-read-whole" else valid
        hits = [r for r in range(row0, row0 + width) if passes[r]]
        if not hits:
            continue
        if len(buf) + len(hits) > HIT_BUF:
            flush(len(hits))
            if wrong == "drops-the-chunk-that-triggers-a-flush":
                continue
        elif len(buf) + len(hits) == HIT_BUF:
            out.fits.append((len(buf), len(hits)))
        buf += hits
    flush()
    return out


def launches(passes, ranges=None, cap=None):
    """Scan launches of one threshold query: a second one when the first pass counted more hits than it had slots for."""
    n_virtual = len(eligible(len(passes), ranges))
    return 2 if collect_one_wave(passes, ranges).count > min(n_virtual, cap if cap is not None else 1 << 20) else 1


# ------------------------------------------------------------------------------------------------------------------ wrong variants
WRONG = {
    "drops-the-chunk-that-triggers-a-flush": "the collect flushes the full buffer and forgets the chunk that did not fit",
    "flush-keeps-256-minus-cnt": "a flush in front of a chunk of cnt hits stores only the first 256 - cnt pending entries",
    "short-chunk-read-whole": "the last, short chunk of a range is read as four rows",
    "cut-with-<=": "the exact test keeps distance <= max_distance",
    "cut-at-the-f32-prefilter": "the cut is made on the serial f32 distance, not on the f64 value",
    "second-sort-not-stable": "above 2048 hits equal distances come back in arrival order, not in row order",
}


def prefilter_passes(emb, q, max_distance):
    """Which rows the f32 prefilter lets through, from the exact distances: true for the band-separated cases, whose rows keep away
    from max_distance by far more than f32 noise, and for the strictness cases, whose cluster lies inside the 8e-6 guard."""
    return distances(emb, q) < max_distance + PREFILTER_GUARD


def wrong_answer(kind, emb, q, max_distance, ranges=None, top_k=None):
    """The answer a threshold search with mistake `kind` would give (the one-wave launch where the collect matters)."""
    emb = np.asarray(emb)
    rows = eligible(len(emb), ranges)
    d_all = distances(emb, q)
    if kind in ("drops-the-chunk-that-triggers-a-flush", "flush-keeps-256-minus-cnt", "short-chunk-read-whole"):
        rows = np.array(sorted(collect_one_wave(d_all < max_distance + PREFILTER_GUARD, ranges, wrong=kind).rows), dtype=np.int64)
    d = d_all[rows]
    if kind == "cut-with-<=":
        keep = d <= max_distance
    elif kind == "cut-at-the-f32-prefilter":
        keep = distances_serial(emb[rows], q) < max_distance
    else:
        keep = d < max_distance
    device_order = int((d < max_distance + PREFILTER_GUARD).sum()) > HOST_ORDER_MAX     # (decided by what the scan collected)
    rows, d = rows[keep], d[keep]
    tie_break = rows
    if kind == "second-sort-not-stable" and device_order:
        tie_break = (rows // CHUNK % 8) * len(emb) + rows            # eight waves, each one's hits arriving together
    order = np.lexsort((tie_break, d))[:top_k]
    return rows[order].astype(np.uint64), d[order]


# ------------------------------------------------------------------------------------------------------------------------ rows
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _unit(x):
    x = np.asarray(x, dtype=np.float64)
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(F)


def _query(rng):
    return _unit(rng.standard_normal(DIM))


def _near(q, rng, n, t=0.9):
    return _unit(q.astype(np.float64)[None, :] + t * _unit(rng.standard_normal((n, DIM))).astype(np.float64))


def _scaled(rows, rng):
    """every row times a power of two in 2^-3 .. 2^3: exact in f32, and the f64 distance keeps its bits"""
    return (rows * (2.0 ** rng.integers(-3, 4, size=(len(rows), 1))).astype(F)).astype(F)


def _from_mask(q, mask, rng, far=False):
    """hit rows where the mask is set, miss rows elsewhere (far: rows around -q, distance about 1.7, for thresholds at 1)"""
    mask = np.asarray(mask, dtype=bool)
    emb = _near(-q, rng, len(mask)) if far else _unit(rng.standard_normal((len(mask), DIM)))
    emb[mask] = _near(q, rng, int(mask.sum()))
    return _scaled(emb, rng)


def assert_band(emb, qs, masks, below=HIT_BELOW, above=MISS_ABOVE):
    for q, mask in zip(qs, masks):
        d = distances(emb, q)
        assert not mask.any() or d[mask].max() < below, ("a hit row inside the band", float(d[mask].max()))
        assert mask.all() or d[~mask].min() > above, ("a miss row inside the band", float(d[~mask].min()))


class Case:
    """One corpus with its queries, thresholds and (optional) ranges.  masks[i]: the rows planted as hits of query i.  A case with
    ranges is searched unfiltered AND inside them."""

    def __init__(self, name, emb, qs, masks, mds=(MAX_DISTANCE,), ranges=None, top_k=None, **notes):
        self.name, self.emb, self.qs = name, np.ascontiguousarray(emb, dtype=F), np.ascontiguousarray(qs, dtype=F).reshape(-1, DIM)
        self.masks, self.mds, self.ranges, self.top_k = [np.asarray(m, dtype=bool) for m in masks], tuple(mds), ranges, top_k
        self.n = len(self.emb)
        self.__dict__.update(notes)
        self._answers = {}
        if ranges is not None:
            assert all(0 <= b < e <= self.n for b, e in ranges) and all(x[1] <= y[0] for x, y in zip(ranges, ranges[1:])), name

    def range_options(self):
        return (None,) if self.ranges is None else (None, self.ranges)

    def answer(self, qi=0, md=None, ranges=None, top_k=None):
        md = self.mds[0] if md is None else md
        key = (qi, md, None if ranges is None else tuple(ranges), top_k)
        if key not in self._answers:
            self._answers[key] = answer(self.emb, self.qs[qi], md, ranges, top_k)
        return self._answers[key]

    def passes(self, qi=0, md=None):
        return prefilter_passes(self.emb, self.qs[qi], self.mds[0] if md is None else md)

    def runs(self):
        """every (query, max_distance, ranges) a test of the plain threshold search goes through"""
        return [(qi, md, rg) for qi in range(len(self.qs)) for md in self.mds for rg in self.range_options()]


# -------------------------------------------------------------------------------------------------- family 1: the hit buffer's flushes
def _reach(pending, target):
    """chunk hit counts that bring a buffer of `pending` entries to exactly `target`"""
    left = target - pending
    assert left >= 0
    return [CHUNK] * (left // CHUNK) + ([left % CHUNK] if left % CHUNK else [])


def _counts_for(steps, tail=()):
    """steps [(target, trigger)]: fill the buffer to `target` pending hits, then a chunk of `trigger` hits arrives."""
    counts, pending = [], 0
    for target, trigger in steps:
        counts += _reach(pending, target) + [trigger]
        pending = trigger
    return counts + list(tail)


def _counts_total(total, target=253, trigger=CHUNK):
    """flushes of `target` entries until `total` hits have been dealt"""
    counts, pending = [], 0
    while sum(counts) < total:
        counts += _reach(pending, target) + [trigger]
        pending = trigger
    while sum(counts) > total:
        over = sum(counts) - total
        counts[-1] -= min(over, counts[-1])
        if counts[-1] == 0:
            counts.pop()
    return counts


def _chunk_masks(counts, n_chunks, rng):
    """[n_chunks][4] hit patterns: the chunks with hits in the given order, chunks without hits dealt between them at random."""
    assert n_chunks >= len(counts)
    slots = np.sort(rng.permutation(n_chunks)[:len(counts)])
    m = np.zeros((n_chunks, CHUNK), dtype=bool)
    for s, c in zip(slots, counts):
        m[s, rng.permutation(CHUNK)[:c]] = True
    return m


FLUSH_SPECS = {     # name: (steps, tail counts, hits in the short last chunk of 3 rows)
    "flush-253+4": ([(253, 4), (253, 4)], (), 0),
    "flush-254+3": ([(254, 3), (254, 3)], (), 0),
    "flush-255+2": ([(255, 2), (255, 2)], (), 0),
    "flush-256+1": ([(256, 1), (256, 1)], (), 0),
    "flush-256+4": ([(256, 4), (256, 4)], (), 0),
    "flush-mixed": ([(253, 4), (254, 3), (255, 2), (256, 1), (256, 4), (254, 4), (255, 3), (255, 4), (253, 4)], (2, 1), 2),
    "fit-255+1": ([(255, 1)], (), 0),                       # 255 pending, one arrives: exactly full, no flush, then the end
    "total-512": ([(256, 4)], _reach(4, 256), 0),           # 128 chunks of four: the hit total is a multiple of the buffer
    "none": ([], (), 0),
}
# what the model must report for the unfiltered corpus and for its ranged twin, in this order
FLUSH_SIZES = {
    "flush-253+4": [253, 253, 4], "flush-254+3": [254, 254, 3], "flush-255+2": [255, 255, 2], "flush-256+1": [256, 256, 1],
    "flush-256+4": [256, 256, 4], "flush-mixed": [253, 254, 255, 256, 256, 254, 255, 255, 253, 9], "fit-255+1": [256],
    "total-512": [256, 256], "none": [],
}
N_FLUSH_CHUNKS = 750


def _flush_case(name, ranged):
    steps, tail, last_hits = FLUSH_SPECS[name]
    rng = _rng(name)
    q = _query(rng)
    m = _chunk_masks(_counts_for(steps, tail), N_FLUSH_CHUNKS, rng)
    last = np.zeros(3, dtype=bool)
    last[:last_hits] = True                                  # the short last chunk: 3 rows
    if not ranged:
        mask = np.concatenate([m.reshape(-1), last])
        ranges = None
    else:
        # the same chunks cut into pieces, one range each; between the ranges 1 .. 7 rows that WOULD be hits.  Every piece but the
        # last is whole chunks, so the wave meets the same hit counts in the same order; the last range ends on the last row.
        parts, ranges, at, c = [], [], 0, 0
        while c < N_FLUSH_CHUNKS:
            gap = int(rng.integers(1, 8))
            parts.append(np.ones(gap, dtype=bool))
            at += gap
            take = min(int(rng.integers(1, 40)), N_FLUSH_CHUNKS - c)
            piece = m[c:c + take].reshape(-1)
            c += take
            if c == N_FLUSH_CHUNKS:
                piece = np.concatenate([piece, last])
            parts.append(piece)
            ranges.append((at, at + len(piece)))
            at += len(piece)
        mask = np.concatenate(parts)
    emb = _from_mask(q, mask, rng)
    assert_band(emb, [q], [mask])
    return Case(name + ("-ranges" if ranged else ""), emb, q, [mask], ranges=ranges, flush_sizes=FLUSH_SIZES[name])


def _rerun_case(name, total):
    """`total` hits collected in flushes of 253: with thr_hit_cap = 512 the third flush starts at slot 506 and the capacity falls
    inside it.  The ranges are two adjacent ones that cover every chunk (the second begins on a chunk border, so the wave meets the
    same chunks) and leave six miss rows out."""
    rng = _rng(name)
    q = _query(rng)
    n_chunks = max(N_FLUSH_CHUNKS, total // 2)
    mask = np.concatenate([_chunk_masks(_counts_total(total), n_chunks, rng).reshape(-1), np.zeros(6, dtype=bool)])
    ranges = [(0, CHUNK * 100), (CHUNK * 100, CHUNK * n_chunks)]
    emb = _from_mask(q, mask, rng)
    assert_band(emb, [q], [mask])
    return Case(name, emb, q, [mask], ranges=ranges, total=total)


# ---------------------------------------------------------------------------------------------------------- family 2: short ranges
RANGE_LENGTHS = (1, 2, 3, 4, 5, 7, 9)


def _ranges_layout(n=2003):
    """Ranges of every length in RANGE_LENGTHS: first touching one another, then far apart at odd offsets, the last one ending on
    the corpus' last row."""
    out, at = [], 13
    for length in RANGE_LENGTHS + RANGE_LENGTHS[::-1]:          # adjacent: each begins where the one before ends
        out.append((at, at + length))
        at += length
    at += 50
    for i, length in enumerate(RANGE_LENGTHS * 3):              # far apart
        out.append((at, at + length))
        at += length + 37 + 2 * i
    assert at < n - 9
    out.append((n - 5, n))
    return out


def _ranges_case(name):
    rng = _rng(name)
    q = _query(rng)
    n = 2003
    ranges = _ranges_layout(n)
    inside = np.zeros(n, dtype=bool)
    for b, e in ranges:
        inside[b:e] = True
    if name == "ranges-hits-inside":
        mask = inside.copy()                                    # every row of a range is a hit, every row outside a miss
    else:
        # "ranges-hits-outside": the four rows in front of and behind every range are hits the call must not return; inside, the
        # last row of every range -- in its short last chunk -- is a hit and the others are misses
        mask = np.zeros(n, dtype=bool)
        for b, e in ranges:
            mask[max(0, b - CHUNK):b] = True
            mask[e:e + CHUNK] = True
        mask &= ~inside
        for b, e in ranges:
            mask[e - 1] = True
    emb = _from_mask(q, mask, rng)
    assert_band(emb, [q], [mask])
    return Case(name, emb, q, [mask], ranges=ranges)


# ------------------------------------------------------------------------------------ family 3: 2048 hits, host order / device order
BORDER_COUNTS = (2047, 2048, 2049, 4100)
N_ZERO, N_SAME, N_DUP = 3, 3, 600


def _border_case(name, collected):
    """`collected` rows pass the prefilter at max_distance = 1 and one step above it: N_SAME rows identical to the query (distance 0;
    one of them times 4, one times 1/4), N_ZERO zero rows (distance exactly 1: kept one step above 1, cut at 1), N_DUP copies of one
    hit row at power-of-two scales (equal f64 distances: row order decides) and ordinary hits.  The misses lie around -q.  The copies
    sit in the sorted answer from about position 1748 on where there are that many hits, so they straddle position 2048."""
    rng = _rng(name)
    q = _query(rng)
    n_plain = collected - N_ZERO - N_SAME - (N_DUP - 1)
    n = collected + 1200
    spots = rng.permutation(n)
    emb = _near(-q, rng, n)
    plain = _near(q, rng, n_plain)
    order = np.argsort(distances(plain, q), kind="stable")
    src = plain[order[min(1748 - N_SAME, n_plain - 4)]]
    at = 0
    emb[spots[at:at + n_plain]] = plain
    at += n_plain
    emb[spots[at:at + N_DUP - 1]] = src
    at += N_DUP - 1
    emb = _scaled(emb, rng)
    emb[spots[at:at + N_SAME]] = np.stack([q, q * F(4), q * F(0.25)])
    at += N_SAME
    zero = spots[at:at + N_ZERO]
    emb[zero] = 0.0
    at += N_ZERO
    assert at == collected
    mask = np.zeros(n, dtype=bool)
    mask[spots[:collected]] = True
    d = distances(emb, q)
    assert (d[zero] == 1.0).all() and d[mask & (d != 1.0)].max() < 0.9 and d[~mask].min() > 1.1
    ties = np.unique(d[mask], return_counts=True)[1]
    assert ties.max() == N_DUP, ties.max()
    return Case(name, emb, q, [mask], mds=(1.0, float(np.nextafter(1.0, 2.0))), collected=collected, zero_rows=zero)


# --------------------------------------------------------------------------------------------- family 4: max_distance IS a distance
N_CLUSTER = 600


def _strict_case(name, pad):
    """A cluster base + eps g around distance 0.26, max_distance the exact distance of one member (and one f64 step above and below
    it), copies of that member in three other chunks.  Query 0 is the cluster's; query 2 is twice query 0 (the same f64 distances);
    queries 1 and 3 have twenty plain hits each.  pad: that many plain hits of query 0 well below the cluster."""
    rng = _rng(name)
    q, q1, q3 = _query(rng), _query(rng), _query(rng)
    base = _near(q, rng, 1)[0].astype(np.float64)
    g = _unit(rng.standard_normal((N_CLUSTER, DIM))).astype(np.float64)
    n = 2400 + pad
    spots = rng.permutation(n)
    cl = np.sort(spots[:N_CLUSTER])
    eps = 2e-5
    while True:
        members = (base[None, :] + eps * g).astype(F)
        exact, serial = distances(members, q), distances_serial(members, q)
        star = int(np.argsort(exact, kind="stable")[N_CLUSTER // 2])
        md = float(exact[star])
        straddle = int(((serial < md) != (exact < md)).sum())
        if straddle >= 5 and np.abs(exact - md).max() <= PREFILTER_GUARD:
            break
        eps /= 2
        assert eps > 1e-8, "no eps puts five members' f32 and f64 distances on opposite sides of max_distance"
    emb = _unit(rng.standard_normal((n, DIM)))
    emb[cl] = members
    copies = []
    for s in spots[N_CLUSTER:]:                                 # copies of the member max_distance was taken from, in three other chunks
        if all(s // CHUNK != c // CHUNK for c in copies + [int(cl[star])]):
            copies.append(int(s))
        if len(copies) == 3:
            break
    emb[copies] = members[star]
    used = set(cl.tolist()) | set(copies)
    free = np.array([s for s in spots if s not in used])
    masks = [np.zeros(n, dtype=bool) for _ in range(4)]
    masks[0][cl] = masks[0][copies] = True
    emb[free[:pad]] = _near(q, rng, pad, t=0.5)
    masks[0][free[:pad]] = True
    emb[free[pad:pad + 20]] = _near(q1, rng, 20, t=0.5)
    masks[1][free[pad:pad + 20]] = True
    emb[free[pad + 20:pad + 40]] = _near(q3, rng, 20, t=0.5)
    masks[3][free[pad + 20:pad + 40]] = True
    masks[2] = masks[0]
    qs = np.stack([q, q1, q * F(2), q3])
    d = distances(emb, q)
    assert (d[copies] == md).all() and d[cl[star]] == md
    assert np.abs(d[cl] - md).max() <= PREFILTER_GUARD
    assert pad == 0 or d[free[:pad]].max() < 0.2
    rest = np.ones(n, dtype=bool)
    rest[cl] = rest[copies] = rest[free[:pad]] = False
    assert d[rest].min() > MISS_ABOVE
    assert_band(emb, [q1, q3], [masks[1], masks[3]], below=0.2)
    mds = (md, float(np.nextafter(md, 2.0)), float(np.nextafter(md, 0.0)))
    ranges = [(3, n // 3), (n // 3 + 2, n // 3 + 9), (n // 3 + 11, n - 2)]
    return Case(name, emb, qs, masks, mds=mds, ranges=ranges, straddle=straddle, eps=eps, star=int(cl[star]), copies=copies,
                cluster=cl)


# ------------------------------------------------------------------------------------------ family 5: the sweep's candidate capacity
SWEEP_COUNTS = (0, 1, 2047, 2048, 2049, 3000)


def _sweep_case(name):
    """Six queries over one corpus, each with its own planted hits: SWEEP_COUNTS of them."""
    rng = _rng(name)
    qs = np.stack([_query(rng) for _ in SWEEP_COUNTS])
    n = 12000
    spots = rng.permutation(n)
    emb = _unit(rng.standard_normal((n, DIM)))
    masks, at = [], 0
    for q, count in zip(qs, SWEEP_COUNTS):
        mask = np.zeros(n, dtype=bool)
        mask[spots[at:at + count]] = True
        emb[mask] = _near(q, rng, count)
        masks.append(mask)
        at += count
    emb = _scaled(emb, rng)
    assert_band(emb, qs, masks)
    return Case(name, emb, qs, masks)


# ------------------------------------------------------------------------------- family 6: a top-k re-answer with more than 2048 ties
N_TIED = 2100


def _reanswer_case(name):
    """Five rows nearer than N_TIED exact copies of one row: top_k = 10 ends inside the copies, the scan cannot prove its list, and
    the exhaustive re-answer collects 5 + N_TIED rows.  The answer: the five, then the first five copies by row."""
    rng = _rng(name)
    q = _query(rng)
    n = 6001
    spots = rng.permutation(n)
    emb = _scaled(_unit(rng.standard_normal((n, DIM))), rng)
    near, tied = spots[:5], np.sort(spots[5:5 + N_TIED])
    for i, s in enumerate(near):
        emb[s] = _near(q, rng, 1, t=0.3 + 0.05 * i)[0]
    emb[tied] = _near(q, rng, 1)[0]
    mask = np.zeros(n, dtype=bool)
    mask[near] = mask[tied] = True
    assert_band(emb, [q], [mask])
    d = distances(emb, q)
    assert len(np.unique(d[tied])) == 1 and d[near].max() < d[tied[0]]
    ranges = [(int(tied[7]), 2500), (2600, n)]                  # leaves the first seven copies out
    inside = eligible(n, ranges)
    assert np.isin(near, inside).all() and np.isin(tied, inside).sum() > HOST_ORDER_MAX
    return Case(name, emb, q, [mask], mds=(float("inf"),), ranges=ranges, top_k=10, near=near, tied=tied)


# ------------------------------------------------------------------------------------------------------------------------ the cases
_BUILDERS = {}
for _name in FLUSH_SPECS:
    _BUILDERS[_name] = lambda name=_name: _flush_case(name, False)
    _BUILDERS[_name + "-ranges"] = lambda name=_name: _flush_case(name, True)
for _name in ("ranges-hits-inside", "ranges-hits-outside"):
    _BUILDERS[_name] = lambda name=_name: _ranges_case(name)
for _c in BORDER_COUNTS:
    _BUILDERS["border-%d" % _c] = lambda c=_c: _border_case("border-%d" % c, c)
_BUILDERS["strict"] = lambda: _strict_case("strict", 0)
_BUILDERS["strict-padded"] = lambda: _strict_case("strict-padded", 1700)
_BUILDERS["sweep-capacity"] = lambda: _sweep_case("sweep-capacity")
_BUILDERS["reanswer"] = lambda: _reanswer_case("reanswer")
RERUN_TOTALS = (511, 512, 513, 1500, 2500)
for _t in RERUN_TOTALS:
    _BUILDERS["rerun-%d" % _t] = lambda t=_t: _rerun_case("rerun-%d" % t, t)

NAMES = list(_BUILDERS)
FLUSH_NAMES = [n for n in NAMES if n.split("-ranges")[0] in FLUSH_SPECS]
_CASES = {}


def case(name):
    """The case, built once per process and never changed."""
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
        _CASES[name].emb.setflags(write=False)
    return _CASES[name]
