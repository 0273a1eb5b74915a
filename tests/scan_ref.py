"""The scan stage (K2) restated in NumPy: which rows a block owns, what its list must hold, and models of scans that get it wrong.

A top-k answer with top_k <= 56 is made in two stages.  The scan kernels fill one sorted list of k' = min(64, top_k + guard_band) keys
per (query, block), key = f32 distance bits << 32 | row; final_select_kernel re-scores in f64 and proves the answer complete.  The
proof rests on two properties of the scan stage, and this module states both without the library:

  1. every block list holds the k' smallest keys of exactly the rows chunk_deal.h gives that block -- no row lost, doubled or taken
     from outside, the padding written;
  2. |d32 - d64| <= F32_ERR_SCAN (common.h) for every key a scan kernel writes.

The deal (chunk_deal.h, scan_topk.hip): the scanned rows are cut into chunks of U rows -- unfiltered: chunk c = rows [c U, c U + U),
the last one ragged; filtered: the chunk table of range_tables.hip, U = 4, every range ending in a chunk of its own -- and chunk c
belongs to block (c // waves) % blocks, waves = scan_threads / 64.  A pass of two or four query slots planned at scan_unroll = 2 runs
the kernel built for 8 rows per chunk (scan_kernel_for), so the deal of a call may differ from pass to pass.  STEAL deals the last
groups at run time: only the union of the lists can be checked then.

check_lists is the judge of tests/test_gpu_scan_lists.py; tests/test_scan_ref_cpu.py holds it to account: the reference lists merge
to the oracle's answer, and every wrong scan of WRONG_SCANS fails a named case.  NumPy only, nothing of the library is imported."""
import numpy as np

from tests import nominate_ref
from tests.rollcall import chunk_table

DIM = 256
F32_ERR_SCAN = 4e-6                     # csrc/common.h
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)     # KEY_PAD
POISON = np.uint64(0x5A5A5A5A5A5A5A5A)  # what smt_debug_scan_lists presets the list area to
POISON32 = 0x5A5A5A5A
SEL_MAX_LISTS = 512
FILTER_CHUNK = 4
UNCLEAR_CAP = 0.02                      # at most this share of a case's lists may have an unclear border

exact_distances = nominate_ref.exact_distances


# ---------------------------------------------------------------------------------------------------------------- the plan
def kprime(top_k, guard_band=8):
    """candidates_per_list (scan_launch.hip)"""
    return min(64, top_k + guard_band)


def passes(nq):
    """launch_scan_topk's pass loop: [(first query, queries, slots)]; three queries ride in four slots."""
    out, q0 = [], 0
    while q0 < nq:
        left = nq - q0
        out.append((q0, min(left, 4), 4 if left >= 3 else left))
        q0 += min(left, 4)
    return out


def kernel_unroll(U, slots):
    """scan_kernel_for: two and four slots are built for 4 and 8 rows per chunk."""
    return 8 if slots > 1 and U == 2 else U


def n_chunks_of(n, U, ranges=None):
    return len(chunk_table(ranges)) if ranges is not None else -(-n // U)


def planned_blocks(n, scan_blocks, threads, U, num_cus, ranges=None):
    """plan_scan's grid: scan_blocks (0 = one block per CU), at most 512, and no idle blocks for tiny inputs.  n: the corpus' rows
    (unfiltered); U: scan_unroll as set (a filtered call plans with 4)."""
    n_chunks = n_chunks_of(n, FILTER_CHUNK if ranges is not None else U, ranges)
    blocks = min(scan_blocks if scan_blocks > 0 else num_cus, SEL_MAX_LISTS)
    waves = threads // 64
    if blocks * waves > n_chunks:
        blocks = max(1, -(-n_chunks // waves))
    return blocks


def steal_on(n, blocks, threads, U, scan_steal, ranges=None):
    """steal_setup: the condition under which a pass runs the STEAL kernel."""
    return ranges is None and U == 4 and threads == 512 and scan_steal > 0 and n_chunks_of(n, U) >= blocks * 8 * scan_steal * 8


def route_word(U, nt, threads, nq, filtered=False, steal=False):
    """out_route of smt_debug_scan_lists (include/semtools_hip.h)"""
    w = (FILTER_CHUNK if filtered else U) | (0x10 if nt else 0) | (0x20 if filtered else 0) | (0x40 if steal else 0) | threads << 8
    for i, (_, _, slots) in enumerate(passes(nq)):
        w |= slots << (20 + 4 * i)
    return w


class Deal:
    """The chunks of one pass and the block each belongs to: row0, cnt (valid rows), block, lane (c % waves: the wave that starts on
    the chunk's ticket) per chunk; rows[b]: the rows of block b, ascending."""

    def __init__(self, n, blocks, waves, U, ranges=None):
        self.n, self.blocks, self.waves, self.ranges = n, blocks, waves, ranges
        if ranges is not None:
            table = chunk_table(ranges)
            self.U = FILTER_CHUNK
            self.row0 = np.array([t[0] for t in table], dtype=np.int64)
            self.cnt = np.array([t[1] for t in table], dtype=np.int64)
        else:
            self.U = U
            self.row0 = np.arange(0, n, U, dtype=np.int64)
            self.cnt = np.minimum(n - self.row0, U)
        c = np.arange(len(self.row0), dtype=np.int64)
        self.block = (c // waves) % blocks
        self.lane = c % waves
        self.rows = [self._rows(self.block == b) for b in range(blocks)]
        self.scanned = self._rows(np.ones(len(c), dtype=bool))

    def _rows(self, pick):
        parts = [np.arange(r, r + k, dtype=np.int64) for r, k in zip(self.row0[pick], self.cnt[pick])]
        return np.sort(np.concatenate(parts)) if parts else np.zeros(0, dtype=np.int64)


def block_rows(n, blocks, waves, U, ranges=None):
    """The rows of each block (chunk c belongs to block (c // waves) % blocks; filtered chunks follow the chunk table)."""
    return Deal(n, blocks, waves, U, ranges).rows


def deals_of(n, blocks, threads, U, nq, ranges=None):
    """One Deal per query of a call: the pass the query rides in decides the rows per chunk."""
    made, out = {}, []
    for _, active, slots in passes(nq):
        ku = FILTER_CHUNK if ranges is not None else kernel_unroll(U, slots)
        if ku not in made:
            made[ku] = Deal(n, blocks, threads // 64, ku, ranges)
        out += [made[ku]] * active
    return out


# ---------------------------------------------------------------------------------------------------------------- keys
def make_keys(d32, rows):
    return (np.ascontiguousarray(d32, dtype=np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(rows).astype(np.uint64)


def key_rows(keys):
    return (np.asarray(keys, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)


def key_dist(keys):
    return (np.asarray(keys, dtype=np.uint64) >> np.uint64(32)).astype(np.uint32).view(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the judge
class Report:
    def __init__(self):
        self.max_err, self.worst, self.unclear, self.lists = 0.0, None, 0, 0

    def ok_cap(self):
        return self.unclear <= UNCLEAR_CAP * self.lists


def _border(ds, m, err):
    """R_b sorted by (d64, row), ds its distances: is the border behind place m clear (gap > 2 err, or nothing behind it)."""
    return len(ds) <= m or ds[m] - ds[m - 1] > 2 * err


def unclear_lists(d64, deals, kp, err=F32_ERR_SCAN):
    """(lists with an unclear border, lists) of a case, from the reference alone: the condition a builder asserts on its inputs."""
    unclear = total = 0
    for q, deal in enumerate(deals):
        for rows in deal.rows:
            total += 1
            if len(rows) > kp:
                ds = np.sort(d64[rows, q])
                unclear += 0 if _border(ds, kp, err) else 1
    return unclear, total


def check_lists(keys, d64, deals, kp, err=F32_ERR_SCAN, steal=False, where=""):
    """keys uint64 [nq + 1][blocks][kp] as smt_debug_scan_lists returns them, d64 [rows][nq] the exact distances, deals one Deal per
    query.  Raises AssertionError at the first list that is not what the scan stage promises; returns a Report (the largest
    |d32 - d64| seen, the lists whose border was unclear)."""
    keys = np.asarray(keys, dtype=np.uint64)
    nq = len(deals)
    rep = Report()
    assert keys.ndim == 3 and keys.shape[0] == nq + 1 and keys.shape[2] == kp, (where, keys.shape, nq, kp)
    assert (keys[nq] == POISON).all(), (where, "the guard set was written", np.argwhere(keys[nq] != POISON)[:5].tolist())
    body = keys[:nq]
    bad = ((body >> np.uint64(32)) == np.uint64(POISON32)) | ((body & np.uint64(0xFFFFFFFF)) == np.uint64(POISON32))
    assert not bad.any(), (where, "a slot was never written (query, block, slot)", np.argwhere(bad)[:5].tolist())
    for q, deal in enumerate(deals):
        K = keys[q]
        assert K.shape[0] == deal.blocks, (where, K.shape, deal.blocks)
        valid = K != PAD
        count = valid.sum(axis=1)
        assert (valid == (np.arange(kp)[None, :] < count[:, None])).all(), (where, q, "padding inside a list")
        rows, d32 = key_rows(K), key_dist(K).astype(np.float64)
        assert (rows[valid] < deal.n).all(), (where, q, "a key names a row outside the corpus", rows[valid].max())
        asc = (K[:, 1:] > K[:, :-1]) | ~valid[:, 1:]
        assert asc.all(), (where, q, "keys not strictly ascending (block, slot)", np.argwhere(~asc)[:5].tolist())
        flat = rows[valid]
        assert len(np.unique(flat)) == len(flat), (where, q, "a row is named twice")
        dx = d64[rows.clip(0, deal.n - 1), q]
        e = np.where(valid, np.abs(d32 - dx), 0.0)
        if e.max() > rep.max_err:
            b, i = np.unravel_index(np.argmax(e), e.shape)
            rep.max_err, rep.worst = float(e.max()), (q, int(b), int(rows[b, i]))
        assert e.max() <= err, (where, q, "|d32 - d64| beyond the band", float(e.max()), rep.worst)
        run = np.maximum.accumulate(np.where(valid, dx, -np.inf), axis=1)
        order = (run[:, :-1] <= dx[:, 1:] + 2 * err) | ~valid[:, 1:]
        assert order.all(), (where, q, "f64 order broken by more than 2 err (block, slot)", np.argwhere(~order)[:5].tolist())
        if steal:
            _check_union(rows[valid], d64[:, q], deal, kp, err, rep, (where, q))
            continue
        owner = np.full(deal.n, -1, dtype=np.int64)
        for b, rb in enumerate(deal.rows):
            owner[rb] = b
        own = np.where(valid, owner[rows.clip(0, deal.n - 1)], np.arange(deal.blocks)[:, None])
        assert (own == np.arange(deal.blocks)[:, None]).all(), (where, q, "a row of another block, or of none (block, slot)",
                                                                 np.argwhere(own != np.arange(deal.blocks)[:, None])[:5].tolist())
        sizes = np.array([len(rb) for rb in deal.rows])
        want = np.minimum(sizes, kp)
        assert (count == want).all(), (where, q, "keys per list (block, got, expected)",
                                       [(int(b), int(count[b]), int(want[b])) for b in np.flatnonzero(count != want)[:5]])
        rep.lists += deal.blocks
        # (a list of min(k', |R_b|) distinct rows of R_b IS R_b when the block owns no more than k' rows)
        for b in np.flatnonzero(sizes > kp):
            rb = deal.rows[b]
            o = np.lexsort((rb, d64[rb, q]))
            ds, got = d64[rb[o], q], set(rows[b].tolist())
            if _border(ds, kp, err):
                assert got == set(rb[o][:kp].tolist()), (where, q, int(b), "not the f64 top-k' of the block's rows",
                                                         sorted(got ^ set(rb[o][:kp].tolist()))[:8])
            else:
                rep.unclear += 1
                must = set(rb[o][ds <= ds[kp - 1] - 2 * err].tolist())
                never = set(rb[o][ds >= ds[kp - 1] + 2 * err].tolist())
                assert must <= got and not (never & got), (where, q, int(b), "outside the border's band", sorted(must - got)[:5],
                                                           sorted(never & got)[:5])
    return rep


def _check_union(rows, dq, deal, kp, err, rep, where):
    """STEAL: which block scans a row is decided at run time; the union of the lists must still hold the f64 top-k' of the corpus."""
    rep.lists += 1
    o = np.lexsort((deal.scanned, dq[deal.scanned]))
    s, ds = deal.scanned[o], dq[deal.scanned][o]
    m = min(kp, len(s))
    assert set(rows.tolist()) <= set(s.tolist()), (where, "a row that was not scanned")
    assert len(rows) >= m, (where, "fewer keys than k' in all lists together", len(rows))
    got = set(rows.tolist())
    if _border(ds, m, err):
        assert set(s[:m].tolist()) <= got, (where, "the f64 top-k' is not in the union", sorted(set(s[:m].tolist()) - got)[:8])
    else:
        rep.unclear += 1
        assert set(s[ds <= ds[m - 1] - 2 * err].tolist()) <= got, (where, "a row in front of the border's band is missing")


def merged_topk(keys, d64, q, k):
    """What the select makes of the lists of query q: their rows re-scored exactly, the k best by (d64, row)."""
    K = np.asarray(keys, dtype=np.uint64)[q].reshape(-1)
    rows = np.unique(key_rows(K[K != PAD]))
    o = np.lexsort((rows, d64[rows, q]))[:k]
    return rows[o], d64[rows[o], q]


# ---------------------------------------------------------------------------------------------------------------- model scans
WRONG_SCANS = ("ragged-dropped", "clamped-reread", "next-block", "ties-rejected", "kp-minus-1", "pad-wrong-slot", "wave0-only",
               "off-1e-4", "guard-touched")


def model_scan(d64, deals, kp, wrong=None):
    """A scan as lists: per (query, block) the k' best keys of the block's rows with d32 = float32(d64), [nq + 1][blocks][kp] with the
    guard set untouched -- or, with `wrong`, one of the subtly wrong scans of WRONG_SCANS:
      ragged-dropped   a chunk with fewer than U valid rows is skipped
      clamped-reread   the clamped re-reads of a ragged chunk (the last row; filtered: the chunk's first) count as rows
      next-block       list b holds the rows of block b + 1
      ties-rejected    a candidate whose distance equals one already in the list is rejected instead of ranked by row
      kp-minus-1       the list keeps k' - 1 keys
      pad-wrong-slot   the padding starts one slot late
      wave0-only       only the chunks of wave 0's tickets reach the list
      off-1e-4         one distance is off by 1e-4
      guard-touched    slot 3 of a three-query pass writes its (query 0's) list"""
    assert wrong is None or wrong in WRONG_SCANS, wrong
    nq, blocks = len(deals), deals[0].blocks
    out = np.full((nq + 1, blocks, kp), POISON, dtype=np.uint64)
    for q, deal in enumerate(deals):
        for b in range(blocks):
            pick = deal.block == ((b + 1) % blocks if wrong == "next-block" else b)
            if wrong == "ragged-dropped":
                pick &= deal.cnt == deal.U
            if wrong == "wave0-only":
                pick &= deal.lane == 0
            rows = deal._rows(pick)
            if wrong == "clamped-reread":
                rag = pick & (deal.cnt < deal.U)
                clamp = [np.full(deal.U - k, r if deal.ranges is not None else deal.n - 1, dtype=np.int64)
                         for r, k in zip(deal.row0[rag], deal.cnt[rag])]
                rows = np.concatenate([rows] + clamp)
            d32 = d64[rows, q].astype(np.float32)
            if wrong == "off-1e-4" and b == 0 and q == 0 and len(rows):
                d32[np.argmin(d32)] += np.float32(1e-4)
            o = np.lexsort((rows, d32))
            rows, d32 = rows[o], d32[o]
            if wrong == "ties-rejected" and len(rows):
                first = np.concatenate([[True], d32[1:] != d32[:-1]])
                rows, d32 = rows[first], d32[first]
            keep = kp - 1 if wrong == "kp-minus-1" else kp
            rows, d32 = rows[:keep], d32[:keep]
            out[q, b, :len(rows)] = make_keys(d32, rows)
            out[q, b, len(rows) + (1 if wrong == "pad-wrong-slot" else 0):] = PAD
    if wrong == "guard-touched":
        for q0, active, slots in passes(nq):
            if active == 3:
                out[q0 + 3] = out[q0]
    return out


# ---------------------------------------------------------------------------------------------------------------- tie cases
ONE_BITS = np.uint64(0x3F800000)        # dist_f32 returns exactly 1.0f for a zero row, and for every non-zero row under a zero query


def zero_query_lists(deal, kp):
    """Tie case (a): under the zero query every non-zero row is at exactly 1.0, so every list is the lowest rows of its block."""
    out = np.full((deal.blocks, kp), PAD, dtype=np.uint64)
    for b, rb in enumerate(deal.rows):
        m = min(kp, len(rb))
        out[b, :m] = (ONE_BITS << np.uint64(32)) | rb[:m].astype(np.uint64)
    return out


def planted_tie_corpus(deal, kp, seed):
    """Tie case (b): per block k' - 3 planted near rows of one query (distinct distances 0.1 .. 0.6), zero rows at every seventh of
    the block's other rows (at least four), every remaining row anti-correlated with the query (d64 > 1.05).  Every list is the near
    rows and then the three LOWEST zero rows of the block, at exactly 1.0.  Returns (rows f32, query f32, near[b], zeros[b])."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal(DIM)
    q /= np.linalg.norm(q)
    emb = np.zeros((deal.n, DIM), dtype=np.float64)
    near, zeros = [], []

    def around(cos, m):
        u = rng.standard_normal((m, DIM))
        u -= (u @ q)[:, None] * q[None, :]
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        return cos[:, None] * q[None, :] + np.sqrt(1.0 - cos ** 2)[:, None] * u

    filler = np.setdiff1d(np.arange(deal.n), deal.scanned)
    emb[filler] = around(np.full(len(filler), -0.2), len(filler))
    for rb in deal.rows:
        assert len(rb) >= kp + 8, (len(rb), kp)
        pick = rng.permutation(len(rb))
        nb = np.sort(rb[pick[:kp - 3]])
        rest = np.sort(rb[pick[kp - 3:]])
        zb = rest[::7] if len(rest[::7]) >= 4 else rest[:4]
        anti = np.setdiff1d(rest, zb)
        emb[nb] = around(1.0 - rng.permutation(np.linspace(0.1, 0.6, kp - 3)), kp - 3)
        emb[anti] = around(-rng.uniform(0.1, 0.3, len(anti)), len(anti))
        near.append(nb)
        zeros.append(zb)
    return np.ascontiguousarray(emb, dtype=np.float32), np.ascontiguousarray(q, dtype=np.float32), near, zeros


def planted_tie_rows(near, zeros):
    """The rows every list of tie case (b) must hold, as sets per block, and the three zero rows that close it."""
    return [set(nb.tolist()) | set(zb[:3].tolist()) for nb, zb in zip(near, zeros)], [zb[:3] for zb in zeros]


# ---------------------------------------------------------------------------------------------------------------- cases
class Cap:
    """The cap on unclear borders over the calls of one test case: at most UNCLEAR_CAP of its (block, query) lists.  Counted from the
    reference alone (unclear_lists), so it is a condition on the inputs: a case that misses it needs another seed."""

    def __init__(self):
        self.unclear = self.total = 0

    def add(self, unclear, total):
        self.unclear += unclear
        self.total += total

    def check(self, name=""):
        assert self.unclear <= UNCLEAR_CAP * self.total, (name, "too many unclear borders: pick another seed", self.unclear, self.total)


class Case:
    """One call at one launch shape: rows, qs, d64 [rows][nq], the plan (blocks, threads, U, kp, ranges, steal) and the deals."""


def make_case(name, rows, qs, top_k, scan_blocks, threads, U, num_cus=256, ranges=None, guard_band=8, scan_steal=0, d64=None, ties=False, cap=None):
    """Plans the call as plan_scan does and asserts the cap on unclear borders -- a condition on the inputs, met by the reference
    alone, at once or (cap: a Cap) summed over the calls of a test case.  ties: a tie case, whose borders are unclear on purpose (rows at exactly 1.0) and whose keys the test pins one by one."""
    c = Case()
    c.name, c.rows, c.qs = name, rows, np.ascontiguousarray(qs, dtype=np.float32).reshape(-1, DIM)
    c.n, c.nq, c.top_k, c.threads, c.U, c.ranges = len(rows), len(c.qs), top_k, threads, U, ranges
    c.kp = kprime(top_k, guard_band)
    c.blocks = planned_blocks(c.n, scan_blocks, threads, U, num_cus, ranges)
    c.steal = steal_on(c.n, c.blocks, threads, U, scan_steal, ranges)
    c.d64 = exact_distances(rows, c.qs) if d64 is None else d64
    c.deals = deals_of(c.n, c.blocks, threads, U, c.nq, ranges)
    c.ties = ties
    if not c.steal and not ties:
        tally = Cap() if cap is None else cap
        tally.add(*unclear_lists(c.d64, c.deals, c.kp))
        if cap is None:
            tally.check(name)
    return c
