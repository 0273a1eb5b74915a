"""IVF index searched inside row ranges: NumPy helpers (no GPU).  TEST INFRASTRUCTURE, beside tests/ivf_ref.py.

A range set is a list of (begin, end) pairs of corpus rows, half-open, sorted and disjoint; empty members (begin == end) are allowed
(include/semtools_hip.h, smt_ivfpq_search_ranges).  `ix` is the dict of ivf_ref.read_index."""
import numpy as np


def in_ranges(rows, ranges):
    """Boolean per row: the row lies in one of the ranges (sorted, disjoint: the last range that begins at or before the row is the
    only one that can hold it)."""
    rows = np.asarray(rows, dtype=np.int64)
    r = np.array([(b, e) for b, e in ranges if e > b], dtype=np.int64).reshape(-1, 2)
    if len(r) == 0:
        return np.zeros(rows.shape, dtype=bool)
    j = np.searchsorted(r[:, 0], rows, side="right") - 1
    return (j >= 0) & (rows < r[np.maximum(j, 0), 1])


def list_order_mask(ix, ranges):
    """The bitmap ivf_range_mask_kernel documents, as uint64 words: bit p % 64 of word p // 64 is set iff ids[p] lies in a range;
    positions at or past n_rows in the last word are 0."""
    bits = in_ranges(ix["ids"], ranges)
    n_words = (len(bits) + 63) // 64
    padded = np.zeros(n_words * 64, dtype=np.uint8)
    padded[:len(bits)] = bits
    return np.packbits(padded.reshape(n_words, 64), axis=1, bitorder="little").view("<u8").reshape(n_words)


# ---------------------------------------------------------------------------------------------- range-set builders
def alternate_blocks(n, block=100):
    """Every second block of `block` rows: [0, block), [2 block, 3 block), ... clipped to n."""
    return [(b, min(b + block, n)) for b in range(0, n, 2 * block)]


def scattered_rows(n, count=40, seed=5):
    """`count` single-row ranges at distinct random rows."""
    rows = np.sort(np.random.default_rng(seed).choice(n, count, replace=False))
    return [(int(r), int(r) + 1) for r in rows]


def with_empty_members(n):
    """Four real ranges with empty ones before, between, touching and after them (begin == end, at 0 and at n too)."""
    q = n // 8
    return [(0, 0), (q, 2 * q), (2 * q, 2 * q), (3 * q, 3 * q), (3 * q, 3 * q + 1), (4 * q, 4 * q), (5 * q, 6 * q), (6 * q, 6 * q),
            (7 * q, n), (n, n)]


def every_second_row(n):
    """n / 2 single-row ranges: more ranges than the mask kernel stages in LDS (1024), so it searches them in global memory."""
    return [(r, r + 1) for r in range(0, n, 2)]


def borders_at(ix, list_id, p0, p1):
    """One range [ids[off + p0], ids[off + p1 - 1] + 1) of list `list_id`: lists are sorted by row, so of THAT list the range holds
    exactly the positions p0 .. p1 - 1 (and whatever rows of other lists lie between the two rows)."""
    off = int(ix["offsets"][list_id])
    ids = ix["ids"]
    assert 0 <= p0 < p1 <= int(ix["offsets"][list_id + 1]) - off
    return [(int(ids[off + p0]), int(ids[off + p1 - 1]) + 1)]
