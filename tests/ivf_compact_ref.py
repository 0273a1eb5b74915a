"""smt_ivfpq_compact's contract in NumPy, over the dict tests/ivf_ref.read_index returns.  TEST INFRASTRUCTURE.

The keep list (sorted, disjoint row ranges) maps old row keep[i].begin + j to row prefix[i] + j.  Carrying an index through the
compaction keeps the entries whose row is kept, in their old order, renames their rows through that map and counts, per list, the
kept entries in front of it; nothing else of the index changes."""
import numpy as np


def prefix_map(keep):
    """(begins, ends, prefix) of the non-empty ranges: old row begins[i] + j -> prefix[i] + j."""
    kr = [(int(b), int(e)) for b, e in keep if e > b]
    begins = np.array([b for b, _ in kr], dtype=np.int64)
    ends = np.array([e for _, e in kr], dtype=np.int64)
    prefix = np.concatenate([[0], np.cumsum(ends - begins)])[:-1].astype(np.int64)
    return begins, ends, prefix


def remap(rows, keep):
    """(alive, new): alive[i] = rows[i] lies in a kept range; new[i] = its row after the compaction (only where alive)."""
    rows = np.asarray(rows, dtype=np.int64)
    begins, ends, prefix = prefix_map(keep)
    if len(begins) == 0:
        return np.zeros(len(rows), dtype=bool), np.zeros(len(rows), dtype=np.int64)
    j = np.maximum(np.searchsorted(begins, rows, side="right") - 1, 0)
    alive = (rows >= begins[j]) & (rows < ends[j])
    return alive, prefix[j] + rows - begins[j]


def carry(ix, keep):
    """The index after smt_ivfpq_compact(index, keep): a new dict; the arrays that do not change are the same objects."""
    alive, new = remap(ix["ids"], keep)
    out = dict(ix)
    out["ids"] = new[alive].astype("<u4")
    out["codes"] = np.ascontiguousarray(ix["codes"][alive])
    kept_before = np.concatenate([[0], np.cumsum(alive)])            # kept entries in front of every list position
    out["offsets"] = kept_before[ix["offsets"].astype(np.int64)].astype("<u8")
    out["n_rows"] = int(alive.sum())
    return out


def same_index(a, b):
    """Every field of two parsed indexes, byte for byte; returns the names that differ."""
    bad = [k for k in a if isinstance(a[k], np.ndarray) and (k not in b or a[k].dtype != b[k].dtype or a[k].shape != b[k].shape
                                                             or a[k].tobytes() != b[k].tobytes())]
    bad += [k for k in a if not isinstance(a[k], np.ndarray) and a[k] != b.get(k)]
    return bad + [k for k in b if k not in a]
