"""CPU: the NumPy merge the GPU merge tests compare against (tests/merge_ref.py) is right, the host merge agrees with it, and its
cases discriminate.

  * merge_ref.merge_lists == a brute-force rank count (the output slot of an entry is the number of entries before it) on every
    case of up to 512 candidates;
  * smt.merge_topk (smt_merge_topk, host code) == merge_ref.merge_lists on every case, bit for bit, counts included;
  * three subtly wrong merges, written below, each differ from the reference on at least one case -- so a kernel that broke ties
    by list, compared rows by their low word or compared distances in f32 would fail tests/test_gpu_merge.py."""
import numpy as np
import pytest

import semtools_amd as smt
from tests import merge_ref as mr

NAMES = mr.case_names()


def _same(got_rows, got_dist, want_rows, want_dist):
    return np.array_equal(got_rows, want_rows) and np.array_equal(np.ascontiguousarray(got_dist).view(np.uint64),
                                                                  np.ascontiguousarray(want_dist).view(np.uint64))


def _brute(rows, dist, k_out):
    n_lists, nq, k_in = rows.shape
    out_r = np.full((nq, k_out), mr.PAD, dtype=np.uint64)
    out_d = np.full((nq, k_out), np.inf)
    counts = np.zeros(nq, dtype=np.uint64)
    for q in range(nq):
        r, d = rows[:, q, :].reshape(-1), dist[:, q, :].reshape(-1)
        live = r != mr.PAD
        before = (d[None, :] < d[:, None]) | ((d[None, :] == d[:, None]) & (r[None, :] < r[:, None]))
        rank = (before & live[None, :]).sum(axis=1)
        for e in np.nonzero(live & (rank < k_out))[0]:
            assert out_r[q, rank[e]] == mr.PAD, "two entries of one rank: the case's rows are not distinct"
            out_r[q, rank[e]], out_d[q, rank[e]] = r[e], d[e]
        counts[q] = min(int(live.sum()), k_out)
    return out_r, out_d, counts


def test_the_cases_cover_every_shape_and_keep_the_preconditions():
    assert len(NAMES) == len(set(NAMES)) and [n for n, *_ in mr.cases()] == NAMES
    shapes = set()
    for name, rows, dist, k_out in mr.cases():
        n_lists, nq, k_in = rows.shape
        shapes.add((n_lists, k_in, k_out, nq))
        assert rows.dtype == np.uint64 and dist.dtype == np.float64 and dist.shape == rows.shape and n_lists * k_in <= 8192
        live = rows != mr.PAD
        assert not np.isnan(dist).any() and np.isfinite(dist[live]).all() and not np.signbit(dist[live]).any()
        for q in range(nq):
            r = rows[:, q, :][live[:, q, :]]
            assert len(np.unique(r)) == len(r), (name, q)                      # distinct rows within a query
            for l in range(n_lists):
                n = int(live[l, q].sum())
                assert live[l, q, :n].all(), (name, q, l)                      # padding at the tail only
                assert (np.lexsort((rows[l, q, :n], dist[l, q, :n])) == np.arange(n)).all(), (name, q, l)   # (distance, row) order
        if nq > 1:   # every query of a case has its own content
            assert len({(rows[:, q].tobytes(), dist[:, q].tobytes()) for q in range(nq)}) == nq, name
    assert shapes == set(mr.SHAPES)
    for content, _, _, _ in mr.CONTENTS:
        assert sum(n.startswith(content + "-") for n in NAMES) >= 14, content


def test_what_the_contents_promise():
    for name, rows, dist, k_out in mr.cases():
        n_lists, nq, k_in = rows.shape
        content = name.split("-")[0]
        live = rows != mr.PAD
        ref_r, ref_d, cnt = mr.merge_lists(rows, dist, k_out)
        if content == "ties":
            for q in range(nq):
                assert len(np.unique(dist[:, q])) <= 4 and (dist[:, q] == 0.0).any(), name
                if n_lists > 1:     # higher-numbered lists hold the lower rows
                    assert all(rows[l, q].min() > rows[l + 1, q].max() for l in range(n_lists - 1)), name
                if 1 <= k_out < n_lists * k_in:   # a tie group straddles position k_out
                    full = mr.merge_lists(rows[:, q:q + 1], dist[:, q:q + 1], k_out + 1)[1][0]
                    assert full[k_out - 1] == full[k_out], name
            r = rows[live]
            if len(r) >= 9:
                lo, hi = r & np.uint64(0xFFFFFFFF), r >> np.uint64(32)
                assert len(np.unique(lo)) < len(r) and len(np.unique(hi)) < len(r) and hi.max() > 0, name
        if content == "ragged":
            n_live = live.sum(axis=2)
            for q in range(nq - 1 if nq >= 2 else nq):
                assert (n_live[:, q] == 0).any() and (n_live[:, q] == 1).any(), name
            if nq >= 2:
                assert n_live[:, -1].sum() == 0 and cnt[-1] == 0 and (ref_r[-1] == mr.PAD).all() and np.isinf(ref_d[-1]).all(), name
            assert (dist[~live] == 0.0).any()     # a distance that would win beside a padding row
        if content == "last_list_wins":
            for q in range(nq):
                n = min(k_out, k_in)
                assert set(ref_r[q, :n].tolist()) <= set(rows[-1, q].tolist()), name
        if content == "neighbours":
            for q in range(nq):
                d = np.sort(dist[:, q].reshape(-1))
                assert d[1] == np.nextafter(d[0], np.inf) and len(np.unique(d.astype(np.float32))) == 1 and len(np.unique(d)) == len(d), name


@pytest.mark.parametrize("name", [n for n in NAMES if mr.case(n)[0].shape[0] * mr.case(n)[0].shape[2] <= 512])
def test_reference_equals_a_brute_force_rank_count(name):
    rows, dist, k_out = mr.case(name)
    ref_r, ref_d, ref_c = mr.merge_lists(rows, dist, k_out)
    br_r, br_d, br_c = _brute(rows, dist, k_out)
    assert _same(ref_r, ref_d, br_r, br_d) and np.array_equal(ref_c, br_c)


@pytest.mark.parametrize("name", NAMES)
def test_host_merge_equals_the_reference(name):
    rows, dist, k_out = mr.case(name)
    ref_r, ref_d, ref_c = mr.merge_lists(rows, dist, k_out)
    got_r, got_d, got_c = smt.merge_topk(rows, dist, k_out)
    assert _same(got_r, got_d, ref_r, ref_d), name
    assert np.array_equal(np.asarray(got_c, dtype=np.uint64), ref_c), name


def test_pack_round_trip_and_status_combine():
    rows, dist, _ = mr.case("ragged-3x7_to_7_nq33")
    words = mr.pack(rows, dist)
    assert words.shape == (3, 33, 2, 7) and words.dtype == np.uint64
    assert np.array_equal(words[:, :, 0, :], rows) and np.array_equal(words[:, :, 1, :], dist.view(np.uint64))
    back_r, back_d = mr.unpack(words)
    assert _same(back_r, back_d, rows, dist)
    w = np.array([[0, 1, 0, 3], [2, 0, 0, 1], [0, 0, 0, 2]], dtype=np.uint64)
    out = mr.combine_status(w)
    assert out.dtype == np.uint32 and out.tolist() == [2, 1, 0, 3]
    assert mr.combine_status(np.zeros((0, 4), dtype=np.uint64)).tolist() == [0, 0, 0, 0]


# --------------------------------------------------------------------------------------------------- three subtly wrong merges
def _merge_by(rows, dist, k_out, keys):
    """The reference merge with another order: keys(rows, dist, list index, slot) -> lexsort keys (the last one is the primary)."""
    n_lists, nq, k_in = rows.shape
    out_r = np.full((nq, k_out), mr.PAD, dtype=np.uint64)
    out_d = np.full((nq, k_out), np.inf)
    lst, slot = np.repeat(np.arange(n_lists), k_in), np.tile(np.arange(k_in), n_lists)
    for q in range(nq):
        r, d = rows[:, q, :].reshape(-1), dist[:, q, :].reshape(-1)
        keep = r != mr.PAD
        order = np.lexsort(keys(r[keep], d[keep], lst[keep], slot[keep]))[:k_out]
        out_r[q, :len(order)], out_d[q, :len(order)] = r[keep][order], d[keep][order]
    return out_r, out_d


MUTANTS = {
    "ties broken by list order, not by row": lambda r, d, lst, slot: (slot, lst, d),
    "rows compared as their low 32 bits": lambda r, d, lst, slot: (slot, lst, r & np.uint64(0xFFFFFFFF), d),
    "distances compared after rounding to f32": lambda r, d, lst, slot: (r, d.astype(np.float32)),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_the_cases_catch_a_subtly_wrong_merge(mutant):
    caught = []
    for name, rows, dist, k_out in mr.cases():
        ref_r, ref_d, _ = mr.merge_lists(rows, dist, k_out)
        bad_r, bad_d = _merge_by(rows, dist, k_out, MUTANTS[mutant])
        if not _same(bad_r, bad_d, ref_r, ref_d):
            caught.append(name)
    assert caught, mutant
    # ... and not by one lucky case: the content written for this mistake catches it at every shape where entries can be confused
    meant = {"ties broken by list order, not by row": "ties", "rows compared as their low 32 bits": "ties",
             "distances compared after rounding to f32": "neighbours"}[mutant]
    assert sum(n.startswith(meant + "-") for n in caught) >= 10, (mutant, caught)


def test_the_right_order_is_not_caught():
    for name, rows, dist, k_out in mr.cases():
        ref_r, ref_d, _ = mr.merge_lists(rows, dist, k_out)
        ok_r, ok_d = _merge_by(rows, dist, k_out, lambda r, d, lst, slot: (r, d))
        assert _same(ok_r, ok_d, ref_r, ref_d), name
