"""CPU: the NumPy threshold reference the GPU threshold tests compare against (tests/threshold_ref.py) is right, its cases reach the
branches they were written for, and they discriminate.

  * threshold_ref.answer == the C oracle's accurate threshold search (orc.search_documents(accurate=True)), rows and f64 bits, for
    every query, max_distance and range list of every case; the vectorised distances == oracle_np.cosine_accurate / cosine_serial;
  * the one-wave model reports the flush sizes each flush case claims (253, 254, 255 and 256 in front of chunks of 4, 3, 2, 1 and
    4 hits; the fit 255 + 1 = 256 without a flush), for the unfiltered corpus and for its ranged twin, and with thr_hit_cap = 512
    it puts the capacity inside a flush and counts 1, 1, 2, 2 launches;
  * what the builders promise about their inputs: hit counts, the empty band, the straddling cluster, the ties;
  * six subtly wrong threshold searches, threshold_ref.WRONG, each differ from the reference on a named case -- so a kernel or a
    host path with that mistake would fail tests/test_gpu_threshold.py."""
import numpy as np
import pytest

from oracle import oracle as orc
from oracle import oracle_np
from tests import threshold_ref as T


def _same(got, want):
    return np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes()


def _oracle(emb, q, md, ranges, top_k):
    rows = T.eligible(len(emb), ranges)
    sub = np.ascontiguousarray(emb[rows])
    res = orc.search_documents(sub, [len(sub)], q, n_lines=0, top_k=top_k or 3, max_distance=None if np.isinf(md) else md, accurate=True)
    return rows[[r["match_line"] for r in res]].astype(np.uint64), np.array([r["distance"] for r in res], dtype=np.float64)


@pytest.mark.parametrize("name", T.NAMES)
def test_reference_equals_the_accurate_oracle(name):
    c = T.case(name)
    for qi, md, ranges in c.runs():
        assert _same(c.answer(qi, md, ranges, c.top_k), _oracle(c.emb, c.qs[qi], md, ranges, c.top_k)), (name, qi, md, ranges is not None)


def test_vectorised_distances_equal_the_numpy_oracle_row_by_row():
    c = T.case("strict")
    rows = np.concatenate([c.cluster[:40], np.arange(25)])
    for q in c.qs[:2]:
        assert T.distances(c.emb[rows], q).tolist() == [oracle_np.cosine_accurate(q, c.emb[r]) for r in rows]
        assert T.distances_serial(c.emb[rows], q).tolist() == [oracle_np.cosine_serial(q, c.emb[r]) for r in rows]
    b = T.case("border-2047")
    rows = np.concatenate([b.zero_rows, np.nonzero(b.masks[0])[0][:30]])
    assert T.distances(b.emb[rows], b.qs[0]).tolist() == [oracle_np.cosine_accurate(b.qs[0], b.emb[r]) for r in rows]
    zero_q = np.zeros(T.DIM, dtype=np.float32)
    assert T.distances(b.emb[rows], zero_q).tolist() == [oracle_np.cosine_accurate(zero_q, b.emb[r]) for r in rows]


# ------------------------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("name", T.FLUSH_NAMES)
def test_model_reports_the_flush_sizes_the_case_claims(name):
    c = T.case(name)
    got = T.collect_one_wave(c.passes(), c.ranges)
    assert got.sizes == c.flush_sizes, (name, got.sizes)
    inside = T.eligible(c.n, c.ranges)
    assert got.count == int(c.masks[0][inside].sum()) == len(c.answer(0, None, c.ranges)[0])
    assert sorted(got.rows) == sorted(c.answer(0, None, c.ranges)[0].tolist())
    if c.ranges is not None:        # the rows between the ranges would be hits: the unfiltered search of the twin finds more
        assert len(c.answer(0)[0]) > got.count and c.ranges[-1][1] == c.n


def test_model_covers_every_residue_and_the_exact_fit():
    triggers = {}
    for name in T.FLUSH_NAMES:
        c = T.case(name)
        passes = c.passes()
        counts = [int(passes[r:r + v].sum()) for r, v in T.chunks_of(c.n, c.ranges)]
        pending = 0
        for cnt in (x for x in counts if x):
            if pending + cnt > T.HIT_BUF:
                triggers.setdefault((pending, cnt), set()).add(name)
                pending = 0
            pending += cnt
    for pair in ((253, 4), (254, 3), (255, 2), (256, 1), (256, 4)):
        assert len(triggers.get(pair, ())) >= 4, (pair, triggers.get(pair))      # its own case and flush-mixed, with and without ranges
    assert all(pending + cnt > T.HIT_BUF for pending, cnt in triggers)
    fit = T.collect_one_wave(T.case("fit-255+1").passes())
    assert (255, 1) in fit.fits and fit.sizes == [256] and fit.flushes == [(0, 256)]
    total = T.collect_one_wave(T.case("total-512").passes())
    assert total.count == 512 and total.sizes == [256, 256]                       # (the last flush is a full buffer, not an empty one)
    none = T.collect_one_wave(T.case("none").passes())
    assert none.count == 0 and none.sizes == [] and none.rows == []
    mixed = T.case("flush-mixed")
    assert mixed.masks[0][-3:].tolist() == [True, True, False]                    # hits in the short last chunk


@pytest.mark.parametrize("total,want", [(511, 1), (512, 1), (513, 2), (1500, 2), (2500, 2)])
def test_model_puts_the_capacity_inside_a_flush(total, want):
    c = T.case("rerun-%d" % total)
    for ranges in c.range_options():
        passes = c.passes()
        first = T.collect_one_wave(passes, ranges, cap=512)
        assert first.count == total == len(c.answer(0, None, ranges)[0])
        assert T.launches(passes, ranges, cap=512) == want and T.launches(passes, ranges) == 1
        assert first.flushes[:3] == [(0, 253), (253, 253), (506, min(253, total - 506))]
        if want == 2:               # the third flush holds slot 512: its first six entries are stored, the rest only counted
            assert first.flushes[2][0] < 512 < sum(first.flushes[2]) and len(first.rows) == 512
            assert sorted(T.collect_one_wave(passes, ranges, cap=total).rows) == sorted(c.answer(0, None, ranges)[0].tolist())
        else:
            assert len(first.rows) == total


# ------------------------------------------------------------------------------------------------------------- the builders' promises
def test_ranges_cases_hold_every_length_adjacent_and_apart():
    for name in ("ranges-hits-inside", "ranges-hits-outside"):
        c = T.case(name)
        lengths = [e - b for b, e in c.ranges]
        assert set(lengths) == set(T.RANGE_LENGTHS) and c.ranges[-1][1] == c.n
        touching = [x[1] == y[0] for x, y in zip(c.ranges, c.ranges[1:])]
        assert sum(touching) >= 13 and sum(not t for t in touching) >= 21
        assert {e - b for (b, e), t in zip(c.ranges[1:], touching) if t} == set(T.RANGE_LENGTHS)
        inside = np.zeros(c.n, dtype=bool)
        inside[T.eligible(c.n, c.ranges)] = True
        hit = c.masks[0]
        if name == "ranges-hits-inside":
            assert (hit == inside).all()                                          # misses directly outside every range
        else:
            for b, e in c.ranges:
                assert hit[e - 1] and (e - b == 1 or not hit[b:e - 1].any())      # the hit sits in the range's last chunk, the short one
                assert (hit | inside)[max(0, b - 4):min(c.n, e + 4)].all()        # hits directly outside, which the call must not return
        assert len(c.answer(0, None, c.ranges)[0]) == int((hit & inside).sum()) > 0


@pytest.mark.parametrize("collected", T.BORDER_COUNTS)
def test_border_cases_collect_exactly_the_count_they_are_named_after(collected):
    c = T.case("border-%d" % collected)
    q, (at_one, above_one) = c.qs[0], c.mds
    assert at_one == 1.0 and above_one == np.nextafter(1.0, 2.0)
    assert int(c.passes(0, at_one).sum()) == int(c.passes(0, above_one).sum()) == collected    # zero rows: f32 distance exactly 1
    rows1, d1 = c.answer(0, at_one)
    rows2, d2 = c.answer(0, above_one)
    assert len(rows1) == collected - T.N_ZERO and len(rows2) == collected
    assert sorted(rows2[-T.N_ZERO:].tolist()) == sorted(c.zero_rows.tolist()) and (d2[-T.N_ZERO:] == 1.0).all()
    assert (d2[:T.N_SAME] < 1e-15).all() and len(set(d2[:T.N_SAME].tolist())) == 1            # the rows identical to the query
    values, counts = np.unique(d2, return_counts=True)
    dup = np.nonzero(d2 == values[counts.argmax()])[0]
    assert len(dup) == T.N_DUP and (np.diff(rows2[dup].astype(np.int64)) > 0).all()
    if collected == 4100:
        assert dup[0] < T.HOST_ORDER_MAX < dup[-1]                                            # the ties straddle position 2048
    assert len({c.emb[int(r)].tobytes() for r in rows2[dup]}) > 1                              # equal distances from other bits


@pytest.mark.parametrize("name", ["strict", "strict-padded"])
def test_strict_cases_straddle_and_stay_inside_the_guard(name):
    c = T.case(name)
    q, (md, up, down) = c.qs[0], c.mds
    exact = T.distances(c.emb[c.cluster], q)
    serial = np.array([oracle_np.cosine_serial(q, c.emb[r]) for r in c.cluster])
    assert int(((serial < md) != (exact < md)).sum()) == c.straddle >= 5
    assert np.abs(exact - md).max() <= 8e-6
    assert exact[c.cluster.tolist().index(c.star)] == md and (T.distances(c.emb[c.copies], q) == md).all()
    assert len({r // T.CHUNK for r in c.copies + [c.star]}) == 4
    assert up > md > down and np.nextafter(down, 2.0) == md
    base = len(c.answer(0, md)[0])
    assert len(c.answer(0, up)[0]) == base + 4                                    # the member and its three copies
    assert base - len(c.answer(0, down)[0]) == int((exact == down).sum())
    for ranges in c.range_options():    # what the scan collects (the whole cluster: it lies inside the prefilter's guard) picks the ordering
        collected = int(c.passes(0, md)[T.eligible(c.n, ranges)].sum())
        assert (collected > T.HOST_ORDER_MAX) == (name == "strict-padded") and collected > len(c.answer(0, md, ranges)[0]) + 250
    assert _same(c.answer(2, md), c.answer(0, md))                                # twice the query: the same f64 distances
    assert len(c.answer(1, md)[0]) == len(c.answer(3, md)[0]) == 20


def test_sweep_case_counts_and_reanswer_case_order():
    c = T.case("sweep-capacity")
    assert tuple(len(c.answer(qi)[0]) for qi in range(6)) == T.SWEEP_COUNTS == (0, 1, 2047, 2048, 2049, 3000)
    assert sum(n > T.CAND_CAP for n in T.SWEEP_COUNTS) == 2
    r = T.case("reanswer")
    for ranges in r.range_options():
        rows, dist = r.answer(0, r.mds[0], ranges, 10)
        tied = r.tied[np.isin(r.tied, T.eligible(r.n, ranges))]
        assert ranges is None or tied[0] == r.tied[7]                             # the ranges leave the first seven copies out
        d = T.distances(r.emb, r.qs[0])
        assert rows[:5].tolist() == sorted(r.near.tolist(), key=lambda x: d[x]) and rows[5:].tolist() == tied[:5].tolist()
        assert len(set(dist[5:].tolist())) == 1
        collected = T.answer(r.emb, r.qs[0], np.nextafter(dist[-1], 2.0), ranges)[0]
        assert len(collected) == 5 + len(tied) > T.HOST_ORDER_MAX                 # what the re-answer's K4 scan has to order


# ------------------------------------------------------------------------------------------------------------------ wrong variants
MEANT = {       # the cases written for each mistake
    "drops-the-chunk-that-triggers-a-flush": ["flush-253+4", "flush-254+3", "flush-255+2", "flush-256+1", "flush-256+4", "flush-mixed",
                                              "flush-253+4-ranges", "flush-mixed-ranges", "rerun-1500"],
    "flush-keeps-256-minus-cnt": ["flush-253+4", "flush-254+3", "flush-255+2", "flush-256+1", "flush-256+4", "flush-mixed",
                                  "flush-256+1-ranges", "flush-mixed-ranges", "total-512"],
    "short-chunk-read-whole": ["ranges-hits-outside"],
    "cut-with-<=": ["strict", "strict-padded", "border-2047", "border-2048", "border-2049", "border-4100"],
    "cut-at-the-f32-prefilter": ["strict", "strict-padded"],
    "second-sort-not-stable": ["border-2049", "border-4100", "strict-padded", "reanswer"],
}


def _caught(kind, name):
    c = T.case(name)
    out = []
    for qi, md, ranges in c.runs():
        if c.top_k is not None:     # the re-answer: K4 runs one f64 step above the k-th distance
            md = float(np.nextafter(c.answer(qi, md, ranges, c.top_k)[1][-1], 2.0))
        if not _same(T.wrong_answer(kind, c.emb, c.qs[qi], md, ranges, c.top_k), c.answer(qi, md, ranges, c.top_k)):
            out.append((qi, md, ranges is not None))
    return out


@pytest.mark.parametrize("kind", sorted(T.WRONG))
def test_the_cases_catch_a_subtly_wrong_threshold_search(kind):
    assert set(MEANT) == set(T.WRONG)
    for name in MEANT[kind]:
        assert _caught(kind, name), "%s (%s) is not caught by case %s" % (kind, T.WRONG[kind], name)


def test_the_right_search_is_not_caught():
    for name in T.NAMES:
        assert not _caught(None, name), name
