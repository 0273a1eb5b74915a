"""GPU: the threshold search (K4, csrc/threshold.hip) and the paths that answer through it, on the constructed corpora of
tests/threshold_ref.py (their conditions and the wrong searches they tell apart: tests/test_threshold_ref_cpu.py).

Every case goes through Corpus.search and is compared with the NumPy reference, rows and f64 distances bit for bit.  What a case was
written for is witnessed from the profile counters: "scan" counts the scan launches of a call (a rerun after a hit buffer that was
too small is a second one), "gemm_thr" the batched threshold sweep, "thr_sort" the device ordering of more than 2048 collected hits.
With scan_blocks = 1 and scan_threads = 64 the scan is one wave that takes the chunks in order, and the flush sizes are those the
one-wave model reports on the CPU; with more waves only the answer is checked, since the deal is timing dependent."""
import contextlib

import numpy as np
import pytest

from tests import threshold_ref as T

pytestmark = pytest.mark.gpu

DEFAULTS = dict(scan_blocks=0, scan_threads=512, thr_hit_cap=1 << 20, fallback_batch_min_rows=100_000)
ONE_WAVE = dict(scan_blocks=1, scan_threads=64)
COUNTERS = ("scan", "gemm", "gemm_thr", "thr_sort")


@contextlib.contextmanager
def tuned(ctx, **keys):
    try:
        for key, value in keys.items():
            ctx.set_tuning(key, value)
        yield
    finally:
        for key in keys:
            ctx.set_tuning(key, DEFAULTS[key])


def ran(ctx, fn):
    """(fn(), launches per profile counter)"""
    ctx.set_tuning("prof_every", 1)
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        out = fn()
        return out, {name: ctx.prof_read(name)[0] for name in COUNTERS}
    finally:
        ctx.prof_enable(False)


def same(got, want, note):
    rows, dist = got
    assert len(rows) == len(want[0]), (note, len(rows), len(want[0]))
    assert np.array_equal(np.asarray(rows, dtype=np.uint64), want[0]), (note, np.asarray(rows)[:6].tolist(), want[0][:6].tolist())
    assert np.ascontiguousarray(dist, dtype=np.float64).tobytes() == want[1].tobytes(), note


@pytest.fixture(scope="module")
def corpora(gpu_ctx):
    """One device corpus per case, made on first use and shared by the tests of this module (no test changes one)."""
    import semtools_amd as smt

    made = {}

    def get(name):
        if name not in made:
            made[name] = smt.Corpus(gpu_ctx)
            made[name].append(T.case(name).emb)
        return made[name]

    yield get
    for c in made.values():
        c.close()


def collected(case, qi, md, ranges):
    """rows the scan of this call collects (tests/threshold_ref.py: the prefilter's verdicts follow from the exact distances)"""
    return int(case.passes(qi, md)[T.eligible(case.n, ranges)].sum())


def check_k4(ctx, c, case, qi, md, ranges, note, scans=1):
    """One threshold query through scan_threshold_kernel: the answer, the scan launches, and which ordering ran."""
    got, r = ran(ctx, lambda: c.search(case.qs[qi], top_k=3, max_distance=md, ranges=ranges))
    same(got[0], case.answer(qi, md, ranges), note)
    assert r["scan"] == scans and r["gemm_thr"] == 0 and r["gemm"] == 0, (note, r)
    assert r["thr_sort"] == (1 if collected(case, qi, md, ranges) > T.HOST_ORDER_MAX else 0), (note, r)


# ------------------------------------------------------------------------------------------------------------------ flush residues
@pytest.mark.parametrize("name", T.FLUSH_NAMES)
def test_one_wave_flushes_its_buffer_at_every_residue(gpu_ctx, corpora, name):
    """253 + 4, 254 + 3, 255 + 2, 256 + 1, 256 + 4, the exact fit 255 + 1, a hit total of 512, no hit: the sizes are the model's
    (test_model_reports_the_flush_sizes_the_case_claims).  Unfiltered and inside the case's ranges; a ranged twin searched unfiltered
    also returns the hit rows between its ranges."""
    case, c = T.case(name), corpora(name)
    with tuned(gpu_ctx, **ONE_WAVE):
        for ranges in case.range_options():
            check_k4(gpu_ctx, c, case, 0, T.MAX_DISTANCE, ranges, (name, ranges is not None))


@pytest.mark.parametrize("name", T.FLUSH_NAMES)
def test_many_waves_give_the_same_answer(gpu_ctx, corpora, name):
    case, c = T.case(name), corpora(name)
    for threads in (512, 1024):
        for blocks in (1, 2):
            with tuned(gpu_ctx, scan_blocks=blocks, scan_threads=threads):
                for ranges in case.range_options():
                    check_k4(gpu_ctx, c, case, 0, T.MAX_DISTANCE, ranges, (name, threads, blocks, ranges is not None))


# --------------------------------------------------------------------------------------------------------------------------- ranges
@pytest.mark.parametrize("launch", [ONE_WAVE, {}], ids=["one-wave", "default"])
@pytest.mark.parametrize("name", ["ranges-hits-inside", "ranges-hits-outside"])
def test_short_ranges(gpu_ctx, corpora, name, launch):
    """Ranges of 1, 2, 3, 4, 5, 7 and 9 rows, touching and far apart, one ending on the last row: hits inside with misses right
    outside, and hits right outside with the only hit inside in the short last chunk."""
    case, c = T.case(name), corpora(name)
    with tuned(gpu_ctx, **launch):
        for sight in range(3):                                     # (the third call answers from the range set kept on the corpus)
            check_k4(gpu_ctx, c, case, 0, T.MAX_DISTANCE, case.ranges, (name, sight))
        check_k4(gpu_ctx, c, case, 0, T.MAX_DISTANCE, None, (name, "unfiltered"))
        for one in (case.ranges[0], case.ranges[-1], case.ranges[20]):
            check_k4(gpu_ctx, c, case, 0, T.MAX_DISTANCE, [one], (name, one))


# ------------------------------------------------------------------------------------------------------------------ ordering border
@pytest.mark.parametrize("launch", [ONE_WAVE, {}], ids=["one-wave", "default"])
@pytest.mark.parametrize("n_collected", T.BORDER_COUNTS)
def test_host_order_up_to_2048_collected_hits_device_order_above(gpu_ctx, corpora, n_collected, launch):
    """2047, 2048, 2049 and 4100 collected hits with 600 equal distances, rows equal to the query and zero rows among them.  At
    max_distance = 1 the zero rows are collected and cut (by `<` on the host, by lower_bound behind the device sorts); one f64 step
    above 1 they are the answer's tail, in row order."""
    case, c = T.case("border-%d" % n_collected), corpora("border-%d" % n_collected)
    with tuned(gpu_ctx, **launch):
        for md in case.mds:
            assert collected(case, 0, md, None) == n_collected
            check_k4(gpu_ctx, c, case, 0, md, None, (n_collected, md))


def test_max_distance_zero_and_max_distance_above_every_row(gpu_ctx, corpora):
    case, c = T.case("border-2047"), corpora("border-2047")
    assert collected(case, 0, 0.0, None) == T.N_SAME and len(case.answer(0, 0.0)[0]) == 0     # rows equal to the query: 0 is not < 0
    check_k4(gpu_ctx, c, case, 0, 0.0, None, "max_distance 0")
    assert len(case.answer(0, 2.5)[0]) == case.n
    check_k4(gpu_ctx, c, case, 0, 2.5, None, "max_distance 2.5")


# ----------------------------------------------------------------------------------------------------------------------- strictness
@pytest.mark.parametrize("launch", [ONE_WAVE, {}], ids=["one-wave", "default"])
@pytest.mark.parametrize("name", ["strict", "strict-padded"])
def test_cut_is_strict_on_the_f64_value(gpu_ctx, corpora, name, launch):
    """max_distance equal to a cluster member's exact distance, one f64 step above and one below; the unfiltered and the filtered
    kernel; up to 2048 collected hits (the host's `<`) and above (lower_bound on the sorted distances)."""
    case, c = T.case(name), corpora(name)
    with tuned(gpu_ctx, **launch):
        for md in case.mds:
            for ranges in case.range_options():
                check_k4(gpu_ctx, c, case, 0, md, ranges, (name, md, ranges is not None))


@pytest.mark.parametrize("name", ["strict", "strict-padded"])
def test_sweep_cut_is_strict_on_the_f64_value(gpu_ctx, corpora, name):
    """Four queries in one batched threshold sweep (two of them the cluster's query).  Padded, the cluster's queries collect more
    than a candidate buffer holds and take one scan each."""
    case, c = T.case(name), corpora(name)
    over = sum(collected(case, qi, case.mds[0], None) > T.CAND_CAP for qi in range(4))
    assert over == (2 if name == "strict-padded" else 0)
    with tuned(gpu_ctx, fallback_batch_min_rows=0):
        for md in case.mds:
            got, r = ran(gpu_ctx, lambda: c.search(case.qs, top_k=3, max_distance=md))
            assert r["gemm_thr"] == 1 and r["scan"] == over and r["thr_sort"] == over, (name, md, r)
            for qi in range(4):
                same(got[qi], case.answer(qi, md), (name, md, qi))


# ------------------------------------------------------------------------------------------------------------------ sweep capacity
@pytest.mark.parametrize("prepack", [False, True], ids=["rows", "image"])
def test_sweep_capacity(gpu_ctx, prepack):
    """One call of six queries with 0, 1, 2047, 2048, 2049 and 3000 hits: one sweep, and one scan for each of the two queries that
    overflow their 2048 candidate slots."""
    import semtools_amd as smt

    case = T.case("sweep-capacity")
    c = smt.Corpus(gpu_ctx)
    try:
        c.append(case.emb)
        if prepack:
            c.prepack()
            assert c.image_bytes > 0
        with tuned(gpu_ctx, fallback_batch_min_rows=0):
            got, r = ran(gpu_ctx, lambda: c.search(case.qs, top_k=3, max_distance=T.MAX_DISTANCE))
        want = [case.answer(qi) for qi in range(len(case.qs))]
        assert tuple(len(w[0]) for w in want) == T.SWEEP_COUNTS
        assert r["gemm_thr"] == 1 and r["scan"] == sum(len(w[0]) > T.CAND_CAP for w in want) == 2, r
        for qi in range(len(case.qs)):
            same(got[qi], want[qi], (prepack, qi))
    finally:
        c.close()


# -------------------------------------------------------------------------------------------------------------- re-answer past 2048
@pytest.mark.parametrize("mode", ["documents", "workspace"])
def test_top_k_re_answer_through_the_device_ordering(gpu_ctx, corpora, mode):
    """top_k = 10 ends inside 2100 equal distances: the exhaustive re-answer collects more than 2048 rows, orders them on the device
    and cuts at k.  Five nearer rows, then the first five copies by row; again inside ranges that leave the first seven copies out."""
    import semtools_amd as smt

    case, c = T.case("reanswer"), corpora("reanswer")
    for ranges in case.range_options():
        if mode == "documents":
            got, r = ran(gpu_ctx, lambda: c.search(case.qs[0], top_k=10, ranges=ranges))
        else:                                                       # a score threshold that admits every row
            got, r = ran(gpu_ctx, lambda: c.search(case.qs[0], top_k=10, max_distance=2.5, mode=smt.MODE_WORKSPACE, ranges=ranges))
        want = case.answer(0, float("inf"), ranges, 10)
        same(got[0], want, (mode, ranges is not None))
        assert r["thr_sort"] == 1 and r["scan"] == 2, (mode, r)     # the top-k scan, then the K4 scan of the re-answer
        first = case.tied[np.isin(case.tied, T.eligible(case.n, ranges))][:5]
        assert got[0][0][5:].tolist() == first.tolist()


# ---------------------------------------------------------------------------------------------------------------- resize and rerun
@pytest.mark.parametrize("launch", [ONE_WAVE, {}], ids=["one-wave", "default"])
@pytest.mark.parametrize("total,scans", [(511, 1), (512, 1), (513, 2), (1500, 2), (2500, 2)])
def test_hit_buffer_too_small_is_resized_and_the_scan_rerun(gpu_ctx, corpora, total, scans, launch):
    """thr_hit_cap = 512: a pass that counts more hits runs again with a buffer of exactly that size.  In the one-wave launch the
    capacity falls inside the third flush (test_model_puts_the_capacity_inside_a_flush).  Filtered, the rerun rebuilds the chunk
    table; 2500 hits go on to the device ordering."""
    case, c = T.case("rerun-%d" % total), corpora("rerun-%d" % total)
    with tuned(gpu_ctx, thr_hit_cap=512, **launch):
        for ranges in case.range_options():
            assert T.launches(case.passes(), ranges, cap=512) == scans
            check_k4(gpu_ctx, c, case, 0, T.MAX_DISTANCE, ranges, (total, ranges is not None), scans=scans)
    check_k4(gpu_ctx, c, case, 0, T.MAX_DISTANCE, None, (total, "default capacity"))


def test_hit_capacity_key_refuses_values_below_one(gpu_ctx):
    for bad in (0, -1):
        with pytest.raises(RuntimeError):
            gpu_ctx.set_tuning("thr_hit_cap", bad)
    gpu_ctx.set_tuning("thr_hit_cap", 1)
    gpu_ctx.set_tuning("thr_hit_cap", DEFAULTS["thr_hit_cap"])
