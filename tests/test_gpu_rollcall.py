"""GPU: no search route may MISS a row it was given (inputs and their conditions: tests/rollcall.py, tests/test_rollcall_cpu.py).

The mirror image of tests/test_gpu_decoys.py, whose route families, tuning keys and profile-counter witnesses this file takes.  Every
fixture is a roll call: each allowed row is in the expected answer of exactly one axis query, at a known place, 0.4 in front of any
other row.  A row that no lane read, or that was credited to another query, leaves a stranger or padding in one list.  Every case
asserts the same things: host form -- rows equal to the constructed list and to the oracle's accurate answer over the allowed rows,
f64 distances byte for byte; device form -- the list passes soundness.check_list and every status word is PROVED (these margins are
orders of magnitude wider than any guard band, so PROVED is a condition here, not a measurement)."""
import contextlib

import numpy as np
import pytest

from tests import decoys as D
from tests import rollcall as R
from tests import soundness as S
from tests.test_gpu_decoys import K3_FROM_IMAGE, K3_FROM_ROWS, Ref, check_host, k3_keys, on_gemm, on_scan, ran, tuned

pytestmark = pytest.mark.gpu

GEMM_MIN_NQ = 5                  # the default of gemm_min_nq: an unfiltered call of fewer queries takes the scan kernel at these sizes
TAKE_DEFAULT = 15                # common.h Tuning::scan_pair: what a context starts with
G = D.G


# ---------------------------------------------------------------------------------------------------------------- fixtures
_REFS = {}


def ref_of(fx):
    """The oracle over the allowed rows of a fixture, shared by every case over it."""
    if fx.name not in _REFS:
        _REFS[fx.name] = Ref(fx.rc.rows, fx.ids)
    return _REFS[fx.name]


def owned(ctx, buf, rows=None):
    """An owned corpus holding buf[:rows] (filler rows behind them in its capacity when rows < len(buf))."""
    import semtools_amd as smt

    c = smt.Corpus(ctx)
    c.append(np.ascontiguousarray(buf))
    if rows is not None and rows < len(buf):
        c.truncate(rows)
    return c


@contextlib.contextmanager
def corpus_of(ctx, name, prepack=False):
    fx = R.fixture(name)
    c = owned(ctx, fx.buf)
    try:
        if prepack:
            c.prepack()
            assert c.image_bytes > 0
        yield fx, c
    finally:
        c.close()


def wanted(fx, js, k):
    """The oracle's answers of the queries js at top_k = k; where k is the size of the query's set, they ARE the constructed list."""
    want = ref_of(fx).topk(fx.rc.queries[js], k)
    for j, (rows, dist) in zip(js, want):
        own = fx.global_rows(j)
        assert rows[:len(own)] == own[:k] and len(rows) == min(k, fx.rc.n), (fx.name, j)
    return want


def check_call(c, fx, js, k, note, route=None, ranges=None, device=True, trace=None, route_host=None):
    """One call of the roll call in both forms (the device form takes no ranges).  route: the witness read from the profile counters,
    for both forms unless route_host says otherwise for the host form."""
    ctx, ref = c.ctx, ref_of(fx)
    qs = np.ascontiguousarray(fx.rc.queries[js])
    want = wanted(fx, js, k)
    got, r = ran(ctx, lambda: c.search(qs, top_k=k, ranges=ranges))
    if (route_host or route) is not None:
        (route_host or route)(r)
    check_host(ref, got, want, (note, "host", js[0]), trace)
    if device and ranges is None:
        (rows, dist, st, _), r = ran(ctx, lambda: S.device_topk(c, qs, k))
        if route is not None:
            route(r)
        for i in range(len(js)):
            S.check_list(rows[i], dist[i], want[i][0], want[i][1], k, (note, "device", js[i]))
        assert (st == 0).all(), (note, "not PROVED", js, st.tolist())


def roll_call(c, fx, nq, note, route=None, route_small=None, min_nq=1, **kw):
    """Every query of the fixture once, nq per call, sets of one size per call.  route_small: the witness of calls below min_nq."""
    for js, k in fx.rc.calls(nq):
        check_call(c, fx, js, k, (note, fx.name, nq), route if len(js) >= min_nq else route_small, **kw)


# ================================================================================================ K2, 1 to 4 queries
@pytest.mark.parametrize("nq", [1, 2, 3, 4])
@pytest.mark.parametrize("name", ["P-56-strided-shuffled", "P-56-strided-descending", "P-56-contiguous-ascending",
                                  "P-56-contiguous-shuffled", "P-1-first", "P-1-last"])
def test_scan_kernel(gpu_ctx, name, nq):
    """k = 56 over 4097 rows in both assignments, and k = 1 with 192 queries over the first and the last 192 rows: the first and the
    last chunks, waves and blocks."""
    with corpus_of(gpu_ctx, name) as (fx, c), tuned(gpu_ctx, gemm_min_nq=8):
        roll_call(c, fx, nq, "K2", on_scan)


@pytest.mark.parametrize("steal", [1, 4])
@pytest.mark.parametrize("name", ["P-2049-56", "P-2049-56-contiguous", "P-56-strided-shuffled", "P-56-contiguous-shuffled"])
def test_scan_kernel_with_rows_dealt_while_it_runs(gpu_ctx, name, steal):
    """scan_steal with two blocks: the rows of the last dynamically dealt group, the ragged chunk among them."""
    with corpus_of(gpu_ctx, name) as (fx, c):
        assert (fx.rc.n + 3) // 4 >= 2 * 64 * steal
        with tuned(gpu_ctx, gemm_min_nq=8, scan_blocks=2, scan_steal=steal, scan_steal_pct=50):
            roll_call(c, fx, 1, ("steal", steal), on_scan)


# ================================================================================================ queued one-query calls sharing a pass
class _Piped:
    pass


@pytest.fixture(scope="module")
def piped():
    """A context of its own on a torch stream with the async select pipeline on, as in tests/test_gpu_scan_groups_decoys.py: on a
    stream where queued calls can be taken along at all (tests/test_gpu_scan_groups.py says why some cannot)."""
    import torch
    import semtools_amd as smt

    p = _Piped()
    p.torch = torch
    x = torch.zeros(1000, 256, device="cuda:0")
    x[:, 0] = 1.0
    torch.cuda.synchronize()
    for attempt in range(6):
        p.stream = torch.cuda.Stream(torch.device("cuda:0"))
        p.ctx = smt.Context(0, stream=p.stream.cuda_stream)
        p.ctx.set_tuning("async_select", 1)
        probe = smt.Corpus(p.ctx, device_ptr=x.data_ptr(), rows=1000)
        p.ctx.set_tuning("scan_pair", 1)
        p.ctx.set_tuning("scan_pair_wait_us", 2000)
        paired = _series(p, probe, x[:1].repeat(8, 1), 10)[3][0]
        p.ctx.set_tuning("scan_pair_wait_us", 0)
        p.ctx.set_tuning("scan_deep", TAKE_DEFAULT)
        probe.close()
        if paired > 0 or attempt == 5:                             # (the last one stays: the test then says what is wrong)
            break
        p.ctx.close()
    yield p
    p.ctx.set_tuning("async_select", 0)
    p.ctx.close()


def _series(p, c, qd, k):
    """One back-to-back one-query device call per row of qd.  (rows, dist, status, (paired, alone, absorbed))"""
    torch, ctx, stream = p.torch, p.ctx, p.stream
    calls = len(qd)
    with torch.cuda.stream(stream):
        rows = torch.full((calls, k), -7, dtype=torch.int64, device="cuda:0")
        dist = torch.full((calls, k), -7.0, dtype=torch.float64, device="cuda:0")
        st = torch.full((calls,), 7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()                                       # (the queries were uploaded on another stream)
    before = ctx.scan_pairs()
    for i in range(calls):
        c.search_topk_device(qd[i].data_ptr(), 1, k, 0, rows[i].data_ptr(), dist[i].data_ptr(), out_status_ptr=st[i:].data_ptr())
    ctx.synchronize()
    counts = tuple(int(y - x) for x, y in zip(before, ctx.scan_pairs()))
    return rows.cpu().numpy().view(np.uint64), dist.cpu().numpy(), st.cpu().numpy(), counts


# (tuning key, limit, which histogram).  A pass takes the calls i + 2, i + 4, ... of its stream along, so a full group of sixteen
# needs 32 queued calls; a series is CALLS = 64 calls, as in tests/test_gpu_scan_deep.py (the deciding block waits up to 2 ms for
# the host to queue them).  The wide and the deep kernel serve lists of k' = k + 8 <= 32 keys: above that (k = 32) every limit runs
# the four-call kernel.
CALLS = 64
LIMITS = {"pair-1": ("scan_pair", 1, "scan_groups"), "pair-3": ("scan_pair", 3, "scan_groups"),
          "wide-7": ("scan_take", 7, "scan_groups_wide"), "deep-15": ("scan_deep", 15, "scan_groups_deep"),
          "default": (None, TAKE_DEFAULT, "scan_groups_deep")}


@pytest.mark.parametrize("limit", list(LIMITS))
@pytest.mark.parametrize("name", ["P-10-first", "P-10-last", "P-24-contiguous", "P-24-strided", "P-32-contiguous", "P-32-strided"])
def test_queued_one_query_calls_sharing_a_pass(piped, name, limit):
    """Series of back-to-back device calls, each a different roll-call query, so that every slot of a group has winners of its own
    somewhere in the corpus; four rotations of the queries, so that a query meets different slots.  k = 10 (J = 192 over the first
    and over the last 1920 rows), k = 24 (J = 171, the longest list of the wide and deep kernels) and k = 32 (J = 129, the four-call
    kernel under every limit); the limits that select each kernel, and the context's default.  Grouping races
    with the host, as in tests/test_gpu_scan_deep.py: every call of every series is checked, and over all series a group of the
    family's largest size must have formed -- up to four more rotations are run, and checked, until one has."""
    torch, ctx = piped.torch, piped.ctx
    key, limit_value, histogram = LIMITS[limit]
    fx = R.fixture(name)
    rc, k, calls, take = fx.rc, fx.rc.k, CALLS, limit_value
    if k + 8 > 32:
        take, histogram = min(limit_value, 3), "scan_groups"         # (the largest group the four-call kernel forms)
    want = wanted(fx, list(range(rc.J)), k)
    c = owned(ctx, fx.buf)
    torch.cuda.synchronize()
    before = getattr(ctx, histogram)()
    try:
        if key is not None:
            ctx.set_tuning(key, limit_value)
        ctx.set_tuning("scan_pair_wait_us", 2000)
        for rotation in (0, 3, 6, 9, 12, 15, 18, 21):
            if rotation >= 12 and int(getattr(ctx, histogram)()[take] - before[take]) > 0:
                break
            order = (np.arange(rc.J) + rotation) % rc.J
            for b in range(0, rc.J, calls):
                js = order[b:b + calls]
                qd = torch.from_numpy(np.ascontiguousarray(rc.queries[js])).to("cuda:0")
                torch.cuda.synchronize()
                rows, dist, st, _ = _series(piped, c, qd, k)
                for i, j in enumerate(js):
                    S.check_list(rows[i], dist[i], want[j][0], want[j][1], k, (name, limit, rotation, "query", int(j), "call", i))
                assert (st == 0).all(), (name, limit, rotation, "not PROVED", js.tolist(), st.tolist())
        by_size = [int(y - x) for x, y in zip(before, getattr(ctx, histogram)())]
    finally:
        ctx.set_tuning("scan_pair_wait_us", 0)
        ctx.set_tuning("scan_deep", TAKE_DEFAULT)
        c.close()
    assert all(v == 0 for v in by_size[take + 1:]) and by_size[take] > 0, (name, limit, by_size)


# ================================================================================================ K4
@pytest.mark.parametrize("name", R.SWEEP_FIXTURES)
def test_threshold_scan_returns_every_row(gpu_ctx, name):
    """One extra query owns every allowed row: max_distance = 0.9 returns them all, in row order -- from the one-query scan, and from
    a call of six (the other five ordinary roll-call queries, which get their own sets): unfiltered that is one sweep of the batched
    kernel, whose 2048 candidate slots the owner of everything overflows, so it is re-answered by a scan; filtered, six scans."""
    md = R.SWEEP_MAX_DISTANCE
    with corpus_of(gpu_ctx, name) as (fx, c):
        rc, ref = fx.rc, ref_of(fx)
        ranges = None if fx.ids is None else R.range_ids(name.split("-")[1])[0]
        everything = (np.arange(rc.n) if fx.ids is None else fx.ids).tolist()
        js = [rc.J] + [j for j in (0, 1, rc.J // 2, rc.J - 2, rc.J - 1)]
        qs = np.ascontiguousarray(rc.queries[js])
        want = ref.under(qs, md)
        assert want[0][0] == everything and [w[0] for w in want[1:]] == [fx.global_rows(j) for j in js[1:]]
        got, r = ran(gpu_ctx, lambda: c.search(qs[:1], top_k=3, max_distance=md, ranges=ranges))
        assert r["scan"] >= 1 and r["gemm_thr"] == 0 and r["gemm"] == 0, r
        check_host(ref, got, want[:1], (name, "K4"))
        with tuned(gpu_ctx, fallback_batch_min_rows=0):
            got, r = ran(gpu_ctx, lambda: c.search(qs, top_k=3, max_distance=md, ranges=ranges))
        assert (r["gemm_thr"] == 1 and r["scan"] >= 1) if ranges is None else (r["gemm_thr"] == 0 and r["scan"] >= 6), r
        check_host(ref, got, want, (name, "K4-six"))


# ================================================================================================ large k
@pytest.mark.parametrize("name", ["L-1024", "L-1024-strided"])
def test_large_k(gpu_ctx, name):
    """16385 rows (one past the large-k shortcut), k = 1024, J = 17: the sampled route with one query per call (a streaming collect)
    and six (one sweep of the batched kernel), and the all-keys route.  The last set takes a call of its own at its own size."""
    with corpus_of(gpu_ctx, name) as (fx, c):
        assert fx.rc.n == D.N_LARGEK > 16384 and fx.rc.J == 17

        def sampled(nq):
            def route(r):
                assert r["largek_finish"] >= 1 and r["largek_tau"] >= 1, r
                assert nq not in (1, 6) or r["largek_collect"] == (0 if nq == 6 else 1), r
            return route

        def finished(r):
            assert r["largek_finish"] >= 1, r

        for nq in (1, 6):
            for js, k in fx.rc.calls(nq):
                check_call(c, fx, js, k, (name, "sampled", nq), sampled(len(js)) if k > 56 else None, route_host=finished if k > 56 else None)
        with tuned(gpu_ctx, largek_sampled=0):
            def allkeys(r):
                assert r["largek_finish"] == 0 and r["scan"] >= 2, r
            for js, k in fx.rc.calls(2):
                check_call(c, fx, js, k, (name, "allkeys"), allkeys if k > 56 and len(js) == 2 else None, device=False)


def test_large_k_inside_ranges(gpu_ctx):
    """k = 57 over the dense range list: the large-k route's virtual-row map."""
    with corpus_of(gpu_ctx, "R-dense-57") as (fx, c):
        ranges = R.range_ids("dense")[0]

        def route(r):
            assert r["largek_collect"] >= 1 and r["largek_finish"] >= 1, r
        for nq in (1, 6):
            for js, k in fx.rc.calls(nq):
                check_call(c, fx, js, k, ("largek-ranges", nq), route if k > 56 else on_scan, ranges=ranges)
        with tuned(gpu_ctx, largek_sampled=0):
            roll_call(c, fx, 2, "allkeys-ranges", None, ranges=ranges)


# ================================================================================================ K3
def _batched_cases(c, note, f56, f32a, f32b, min_nq=GEMM_MIN_NQ, **kw):
    """nq = 8 at k = 56 (ten calls), nq = 33 at k = 32, and 130 queries at k = 32 in one call: the 128 full sets of the contiguous
    fixture and the first two queries again (its last set, one row, takes a call of its own).  min_nq: the smallest call -- the last
    of a set size -- that the batched kernel answers under the tuning of the case."""
    roll_call(c(f56), R.fixture(f56), 8, note, on_gemm, on_scan, min_nq=min_nq, **kw)
    roll_call(c(f32a), R.fixture(f32a), 33, note, on_gemm, on_scan, min_nq=min_nq, **kw)
    fx = R.fixture(f32b)
    assert fx.rc.J == 129 and len(fx.rc.by_size[32]) == 128
    check_call(c(f32b), fx, fx.rc.by_size[32] + [0, 1], 32, (note, f32b, 130), on_gemm, **kw)
    check_call(c(f32b), fx, fx.rc.by_size[1], 1, (note, f32b, "the last set"), on_scan, **kw)


@pytest.mark.parametrize("mode", list(K3_FROM_ROWS))
def test_batched_kernels_from_the_rows(gpu_ctx, mode):
    with contextlib.ExitStack() as stack:
        live = {n: stack.enter_context(corpus_of(gpu_ctx, n))[1] for n in ("P-56-strided-shuffled", "P-32-strided", "P-32-contiguous")}
        # (without the row-register kernel only calls of eight queries and more are batched: search.cpp topk_route)
        min_nq = GEMM_MIN_NQ if mode.startswith("rowreg") else 8
        for boot in ((1, 0) if mode.startswith("rowreg") else (1,)):
            with tuned(gpu_ctx, gemm_bootstrap=boot, gemm_image=0, **k3_keys(mode)):
                _batched_cases(live.__getitem__, ("K3", mode, boot), "P-56-strided-shuffled", "P-32-strided", "P-32-contiguous", min_nq=min_nq)


@pytest.mark.parametrize("mode", list(K3_FROM_IMAGE))
def test_batched_kernel_and_scans_from_the_image(gpu_ctx, mode):
    """Layout I: 4097 rows with the fp16 image, whose last tile straddles `rows`; one and three queries scanned from the image."""
    with contextlib.ExitStack() as stack:
        live = {n: stack.enter_context(corpus_of(gpu_ctx, n, prepack=True))[1]
                for n in ("P-56-contiguous-shuffled", "P-32-strided", "P-32-contiguous")}
        with tuned(gpu_ctx, **k3_keys(mode)):
            _batched_cases(live.__getitem__, ("image", mode), "P-56-contiguous-shuffled", "P-32-strided", "P-32-contiguous")
            with tuned(gpu_ctx, image_scan_min_rows=1):
                for nq in (1, 3):
                    roll_call(live["P-56-contiguous-shuffled"], R.fixture("P-56-contiguous-shuffled"), nq, ("image-scan", mode), on_gemm)


def test_image_after_truncate_and_append(gpu_ctx):
    """Truncate to 4001 rows, append 50: the tile that straddled the old row count is filled by the append, and a new one straddles
    the new count.  The roll call is rebuilt for the 4051 rows present (the rows before the cut by write_rows)."""
    with corpus_of(gpu_ctx, "P-56-contiguous-shuffled", prepack=True) as (_, c):
        c.truncate(4001)
        for name, nq in (("I-56-after-append", 8), ("I-32-after-append", 33)):
            fx = R.fixture(name)
            if c.rows == 4001:
                assert c.append(fx.buf[4001:]) == 4001
                c.write_rows(0, fx.buf[:4001])
            else:
                c.write_rows(0, fx.buf)
            assert c.rows == fx.rc.n == R.N_I2 and c.image_bytes > 0
            for mode in K3_FROM_IMAGE:
                with tuned(gpu_ctx, **k3_keys(mode)):
                    roll_call(c, fx, nq, ("image-after-append", mode), on_gemm, on_scan, min_nq=GEMM_MIN_NQ)
            with tuned(gpu_ctx, image_scan_min_rows=1):
                roll_call(c, fx, 3, "image-scan-after-append", on_gemm)


# ================================================================================================ R: inside the ranges
@pytest.mark.parametrize("name", ["R-dense-56", "R-dense-56-strided", "R-sparse-56", "R-sparse-10"])
def test_ranges_scan_kernel(gpu_ctx, name):
    """The chunk table (row0 | valid rows per 4-row chunk) under K2 with 1 to 4 queries."""
    ranges = R.range_ids(name.split("-")[1])[0]
    with corpus_of(gpu_ctx, name) as (fx, c), tuned(gpu_ctx, gemm_min_nq=8):
        for nq in (1, 2, 3, 4):
            roll_call(c, fx, nq, "R-K2", on_scan, ranges=ranges)


@pytest.mark.parametrize("image", [False, True], ids=["rows", "image"])
@pytest.mark.parametrize("name,nq", [("R-dense-56", 8), ("R-dense-32", 33), ("R-sparse-10", 8), ("R-sparse-10", 33)])
def test_ranges_batched_kernels_and_the_kept_range_set(gpu_ctx, name, nq, image):
    """The dense list over the tile table (tile | mask of the wanted rows) on the row-register kernel, the sparse list over the chunk
    table on the LDS-row kernel, from the rows and from the image.  Three sights of the same list: the second builds the kept range
    set, the third answers from it; all three give the same bytes.  A filtered call of fewer than eight queries takes the scan kernel."""
    ranges = R.range_ids(name.split("-")[1])[0]
    with corpus_of(gpu_ctx, name, prepack=image) as (fx, c):
        assert c.range_sets() == (0, 0, 0)
        traces = []
        for sight in range(3):
            traces.append([])
            roll_call(c, fx, nq, ("R-K3", image, sight), on_gemm, on_scan, min_nq=8, ranges=ranges, trace=traces[-1])
        kept, hits, builds = c.range_sets()
        assert kept == 1 and builds == 1 and hits >= 1, (kept, hits, builds)
        assert len(traces[0]) > 0 and traces[0] == traces[1] == traces[2]
        if "dense" in name:
            for mode in ("rowreg-f16x2", "rowreg-f16x1", "ldsrow"):
                with tuned(gpu_ctx, **k3_keys(mode)):
                    roll_call(c, fx, nq, ("R-K3", image, mode), on_gemm, on_scan, min_nq=8, ranges=ranges)


# ================================================================================================ C: truncate, append, compact
def test_owned_corpus_after_truncate_append_and_compact(gpu_ctx):
    """The stages of the decoy module's layout C on one owned corpus with an image.  The roll call of the rows present is written
    after the truncation and after the append; the content before the compaction is the compacted roll call with filler rows in the
    dropped runs, so the rows on either side of each seam are where smt_corpus_compact put them."""
    (_, n, _), (_, n_app, _), (_, n_cmp, keep) = R.stages_c()
    fx = R.fixture("C-truncated")
    c = owned(gpu_ctx, np.concatenate([fx.buf, R.filler_rows(G, seed=92)]))
    try:
        c.prepack()
        c.truncate(n)

        def routes(fx, note):
            assert c.rows == fx.rc.n and c.image_bytes > 0
            with tuned(gpu_ctx, gemm_min_nq=8):
                roll_call(c, fx, 1, (note, "K2"), on_scan)
            with tuned(gpu_ctx, gemm_image=0):
                roll_call(c, fx, 8, (note, "K3-rows"), on_gemm, on_scan, min_nq=GEMM_MIN_NQ)
            roll_call(c, fx, 8, (note, "K3-image"), on_gemm, on_scan, min_nq=GEMM_MIN_NQ)

        routes(fx, "truncated")
        fx = R.fixture("C-appended")
        assert c.append(fx.buf[n:]) == n
        c.write_rows(0, fx.buf[:n])
        routes(fx, "appended")
        fx = R.fixture("C-compacted")
        c.write_rows(0, R.before_compaction(fx.buf, keep, n_app))
        with tuned(gpu_ctx, compact_bounce_rows=64):
            assert c.compact(keep) == n_cmp - keep[0][1]
        assert c.rows == n_cmp and np.array_equal(c.read_rows(0, n_cmp), fx.buf)
        routes(fx, "compacted")
    finally:
        c.close()


# ================================================================================================ S: three unequal shards
def _sharded(transport, buf, sizes):
    import torch
    import semtools_amd as smt

    x = torch.from_numpy(buf).to("cuda:0")
    torch.cuda.synchronize()
    cuts = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    g = smt.Group.logical(0, 3)
    g.set_transport(transport)
    sc = smt.ShardedCorpus(g, device_ptrs=[x[cuts[i]:cuts[i + 1]].data_ptr() for i in range(3)], shard_rows=list(sizes))
    assert g.transport == transport and sc.rows == len(buf)
    return x, g, sc


def _shards_roll_call(fx, g, sc, nqs, note, device_nq=1):
    import torch

    ref = ref_of(fx)
    for nq in nqs:
        for js, k in fx.rc.calls(nq):
            got = sc.search(np.ascontiguousarray(fx.rc.queries[js]), top_k=k)
            check_host(ref, got, wanted(fx, js, k), (note, "host", nq, js[0]))
    # the device-resident form: one packed [2][k] answer per one-query call on local device 0, with its status word
    qd = torch.from_numpy(fx.rc.queries[:fx.rc.J]).to("cuda:0")
    for size, js in fx.rc.by_size.items():
        out = torch.full((len(js), 2, size), -7, dtype=torch.int64, device="cuda:0")
        st = torch.full((len(js),), 7, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        for i, j in enumerate(js):
            sc.search_topk_device([qd[j].data_ptr()] * 3, 1, size, [out[i].data_ptr(), None, None], [st[i:].data_ptr(), None, None])
        g.synchronize()
        torch.cuda.synchronize()
        o, st = out.cpu().numpy(), st.cpu().numpy()
        want = wanted(fx, js, size)
        for i, j in enumerate(js):
            rows, dist = o[i, 0].view(np.uint64), np.ascontiguousarray(o[i, 1]).view(np.float64)
            S.check_list(rows, dist, want[i][0], want[i][1], size, (note, "device", j))
        assert (st == 0).all(), (note, "not PROVED", st.tolist())


@pytest.mark.parametrize("transport", ["peer", "copy"])
@pytest.mark.parametrize("name", ["P-56-contiguous-shuffled", "P-56-strided-shuffled"])
def test_three_unequal_shards(name, transport):
    """smt_sharded_search over shards of 1365, 1 and 2731 rows, the roll call over global rows: k = 56 with one and four queries per
    call; the last row of every shard and the shard of one row are owed to some query."""
    fx = R.fixture(name)
    x, g, sc = _sharded(transport, fx.buf, R.SHARDS)
    try:
        _shards_roll_call(fx, g, sc, (1, 4), ("S", name, transport))
    finally:
        sc.close()
        g.close()


@pytest.mark.parametrize("transport", ["peer", "copy"])
def test_three_shards_large_k(transport):
    """k = 1024 over three shards of about 5500 rows: every shard's large-k answer and the cross-shard merge."""
    fx = R.fixture("S-1024")
    x, g, sc = _sharded(transport, fx.buf, R.SHARDS_LARGEK)
    try:
        _shards_roll_call(fx, g, sc, (1, 6), ("S-1024", transport))
    finally:
        sc.close()
        g.close()
