"""GPU: no search route may look outside the rows it was given (inputs and their conditions: tests/decoys.py, tests/test_decoys_cpu.py).

Every case puts DECOYS -- rows that would rank first for every query of the call -- where a kernel that is off by one would find
them: past both ends of an adopted corpus (layout A), inside the corpus but outside the call's ranges (B), beyond `rows` inside an
owned corpus' capacity (C), between the adopted shards of a sharded corpus.  Every case asserts the same things: no returned id
outside the allowed set; rows and f64 distances equal to the oracle's accurate answer over the ALLOWED rows, bit for bit, host form
and device form, padding as soundness.check_list expects; the device form's status words no worse, per query, than those of the same
call on a corpus without decoys (a decoy that only leaks into a threshold costs proofs, not rows); for layout A the answers with
NaN / Inf guards byte-identical to those with finite guards; and, from the profile counters, that the route the case was written
for really ran."""
import contextlib

import numpy as np
import pytest

from tests import decoys as D
from tests import soundness as S

pytestmark = pytest.mark.gpu

G = D.G
PAD = S.PAD_ROW
DEFAULTS = dict(gemm_min_nq=5, gemm_min_rows_small=1_000_000, gemm_nominate=0, gemm_bf16x3=1, gemm_rowreg=1, gemm_ldsrow=1,
                gemm_bootstrap=1, gemm_image=1, image_scan_min_rows=1_500_000, scan_overlap=1, scan_pair=1, scan_pair_wait_us=0,
                scan_pair_ring=4096, scan_steal=0, scan_steal_pct=6, scan_blocks=0, largek_sampled=1,
                fallback_batch_min_rows=100_000, compact_bounce_rows=65536, async_select=0)
COUNTERS = ("scan", "gemm", "gemm_thr", "largek_tau", "largek_collect", "largek_finish", "ivf_adc", "ivf_mask")
# K3's kernels by tuning: (gemm_bf16x3, gemm_rowreg, gemm_nominate, gemm_ldsrow)
K3_FROM_ROWS = {"rowreg-bf16x3": (1, 1, 1, 1), "rowreg-f16x2": (1, 1, 2, 1), "rowreg-f16x1": (1, 1, 3, 1),
                "level-f32mfma": (0, 0, 0, 0), "level-bf16x3": (1, 0, 0, 0), "ldsrow": (1, 0, 0, 1)}
K3_FROM_IMAGE = {"image-auto": (1, 1, 0, 1), "image-f16x2": (1, 1, 2, 1), "image-f16x1": (1, 1, 3, 1)}


@contextlib.contextmanager
def tuned(ctx, **keys):
    try:
        for key, value in keys.items():
            ctx.set_tuning(key, value)
        yield
    finally:
        for key in keys:
            ctx.set_tuning(key, DEFAULTS[key])


def k3_keys(mode):
    bf16, rowreg, nominate, ldsrow = {**K3_FROM_ROWS, **K3_FROM_IMAGE}[mode]
    return dict(gemm_bf16x3=bf16, gemm_rowreg=rowreg, gemm_nominate=nominate, gemm_ldsrow=ldsrow)


def ran(ctx, fn):
    """(fn(), launches per profile counter): which kernels answered."""
    ctx.set_tuning("prof_every", 1)
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        out = fn()
        return out, {name: ctx.prof_read(name)[0] for name in COUNTERS}
    finally:
        ctx.prof_enable(False)


def on_scan(r):
    assert r["scan"] > 0 and r["gemm"] == 0 and r["largek_finish"] == 0, r


def on_gemm(r):
    """a batched kernel ran (the host form may re-answer a query whose certificate failed with a K4 scan: "scan" is not asserted)"""
    assert r["gemm"] > 0, r


class Ref:
    """The oracle's answers over the allowed rows of one fixture, computed once per (query, k)."""

    def __init__(self, allowed, ids=None):
        self.allowed, self.ids, self.n = np.ascontiguousarray(allowed), ids, len(allowed)
        self.ok = None if ids is None else set(int(i) for i in ids)
        self._topk, self._under = {}, {}

    def topk(self, qs, k):
        out = []
        for q in qs:
            key = (q.tobytes(), k)
            if key not in self._topk:
                self._topk[key] = D.expected(self.allowed, self.ids, q[None, :], k)[0]
            out.append(self._topk[key])
        return out

    def under(self, qs, max_distance):
        out = []
        for q in qs:
            key = (q.tobytes(), max_distance)
            if key not in self._under:
                self._under[key] = D.expected(self.allowed, self.ids, q[None, :], 1, max_distance=max_distance)[0]
            out.append(self._under[key])
        return out

    def inside(self, rows, note):
        """no id outside the allowed set"""
        rows = np.asarray(rows).astype(np.uint64)
        rows = rows[rows != PAD]
        if self.ok is None:
            assert (rows < np.uint64(self.n)).all(), (note, rows[rows >= np.uint64(self.n)][:4])
        else:
            assert set(rows.tolist()) <= self.ok, (note, sorted(set(rows.tolist()) - self.ok)[:4])


def check_host(ref, got, want, note, trace=None):
    assert len(got) == len(want), note
    for i, ((rows, dist), (wrows, wdist)) in enumerate(zip(got, want)):
        ref.inside(rows, (note, i))
        assert rows.tolist() == wrows, (note, i, rows.tolist()[:6], wrows[:6])
        assert dist.tobytes() == wdist.tobytes(), (note, i)
        if trace is not None:
            trace.append((rows.tobytes(), dist.tobytes()))


def check_device(ref, c, ctl, qs, k, note, route=None, trace=None):
    """The device form of a top-k call on `c` against the oracle and against the status words of the same call on `ctl`."""
    ctx = c.ctx
    (rows, dist, st, _), r = ran(ctx, lambda: S.device_topk(c, qs, k))
    if route is not None:
        route(r)
    ctl_st = S.device_topk(ctl, qs, k)[2]
    want = ref.topk(qs, k)
    for i in range(len(qs)):
        ref.inside(rows[i], (note, i, "device"))
        assert st[i] in (0, 1, 2) and st[i] <= ctl_st[i], (note, i, st.tolist(), ctl_st.tolist())
        if st[i] == 0:
            S.check_list(rows[i], dist[i], want[i][0], want[i][1], k, (note, i, "device"))
    if trace is not None:
        trace.append((rows.tobytes(), dist.tobytes(), st.tobytes()))
    return st


def check_topk(ref, c, ctl, qs, k, note, route=None, trace=None, device=True):
    got, r = ran(c.ctx, lambda: c.search(qs, top_k=k))
    if route is not None:
        route(r)
    check_host(ref, got, ref.topk(qs, k), (note, "host"), trace)
    if device:
        check_device(ref, c, ctl, qs, k, note, route, trace)


# ---------------------------------------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def qs():
    return D.queries()


_REFS = {}      # layout A: one reference per corpus size, shared by every case over it


class Adopted:
    """Layout A on the device: the buffer, the corpus adopted from its middle view, a control corpus and the reference."""

    def __init__(self, ctx, n, flavour, ref=None, with_control=True):
        import torch
        import semtools_amd as smt

        buf, first = D.layout_a(n, seed=100 + n, flavour=flavour)
        self.n = n
        self.x = torch.from_numpy(buf).to("cuda:0")
        torch.cuda.synchronize()
        self.view = self.x[first:first + n]
        self.c = smt.Corpus(ctx, device_ptr=self.view.data_ptr(), rows=n)
        self.ref = ref if ref is not None else _REFS.setdefault(n, Ref(buf[first:first + n]))
        self.ctl = D.control(ctx, buf[first:first + n]) if with_control else None

    def close(self):
        self.c.close()
        if self.ctl is not None:
            self.ctl.close()


def both_flavours(ctx, n, body):
    """body(Adopted, trace) with finite and with non-finite guards: the same bytes."""
    traces, ref = [], None
    for flavour in ("finite", "nonfinite"):
        a = Adopted(ctx, n, flavour, ref)
        ref = a.ref
        trace = []
        try:
            body(a, trace)
        finally:
            a.close()
        traces.append(trace)
    assert len(traces[0]) == len(traces[1]) > 0
    for i, (x, y) in enumerate(zip(*traces)):
        assert x == y, (n, "call", i, "differs between finite and non-finite guards")


# ================================================================================================ the routes, over any corpus
# Each takes the corpus under test, its decoy-free control, the reference over the allowed rows, and an optional trace.  Layout A runs
# them on adopted corpora of every size, layout C on one owned corpus at three row counts.
def routes_scan(ctx, c, ctl, ref, qs, note, trace=None):
    """K2 with 1, 2, 3 and 4 queries at k = 1, 10, 56: the valid-row count of the last 4-row chunk."""
    with tuned(ctx, gemm_min_nq=8):                               # (keep 3 and 4 queries on the scan kernel)
        for nq in (1, 2, 3, 4):
            for k in (1, 10, 56):
                check_topk(ref, c, ctl, qs[:nq], k, (note, "K2", nq, k), on_scan, trace)


def routes_steal(ctx, c, ctl, ref, qs, steal, note, trace=None):
    """The stolen-rows scan (scan_steal; with two blocks it is reached from 128 x scan_steal chunks on, asserted here; no counter
    tells a stolen group from a static one, the scan kernel itself is confirmed): the last dynamic group holds the ragged chunk."""
    assert (ref.n + 3) // 4 >= 2 * 64 * steal
    with tuned(ctx, gemm_min_nq=8, scan_blocks=2, scan_steal=steal, scan_steal_pct=50):
        for nq in (1, 2, 3, 4):
            check_topk(ref, c, ctl, qs[:nq], 10, (note, "steal", steal, nq), on_scan, trace)


def routes_threshold(ctx, c, ctl, ref, qs, note, trace=None):
    """K4: every row under max_distance, one query (scan_threshold_kernel) and a batch in one sweep of the batched kernel."""
    for md in D.MAX_DISTANCES:
        got, r = ran(ctx, lambda: c.search(qs[:1], top_k=3, max_distance=md))
        assert r["scan"] == 1 and r["gemm_thr"] == 0 and r["gemm"] == 0, r
        check_host(ref, got, ref.under(qs[:1], md), (note, "K4", md), trace)
        with tuned(ctx, fallback_batch_min_rows=0):
            got, r = ran(ctx, lambda: c.search(qs[:6], top_k=3, max_distance=md))
        assert r["gemm_thr"] == 1, r
        check_host(ref, got, ref.under(qs[:6], md), (note, "K4-sweep", md), trace)


def routes_large_k(ctx, c, ctl, ref, qs, note, trace=None):
    """k = 57, 100, 1024 on the large-k route (device form: always; host form: when min(k, rows) > 56), with one query (a streaming
    collect) and six (above 16384 rows one sweep of the batched kernel); the same k by the all-keys path (largek_sampled = 0), and
    k = 2000, which only that path takes, on corpora of more than 2000 rows."""
    n = ref.n
    for k in (57, 100, 1024):
        for nq in (1, 6):
            def route(r, nq=nq):
                assert r["largek_finish"] >= 1 and r["largek_tau"] >= 1, r
                assert r["largek_collect"] == (0 if n > 16384 and nq >= 5 else 1), r
            check_device(ref, c, ctl, qs[:nq], k, (note, "largek", nq, k), route, trace)
            got, r = ran(ctx, lambda: c.search(qs[:nq], top_k=k))
            assert (r["largek_finish"] >= 1) == (min(k, n) > 56), r
            check_host(ref, got, ref.topk(qs[:nq], k), (note, "largek-host", nq, k), trace)
        with tuned(ctx, largek_sampled=0):
            got, r = ran(ctx, lambda: c.search(qs[:2], top_k=k))
        assert r["largek_finish"] == 0 and r["scan"] >= (2 if min(k, n) > 56 else 1), r
        check_host(ref, got, ref.topk(qs[:2], k), (note, "allkeys", k), trace)
    if n > 2000:
        got, r = ran(ctx, lambda: c.search(qs[:2], top_k=2000))
        assert r["largek_finish"] == 0 and r["scan"] >= 2, r
        check_host(ref, got, ref.topk(qs[:2], 2000), (note, "k2000"), trace)


def routes_k3_rows(ctx, c, ctl, ref, qs, mode, note, trace=None):
    """K3 from the f32 rows (gemm_image = 0: a corpus that has an image reads its rows all the same) with 8, 33 and 130 queries: the
    row-register kernel in its three nomination modes (valid16 / want32, the address clamp, the tile minima of the bootstrap level
    from 33 tiles on -- and the plan without it), the level kernel with f32 and bf16 x 3 MFMAs, the LDS-row kernel (8 and 33
    queries; 130 take the level kernel).  The counter says that a batched kernel ran; which one follows from the tuning keys."""
    for boot in ((1, 0) if mode.startswith("rowreg") and ref.n > 1024 else (1,)):
        with tuned(ctx, gemm_bootstrap=boot, gemm_image=0, **k3_keys(mode)):
            for nq in (8, 33, 130):
                for k in (1, 10):
                    check_topk(ref, c, ctl, qs[:nq], k, (note, "K3", mode, boot, nq, k), on_gemm, trace)


def routes_image(ctx, c, ctl, ref, qs, mode, note, trace=None):
    """K3 from the operand image (both corpora have one): the row-register kernel reads the tile that straddles `rows`; and one and
    three queries scanned from the image."""
    assert c.image_bytes > 0 and ctl.image_bytes > 0
    with tuned(ctx, **k3_keys(mode)):
        for nq in (8, 33, 130):
            check_topk(ref, c, ctl, qs[:nq], 10, (note, "image", mode, nq), on_gemm, trace)
        with tuned(ctx, image_scan_min_rows=1):
            for nq in (1, 3):
                check_topk(ref, c, ctl, qs[:nq], 10, (note, "image-scan", mode, nq), on_gemm, trace)


@pytest.fixture(scope="module")
def piped():
    """A context of its own on a torch stream, with the async select pipeline on (as tests/test_gpu_scan_pairing.py sets one up)."""
    import torch
    import semtools_amd as smt

    stream = torch.cuda.Stream(torch.device("cuda:0"))
    ctx = smt.Context(0, stream=stream.cuda_stream)
    ctx.set_tuning("async_select", 1)
    yield torch, ctx, stream
    ctx.set_tuning("async_select", 0)
    ctx.close()


def _series(torch, ctx, stream, c, qd, calls, k, mid=None):
    """`calls` back-to-back one-query device calls; mid(): run on the host after half of them, without a synchronise of ours."""
    with torch.cuda.stream(stream):
        rows = torch.full((calls, k), -7, dtype=torch.int64, device="cuda:0")
        dist = torch.full((calls, k), -7.0, dtype=torch.float64, device="cuda:0")
        st = torch.full((calls,), 7, dtype=torch.int32, device="cuda:0")
    stream.synchronize()
    before = ctx.scan_pairs()
    for i in range(calls):
        if mid is not None and i == calls // 2:
            mid()
        c.search_topk_device(qd[i % len(qd)].data_ptr(), 1, k, 0, rows[i].data_ptr(), dist[i].data_ptr(), out_status_ptr=st[i:].data_ptr())
    ctx.synchronize()
    counts = tuple(int(y - x) for x, y in zip(before, ctx.scan_pairs()))
    return rows.cpu().numpy().view(np.uint64), dist.cpu().numpy(), st.cpu().numpy(), counts


def _check_series(ref_of_call, rows, dist, st, ctl_st, k, note):
    for i in range(len(rows)):
        ref, want = ref_of_call(i)
        ref.inside(rows[i], (note, i))
        assert st[i] in (0, 1, 2) and st[i] <= ctl_st[i], (note, i, st.tolist(), ctl_st.tolist())
        if st[i] == 0:
            S.check_list(rows[i], dist[i], want[i % 5][0], want[i % 5][1], k, (note, i))


def routes_series(piped, c, ctl, ref, qs, pair, note, trace=None):
    """Series of eight back-to-back device-form calls through the scan_overlap pipeline, alone and sharing corpus passes (scan_pair;
    the deciding block waits up to 2 ms for its partner's descriptor).  Whether a later call may be taken along also depends on a
    query of the caller's stream made on the host, which races with the GPU: as in tests/test_gpu_scan_pairing.py the pairs are
    counted over 120 calls -- fifteen series, every one of them checked -- and every call must be accounted for.
    The unpaired variant has no counter of its own (scan_pair = 0 counts nothing): that its calls take the overlap branch is shown by
    the paired variant, whose accounting 2 x paired + alone == calls is kept inside that branch, for the same calls on the same context."""
    torch, ctx, stream = piped
    k, calls, series = 10, 8, 15 if pair else 2
    qd = torch.from_numpy(qs[:5]).to("cuda:0")
    torch.cuda.synchronize()
    want = ref.topk(qs[:5], k)
    paired = alone = absorbed = 0
    with tuned(ctx, scan_overlap=1, scan_pair=pair, scan_pair_wait_us=2000 if pair else 0):
        ctl_st = _series(torch, ctx, stream, ctl, qd, calls, k)[2]
        for s in range(series):
            rows, dist, st, counts = _series(torch, ctx, stream, c, qd, calls, k)
            paired, alone, absorbed = paired + counts[0], alone + counts[1], absorbed + counts[2]
            _check_series(lambda i: (ref, want), rows, dist, st, ctl_st, k, (note, "series", pair, s))
            if trace is not None:
                trace.append((rows.tobytes(), dist.tobytes(), st.tobytes()))
    if pair:
        assert paired > 0 and 2 * paired + alone == series * calls and absorbed == paired, (note, paired, alone, absorbed)
    else:
        assert (paired, alone, absorbed) == (0, 0, 0), note


# ================================================================================================ A: past both ends of an adopted corpus
@pytest.mark.parametrize("n", D.SIZES_A)
def test_a_scan_kernel(gpu_ctx, qs, n):
    both_flavours(gpu_ctx, n, lambda a, trace: routes_scan(gpu_ctx, a.c, a.ctl, a.ref, qs, ("A", n), trace))


@pytest.mark.parametrize("n", [2049, 4097])
@pytest.mark.parametrize("steal", [1, 4])
def test_a_scan_kernel_with_rows_dealt_while_it_runs(gpu_ctx, qs, n, steal):
    both_flavours(gpu_ctx, n, lambda a, trace: routes_steal(gpu_ctx, a.c, a.ctl, a.ref, qs, steal, ("A", n), trace))


@pytest.mark.parametrize("pair", [0, 1], ids=["unpaired", "paired"])
@pytest.mark.parametrize("n", D.SIZES_A)
def test_a_overlapped_series_of_one_query_calls(piped, qs, n, pair):
    both_flavours(piped[1], n, lambda a, trace: routes_series(piped, a.c, a.ctl, a.ref, qs, pair, ("A", n), trace))


@pytest.mark.parametrize("n", D.SIZES_A)
def test_a_threshold_scan_and_batched_threshold_sweep(gpu_ctx, qs, n):
    both_flavours(gpu_ctx, n, lambda a, trace: routes_threshold(gpu_ctx, a.c, a.ctl, a.ref, qs, ("A", n), trace))


@pytest.mark.parametrize("n", [63, 65, 129, 2049, 4097, D.N_LARGEK])
def test_a_large_k(gpu_ctx, qs, n):
    """Below the 16384-row shortcut border and above it (a sampled threshold: the virtual-row map of the sample)."""
    both_flavours(gpu_ctx, n, lambda a, trace: routes_large_k(gpu_ctx, a.c, a.ctl, a.ref, qs, ("A", n), trace))


@pytest.mark.parametrize("mode", list(K3_FROM_ROWS))
@pytest.mark.parametrize("n", D.SIZES_A)
def test_a_batched_kernels_from_the_rows(gpu_ctx, qs, n, mode):
    both_flavours(gpu_ctx, n, lambda a, trace: routes_k3_rows(gpu_ctx, a.c, a.ctl, a.ref, qs, mode, ("A", n), trace))


@pytest.mark.parametrize("mode", list(K3_FROM_IMAGE))
@pytest.mark.parametrize("n", D.SIZES_A)
def test_a_batched_kernel_and_one_query_from_the_image(gpu_ctx, qs, n, mode):
    """After smt_corpus_prepack on the adopted view: pack_image_kernel's last tile straddles `rows` (inside[u], the zero-row mask)."""
    def body(a, trace):
        a.c.prepack()
        a.ctl.prepack()
        routes_image(gpu_ctx, a.c, a.ctl, a.ref, qs, mode, ("A", n), trace)
    both_flavours(gpu_ctx, n, body)


@pytest.mark.parametrize("n", [n for n in D.SIZES_A if n % 32])
def test_a_image_tile_that_straddles_the_row_count(gpu_ctx, n):
    """pack_image_kernel packs the rows of the last tile that lie at or past `rows` as ZERO rows, whatever the memory there holds
    (inside[u]).  The sweep masks those rows a second time (valid16), so no answer shows it; the tile itself does: its 16 KiB and
    its zero-row mask are the same bytes with finite guards, with NaN / Inf guards and on the control corpus."""
    tile, got = (n - 1) // 32, {}
    for flavour in ("finite", "nonfinite"):
        a = Adopted(gpu_ctx, n, flavour)
        try:
            a.c.prepack()
            a.ctl.prepack()
            got[flavour] = a.c.image_tile(tile)
            got["control"] = a.ctl.image_tile(tile)
        finally:
            a.close()
    past = (0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF
    assert any(got["control"][0])                                  # (not an empty comparison: the tile holds rows)
    for name, (data, zero_mask) in got.items():
        assert zero_mask & past == past, (name, hex(zero_mask))
        assert zero_mask == got["control"][1] and data == got["control"][0], name


def _ivf_search(ix, ctx, qs, k, nlist, ranges=None):
    """(host answers, device answers) at nprobe = nlist and rerank = 512: with lists of <= 512 rows every row is re-scored."""
    import torch

    host = ix.search(qs, top_k=k, nprobe=nlist, rerank=512, ranges=ranges)
    qd = torch.from_numpy(np.ascontiguousarray(qs)).to("cuda:0")
    rows = torch.full((len(qs), k), -7, dtype=torch.int64, device="cuda:0")
    dist = torch.full((len(qs), k), -7.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ix.search_device(qd.data_ptr(), len(qs), k, nlist, 512, 0, rows.data_ptr(), dist.data_ptr(), ranges=ranges)
    ctx.synchronize()
    torch.cuda.synchronize()
    return host, (rows.cpu().numpy().view(np.uint64), dist.cpu().numpy())


def _check_ivf(ref, ix, ctx, qs, nlist, note, ranges=None, trace=None, sizes=None):
    """sizes: the candidate rows per list (default: the list sizes) -- at most 512, so that rerank = 512 re-scores every one."""
    assert (ix.list_sizes() if sizes is None else sizes).max() <= 512
    for k in (10, 56):
        (host, (rows, dist)), r = ran(ctx, lambda: _ivf_search(ix, ctx, qs, k, nlist, ranges))
        assert r["ivf_adc"] >= 2 and (ranges is None or r["ivf_mask"] >= 2), r
        want = ref.topk(qs, k)
        check_host(ref, host, want, (note, k, "host"), trace)
        for i in range(len(qs)):
            ref.inside(rows[i], (note, k, i, "device"))
            S.check_list(rows[i], dist[i], want[i][0], want[i][1], k, (note, k, i, "device"))
        if trace is not None:
            trace.append((rows.tobytes(), dist.tobytes()))


@pytest.mark.parametrize("local_pca", [False, True], ids=["pq", "lpca"])
@pytest.mark.parametrize("n", [2049, 4097])
def test_a_ivf_index_on_the_adopted_view(gpu_ctx, qs, n, local_pca):
    """An IVF index built on the adopted view, both codings, every list probed and every row re-scored: the exact answer."""
    import semtools_amd as smt

    def body(a, trace):
        ix = smt.IvfPq(a.c, nlist=32, train_iters=4, local_pca=local_pca)
        try:
            _check_ivf(a.ref, ix, gpu_ctx, qs[:9], 32, ("A-ivf", n, local_pca), trace=trace)
        finally:
            ix.close()
    both_flavours(gpu_ctx, n, body)


# ================================================================================================ B: inside the corpus, outside the ranges
class Filtered:
    def __init__(self, ctx, name, unit_only=False):
        import semtools_amd as smt

        self.ranges = D.range_lists()[name]
        self.emb, self.elig = D.layout_b(D.N_B, self.ranges, seed=11, unit_only=unit_only)
        self.ref = Ref(self.emb[self.elig], self.elig)
        self.c = smt.Corpus(ctx)
        self.c.append(self.emb)                       # n rows and G guards ...
        self.c.truncate(D.N_B)                        # ... which stay in the corpus' memory

    def close(self):
        self.c.close()


@pytest.fixture(scope="module", params=["dense", "sparse"])
def filtered(request, gpu_ctx):
    f = Filtered(gpu_ctx, request.param)
    f.name = request.param
    yield f
    f.close()


def test_b_scan_kernel_threshold_scan_and_large_k(gpu_ctx, qs, filtered):
    """The chunk table built from the ranges (row0 | valid rows per 4-row chunk) under K2 with 1 .. 4 queries, under K4, and under
    the large-k routes at k = 100 and k = 2000 (the virtual-row maps of topk_large.hip and largek.hip)."""
    f = filtered
    n_el = len(f.elig)
    with tuned(gpu_ctx, gemm_min_nq=8):
        for nq in (1, 2, 3, 4):
            for k in (1, 10, 56):
                got, r = ran(gpu_ctx, lambda: f.c.search(qs[:nq], top_k=k, ranges=f.ranges))
                on_scan(r)
                check_host(f.ref, got, f.ref.topk(qs[:nq], k), ("B-K2", f.name, nq, k))
    for md in D.MAX_DISTANCES:
        got, r = ran(gpu_ctx, lambda: f.c.search(qs[:2], top_k=3, max_distance=md, ranges=f.ranges))
        assert r["scan"] == 2 and r["gemm_thr"] == 0, r
        check_host(f.ref, got, f.ref.under(qs[:2], md), ("B-K4", f.name, md))
    for k in (100, 2000):
        for nq in (1, 6):
            got, r = ran(gpu_ctx, lambda: f.c.search(qs[:nq], top_k=k, ranges=f.ranges))
            if min(k, n_el) > 1024:                             # the all-keys path, one pass per query
                assert r["largek_finish"] == 0 and r["scan"] >= nq, r
            else:
                assert min(k, n_el) > 56 and r["largek_collect"] >= 1 and r["largek_finish"] >= 1, r
            check_host(f.ref, got, f.ref.topk(qs[:nq], k), ("B-largek", f.name, nq, k))
    with tuned(gpu_ctx, largek_sampled=0):
        got, r = ran(gpu_ctx, lambda: f.c.search(qs[:2], top_k=100, ranges=f.ranges))
        assert r["largek_finish"] == 0 and r["scan"] >= 2, r   # one all-keys pass per query
        check_host(f.ref, got, f.ref.topk(qs[:2], 100), ("B-allkeys", f.name))


@pytest.mark.parametrize("image", [False, True], ids=["rows", "image"])
def test_b_batched_kernels_and_the_kept_range_set(gpu_ctx, qs, image):
    """Filtered K3: the dense list over the TILE table (tile | mask of the wanted rows) on the row-register kernel, from the rows and
    from the image; both lists over the CHUNK table on the LDS-row kernel; MODE_WORKSPACE with max_distance; and the second and
    third call over the same list, which answer from the range set kept on the device."""
    f = Filtered(gpu_ctx, "dense")
    g = Filtered(gpu_ctx, "sparse")
    try:
        if image:
            f.c.prepack()
            g.c.prepack()
            assert f.c.image_bytes > 0
        assert f.c.range_sets() == (0, 0, 0)
        for sight in range(3):
            for nq in (8, 33, 130):
                got, r = ran(gpu_ctx, lambda: f.c.search(qs[:nq], top_k=10, ranges=f.ranges))
                on_gemm(r)
                check_host(f.ref, got, f.ref.topk(qs[:nq], 10), ("B-K3-tiles", image, sight, nq))
            got, r = ran(gpu_ctx, lambda: f.c.search(qs[:1], top_k=10, ranges=f.ranges))     # one query: the set's chunk table
            on_scan(r)
            check_host(f.ref, got, f.ref.topk(qs[:1], 10), ("B-K2-kept", image, sight))
        kept, hits, builds = f.c.range_sets()
        assert kept == 1 and builds == 1 and hits >= 6, (kept, hits, builds)
        # WHICH table: with gemm_ldsrow = 0 a filtered batch that does not get the row-register kernel (over the tile table) is
        # refused by the batched path and answered by the scan kernel -- so a batched launch here is the tile table ...
        with tuned(gpu_ctx, gemm_ldsrow=0):
            got, r = ran(gpu_ctx, lambda: f.c.search(qs[:33], top_k=10, ranges=f.ranges))
            assert r["gemm"] > 0, r
            check_host(f.ref, got, f.ref.topk(qs[:33], 10), ("B-K3-tiles-only", image))
            # ... and the sparse list, which takes the chunk table otherwise, gets no batched launch at all
            got, r = ran(gpu_ctx, lambda: g.c.search(qs[:33], top_k=10, ranges=g.ranges))
            assert r["gemm"] == 0 and r["scan"] > 0, r
            check_host(g.ref, got, g.ref.topk(qs[:33], 10), ("B-K2-instead-of-chunks", image))
        for md in D.MAX_DISTANCES:
            for nq in (1, 8):
                got, r = ran(gpu_ctx, lambda: f.c.search(qs[:nq], top_k=5, max_distance=md, mode=1, ranges=f.ranges))
                (on_scan if nq == 1 else on_gemm)(r)
                check_host(f.ref, got, D.expected_workspace(f.ref.allowed, f.ref.ids, qs[:nq], 5, md), ("B-workspace", image, md, nq))
        for mode in ("rowreg-f16x2", "rowreg-f16x1", "ldsrow"):
            with tuned(gpu_ctx, **k3_keys(mode)):
                got, r = ran(gpu_ctx, lambda: f.c.search(qs[:33], top_k=10, ranges=f.ranges))
                on_gemm(r)
                check_host(f.ref, got, f.ref.topk(qs[:33], 10), ("B-K3", mode, image))
        # the sparse list does not fill its tiles: the LDS-row kernel gathers 4-row chunks
        for sight in range(2):
            got, r = ran(gpu_ctx, lambda: g.c.search(qs[:33], top_k=10, ranges=g.ranges))
            on_gemm(r)
            check_host(g.ref, got, g.ref.topk(qs[:33], 10), ("B-K3-chunks", image, sight))
    finally:
        f.close()
        g.close()


@pytest.mark.parametrize("local_pca", [False, True], ids=["pq", "lpca"])
def test_b_ivf_index_searched_inside_the_ranges(gpu_ctx, qs, local_pca, tmp_path):
    """smt_ivfpq_search_ranges, host and device form, every list probed: ivf_range_mask_kernel.  (The index refuses rows that are
    not unit rows, and it is built over the decoys too: they are the centre itself here, without the power-of-two scales.  The
    decoys share one list, which is long; what rerank = 512 has to cover is the IN-RANGE rows of a list, read from the saved index.)"""
    import semtools_amd as smt
    from tests import ivf_ref

    for name in ("dense", "sparse"):
        f = Filtered(gpu_ctx, name, unit_only=True)
        ix = smt.IvfPq(f.c, nlist=32, train_iters=4, local_pca=local_pca)
        try:
            ix.save(tmp_path / f"{name}.ivf")
            idx = ivf_ref.read_index(tmp_path / f"{name}.ivf")
            wanted = D.in_ranges(D.N_B, f.ranges)[idx["ids"].astype(np.int64)]
            off = idx["offsets"].astype(np.int64)
            sizes = np.array([int(wanted[off[l]:off[l + 1]].sum()) for l in range(32)])
            assert sizes.sum() == len(f.elig)
            _check_ivf(f.ref, ix, gpu_ctx, qs[:9], 32, ("B-ivf", name, local_pca), ranges=f.ranges, sizes=sizes)
        finally:
            ix.close()
            f.close()


@pytest.mark.parametrize("transport", ["peer", "copy"])
def test_b_ranges_across_the_borders_of_three_shards(qs, transport):
    """Three logical shards (consecutive views of one buffer, guards behind the last), the dense list's ranges crossing both shard
    borders: every shard localises the list.  (Which kernel answers on a shard is that shard's own dispatch, confirmed for one GPU in
    the tests above; the shards' counters are not read here.)"""
    import torch
    import semtools_amd as smt

    n = D.N_B
    ranges = D.range_lists()["dense"]
    emb, elig = D.layout_b(n, ranges, seed=11)
    ref = Ref(emb[elig], elig)
    x = torch.from_numpy(emb).to("cuda:0")
    torch.cuda.synchronize()
    cut = -(-n // 3)
    cuts = [0, cut, 2 * cut, n]
    g = smt.Group.logical(0, 3)
    g.set_transport(transport)
    sc = smt.ShardedCorpus(g, device_ptrs=[x[cuts[i]:cuts[i + 1]].data_ptr() for i in range(3)],
                           shard_rows=[cuts[i + 1] - cuts[i] for i in range(3)])
    try:
        assert g.transport == transport and sc.rows == n
        for sight in range(2):
            for nq, k in ((1, 10), (4, 10), (33, 10), (2, 100)):
                got = sc.search(qs[:nq], top_k=k, ranges=ranges)
                check_host(ref, got, ref.topk(qs[:nq], k), ("B-shards", transport, sight, nq, k))
        got = sc.search(qs[:2], top_k=3, max_distance=D.MAX_DISTANCES[1], ranges=ranges)
        check_host(ref, got, ref.under(qs[:2], D.MAX_DISTANCES[1]), ("B-shards-K4", transport))
    finally:
        sc.close()
        g.close()


# ================================================================================================ C: beyond `rows`, inside the capacity
def _owned_after_truncation(ctx, n):
    import semtools_amd as smt

    rows = D.layout_c(n, seed=300 + n)
    c = smt.Corpus(ctx)
    c.append(rows)
    c.prepack()                                   # the library's own image, built while the decoys were rows ...
    c.truncate(n)                                 # ... and kept current from here on
    assert c.rows == n and c.image_bytes > 0
    return c, rows[:n]


def _routes_c(ctx, c, ctl, ref, qs, note):
    """Every route of layout A that runs on a plain context, on the owned corpus `c` as it stands (the overlapped series need a
    context of their own: test_c_overlapped_series_at_three_row_counts).  The stolen-rows scan needs 128 chunks: not at n = 33."""
    assert c.rows == ctl.rows == ref.n and c.rows % 32 != 0
    last = (c.rows - 1) // 32                     # the image tile that straddles `rows`: zero rows behind them, as on the control
    assert c.image_tile(last) == ctl.image_tile(last), note
    routes_scan(ctx, c, ctl, ref, qs, note)
    for steal in (1, 4):
        if (ref.n + 3) // 4 >= 2 * 64 * steal:
            routes_steal(ctx, c, ctl, ref, qs, steal, note)
    routes_threshold(ctx, c, ctl, ref, qs, note)
    routes_large_k(ctx, c, ctl, ref, qs, note)
    for mode in K3_FROM_ROWS:
        routes_k3_rows(ctx, c, ctl, ref, qs, mode, note)
    for mode in K3_FROM_IMAGE:
        routes_image(ctx, c, ctl, ref, qs, mode, note)


def _stages_c(ctx, n):
    """The three states of layout C, one after the other on ONE owned corpus: yields (stage, corpus, control, rows allowed), and the
    caller may search between the yields.  truncated: n rows, decoys behind them; appended: ten ordinary rows over the first decoys,
    the last of them the nearest row of every query; compacted: smt_corpus_compact with a keep list that leaves the row count
    mid-tile -- the stale rows behind it are copies of kept rows, that nearest row among them, so a leak is an id >= rows."""
    c, allowed = _owned_after_truncation(ctx, n)
    ctl = D.control(ctx, allowed)
    ctl.prepack()
    try:
        yield "truncated", c, ctl, allowed
        more = D.allowed_rows(10, seed=400 + n)
        more[9] = D.near_row()
        if c.rows == n:                                               # (a caller may have appended them itself, between two calls)
            assert c.append(more) == n and ctl.append(more) == n
        allowed = np.ascontiguousarray(np.concatenate([allowed, more]))
        assert c.rows == ctl.rows == n + 10
        yield "appended", c, ctl, allowed
        keep = [(0, n // 2), (n // 2 + 5, n + 10)]
        with tuned(ctx, compact_bounce_rows=64 if n > 1000 else 65536):
            assert c.compact(keep) == n + 10 - (n // 2 + 5)
        kept = np.ascontiguousarray(np.concatenate([allowed[b:e] for b, e in keep]))
        assert c.rows == len(kept) == n + 5 and c.rows % 32 != 0
        ctl.close()
        ctl = D.control(ctx, kept)
        ctl.prepack()
        assert Ref(kept).topk(D.queries(1), 2)[0][0][0] == n + 4      # the nearest row is the last one: its stale copy sits at n + 9
        yield "compacted", c, ctl, kept
    finally:
        c.close()
        ctl.close()


@pytest.mark.parametrize("n", D.SIZES_C)
def test_c_truncated_owned_corpus_then_append_then_compact(gpu_ctx, qs, n):
    """An owned corpus after a truncation, after an append and after a compaction (_stages_c): the routes of layout A at each."""
    for stage, c, ctl, allowed in _stages_c(gpu_ctx, n):
        _routes_c(gpu_ctx, c, ctl, Ref(allowed), qs, ("C", stage, n))


@pytest.mark.parametrize("pair", [0, 1], ids=["unpaired", "paired"])
@pytest.mark.parametrize("n", D.SIZES_C)
def test_c_overlapped_series_at_three_row_counts(piped, qs, n, pair):
    """The overlapped series on ONE corpus pointer at three row counts (n, n + 10, n + 5), with decoys or stale copies right behind
    each: a scan takes a partner only when corpus AND row count agree (pair_decide).  One series straddles the append -- four calls
    over n rows, the append, four calls over n + 10 rows, no synchronise of the test's in between: a call from before the append
    that took one from after it along would answer it over the wrong rows."""
    torch, ctx, stream = piped
    k = 10
    qd = torch.from_numpy(qs[:5]).to("cuda:0")
    torch.cuda.synchronize()
    more = D.allowed_rows(10, seed=400 + n)
    more[9] = D.near_row()
    for stage, c, ctl, allowed in _stages_c(ctx, n):
        ref = Ref(allowed)
        routes_series(piped, c, ctl, ref, qs, pair, ("C", stage, n))
        if stage == "truncated":
            after = Ref(np.ascontiguousarray(np.concatenate([allowed, more])))
            want = (ref.topk(qs[:5], k), after.topk(qs[:5], k))
            with tuned(ctx, scan_overlap=1, scan_pair=pair, scan_pair_wait_us=2000 if pair else 0):
                ctl_st = _series(torch, ctx, stream, ctl, qd, 8, k, mid=lambda: ctl.append(more))[2]
                rows, dist, st, counts = _series(torch, ctx, stream, c, qd, 8, k, mid=lambda: c.append(more))
            _check_series(lambda i: (ref, want[0]) if i < 4 else (after, want[1]), rows, dist, st, ctl_st, k, ("C-straddle", n, pair))
            assert (rows[4:, 0] == np.uint64(n + 9)).all() and (rows[:4] < np.uint64(n)).all()   # the appended near row, and only after
            paired, alone, absorbed = counts
            assert (2 * paired + alone == 8 and absorbed == paired) if pair else counts == (0, 0, 0), counts


@pytest.mark.parametrize("local_pca", [False, True], ids=["pq", "lpca"])
def test_c_ivf_index_follows_a_compaction(gpu_ctx, qs, local_pca):
    """The same with an index carried through smt_ivfpq_compact: every list probed, every row re-scored, no id >= rows."""
    import semtools_amd as smt

    n = 4097
    c, allowed = _owned_after_truncation(gpu_ctx, n)
    more = D.allowed_rows(10, seed=400 + n)
    more[9] = D.near_row()
    c.append(more)
    allowed = np.ascontiguousarray(np.concatenate([allowed, more]))
    ix = smt.IvfPq(c, nlist=32, train_iters=4, local_pca=local_pca)
    try:
        _check_ivf(Ref(allowed), ix, gpu_ctx, qs[:9], 32, ("C-ivf", local_pca))
        keep = [(0, n // 2), (n // 2 + 5, n + 10)]
        moved, dropped = ix.compact(keep)
        assert (moved, dropped) == (n + 10 - (n // 2 + 5), 5) and c.rows == n + 5
        kept = np.ascontiguousarray(np.concatenate([allowed[b:e] for b, e in keep]))
        _check_ivf(Ref(kept), ix, gpu_ctx, qs[:9], 32, ("C-ivf-compacted", local_pca))
        check_host(Ref(kept), c.search(qs[:4], top_k=10), Ref(kept).topk(qs[:4], 10), ("C-ivf-corpus", local_pca))
    finally:
        ix.close()
        c.close()


# ================================================================================================ sharded, adopted
@pytest.mark.parametrize("transport", ["peer", "copy"])
def test_adopted_shards_with_decoys_between_them(qs, transport):
    """smt_sharded_corpus_from_device over three views of one buffer, G decoy rows in front of, between and behind the shards: the
    per-shard row counts.  One query, a batch and k = 100; the device-resident form with its status words against those of the
    same shards with ZERO rows for guards.  (Which kernel answers on a shard is that shard's own dispatch, confirmed for one GPU in
    the tests above; the shards' counters are not read here.)"""
    import torch
    import semtools_amd as smt

    sizes = (1301, 33, 1666)
    buf, first, rows = D.layout_shards(sizes, seed=21)
    ref = Ref(rows)
    x = torch.from_numpy(buf).to("cuda:0")
    torch.cuda.synchronize()
    g = smt.Group.logical(0, 3)
    g.set_transport(transport)
    sc = smt.ShardedCorpus(g, device_ptrs=[x[f:f + s].data_ptr() for f, s in zip(first, sizes)], shard_rows=sizes)
    blank = buf.copy()                                            # the control: the same shards, zero rows (distance 1) for guards
    inside = np.zeros(len(buf), dtype=bool)
    for f, s in zip(first, sizes):
        inside[f:f + s] = True
    blank[~inside] = 0.0
    xc = torch.from_numpy(blank).to("cuda:0")
    torch.cuda.synchronize()
    ctl = smt.ShardedCorpus(g, device_ptrs=[xc[f:f + s].data_ptr() for f, s in zip(first, sizes)], shard_rows=sizes)
    try:
        assert sc.rows == sum(sizes) and g.transport == transport
        for nq, k in ((1, 1), (1, 10), (4, 56), (33, 10), (130, 10), (1, 100), (3, 100)):
            got = sc.search(qs[:nq], top_k=k)
            check_host(ref, got, ref.topk(qs[:nq], k), ("shards", transport, nq, k))
        for md in D.MAX_DISTANCES:
            got = sc.search(qs[:2], top_k=3, max_distance=md)
            check_host(ref, got, ref.under(qs[:2], md), ("shards-K4", transport, md))
        # the device-resident form: one packed [2][k] answer per query on local device 0
        qd = torch.from_numpy(qs[:3]).to("cuda:0")

        def device_form(corpus, k):
            out = torch.full((3, 2, k), -7, dtype=torch.int64, device="cuda:0")
            st = torch.full((3,), 7, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            for i in range(3):
                corpus.search_topk_device([qd[i].data_ptr()] * 3, 1, k, [out[i].data_ptr(), None, None], [st[i:].data_ptr(), None, None])
            g.synchronize()
            torch.cuda.synchronize()
            return out.cpu().numpy(), st.cpu().numpy()

        for k in (10, 100):
            o, st = device_form(sc, k)
            ctl_st = device_form(ctl, k)[1]
            want = ref.topk(qs[:3], k)
            for i in range(3):
                r, d = o[i, 0].view(np.uint64), np.ascontiguousarray(o[i, 1]).view(np.float64)
                ref.inside(r, ("shards-device", transport, k, i))
                assert st[i] in (0, 1, 2) and st[i] <= ctl_st[i], (transport, k, i, st.tolist(), ctl_st.tolist())
                if st[i] == 0:
                    S.check_list(r, d, want[i][0], want[i][1], k, ("shards-device", transport, k, i))
    finally:
        ctl.close()
        sc.close()
        g.close()
