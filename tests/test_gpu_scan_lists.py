"""The scan stage (K2) judged by what it WRITES: the block lists, before the select's guard band and f64 re-score can hide a wrong one.

smt_debug_scan_lists runs the synchronous path of launch_scan_topk up to the select -- the same functions, under the current tuning --
with the list area preset to 0x5A and an extra, guard set behind the call's; smt_debug_scan_ring reads the list set of an earlier call
of the one-query pipeline.  tests/scan_ref.py restates the deal of chunk_deal.h and judges the lists against float64 distances
(tests/test_scan_ref_cpu.py shows on the CPU that the judge bites).  Every call asserts the route word it got.

  * the bound: |d32 - d64| <= F32_ERR_SCAN (common.h) for EVERY (row, query) pair, on launch shapes where each pair comes back
    exactly once -- every instantiation of scan_topk_kernel a search can reach, unfiltered and filtered.  The maxima go to
    scan_nomination_errors.json in the directory SMT_PROFILE_OUT names (committed as profiles/scan_nomination_errors.json);
  * the lists at the shapes where the deal goes wrong: tiny and ragged corpora, one / two / the default number of blocks, 1 to 16
    waves, four list sizes, 1 to 7 queries, range lists with chunks short by 1, 2 and 3 rows, rows dealt at run time (STEAL), and two
    tie cases whose every key is known in advance;
  * the grouped kernels (scan_pair_kernel, scan_wide_kernel, scan_deep_kernel) byte for byte against scan_topk_kernel<1, 4>;
  * the refusals of both hooks."""
import functools
import json
import os

import numpy as np
import pytest

from tests import scan_ref as R
from tests import synth
from tests.threshold_ref import _ranges_layout

pytestmark = pytest.mark.gpu

DEFAULTS = dict(scan_blocks=0, scan_threads=512, scan_unroll=4, scan_nontemporal=1, scan_steal=0, scan_steal_pct=6, guard_band=8)


@functools.lru_cache(maxsize=None)
def num_cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def scan(ctx, corpus, rows, qs, d64, top_k, name, blocks=0, threads=512, U=4, nt=1, ranges=None, steal=0, guard=8, ties=False, cap=None):
    """One hook call at one launch shape, judged: the grid is the planned one, the route the expected one, every list what the scan
    stage promises.  Returns (keys, case, report)."""
    keys_tuning = dict(scan_blocks=blocks, scan_threads=threads, scan_unroll=U, scan_nontemporal=nt, scan_steal=steal,
                       scan_steal_pct=50 if steal else 6, guard_band=guard)
    case = R.make_case(name, rows, qs, top_k, blocks, threads, U, num_cus(), ranges, guard, steal, d64=d64, ties=ties, cap=cap)
    try:
        for k, v in keys_tuning.items():
            ctx.set_tuning(k, v)
        keys, route = corpus.debug_scan_lists(case.qs, top_k, ranges=ranges)
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_tuning(k, v)
    where = (name, dict(blocks=blocks, threads=threads, U=U, nt=nt, nq=case.nq, top_k=top_k, steal=steal, guard=guard,
                        filtered=ranges is not None))
    assert keys.shape == (case.nq + 1, case.blocks, case.kp), (where, keys.shape, (case.nq + 1, case.blocks, case.kp))
    want = R.route_word(U, nt, threads, case.nq, ranges is not None, case.steal)
    assert route == want, (where, hex(route), hex(want))
    rep = R.check_lists(keys, d64, case.deals, case.kp, steal=case.steal, where=where)
    return keys, case, rep


# ================================================================================================ the bound, every pair measured
BOUND_KINDS = ("isotropic", "all-positive", "spiky", "unnormalised", "constructed", "scaled-domain")
NQS = (1, 2, 3, 4, 7)


@functools.lru_cache(maxsize=None)
def bound_inputs(kind):
    """(rows, queries, float64 distances): the five kinds of tests/test_gpu_nominations.py (33 queries, the last the zero query), and
    2048 rows of the domain test's scaled corpus with queries scaled to both ends of the domain."""
    if kind == "scaled-domain":
        from tests.test_gpu_domain import _queries, _scaled_corpus

        rows = np.ascontiguousarray(_scaled_corpus(2048, seed=33)[1])
        qs = np.concatenate([_queries(16, 34), np.zeros((1, 256), dtype=np.float32)])
        return rows, qs, R.exact_distances(rows, qs)
    from tests.test_gpu_nominations import inputs

    return inputs(kind)


def _ragged_ranges(n):
    """threshold_ref._ranges_layout cut to n rows: ranges of 1 .. 9 rows, touching and far apart, the last one ending on the last row."""
    if n >= 2003:
        return _ranges_layout(n)
    return [r for r in _ranges_layout(2003) if r[1] <= n - 9] + [(n - 5, n)]


@pytest.mark.parametrize("kind", BOUND_KINDS)
def test_every_distance_a_scan_kernel_writes_is_within_the_certificate_bound(gpu_ctx, kind, tmp_path_factory):
    """scan_threads = 64, scan_blocks = 32, top_k = 56 (k' = 64): a block owns at most 64 rows at 2, 4 and 8 rows per chunk (exactly
    64 of 2048; the constructed kind has 1280), so every list holds ALL of its block's rows and every (row, query) pair of a call
    comes back exactly once -- check_lists asserts that, and the band on each of them.  The bound is the project's constant, not a
    figure taken from these runs."""
    import semtools_amd as smt

    rows, qs, exact = bound_inputs(kind)
    n = len(rows)
    routes = [("U%d-nt%d" % (U, nt), dict(U=U, nt=nt)) for U in (2, 4, 8) for nt in (0, 1)]
    routes += [("filtered-%s-nt%d" % (name, nt), dict(nt=nt, ranges=rg)) for name, rg in (("all", [(0, n)]), ("ragged", _ragged_ranges(n)))
               for nt in (0, 1)]
    maxima = {}
    c = smt.Corpus(gpu_ctx)
    c.append(rows)
    try:
        at = 0
        for rname, kw in routes:
            for nq in NQS:
                idx = [(at + 5 * j) % len(qs) for j in range(nq)]      # (5 and 33 / 17 are coprime: every query gets its turns)
                at += 1
                if nq == 7 and len(qs) - 1 not in idx:
                    idx[3] = len(qs) - 1                               # the zero query rides in every seven-query call
                _, case, rep = scan(gpu_ctx, c, rows, qs[idx], exact[:, idx], 56, kind, blocks=32, threads=64, **kw)
                assert case.kp == 64 and max(len(r) for d in case.deals for r in d.rows) <= 64
                key = "%s-nq%d" % (rname, nq)
                maxima[key] = rep.max_err
                print("SCANERR %s %s max %.4e ratio %.4f %s" % (kind, key, rep.max_err, rep.max_err / R.F32_ERR_SCAN, rep.worst))
    finally:
        c.close()
    _record(kind, maxima, os.environ.get("SMT_PROFILE_OUT") or str(tmp_path_factory.getbasetemp()))
    assert max(maxima.values()) <= R.F32_ERR_SCAN


def _record(kind, maxima, out_dir):
    """scan_nomination_errors.json in out_dir (the environment's SMT_PROFILE_OUT, else the session's temporary directory):
    {corpus kind: {route: max |d32 - d64|}}, one kind per test case."""
    path = os.path.join(out_dir, "scan_nomination_errors.json")
    os.makedirs(out_dir, exist_ok=True)
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc.setdefault("bound", R.F32_ERR_SCAN)
    doc.setdefault("max_abs_error", {})[kind] = {k: float("%.4e" % v) for k, v in sorted(maxima.items())}
    doc["worst"] = max(v for per in doc["max_abs_error"].values() for v in per.values())
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("SCANERR written to", path)


# ================================================================================================ the lists, where the deal goes wrong
ROWS = (1, 2, 3, 4, 5, 7, 33, 1000, 4099)
TOP_KS = (1, 10, 24, 56)
N_MAX = ROWS[-1]


@functools.lru_cache(maxsize=None)
def list_inputs():
    rows = synth.unit_rows(N_MAX, seed=8201, dup_frac=0.0, zero_frac=0.0)
    qs = synth.unit_query(8202, nq=7)
    exact = R.exact_distances(rows, qs)
    for a in (rows, qs, exact):
        a.setflags(write=False)
    return rows, qs, exact


@pytest.fixture(scope="module")
def corpora(gpu_ctx):
    import semtools_amd as smt

    rows = list_inputs()[0]
    made = {}
    for n in ROWS:
        made[n] = smt.Corpus(gpu_ctx)
        made[n].append(rows[:n])
    yield made
    for c in made.values():
        c.close()


@pytest.mark.parametrize("n", ROWS)
def test_unfiltered_lists(gpu_ctx, corpora, n):
    """scan_blocks 1, 2 and the default x scan_threads 64, 128, 512, 1024 x 1, 2, 3, 4, 7 queries, top_k 1, 10, 24, 56 and 2, 4, 8 rows
    per chunk in turn; then every (top_k, query count) pair at the default shape, and guard_band = 16 once."""
    rows, qs, exact = list_inputs()
    i, cap = 0, R.Cap()
    for blocks in (1, 2, 0):
        for threads in (64, 128, 512, 1024):
            for nq in NQS:
                scan(gpu_ctx, corpora[n], rows[:n], qs[:nq], exact[:n, :nq], TOP_KS[i % 4], n, blocks=blocks, threads=threads,
                     U=(4, 2, 8)[i % 3], nt=i & 1, cap=cap)
                i += 1
    for top_k in TOP_KS:
        for nq in NQS:
            scan(gpu_ctx, corpora[n], rows[:n], qs[:nq], exact[:n, :nq], top_k, n, cap=cap)
    _, case, _ = scan(gpu_ctx, corpora[n], rows[:n], qs[:3], exact[:n, :3], 24, n, guard=16, cap=cap)
    assert case.kp == 40
    cap.check(n)


@pytest.mark.parametrize("n", ROWS)
def test_filtered_lists(gpu_ctx, corpora, n):
    """One range over everything, a range ending on the last row, and from 33 rows on ranges of 1 .. 9 rows: chunks short by 1, 2
    and 3 rows.  (A list seen twice is kept on the corpus: later calls read its kept chunk table.)"""
    rows, qs, exact = list_inputs()
    layouts = [[(0, n)], [(n - 1, n)], [(0, 0), (0, max(1, n // 2)), (n - 1 if n > 1 else 1, n)]]
    if n >= 33:
        layouts.append(_ragged_ranges(n) if n >= 1000 else [(1, 2), (2, 4), (4, 7), (9, 14), (15, 22), (24, n)])
    i, cap = 0, R.Cap()
    for ranges in layouts:
        deal = R.Deal(n, 1, 1, 4, ranges)
        if len(ranges) > 4:
            assert {1, 2, 3} <= set(deal.cnt.tolist()) and deal.scanned[-1] == n - 1
        for blocks, threads in ((1, 64), (2, 128), (0, 512), (2, 1024)):
            for nq in NQS:
                scan(gpu_ctx, corpora[n], rows[:n], qs[:nq], exact[:n, :nq], TOP_KS[i % 4], n, blocks=blocks, threads=threads, nt=i & 1,
                     U=(4, 2, 8)[i % 3], ranges=ranges, cap=cap)
                i += 1
    cap.check(n)


@pytest.mark.parametrize("n", [1000, 4099])
def test_lists_of_rows_dealt_at_run_time(gpu_ctx, corpora, n):
    """scan_steal = 1 with scan_steal_pct = 50 at one and two blocks of 512 threads: which block scans a row of the last groups is
    decided while the kernel runs, so the lists are judged together (structure, band, the merged top-k' against the f64 top-k')."""
    rows, qs, exact = list_inputs()
    i = 0
    for blocks in (1, 2):
        for nq in NQS:
            for top_k in TOP_KS[i % 2::2]:
                _, case, _ = scan(gpu_ctx, corpora[n], rows[:n], qs[:nq], exact[:n, :nq], top_k, n, blocks=blocks, steal=1)
                assert case.steal
            i += 1
    _, case, _ = scan(gpu_ctx, corpora[n], rows[:n], qs[:1], exact[:n, :1], 56, n, steal=1)
    assert not case.steal                                          # the default grid leaves too few chunks per block: the static deal


SHAPES = [(2, 512, 4, None), (1, 64, 8, None), (2, 128, 2, None), (2, 512, 4, "all"), (0, 512, 4, None)]


@pytest.mark.parametrize("blocks,threads,U,ranges", SHAPES)
def test_tie_case_zero_query(gpu_ctx, corpora, blocks, threads, U, ranges):
    """dist_f32 returns exactly 1.0 for every non-zero row under a zero query: every list is the lowest rows of its block, ascending
    -- ties are broken by row, not rejected, whichever wave met the row first."""
    rows, qs, exact = list_inputs()
    for nq, zero_at in ((1, 0), (2, 1), (3, 2), (4, 0), (7, 5)):
        q = qs[:nq].copy()
        q[zero_at] = 0.0
        d64 = exact[:, :nq].copy()
        d64[:, zero_at] = 1.0
        keys, case, _ = scan(gpu_ctx, corpora[N_MAX], rows, q, d64, 10, "tie-zero-query", blocks=blocks, threads=threads, U=U,
                             ranges=[(0, N_MAX)] if ranges else None, ties=True)
        want = R.zero_query_lists(case.deals[zero_at], case.kp)
        assert np.array_equal(keys[zero_at], want), (nq, zero_at, np.argwhere(keys[zero_at] != want)[:5].tolist())


@pytest.mark.parametrize("blocks,threads,U,ranges", SHAPES[:4])
def test_tie_case_planted_rows_and_zero_rows(gpu_ctx, blocks, threads, U, ranges):
    """k' - 3 planted near rows per block, zero rows at exactly 1.0, every other row beyond 1.05: every list is the near rows and then
    the three LOWEST zero rows of its block."""
    import semtools_amd as smt

    waves = threads // 64
    for nq in NQS:
        # (every pass of these query counts has the same number of slots, so a call has ONE deal: the corpus is planted for it)
        ku = 4 if ranges else R.kernel_unroll(U, R.passes(nq)[0][2])
        assert len({slots for _, _, slots in R.passes(nq)}) == 1
        deal = R.Deal(N_MAX, blocks, waves, ku)
        emb, q, near, zeros = R.planted_tie_corpus(deal, 18, seed=8300 + nq)
        qs = np.stack([q * np.float32(2.0 ** (j - 3)) for j in range(nq)])
        d64 = R.exact_distances(emb, qs)
        c = smt.Corpus(gpu_ctx)
        c.append(emb)
        try:
            keys, case, _ = scan(gpu_ctx, c, emb, qs, d64, 10, "tie-planted", blocks=blocks, threads=threads, U=U,
                                 ranges=[(0, N_MAX)] if ranges else None, ties=True)
        finally:
            c.close()
        want, last3 = R.planted_tie_rows(near, zeros)
        for qi in range(nq):
            for b in range(blocks):
                assert set(R.key_rows(keys[qi, b]).tolist()) == want[b], (nq, qi, b)
                assert np.array_equal(keys[qi, b, -3:], (R.ONE_BITS << np.uint64(32)) | last3[b].astype(np.uint64)), (nq, qi, b)


# ================================================================================================ grouped kernels, byte for byte
CALLS = 24
LIMITS = [("scan_pair", 1), ("scan_pair", 3), ("scan_take", 7), ("scan_deep", 15)]
TINY = (1, 2, 3, 4, 5, 7, 33)
ADV_SEEDS = (55, 56, 57)


class _Setup:
    pass


@pytest.fixture(scope="module")
def S():
    """A context of its own on a torch stream that can pair (tests/test_gpu_scan_groups.py says why some cannot), the corpora of
    tests/test_gpu_scan_group_loop.py."""
    import torch
    import semtools_amd as smt
    from tests.test_gpu_nearties import adversarial_corpus
    from tests.test_gpu_scan_deep import _series
    from tests.test_gpu_scan_group_loop import DUP_ROWS, N_PLANT, ZERO_ROWS, _planted

    s = _Setup()
    s.torch, s.series = torch, _series
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(67)
    x = torch.randn(N_PLANT, 256, device=dev, generator=g)
    x /= x.norm(dim=1, keepdim=True)
    qs = torch.randn(24, 256, device=dev, generator=g)
    qs /= qs.norm(dim=1, keepdim=True)
    xz = x.clone()
    for r in ZERO_ROWS:
        xz[r] = 0.0
    for r in DUP_ROWS[1:]:
        xz[r] = xz[DUP_ROWS[0]]
    qz = qs.clone()
    qz[0::4] = 0.0                                                 # the zero query and
    qz[1::4] = xz[DUP_ROWS[0]]                                     # a query that IS a (duplicated) row, in every group
    emb_plant, qs_plant, _ = _planted()
    s.host = {"plant": emb_plant, "zero": xz.cpu().numpy(), "tiny": x.cpu().numpy()}
    s.queries = {"plant": torch.from_numpy(np.tile(qs_plant, (6, 1))).to(dev), "zero": qz, "tiny": qs}
    s.keep = [x, xz, torch.from_numpy(emb_plant).to(dev)]
    for seed in ADV_SEEDS:
        q_adv, emb_adv, _ = adversarial_corpus(seed=seed)
        s.host[("adv", seed)] = emb_adv
        s.queries[("adv", seed)] = torch.from_numpy(np.ascontiguousarray(q_adv, dtype=np.float32)).to(dev).reshape(1, 256)
    s.qs = qs
    torch.cuda.synchronize()
    for attempt in range(6):
        s.stream = torch.cuda.Stream(dev)
        s.ctx = smt.Context(0, stream=s.stream.cuda_stream)
        s.corpora = {1000: smt.Corpus(s.ctx, device_ptr=x.data_ptr(), rows=1000)}
        s.ctx.set_tuning("async_select", 1)
        if _series(s, (1000,), 8, (10,), 15)[2][0] > 0 or attempt == 5:   # (the last one stays: the tests then say what is wrong)
            break
        s.corpora[1000].close()
        s.ctx.close()
    for n in TINY:
        s.corpora[("tiny", n)] = smt.Corpus(s.ctx, device_ptr=x.data_ptr(), rows=n)
    s.corpora["plant"] = smt.Corpus(s.ctx, device_ptr=s.keep[2].data_ptr(), rows=N_PLANT)
    s.corpora["zero"] = smt.Corpus(s.ctx, device_ptr=xz.data_ptr(), rows=N_PLANT)
    for seed in ADV_SEEDS:
        s.corpora[("adv", seed)] = smt.Corpus(s.ctx)
        s.corpora[("adv", seed)].append(s.host[("adv", seed)])
    s.ctx.set_tuning("async_select", 1)
    yield s
    for c in s.corpora.values():
        c.close()
    s.ctx.close()


GROUPED = ["plant", "zero"] + [("adv", seed) for seed in ADV_SEEDS] + [("tiny", n) for n in TINY]


@pytest.mark.parametrize("key,limit", LIMITS, ids=["%s-%d" % kl for kl in LIMITS])
@pytest.mark.parametrize("name", GROUPED, ids=[str(g) if isinstance(g, str) else "%s-%d" % g for g in GROUPED])
def test_grouped_kernels_write_the_plain_kernels_lists(S, name, key, limit):
    """A series of 24 queued one-query calls under each limit (scan_pair_wait_us = 2000, so that passes of several calls form), then
    every call's list set read back through smt_debug_scan_ring and compared, byte for byte, with what scan_topk_kernel<1, 4> writes
    for the same query at the same grid, block size and k' (smt_debug_scan_lists; it reuses the scratch, so the ring is read first).
    The documented claim "bit for bit the arithmetic of scan_topk_kernel<1, 4>", checked on the lists themselves."""
    kind = name if isinstance(name, str) else name[0]
    queries = S.queries[name if kind == "adv" else kind]
    rows = S.corpora[name].rows
    formed = 0
    for top_k in (1, 10, 24):
        kp = R.kprime(top_k)
        blocks = R.planned_blocks(rows, 0, 512, 4, num_cus())
        _, deep, counts, wide = S.series(S, (name,), CALLS, (top_k,), limit, queries=queries, key=key)
        ring = [S.ctx.debug_scan_ring(CALLS - 1 - i, blocks * kp) for i in range(CALLS)]
        formed += sum(deep[1:]) if key == "scan_deep" else sum(wide[1:]) if key == "scan_take" else counts[0]
        assert counts[0] + counts[1] + counts[2] == CALLS, counts
        plain = {}
        for i in range(CALLS):
            qi = i % len(queries)
            if qi not in plain:
                keys, route = S.corpora[name].debug_scan_lists(queries[qi].cpu().numpy(), top_k)
                assert route == R.route_word(4, 1, 512, 1) and keys.shape == (2, blocks, kp), (hex(route), keys.shape)
                assert (keys[1] == R.POISON).all()
                plain[qi] = keys[0].reshape(-1)
            assert ring[i].tobytes() == plain[qi].tobytes(), (name, key, limit, top_k, i, np.flatnonzero(ring[i] != plain[qi])[:8].tolist())
    assert formed > 0, (name, key, limit)                          # passes of more than one call formed, in the family the limit selects


# ================================================================================================ refusals
def test_refusals_of_the_list_hook(gpu_ctx, corpora):
    from semtools_amd import _lib as L

    rows, qs, _ = list_inputs()
    c = corpora[1000]
    for bad_k in (0, 57):
        with pytest.raises(L.SmtError):
            c.debug_scan_lists(qs[:1], bad_k)
    with pytest.raises(L.SmtError):
        c.debug_scan_lists(np.zeros((0, 256), dtype=np.float32), 10)           # no query
    with pytest.raises(L.SmtError):
        c.debug_scan_lists(np.concatenate([qs, qs[:2]]), 10)                    # nine queries
    with pytest.raises(L.SmtError):
        c.debug_scan_lists(qs[:1], 10, ranges=[(5, 5)])                         # nothing to scan
    with pytest.raises(L.SmtError):
        c.debug_scan_lists(qs[:1], 10, ranges=[(0, 1001)])                      # a range past the corpus
    keys, _ = c.debug_scan_lists(qs[:2], 10)
    need = keys.size
    with pytest.raises(L.SmtError):
        c.debug_scan_lists(qs[:2], 10, cap_keys=need - 1)                       # one key short
    again, _ = c.debug_scan_lists(qs[:2], 10, cap_keys=need)
    assert again.tobytes() == keys.tobytes()


def test_refusals_of_the_ring_hook(S):
    import semtools_amd as smt
    from semtools_amd import _lib as L

    fresh = smt.Context(0)
    try:
        with pytest.raises(L.SmtError):
            fresh.debug_scan_ring(0, 16)                                        # no pipeline call yet
    finally:
        fresh.close()
    S.series(S, (1000,), 4, (10,), 0, queries=S.qs, key="scan_deep")            # four calls of the overlap pipeline, none grouped
    assert len(S.ctx.debug_scan_ring(3, 18)) == 18
    with pytest.raises(L.SmtError):
        S.ctx.debug_scan_ring(32, 18)                                           # the ring holds 32 sets
    with pytest.raises(L.SmtError):
        S.ctx.debug_scan_ring(0, 512 * 64 + 1)                                  # more than a set
    S.corpora[1000].debug_scan_lists(S.qs[:1].cpu().numpy(), 10)                # a synchronous scan reuses the scratch
    with pytest.raises(L.SmtError):
        S.ctx.debug_scan_ring(0, 18)
