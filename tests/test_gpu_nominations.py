"""K3's certificate rests on |nominating f32 distance - exact distance| <= F32_ERR_* (common.h) for the kernel that NOMINATED the row.
Here that is measured on the kernels that produce answers: smt_debug_nominations builds the launch arguments of a real batched call,
takes the route the tuning picks (gemm_route, shared with launch_gemm_topk), runs the production query preparation and ONE level over
all tiles, and returns every nomination -- value, how often the pair was written, raw counts with the padding queries.

Per kernel family (the fixture forces it through tuning keys, and every call ASSERTS the route it got):
  * bound: every nominated distance within the mode's F32_ERR_* of the float64 distance (tests/nominate_ref.py), on the four random
    corpus kinds of test_gpu_batched.py and on the constructed worst-case rows, which must still be adversarial in the mode they target;
  * completeness: with +inf thresholds every scanned (row, query) pair exactly once and nothing else, over ragged row and query
    counts, zero rows and a zero query, range lists through the tile table and the chunk table;
  * thresholds and the LDS nomination buffer: finite thresholds, buffered and direct, a sweep that overflows the 208-entry buffer;
  * the bit equalities the sources document: image == f32 rows for the fp16 modes, gemm_level_kernel == smt_debug_batched_scores."""
import functools

import numpy as np
import pytest

from tests import nominate_ref as ref
from tests import synth
from tests.nomination_families import ARITH_CODE, FAMILIES, LDSROW, LEVEL, ROWREG, Family, restore, set_family

pytestmark = pytest.mark.gpu


@pytest.fixture(params=list(FAMILIES))
def fam(request, gpu_ctx):
    f = Family(request.param, gpu_ctx)
    set_family(gpu_ctx, f)
    yield f
    restore(gpu_ctx)


# ---------------------------------------------------------------------------------------------- inputs (made once, never changed)
N = 2048
KINDS = ("isotropic", "all-positive", "spiky", "unnormalised", "constructed")
N_BASE = 128


@functools.lru_cache(maxsize=None)
def inputs(kind):
    """(rows f32, queries f32 [33], exact float64 [rows][33]); query 32 is the zero query."""
    rng = np.random.default_rng(5)
    if kind == "constructed":
        # as test_gpu_batched.py's constructed test, 128 rows per generator: 5 scales x 2 generators = 1280 rows
        rng = np.random.default_rng(2024)
        base16 = ref.worst_case_rows_f16x2(rng, N_BASE)
        base_bf = ref.worst_case_rows_bf16x3(rng, N_BASE)
        scales = np.array([1.0, 2.0 ** 5, 2.0 ** -7, 3.7, 1e-3])
        rows = np.concatenate([base16 * s for s in scales] + [base_bf * s for s in scales])
        qs = [base16[:8], base_bf[:8]]
        for base in (base16, base_bf):
            mag = np.where(base[8:16] != 0, 0.5 + rng.random((8, 256)), 0.0)
            qs.append(np.sign(base[8:16]) * mag / 16.0)
        qs = np.concatenate(qs)
    else:
        iso = synth.unit_rows(N, seed=77, dup_frac=0, zero_frac=0)
        pos = np.abs(rng.standard_normal((N, 256)))
        spiky = rng.standard_normal((N, 256)) * np.exp(3.0 * rng.standard_normal((N, 256)))
        scaled = rng.standard_normal((N, 256)) * 37.5
        rows = {"isotropic": iso, "all-positive": pos, "spiky": spiky, "unnormalised": scaled}[kind]
        qs = np.concatenate([synth.unit_query(9, nq=8), np.abs(rng.standard_normal((8, 256))),
                             rng.standard_normal((8, 256)) * np.exp(3.0 * rng.standard_normal((8, 256))),
                             rng.standard_normal((8, 256)) * 1e-3])
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    qs = np.ascontiguousarray(np.concatenate([qs, np.zeros((1, 256))]), dtype=np.float32)
    assert len(rows) <= 2048 and len(qs) == 33
    exact = ref.exact_distances(rows, qs)
    for a in (rows, qs, exact):
        a.setflags(write=False)
    return rows, qs, exact


@functools.lru_cache(maxsize=None)
def ragged_inputs():
    """2048 isotropic rows with zero rows at tile positions 0, 15, 16, 31 of tiles 0 and 2 and in the last tile; 64 queries, query 1
    the zero query; the float64 distances."""
    rows = synth.unit_rows(N, seed=1234, dup_frac=0, zero_frac=0).copy()
    rows[[0, 15, 16, 31, 64, 79, 80, 95, 2047]] = 0.0
    qs = synth.unit_query(4321, nq=64).copy()
    qs[1] = 0.0
    exact = ref.exact_distances(rows, qs)
    for a in (rows, qs, exact):
        a.setflags(write=False)
    return rows, qs, exact


# ---------------------------------------------------------------------------------------------- the bound
@pytest.mark.parametrize("kind", KINDS)
def test_every_nominated_distance_is_within_the_certificate_bound(fam, kind):
    """|nominating - exact| <= F32_ERR_* for EVERY pair the production kernel nominates (all of them: +inf thresholds), no fraction of
    the bound, no pair left out.  Measured maxima of the first run: profiles/nomination_errors.json."""
    rows, qs, exact = inputs(kind)
    c = fam.corpus(rows)
    try:
        got = fam.run_all(c, qs).astype(np.float64)
    finally:
        c.close()
    err = np.abs(got - exact)
    i, q = np.unravel_index(np.argmax(err), err.shape)
    print(f"NOMERR {fam.name} {kind} max {err.max():.4e} ratio {err.max() / fam.bound:.4f} (row {i}, query {q})")
    assert err.max() <= fam.bound, (fam.name, kind, err.max(), fam.bound, int(i), int(q))
    # the zero query: exactly 1 against every (nonzero) row
    assert np.all(got[:, 32] == 1.0)
    if kind == "constructed":
        # still adversarial in the mode it targets: the thresholds test_gpu_batched.py asserts for the 64-thread restatement
        n = N_BASE
        own16 = max(err[blk * n + i, i] for blk in range(3) for i in range(8))
        own_bf = max(err[(5 + blk) * n + i, 8 + i] for blk in range(3) for i in range(8))
        matched16 = max(err[blk * n + 8 + i, 16 + i] for blk in range(3) for i in range(8))
        print(f"NOMADV {fam.name} own16 {own16:.4e} matched16 {matched16:.4e} own_bf {own_bf:.4e}")
        if fam.arith == "f16x2":
            assert own16 > 3.0e-4 and matched16 > 2.0e-4
        elif fam.arith == "f16x1":
            assert own16 > 6.0e-4
        elif fam.arith == "bf16x3":
            assert own_bf > 2.0e-5


# ---------------------------------------------------------------------------------------------- completeness
def _query_counts(fam):
    return [nq for nq in (1, 31, 32, 33, 64) if fam.nq_min <= nq <= fam.nq_max]


def test_all_pass_nominates_every_scanned_pair_exactly_once(fam):
    """Row counts 1, 31, 32, 33, 2047, 2048 x query counts 1, 31, 32, 33, 64 (those the variant takes): every (row, query) pair is
    nominated once, the raw count is the row count, the padding queries of the last query tile get nothing, and every value --
    zero rows and the zero query included -- is within the bound.  Straight to the lists and through the waves' LDS buffers, which
    an all-pass tile overflows at once (32 x 32 pairs against 208 slots): short tiles and few queries stay inside them."""
    rows, qs, exact = ragged_inputs()
    for n in (1, 31, 32, 33, 2047, 2048):
        c = fam.corpus(rows[:n])
        try:
            for nq, buffered in [(nq, b) for nq in _query_counts(fam) for b in (False, True)]:
                dist, hits, counts = fam.run(c, qs[:nq], buffered=buffered)
                where = (fam.name, n, nq, buffered)
                assert dist.shape == (n, nq) and np.all(hits == 1), (where, np.argwhere(hits != 1)[:5].tolist())
                assert np.all(counts[:nq] == n) and np.all(counts[nq:] == 0), (where, counts.tolist())
                assert not np.isnan(dist).any(), where
                err = np.abs(dist.astype(np.float64) - exact[:n, :nq])
                assert err.max() <= fam.bound, (where, err.max())
                if nq > 1:   # the zero query: 0 against a zero row, 1 against the rest, exactly
                    assert np.array_equal(dist[:, 1], exact[:n, 1].astype(np.float32)), where
                zero_rows = [r for r in (0, 15, 16, 31, 64, 79, 80, 95, 2047) if r < n]
                assert np.all(dist[zero_rows, 0] == 1.0), where
        finally:
            c.close()


# range lists over a 2048-row corpus: (name, ranges, fills its tiles well enough for the row-register tile table)
RANGE_SETS = [
    ("inside-a-tile", [(5, 27), (37, 70), (100, 191)], True),                      # begin and end inside tiles, two ranges in one tile
    ("empty-tiles", [(0, 40), (200, 300), (1000, 1100), (2040, 2048)], True),      # whole tiles between the ranges are never visited
    ("one-row-dense", [(3, 4), (10, 60), (64, 65), (70, 128), (2047, 2048)], True),
    ("one-row-sparse", [(3, 4), (31, 32), (32, 33), (500, 501), (2047, 2048)], False),   # 4 tiles for 5 rows: the chunk table
    ("ragged-chunks", [(1, 6), (6, 7), (9, 18), (33, 34), (62, 67), (1999, 2048)], True),    # touching ranges, one across a tile border
]


@pytest.mark.parametrize("name,ranges,dense", RANGE_SETS, ids=[r[0] for r in RANGE_SETS])
def test_filtered_calls_nominate_exactly_the_rows_inside_the_ranges(fam, name, ranges, dense):
    """Range-filtered calls walk the row-register kernel's TILE TABLE when the ranges fill their tiles (and the family is a
    row-register one), else the LDS-row kernel's CHUNK TABLE (gemm_rowreg = 0, or a sparse list): every pair inside the ranges
    once, nothing outside, counts = the rows scanned.  The level kernel has no filtered form: the call must refuse."""
    from semtools_amd import _lib as L

    rows, qs, exact = ragged_inputs()
    c = fam.corpus(rows)
    inside = np.zeros(N, dtype=bool)
    for b, e in ranges:
        inside[b:e] = True
    try:
        if fam.family == LEVEL:
            with pytest.raises(L.SmtError):
                c.debug_nominations(qs[:8], ranges=ranges)
            return
        if fam.family == ROWREG and not dense:
            # a sparse list leaves the row-register route: bf16 x 3 from the f32 rows in the LDS-row kernel
            route = LDSROW | (ARITH_CODE["bf16x3"] << 4) | 0x200
            bound = ref.F32_ERR["bf16x3"]
        else:
            route, bound = fam.route(filtered=True), fam.bound
        for rep, nq in enumerate(_query_counts(fam) * 2):     # (a list seen twice is KEPT on the corpus: later calls read its kept table)
            dist, hits, counts = fam.run(c, qs[:nq], ranges=ranges, buffered=bool(rep & 1), route=route)
            where = (fam.name, name, nq, rep)
            assert np.all(hits[inside] == 1) and np.all(hits[~inside] == 0), (where, np.argwhere(hits != inside[:, None])[:5].tolist())
            assert np.isnan(dist[~inside]).all() and not np.isnan(dist[inside]).any(), where
            assert np.all(counts[:nq] == inside.sum()) and np.all(counts[nq:] == 0), (where, counts.tolist())
            err = np.abs(dist[inside].astype(np.float64) - exact[inside, :nq])
            assert err.max() <= bound, (where, err.max())
    finally:
        c.close()


def test_the_hook_refuses_what_the_candidate_lists_cannot_hold(gpu_ctx):
    import semtools_amd as smt
    from semtools_amd import _lib as L

    rows, qs, _ = ragged_inputs()
    c = smt.Corpus(gpu_ctx)
    c.append(np.concatenate([rows, rows[:1]]))                       # 2049 rows
    try:
        with pytest.raises(L.SmtError):
            c.debug_nominations(qs[:8])                              # more than 2048 scanned rows
        with pytest.raises(L.SmtError):
            c.debug_nominations(np.concatenate([qs, qs[:1]]), ranges=[(0, 100)])   # 65 queries
        dist, hits, counts, _ = c.debug_nominations(qs[:8], ranges=[(1, 2049)])    # 2048 scanned rows of 2049: fine
        assert np.all(hits[1:] == 1) and np.all(hits[0] == 0) and np.all(counts[:8] == 2048)
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------- thresholds, the LDS buffer
def _ulp32(t):
    t = np.asarray(t, dtype=np.float32)
    return np.nextafter(t, np.float32(np.inf)) - t


@pytest.mark.parametrize("share,blocks,qsplit", [(0.05, 0, 1), (0.05, 2, 1), (0.15, 0, 0), (0.5, 0, 1), (0.5, 2, 0)],
                         ids=["5pct", "5pct-2blocks", "15pct-spill-second-tile", "50pct-spill", "50pct-2blocks"])
def test_finite_thresholds_direct_and_buffered(fam, gpu_ctx, share, blocks, qsplit):
    """Per query tau = the `share` quantile of its all-pass distances, one of them exactly.  5 %: what a level admits, the buffered path proper (with two
    blocks a wave sweeps four row tiles and flushes its buffer in the next row phase, not only at the end).  15 % with the query
    tiles unsplit: 32 rows x 32 queries x 0.15 = 154 nominations per product, the second product of a sweep finds the 208-entry
    buffer full and spills to the lists.  50 %: 512 per product, every product spills.  Both with buffered 0 and 1:
      * every pair whose all-pass distance is <= tau is nominated;
      * no pair whose all-pass distance is > tau + 4 ulp(tau) is (score_threshold lowers the bar by two ulps on purpose, and the
        score-domain compare rounds once more);
      * each nominated value is bit-equal to the all-pass value of the pair;
      * the raw count is the size of the set: nothing lost, nothing twice."""
    rows, qs, _ = ragged_inputs()
    nq = fam.nq_max
    q = qs[:nq]
    c = fam.corpus(rows)
    try:
        gpu_ctx.set_tuning("gemm_blocks", blocks)
        gpu_ctx.set_tuning("gemm_qsplit", qsplit)
        allpass, hits, _ = fam.run(c, q)
        assert np.all(hits == 1)
        # (method "lower": tau IS one of the query's all-pass distances, as the thresholds level_select_kernel publishes are -- the
        # pairs at exactly tau are the ones a score-domain compare loses first)
        tau = np.quantile(allpass, share, axis=0, method="lower").astype(np.float32)
        assert all(np.any(allpass[:, i] == tau[i]) for i in range(nq))
        must = allpass <= tau[None, :]
        may_not = allpass.astype(np.float64) > (tau.astype(np.float64) + 4.0 * _ulp32(tau).astype(np.float64))[None, :]
        for buffered in (False, True):
            dist, hits, counts = fam.run(c, q, tau=tau, buffered=buffered)
            where = (fam.name, share, blocks, qsplit, buffered)
            got = hits > 0
            assert np.all(hits <= 1), (where, "a pair was written twice", np.argwhere(hits > 1)[:5].tolist())
            assert np.all(got[must]), (where, "lost", int((must & ~got).sum()), np.argwhere(must & ~got)[:5].tolist())
            assert not np.any(got & may_not), (where, "above the threshold", np.argwhere(got & may_not)[:5].tolist())
            assert np.array_equal(dist[got].view(np.uint32), allpass[got].view(np.uint32)), where
            assert np.array_equal(counts[:nq], got.sum(axis=0)) and np.all(counts[nq:] == 0), (where, counts.tolist(), got.sum(axis=0).tolist())
            assert np.isnan(dist[~got]).all(), where
        if share >= 0.15 and fam.family == ROWREG:
            per_sweep = must.reshape(N // 32, 32, nq).sum(axis=(1, 2)).max() / (1 if qsplit == 0 else (nq + 31) // 32)
            assert per_sweep > 208, per_sweep                     # the case really overflows a wave's buffer
    finally:
        gpu_ctx.set_tuning("gemm_blocks", 0)
        gpu_ctx.set_tuning("gemm_qsplit", 1)
        c.close()


# ---------------------------------------------------------------------------------------------- documented bit equalities
@pytest.mark.parametrize("mode,arith", [(2, "f16x2"), (3, "f16x1")])
@pytest.mark.parametrize("kind", ["isotropic", "spiky", "constructed", "ragged"])
def test_fp16_modes_nominate_the_same_bits_from_the_image_and_from_the_rows(gpu_ctx, mode, arith, kind):
    """pack_image_kernel writes the operands the row phase of gemm_rowreg_kernel<MODE> builds, with the same arithmetic in the same
    order (gemm_rowreg.hip): the nominations of both forms must agree bit for bit -- zero rows, a ragged last tile and a filtered call
    included."""
    import semtools_amd as smt

    rows, qs, _ = ragged_inputs() if kind == "ragged" else inputs(kind)
    rows = rows[:2047 - 32] if kind == "ragged" else rows
    qs = qs[:33]
    c = smt.Corpus(gpu_ctx)
    c.append(rows)
    c.prepack(True)
    try:
        gpu_ctx.set_tuning("gemm_nominate", mode)
        code = ARITH_CODE[arith] << 4
        for ranges in (None, [(5, 27), (37, 70), (100, 191)]):
            out = {}
            for image in (0, 1):
                gpu_ctx.set_tuning("gemm_image", image)
                dist, hits, counts, route = c.debug_nominations(qs, ranges=ranges)
                assert route == ROWREG | code | (0x100 if image else 0) | (0x200 if ranges else 0), hex(route)
                out[image] = (dist, hits, counts)
            assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
            a, b = out[0][0].view(np.uint32), out[1][0].view(np.uint32)
            assert np.array_equal(a, b), (kind, mode, ranges, int((a != b).sum()), np.argwhere(a != b)[:5].tolist())
    finally:
        gpu_ctx.set_tuning("gemm_nominate", 0)
        gpu_ctx.set_tuning("gemm_image", 1)
        c.close()


@pytest.mark.parametrize("bf16", [1, 0], ids=["bf16x3", "f32"])
@pytest.mark.parametrize("kind", ["isotropic", "all-positive", "unnormalised", "constructed"])
def test_level_kernel_nominates_the_bits_of_debug_batched_scores(gpu_ctx, bf16, kind):
    """gemm_debug_scores_kernel is documented as "the same operand preparation and MFMA sequence as gemm_level_kernel"
    (gemm_topk.hip): what test_gpu_batched.py measures on the restatement is what the level kernel nominates, bit for bit."""
    import semtools_amd as smt

    rows, qs, _ = inputs(kind)
    qs = qs[:32]
    c = smt.Corpus(gpu_ctx)
    c.append(rows)
    try:
        gpu_ctx.set_tuning("gemm_bf16x3", bf16)
        gpu_ctx.set_tuning("gemm_rowreg", 0)
        gpu_ctx.set_tuning("gemm_ldsrow", 0)
        gpu_ctx.set_tuning("gemm_nominate", 1)
        dist, hits, counts, route = c.debug_nominations(qs)
        assert route == LEVEL | ((0 if bf16 else 3) << 4), hex(route)
        assert np.all(hits == 1)
        restated = c.debug_batched_scores(qs)
        a, b = dist.view(np.uint32), restated.view(np.uint32)
        diff = np.abs(dist.astype(np.float64) - restated.astype(np.float64))
        print(f"LEVELEQ {'bf16x3' if bf16 else 'f32'} {kind} differing {int((a != b).sum())} of {a.size} max |diff| {diff.max():.3e}")
        assert np.array_equal(a, b), (kind, bf16, int((a != b).sum()), float(diff.max()), np.argwhere(a != b)[:5].tolist())
    finally:
        for k in ("gemm_bf16x3", "gemm_rowreg", "gemm_ldsrow"):
            gpu_ctx.set_tuning(k, 1)
        gpu_ctx.set_tuning("gemm_nominate", 0)
        c.close()
