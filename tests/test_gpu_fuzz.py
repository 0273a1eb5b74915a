"""GPU: randomised shapes (hypothesis) -- rows, k, ranges, duplicates, zero rows, query count --
K2/K3/threshold/large-k all against the oracle.  Small sizes, many cases."""
import os

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

from oracle import oracle as orc
from tests import synth
from tests.compare import assert_topk_tie_aware, reference_distances
from tests.soundness import assert_sound, host_both, oracle_topk

pytestmark = pytest.mark.gpu
SCALE = int(os.environ.get("SMT_FUZZ_SCALE", "1"))  # SMT_FUZZ_SCALE=10: ten times the examples (soak run)
# The default run draws the SAME examples every time (a suite that stops at its first failure must not depend on the day's dice);
# soak runs (SMT_FUZZ_SCALE > 1) draw fresh ones -- thousands per test passed on the last day of round 5.
DERANDOMIZE = SCALE == 1


def _oracle(emb, q, k, thr=None):
    res = orc.search_documents(emb, [len(emb)], q, 0, k, thr, accurate=True)
    return [r["match_line"] for r in res], [r["distance"] for r in res]


@settings(max_examples=40 * SCALE, deadline=None, derandomize=DERANDOMIZE, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(n=st.integers(1, 3000), k=st.integers(1, 80), nq=st.sampled_from([1, 1, 2, 3, 5, 8, 9, 33]),
       seed=st.integers(0, 10_000), dup=st.sampled_from([0.0, 0.05, 0.5]), use_ranges=st.booleans())
def test_topk_random_shapes(gpu_ctx, n, k, nq, seed, dup, use_ranges):
    import semtools_amd as smt

    emb = synth.unit_rows(n, seed=seed, dup_frac=dup, zero_frac=0.01)
    qs = synth.unit_query(seed + 1, nq=nq)
    c = smt.Corpus(gpu_ctx)
    c.append(emb)
    ranges, idx = None, np.arange(n)
    if use_ranges and n > 4:
        rng = np.random.default_rng(seed)
        cuts = np.sort(rng.choice(np.arange(1, n), size=min(6, n - 1), replace=False))
        segs = [(int(a), int(b)) for a, b in zip(cuts[::2], cuts[1::2])]
        if segs:
            ranges = segs
            idx = np.concatenate([np.arange(a, b) for a, b in segs])
    got = c.search(qs, top_k=k, ranges=ranges)
    for i in range(nq):
        orows, odist = _oracle(emb[idx], qs[i], k)
        assert got[i][0].tolist() == idx[np.array(orows, dtype=np.int64)].tolist() if orows else got[i][0].size == 0
        assert np.array_equal(got[i][1], np.array(odist))
        if i == 0:  # and the tie-aware contract against the serial-f32 restatement
            assert_topk_tie_aware(got[i][0], got[i][1], reference_distances(emb, qs[i]), k,
                                  rows_subset=idx.tolist() if ranges else None)
    c.close()


@settings(max_examples=15 * SCALE, deadline=None, derandomize=DERANDOMIZE, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(n=st.integers(1, 5000), seed=st.integers(0, 10_000), thr=st.floats(0.5, 1.2))
def test_threshold_random(gpu_ctx, n, seed, thr):
    import semtools_amd as smt

    emb = synth.unit_rows(n, seed=seed, dup_frac=0.1, zero_frac=0.02)
    q = synth.unit_query(seed + 7)[0]
    c = smt.Corpus(gpu_ctx)
    c.append(emb)
    rows, dist = c.search(q, top_k=3, max_distance=thr)[0]
    orows, odist = _oracle(emb, q, 3, thr)
    assert rows.tolist() == orows and np.array_equal(dist, np.array(odist))
    c.close()


@settings(max_examples=30 * SCALE, deadline=None, derandomize=DERANDOMIZE, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(n=st.integers(1, 5000), k=st.integers(1, 40), nq=st.sampled_from([1, 2, 8, 9, 33, 70, 130]),
       seed=st.integers(0, 10_000), dup=st.sampled_from([0.0, 0.05, 0.5]))
def test_topk_random_shapes_over_the_operand_image(gpu_ctx, n, k, nq, seed, dup):
    """The same contract with the corpus' fp16 operand image in play (smt_corpus_prepack; 1-2 queries routed to it too): ragged
    last tiles, duplicates (ties by row order), zero rows -- rows and f64 distances equal the oracle's."""
    import semtools_amd as smt

    emb = synth.unit_rows(n, seed=seed, dup_frac=dup, zero_frac=0.01)
    qs = synth.unit_query(seed + 1, nq=nq)
    c = smt.Corpus(gpu_ctx)
    c.append(emb)
    c.prepack()
    gpu_ctx.set_tuning("image_scan_min_rows", 1)
    try:
        got = c.search(qs, top_k=k)
    finally:
        gpu_ctx.set_tuning("image_scan_min_rows", 1_500_000)
    for i in range(nq):
        orows, odist = _oracle(emb, qs[i], k)
        assert got[i][0].tolist() == orows, (i, n, k, nq, seed, dup)
        assert np.array_equal(got[i][1], np.array(odist))
    c.close()


@settings(max_examples=30 * SCALE, deadline=None, derandomize=DERANDOMIZE, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(n=st.integers(40, 9000), k=st.integers(1, 40), nq=st.sampled_from([1, 2, 8, 9, 40, 130]), seed=st.integers(0, 10_000),
       max_doc=st.sampled_from([1, 4, 70, 700]), p_want=st.sampled_from([0.1, 0.5, 0.9]), image=st.booleans())
def test_document_subsets_random_shapes(gpu_ctx, n, k, nq, seed, max_doc, p_want, image):
    """Random "documents" (1 .. max_doc lines each), a random subset of them wanted: one-line ranges, ranges meeting inside 32-row
    tiles, dense and sparse subsets (tile table of gemm_rowreg_kernel / chunk table of the LDS-row and scan kernels), with and
    without the operand image -- rows and f64 distances equal the oracle's on the eligible rows."""
    import semtools_amd as smt

    rng = np.random.default_rng(seed)
    emb = synth.unit_rows(n, seed=seed, dup_frac=0.05, zero_frac=0.01)
    qs = synth.unit_query(seed + 1, nq=nq)
    ranges, b = [], 0
    while b < n:
        e = min(n, b + int(rng.integers(1, max_doc + 1)))
        if rng.random() < p_want:
            ranges.append((b, e))
        b = e
    if not ranges:
        ranges = [(0, min(n, 3))]
    idx = np.concatenate([np.arange(a, e) for a, e in ranges])
    c = smt.Corpus(gpu_ctx)
    c.append(emb)
    if image:
        c.prepack()
    gpu_ctx.set_tuning("image_scan_min_rows", 1)
    try:
        got = c.search(qs, top_k=k, ranges=ranges)
    finally:
        gpu_ctx.set_tuning("image_scan_min_rows", 1_500_000)
    for i in range(0, nq, max(1, nq // 6)):
        orows, odist = _oracle(emb[idx], qs[i], k)
        assert got[i][0].tolist() == idx[np.array(orows, dtype=np.int64)].tolist(), (i, n, k, nq, seed, max_doc, p_want, image)
        assert np.array_equal(got[i][1], np.array(odist))
    c.close()


@settings(max_examples=25 * SCALE, deadline=None, derandomize=DERANDOMIZE, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(n_shards=st.sampled_from([2, 3, 4, 7]), transport=st.sampled_from(["peer", "copy"]), seed=st.integers(0, 10_000),
       pieces=st.lists(st.integers(1, 1500), min_size=1, max_size=6), k=st.integers(1, 70), nq=st.sampled_from([1, 1, 2, 4, 9, 40]),
       what=st.sampled_from(["topk", "topk", "subset", "threshold", "workspace"]))
def test_sharded_random_shapes_against_the_oracle(gpu_ctx, n_shards, transport, seed, pieces, k, nq, what):
    """A corpus GROWN by appends of random sizes over 2..7 logical shards (pieces dealt over the ranks: shards smaller than k, empty
    shards, pieces of one row), either transport, every search form of the host API -- checked by the C oracle directly: global rows
    in insertion order, f64 distances bit for bit (workspace mode: the store's f32 scores, 1e-5)."""
    import semtools_amd as smt

    n = sum(pieces)
    emb = synth.unit_rows(n, seed=seed, dup_frac=0.05, zero_frac=0.01)
    qs = synth.unit_query(seed + 1, nq=nq)
    rng = np.random.default_rng(seed)
    g = smt.Group.logical(0, n_shards)
    g.set_transport(transport)
    sc = smt.ShardedCorpus(g, empty=True)
    try:
        b = 0
        for p in pieces:
            sc.append(emb[b:b + p])
            b += p
        ranges, idx = None, np.arange(n)
        if what in ("subset", "workspace") and n > 4:
            cuts = np.sort(rng.choice(np.arange(1, n), size=min(8, n - 1), replace=False))
            segs = [(int(a), int(e)) for a, e in zip(cuts[::2], cuts[1::2])]
            if segs:
                ranges = segs
                idx = np.concatenate([np.arange(a, e) for a, e in segs])
        note = (n_shards, transport, seed, pieces, k, nq, what)
        if what == "threshold":
            thr = float(rng.uniform(0.7, 1.1))
            got = sc.search(qs, top_k=k, max_distance=thr)
            for i in range(nq):
                orows, odist = _oracle(emb, qs[i], k, thr)
                assert got[i][0].tolist() == orows and np.array_equal(got[i][1], np.array(odist)), (note, i)
        elif what == "workspace":
            thr = None if seed % 2 else float(rng.uniform(0.8, 1.0))
            kk = min(k, 28)
            got = sc.search(qs, top_k=kk, max_distance=thr, mode=smt.MODE_WORKSPACE, ranges=ranges)
            row_path = np.zeros(n, dtype=np.uint32)          # path 1 = the wanted rows
            row_path[idx] = 1
            for i in range(0, nq, max(1, nq // 4)):
                res = orc.search_line_embeddings(emb, row_path, np.arange(n, dtype=np.int32), qs[i], np.array([1], np.uint32), kk, thr)
                assert len(got[i][0]) == len(res), (note, i)
                assert np.allclose(got[i][1], [r["distance"] for r in res], rtol=0, atol=1e-5), (note, i)
                for gr, r in zip(got[i][0].tolist(), res):   # only f32-level near-ties of the store's scores may swap
                    assert gr == r["row"] or abs(orc.cosine(qs[i], emb[gr]) - r["distance"]) < 5e-7, (note, i, gr, r)
        else:
            got = sc.search(qs, top_k=k, ranges=ranges)
            for i in range(nq):
                orows, odist = _oracle(emb[idx], qs[i], k)
                want = idx[np.array(orows, dtype=np.int64)].tolist() if orows else []
                assert got[i][0].tolist() == want and np.array_equal(got[i][1], np.array(odist)), (note, i)
    finally:
        sc.close()
        g.close()


@settings(max_examples=12 * SCALE, deadline=None, derandomize=DERANDOMIZE, suppress_health_check=[HealthCheck.function_scoped_fixture])
@given(n=st.integers(16_385, 120_000), k=st.integers(57, 1024), nq=st.sampled_from([1, 2, 4, 5, 9, 33]), seed=st.integers(0, 10_000),
       dup=st.sampled_from([0.0, 0.05, 0.5]), use_ranges=st.booleans(), image=st.booleans(),
       planted=st.sampled_from(["none", "on the sample grid", "off the sample grid"]))
def test_largek_sampled_regime_is_sound(gpu_ctx, n, k, nq, seed, dup, use_ranges, image, planted):
    """The sampled-threshold route (topk_large.hip) above its 16 384-row shortcut, with near rows of query 0 planted at or between the
    sampled positions: every PROVED list of the device form is the oracle's, the host form equals the oracle for every query
    (tests/soundness.py); over ranges, the host form against the oracle on the eligible rows."""
    import semtools_amd as smt

    emb = synth.unit_rows(n, seed=seed, dup_frac=dup, zero_frac=0.01)
    qs = synth.unit_query(seed + 1, nq=nq)
    rng = np.random.default_rng(seed)
    ranges, idx = None, np.arange(n)
    if use_ranges:
        cuts = np.sort(rng.choice(np.arange(1, n), size=40, replace=False))
        ranges = [(int(a), int(b)) for a, b in zip(cuts[::2], cuts[1::2])]
        idx = np.concatenate([np.arange(a, b) for a, b in ranges])
    if planted != "none":
        plan = synth.largek_plan(len(idx), k)      # the sample reads virtual rows of the range list: idx[grid]
        m = int(rng.integers(1, 3 * plan["cap"]))
        synth.plant_near_rows(emb, qs[0], m, seed=seed + 2, on_grid=m if planted.startswith("on") else 0, grid=idx[plan["grid"]],
                              eligible=idx)
    c = smt.Corpus(gpu_ctx)
    c.append(emb)
    if image:
        c.prepack()
    try:
        note = (n, k, nq, seed, dup, use_ranges, image, planted)
        if use_ranges:   # the device form takes no ranges: the host form alone
            got = host_both(c, qs, top_k=k, ranges=ranges)
            for i in range(nq):
                orows, odist = oracle_topk(emb[idx], qs[i], k)
                assert got[i][0].tolist() == idx[np.array(orows, dtype=np.int64)].tolist(), (note, i)
                assert got[i][1].tobytes() == odist.tobytes(), (note, i)
        else:
            assert_sound(c, emb, qs, k, family=None)
    finally:
        c.close()
