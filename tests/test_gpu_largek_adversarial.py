"""GPU: the sampled-threshold route for 57 <= k <= 1024 (topk_large.hip) against corpora that defeat its sample, and at
the borders of its plan.  "tau only moves cost: a bad sample gives an UNCERTAIN / OVERFLOW verdict, never a wrong PROVED" -- every
case here goes through tests/soundness.py::assert_sound: each list the device form marks PROVED is the oracle's answer bit for bit,
and the host form equals the oracle whatever the verdict was.

N = 8192 * 25: the sample reads exactly the rows = 0 (mod 25) (synth.largek_plan).  "Near" rows are the adversarial query plus graded
noise (synth.graded_near_rows): distinct distances, far below the bulk's.  The adversarial query is the LAST of each batch."""
import numpy as np
import pytest

from tests import synth
from tests.soundness import assert_sound, device_topk, dump_verdicts, host_both, oracle_topk, check_list

pytestmark = pytest.mark.gpu

N = 8192 * 25
KS = [57, 100, 1024]
ROUTES = [(1, "collect"), (4, "collect"), (5, "sweep"), (8, "sweep")]
# bands of the three collects (common.h): f32 scan, bf16 x 3 over f32 rows, f16 x 2 over the operand image
F32_ERR_SCAN, F32_ERR_BF16X3, F32_ERR_F16X2 = 4e-6, 7e-5, 5.2e-4


@pytest.fixture(scope="module")
def ctx():
    import torch
    import semtools_amd as smt

    c = smt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()
    dump_verdicts()


@pytest.fixture(scope="module")
def base():
    """The bulk: i.i.d. unit rows without planted duplicates or zero rows, and eight queries (query 0 is the adversarial one)."""
    return synth.unit_rows(N, seed=61, dup_frac=0.0, zero_frac=0.0), synth.unit_query(62, nq=8)


def run_routes(ctx, emb, qs, k, family, routes=ROUTES, image=True, host=True):
    """assert_sound at nq = 1, 4 (streaming collect), 5, 8 (K3 sweep over the f32 rows) and nq = 8 over the fp16 image of the owned
    corpus.  Returns {route label: status word of the adversarial query}, and all the status words seen."""
    import semtools_amd as smt

    c = smt.Corpus(ctx)
    c.append(emb)
    sampled = synth.largek_plan(len(emb), k)["sampled"]
    ref = [oracle_topk(emb, q, k) for q in qs]
    adv, seen = {}, []
    try:
        for nq, route in routes:
            order = list(range(1, nq)) + [0]
            st = assert_sound(c, emb, qs[order], k, route=route if sampled else "collect", ref=[ref[i] for i in order],
                              family=family, host=host)
            adv[(nq, route)] = int(st[-1])
            seen += st.tolist()
        if image:
            c.prepack(True)
            order = list(range(1, 8)) + [0]
            st = assert_sound(c, emb, qs[order], k, route="sweep" if sampled else "collect", ref=[ref[i] for i in order],
                              family=family, host=host, prepacked=True)
            adv[(8, "sweep+image")] = int(st[-1])
            seen += st.tolist()
    finally:
        c.close()
    return adv, seen


# ---------------------------------------------------------------- 1. corpora that defeat the sample

@pytest.mark.parametrize("k", KS)
def test_sample_blind_to_the_near_rows(ctx, base, k):
    """40 000 near rows (more than twice LK_CAP_MAX), none at a sampled position: tau comes from the bulk alone, far too high."""
    emb, qs = base[0].copy(), base[1]
    synth.plant_near_rows(emb, qs[0], 40_000, seed=70, on_grid=0, grid=synth.largek_plan(N, k)["grid"])
    adv, _ = run_routes(ctx, emb, qs, k, "blind")
    assert set(adv.values()) == {2}, adv


@pytest.mark.parametrize("k", KS)
def test_sample_sees_only_near_rows(ctx, base, k):
    """Every sampled position holds a near row, the bulk lies between them: tau is the rank-th of 8192 near rows, rank < k of them
    are under it."""
    emb, qs = base[0].copy(), base[1]
    plan = synth.largek_plan(N, k)
    assert plan["rank"] < k
    synth.plant_near_rows(emb, qs[0], plan["S"], seed=71, on_grid=plan["S"], grid=plan["grid"])
    adv, _ = run_routes(ctx, emb, qs, k, "tight")
    assert set(adv.values()) == {1}, adv


@pytest.mark.parametrize("k", KS)
def test_sweep_of_the_share_of_near_rows_on_the_grid(ctx, base, k):
    """M = 4 x capacity near rows, G of them (a random subset of their ranks) at sampled positions, G halved ten times from min(M, S).
    While G >= rank the collected count is about rank x M / G: it starts at `rank` (< k: UNCERTAIN), doubles per step through
    [k, k + guard) and (k + guard, capacity), and ends above the capacity (G < rank: tau falls into the bulk and all M > capacity
    near rows are under it: OVERFLOW).  The condition is on the status words seen, not on this model."""
    emb0, qs = base
    plan = synth.largek_plan(N, k)
    m = 4 * plan["cap"]
    g0 = min(m, plan["S"])
    assert plan["rank"] * m // g0 < k and (g0 >> 9) < plan["rank"] and m > plan["cap"]
    seen = {}
    for step in range(10):
        emb = emb0.copy()
        synth.plant_near_rows(emb, qs[0], m, seed=72 + step, on_grid=g0 >> step, grid=plan["grid"])
        adv, _ = run_routes(ctx, emb, qs, k, f"sweep/step={step}", routes=[(1, "collect"), (5, "sweep")], image=False)
        seen[g0 >> step] = adv
    words = {s for adv in seen.values() for s in adv.values()}
    assert words == {0, 1, 2}, seen


@pytest.mark.parametrize("k", [57, 100])
def test_answer_inside_one_sampling_gap(ctx, base, k):
    """The k nearest rows sit in consecutive unsampled rows right behind a sampled one (the stride of 25 holds 24 of them per gap, so
    they run on across the next sampled positions without touching one)."""
    emb, qs = base[0].copy(), base[1]
    grid = synth.largek_plan(N, k)["grid"]
    pos = np.setdiff1d(np.arange(100_000, 100_000 + 2 * k), grid)[:k]
    emb[pos] = synth.graded_near_rows(qs[0], k, seed=73)[::-1]
    adv, seen = run_routes(ctx, emb, qs, k, "gap")
    # the sample is the bulk's, as in the control: the same bar, and the adversarial query is among the proved ones at some route
    assert seen.count(0) >= 0.95 * len(seen) and 0 in adv.values(), (adv, seen)


def test_answer_inside_one_sampling_gap_of_a_corpus_past_2m_rows(ctx):
    """n = 2 359 296: n / 256 = 9216 > 8192 sampled rows, 256 rows apart; the 100 nearest rows lie inside one gap."""
    import semtools_amd as smt

    n, k = 2_359_296, 100
    plan = synth.largek_plan(n, k)
    assert plan["S"] == 9216 and plan["grid"][1] == 256
    emb = synth.unit_rows(n, seed=74, dup_frac=0.0, zero_frac=0.0)
    qs = synth.unit_query(75, nq=5)
    emb[1_000_193:1_000_193 + k] = synth.graded_near_rows(qs[0], k, seed=76)
    c = smt.Corpus(ctx)
    c.append(emb)
    try:
        ref = [oracle_topk(emb, q, k) for q in qs]
        assert sorted(ref[0][0]) == list(range(1_000_193, 1_000_193 + k))
        assert_sound(c, emb, qs[:1], k, route="collect", ref=ref[:1], family="gap/2.36M")
        order = [1, 2, 3, 4, 0]
        assert_sound(c, emb, qs[order], k, route="sweep", ref=[ref[i] for i in order], family="gap/2.36M")
    finally:
        c.close()


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("k", KS)
def test_rows_ordered_by_distance(ctx, base, k, descending):
    """The whole answer in the first (last) chunks the collect claims."""
    emb, qs = base
    d = 1.0 - emb.astype(np.float64) @ qs[0].astype(np.float64)
    order = np.argsort(d, kind="stable")
    emb = np.ascontiguousarray(emb[order[::-1] if descending else order])
    run_routes(ctx, emb, qs, k, "ordered/" + ("desc" if descending else "asc"), image=k == 100)


@pytest.mark.parametrize("k", KS)
def test_tie_cluster_larger_than_the_capacity(ctx, base, k):
    """20 000 exact copies of the row at place k / 2: more rows tie under any tau than a buffer holds.  Status 2; the host form returns
    the copies in ascending row order (the oracle's order)."""
    emb, qs = base[0].copy(), base[1]
    orows, _ = oracle_topk(emb, qs[0], k)
    rng = np.random.default_rng(77)
    where = rng.choice(np.setdiff1d(np.arange(N), orows), size=20_000, replace=False)
    emb[where] = emb[orows[k // 2]]
    adv, _ = run_routes(ctx, emb, qs, k, "ties/20000")
    assert set(adv.values()) == {2}, adv


@pytest.mark.parametrize("k", KS)
def test_tie_cluster_of_k_plus_half_the_guard_at_the_first_place(ctx, base, k):
    """k + guard / 2 copies of one near row, all at sampled positions, nothing else near: tau is the cluster's distance, exactly the
    cluster is collected -- fewer rows than are rescored, the branch where no key is left over (next32 = +inf)."""
    emb, qs = base[0].copy(), base[1]
    plan = synth.largek_plan(N, k)
    size = k + plan["guard"] // 2
    assert plan["rank"] <= size
    rng = np.random.default_rng(78)
    emb[rng.choice(plan["grid"], size=size, replace=False)] = synth.graded_near_rows(qs[0], 1, seed=79, lo=0.3, hi=0.3)[0]
    adv, _ = run_routes(ctx, emb, qs, k, "ties/k+guard/2")
    assert 2 not in adv.values(), adv
    if size + 1 <= 1024 and synth.largek_plan(N, size + 1)["rank"] <= size:
        # that exactly the cluster lies under tau is seen one k further: asked for size + 1 rows the route collects `size`, fewer than
        # k under a finite tau, which is UNCERTAIN by the certificate's own rule -- whatever the constants of the plan
        import semtools_amd as smt

        c = smt.Corpus(ctx)
        c.append(emb)
        try:
            st = device_topk(c, qs[:1], size + 1)[2]
        finally:
            c.close()
        assert st.tolist() == [1], st


def near_tie_corpus(emb, q, k, guard, seed):
    """tests/test_gpu_nearties.py::adversarial_corpus at this size: k / 2 clearly better rows, then a cluster of k + 2 guard + 100
    rescaled, 1-ulp-perturbed and duplicated copies of one vector -- the k-th place lies inside it and every gap in it is at f32
    rounding level (~1e-7), below F32_ERR_SCAN and so below the wider bands of the sweeps too."""
    rng = np.random.default_rng(seed)
    n_better, n_cluster = k // 2, k + 2 * guard + 100
    pos = rng.choice(len(emb), size=n_better + n_cluster, replace=False)
    emb[pos[:n_better]] = synth.graded_near_rows(q, n_better, seed + 1, lo=0.05, hi=0.3)
    v = synth.graded_near_rows(q, 1, seed + 2, lo=0.9, hi=0.9)[0]
    for i, p in enumerate(pos[n_better:]):
        if i % 3 == 0:
            row = (v * np.float32(0.37 + 0.003 * i)).astype(np.float32)
        elif i % 3 == 1:
            row = v.copy()
            idx = rng.choice(256, size=6, replace=False)
            row[idx] = np.nextafter(row[idx], np.float32(np.inf if i % 2 else -np.inf), dtype=np.float32)
        else:
            row = v.copy()
        emb[p] = row
    return sorted(pos[n_better:].tolist())


@pytest.mark.parametrize("k", KS)
def test_near_ties_narrower_than_the_bands(ctx, base, k):
    emb, qs = base[0].copy(), base[1]
    plan = synth.largek_plan(N, k)
    cluster = near_tie_corpus(emb, qs[0], k, plan["guard"], seed=80)
    orows, odist = oracle_topk(emb, qs[0], k)
    assert set(orows[k // 2:]) <= set(cluster) and odist[-1] - odist[k // 2] < F32_ERR_SCAN < F32_ERR_BF16X3 < F32_ERR_F16X2
    adv, _ = run_routes(ctx, emb, qs, k, "nearties")
    # more rows than the guard within the band of the k-th distance: no certificate can hold
    assert 0 not in adv.values(), adv


@pytest.mark.parametrize("k", KS)
def test_zero_query_and_zero_rows(ctx, k):
    """A zero query (every distance ties) among ordinary ones, over a corpus with 30 % zero rows."""
    emb = synth.unit_rows(N, seed=81, dup_frac=0.01, zero_frac=0.3)
    qs = synth.unit_query(82, nq=8)
    qs[0] = 0.0
    adv, _ = run_routes(ctx, emb, qs, k, "zero-query+30%-zero-rows", image=k == 100)
    assert 0 not in adv.values(), adv       # N rows tie: no list of k of them is provable by a threshold


@pytest.mark.parametrize("k", KS)
def test_fewer_than_k_rows_below_the_bulk(ctx, base, k):
    emb, qs = base[0].copy(), base[1]
    synth.plant_near_rows(emb, qs[0], 30, seed=83, on_grid=0, grid=synth.largek_plan(N, k)["grid"])
    adv, seen = run_routes(ctx, emb, qs, k, "30-near-rows", image=False)
    assert seen.count(0) >= 0.95 * len(seen), (adv, seen)      # the bulk decides tau, as in the control
    assert 2 not in adv.values(), adv                          # 30 extra rows under tau do not fill a buffer of >= 8 (k + guard)


@pytest.mark.parametrize("up", [True, False])
def test_scaled_rows_and_queries_give_the_same_bytes(ctx, up):
    """Rows x 2^37 with queries x 2^-37, and the reverse: the same bytes as unscaled.  The domain bounds the largest magnitude of a
    vector to [2^-40, 2^40] and a unit vector of 256 components peaks near 2^-2, so 2^-40 itself would leave the domain; 2^37 keeps
    every vector inside it with the largest ones within a factor of 8 of its upper end."""
    import semtools_amd as smt

    n, k = 60_000, 100
    emb = synth.unit_rows(n, seed=84)
    qs = synth.unit_query(85, nq=8)
    s = np.float32(2.0 ** 37)
    emb_s = emb * s if up else emb / s
    qs_s = qs / s if up else qs * s
    c0, c1 = smt.Corpus(ctx), smt.Corpus(ctx)
    c0.append(emb)
    c1.append(emb_s)
    try:
        ref = [oracle_topk(emb, q, k) for q in qs]
        for nq, route in ROUTES:
            assert_sound(c1, emb_s, qs_s[:nq], k, route=route, family="scaled")
            r0, d0, st0, _ = device_topk(c0, qs[:nq], k)
            r1, d1, st1, _ = device_topk(c1, qs_s[:nq], k)
            assert st0.tolist() == st1.tolist() and r0.tobytes() == r1.tobytes() and d0.tobytes() == d1.tobytes()
            got = c1.search(qs_s[:nq], top_k=k)
            for i in range(nq):
                assert got[i][0].tolist() == ref[i][0] and got[i][1].tobytes() == ref[i][1].tobytes()
    finally:
        c0.close()
        c1.close()


def test_control_iid_rows_are_proved(ctx):
    """The same harness on synth.unit_rows proves at least 95 % of its lists (the bar of tests/test_gpu_largek.py): the adversarial
    families do not pass because nothing is ever proved."""
    emb = synth.unit_rows(N, seed=41)
    qs = synth.unit_query(42, nq=8)
    seen = []
    for k in KS:
        seen += run_routes(ctx, emb, qs, k, "control")[1]
    assert len(seen) == 3 * 26 and seen.count(0) >= 0.95 * len(seen), seen


def _workspace_expected(idx, ref, max_distance):
    thr = float(np.float32(1.0) - np.float32(max_distance))   # the score threshold as the library forms it (store.rs:502-503)
    orows, odist = ref                                         # ascending distances: the filter keeps a prefix
    keep = [j for j in range(len(orows)) if (1.0 - odist[j]) > thr]
    return idx[np.array(orows, dtype=np.int64)[keep]].tolist() if keep else [], odist[keep]


@pytest.mark.parametrize("family", ["blind", "tight"])
@pytest.mark.parametrize("k", KS)
def test_workspace_threshold_below_and_above_the_kth_distance(ctx, base, family, k):
    """Host form, MODE_WORKSPACE with max_distance: the threshold clamps tau (ws_clamp) and, below the k-th distance, leaves fewer
    than k valid rows (the `valid < k_eff` certificate).  Unfiltered and over ranges."""
    import semtools_amd as smt
    from semtools_amd import _lib as L

    emb, qs = base[0].copy(), base[1][:4]
    plan = synth.largek_plan(N, k)
    if family == "blind":
        synth.plant_near_rows(emb, qs[0], 40_000, seed=86, on_grid=0, grid=plan["grid"])
    else:
        synth.plant_near_rows(emb, qs[0], plan["S"], seed=87, on_grid=plan["S"], grid=plan["grid"])
    ranges = [(1, 30_003), (50_002, 51_001), (90_000, 160_007), (199_001, N)]
    sub = np.concatenate([np.arange(b, e) for b, e in ranges])
    c = smt.Corpus(ctx)
    c.append(emb)
    try:
        for rng_arg, idx in ((None, np.arange(N)), (ranges, sub)):
            sub_emb = emb if rng_arg is None else emb[idx]
            ref = [oracle_topk(sub_emb, q, k) for q in qs]
            odist = ref[0][1]
            below, above = float(odist[k // 3]), float(odist[-1]) + 0.05
            for md in (below, above, 0.93):
                for nq in (1, 4):
                    order = list(range(1, nq)) + [0]
                    got = host_both(c, qs[order], top_k=k, mode=L.MODE_WORKSPACE, ranges=rng_arg, max_distance=md)
                    for j, i in enumerate(order):
                        wr, wd = _workspace_expected(idx, ref[i], md)
                        assert got[j][0].tolist() == wr and got[j][1].tobytes() == wd.tobytes(), (family, k, md, nq, i)
                    if md == below:
                        assert k // 3 - 1 <= len(got[-1][0]) <= k // 3 + 1
    finally:
        c.close()


# ---------------------------------------------------------------- 2. borders of the plan

@pytest.mark.parametrize("n", [16383, 16384, 16385, 16388, 16400])
@pytest.mark.parametrize("k", [57, 1024])
def test_sample_border(ctx, n, k):
    """Up to LK_CAP_MAX = 16384 rows every row is collected (tau = +inf: no threshold for a sweep, five queries stream like one);
    from 16385 rows on the sample runs and five queries take the sweep -- seen in the profile counters.  The counter `largek_tau`
    itself brackets the tau kernel on both sides of the border, so it cannot tell them apart; the observable is the route at nq = 5
    (a sweep needs a finite tau).  At nq = 1 nothing observable separates 16384 from 16385: those cases check soundness only."""
    import semtools_amd as smt

    emb = synth.unit_rows(n, seed=88)
    qs = synth.unit_query(89, nq=5)
    assert synth.largek_plan(n, k)["sampled"] == (n > 16384)
    c = smt.Corpus(ctx)
    c.append(emb)
    try:
        for nq in (1, 5):
            st = assert_sound(c, emb, qs[:nq], k, route="sweep" if (n > 16384 and nq == 5) else "collect", family=f"border/n={n}")
            if n <= 16384:
                assert (st == 0).all(), st       # every row collected: nothing is left to chance
    finally:
        c.close()


@pytest.mark.parametrize("n,k", [(57, 57), (57, 100), (1023, 1023), (1023, 1024)])
def test_k_at_least_the_row_count(ctx, n, k):
    import semtools_amd as smt

    emb = synth.unit_rows(n, seed=90, dup_frac=0.05)
    qs = synth.unit_query(91, nq=5)
    c = smt.Corpus(ctx)
    c.append(emb)
    try:
        for nq in (1, 5):
            st = assert_sound(c, emb, qs[:nq], k, route="collect", family="k>=n")
            assert (st == 0).all(), st
    finally:
        c.close()


def _filtered_cases(n, k, rng):
    every10 = [(r, r + 1) for r in range(3, n, 10)]                                  # 20 480 one-row ranges
    residues, b = [], 17
    for i in range(64):                                                              # starts and ends at every residue mod 4
        b += 900 + (i % 4)
        e = b + 500 + (i // 4) % 4
        residues.append((b, e))
        b = e
    short, b = [], 0
    for _ in range(5000):
        b += int(rng.integers(1, 30))
        e = b + int(rng.integers(1, 9))
        short.append((b, e))
        b = e
    def exact(m):
        return [(5, 5 + m // 2), (100_001, 100_001 + m - m // 2)]
    return {"one-row": every10, "residues": residues, "5000-short": short, "subset-16384": exact(16384), "subset-16385": exact(16385),
            "subset-under-k": [(7, 7 + (k - 7) // 2), (150_002, 150_002 + 3)]}


@pytest.mark.parametrize("k", [57, 1024])
def test_filtered_host_form_over_ranges(ctx, base, k):
    """lk_map_virtual and the chunk table of the filtered collect, checked against the oracle on emb[idx] like the fuzz suite.  The
    i.i.d. subsets double as a control: the verdicts counted by the context stay under 5 % of the lists, which a sample that does
    not follow the ranges would not manage."""
    import semtools_amd as smt

    emb, qs = base
    c = smt.Corpus(ctx)
    c.append(emb)
    lists = unproved = 0
    try:
        for name, ranges in _filtered_cases(N, k, np.random.default_rng(92)).items():
            idx = np.concatenate([np.arange(b, e) for b, e in ranges])
            assert (np.diff(idx) > 0).all() and idx[-1] < N
            sampled = len(idx) > 16384
            for sel in (qs[:1], qs[4:8]):
                ctx.uncertain_count(reset=True)
                got = c.search(sel, top_k=k, ranges=ranges)
                if sampled:
                    lists += len(sel)
                    unproved += ctx.uncertain_count(reset=True)
                got0 = host_both(c, sel, top_k=k, ranges=ranges)
                for i, q in enumerate(sel):
                    orows, odist = oracle_topk(emb[idx], q, k)
                    want = idx[np.array(orows, dtype=np.int64)].tolist()
                    for g in (got, got0):
                        assert g[i][0].tolist() == want and g[i][1].tobytes() == odist.tobytes(), (name, k, i)
    finally:
        c.close()
    assert lists >= 20 and unproved <= 0.05 * lists, (unproved, lists)


@pytest.mark.parametrize("k", [57, 1024])
def test_filtered_near_rows_all_in_one_range(ctx, base, k):
    import semtools_amd as smt

    emb, qs = base[0].copy(), base[1]
    ranges = [(2, 20_001), (40_003, 60_002), (120_001, 120_002), (150_000, 170_003)]
    idx = np.concatenate([np.arange(b, e) for b, e in ranges])
    emb[40_003:40_003 + 3000] = synth.graded_near_rows(qs[0], 3000, seed=93)
    c = smt.Corpus(ctx)
    c.append(emb)
    try:
        for sel in (qs[:1], qs[[1, 2, 3, 0]]):
            got = host_both(c, sel, top_k=k, ranges=ranges)
            for i, q in enumerate(sel):
                orows, odist = oracle_topk(emb[idx], q, k)
                assert got[i][0].tolist() == idx[np.array(orows, dtype=np.int64)].tolist() and got[i][1].tobytes() == odist.tobytes()
    finally:
        c.close()


@pytest.mark.parametrize("n,k,nq", [(20_000, 57, 256), (20_000, 57, 257), (20_000, 57, 300), (3_000, 1024, 300)])
def test_rounds_of_more_than_256_queries(ctx, n, k, nq):
    """launch_topk_large answers 256 queries per round and offsets the outputs of the next: every list is written (the outputs are
    prefilled with a sentinel), with and without a status pointer, and is sound; i.i.d. rows stay proved."""
    import semtools_amd as smt

    emb = synth.unit_rows(n, seed=94)
    qs = synth.unit_query(95, nq=nq)
    c = smt.Corpus(ctx)
    c.append(emb)
    try:
        st = assert_sound(c, emb, qs, k, host=False, family=f"rounds/n={n}")
        assert (st == 0).sum() >= 0.95 * nq, st
        got = c.search(qs[250:262], top_k=k)
        for i, q in enumerate(qs[250:262]):
            orows, odist = oracle_topk(emb, q, k)
            check_list(got[i][0].astype(np.uint64), got[i][1], orows, odist, len(orows), (n, k, i))
    finally:
        c.close()


# ---------------------------------------------------------------- 5. unequal shards

@pytest.mark.parametrize("transport", ["peer", "copy"])
def test_unequal_shards(ctx, transport):
    """Four logical ranks holding 40 rows (fewer than k), 5000 (between k and 16384), 30 000 (sampled) and none: PROVED lists equal
    the single-corpus oracle; with an over-capacity tie cluster in the sampled shard only, the merged status is that shard's verdict
    for exactly the queries the cluster ranks for (the expected word is the verdict of that shard searched alone: the other shards
    collect every row or hold none, so they prove).  The shards are views of one device allocation, not appends: an append is dealt
    to the emptiest ranks first (water level, layout_deal), so no series of appends leaves one rank empty beside one above 16 384
    rows.  Grown shards of unequal size are the fuzz suite's (test_sharded_random_shapes_against_the_oracle)."""
    import torch
    import semtools_amd as smt

    sizes = [40, 5000, 30_000, 0]
    n = sum(sizes)
    emb = synth.unit_rows(n, seed=96, dup_frac=0.0, zero_frac=0.0)
    qs = synth.unit_query(97, nq=5)
    for tied in (False, True):
        if tied:   # 17 000 copies of query 0's 10th row inside shard 2: under any tau of that shard for query 0, far from the others
            src = synth.graded_near_rows(qs[0], 1, seed=98, lo=0.2, hi=0.2)[0]
            emb[5040 + 100:5040 + 100 + 17_000] = src
        x = torch.from_numpy(emb).to("cuda:0")
        torch.cuda.synchronize()
        g = smt.Group.logical(0, 4)
        sc = alone = None
        try:
            g.set_transport(transport)
            cuts = np.concatenate([[0], np.cumsum(sizes)])
            ptrs = [x.data_ptr() + int(cuts[i]) * 1024 for i in range(4)]
            sc = smt.ShardedCorpus(g, device_ptrs=ptrs, shard_rows=sizes)
            alone = smt.Corpus(ctx, device_ptr=ptrs[2], rows=sizes[2])   # the only shard whose verdict is not 0 by construction
            for k in (100, 1024):
                ref = [oracle_topk(emb, q, k) for q in qs]
                for nq in (1, 5):
                    qd = torch.from_numpy(np.ascontiguousarray(qs[:nq])).cuda()
                    out = torch.full((nq, 2, k), -7, dtype=torch.int64, device="cuda")
                    st = torch.full((nq,), 7, dtype=torch.int32, device="cuda")
                    torch.cuda.synchronize()
                    sc.search_topk_device([qd.data_ptr()] * 4, nq, k, [out.data_ptr(), 0, 0, 0], [st.data_ptr(), 0, 0, 0])
                    g.synchronize()
                    m, s_ = out.cpu().numpy(), st.cpu().numpy()
                    worst = device_topk(alone, qs[:nq], k)[2]
                    assert s_.tolist() == worst.tolist(), (s_, worst)     # shards 0, 1 (every row collected) and 3 (empty) prove
                    if tied:
                        assert s_[0] == 2, s_
                    else:
                        assert (s_ == 0).sum() >= nq - 1, s_
                    for i in range(nq):
                        if s_[i] == 0:
                            check_list(np.ascontiguousarray(m[i, 0]).view(np.uint64), np.ascontiguousarray(m[i, 1]).view(np.float64),
                                       ref[i][0], ref[i][1], k, (transport, tied, k, nq, i))
                got = sc.search(qs, top_k=k)
                for i in range(len(qs)):
                    assert got[i][0].tolist() == ref[i][0] and got[i][1].tobytes() == ref[i][1].tobytes()
        finally:   # the sharded corpus goes before its group, also when an assertion above failed
            if alone is not None:
                alone.close()
            if sc is not None:
                sc.close()
            g.close()
