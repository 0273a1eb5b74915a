"""GPU: the IVF index searched inside row ranges (smt_ivfpq_search_ranges, its device form, the sharded form).

The float64 reference and the corpus, seeds and query sets are those of tests/test_gpu_ivf_search_contract.py; the ranges only remove
candidates, so every expectation there carries over with "rows of the probed lists" read as "rows of the probed lists inside the
ranges": fully determined at rerank 512 on lists of <= 512 rows, and the certain-row rule where the shortlist bites.  The probe does
not see the ranges: queries whose probe is undecided (ivf_ref.probe_reference) are set aside, at most 10 % per (query set, nprobe)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from tests import ivf_ranges_ref as G
from tests import ivf_ref as R
from tests.test_gpu_ivf_search_contract import _corpus, exact_distances, probed_rows, top_rows

pytestmark = pytest.mark.gpu

N, NLIST, SEED, QSEED = R.GPU_N, R.GPU_NLIST, R.GPU_SEED, R.GPU_QSEED
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
SEGMENT = 8192       # codes per segment of a long list (include/semtools_hip.h, smt_ivfpq_search)


def search(ix, ctx, entry, qs, top_k, nprobe, rerank, row_base=0, ranges=None):
    """[(rows, dist)] per query through the host entry points or the device ones; the device form's padding is checked here."""
    if entry == "host":
        return ix.search(qs, top_k=top_k, nprobe=nprobe, rerank=rerank, row_base=row_base, ranges=ranges)
    import torch

    nq = len(qs)
    qd = torch.from_numpy(np.ascontiguousarray(qs, dtype=np.float32)).cuda()
    rows = torch.zeros((nq, top_k), dtype=torch.int64, device="cuda")
    dist = torch.zeros((nq, top_k), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ix.search_device(qd.data_ptr(), nq, top_k, nprobe, rerank, row_base, rows.data_ptr(), dist.data_ptr(), ranges=ranges)
    ctx.synchronize()
    r, d = rows.cpu().numpy().view(np.uint64), dist.cpu().numpy()
    out = []
    for i in range(nq):
        n = int((r[i] != PAD).sum())
        assert (r[i][n:] == PAD).all() and np.isposinf(d[i][n:]).all() and (r[i][:n] != PAD).all()
        out.append((r[i][:n], d[i][:n]))
    return out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and x[1].tobytes() == y[1].tobytes() for x, y in zip(a, b))


@pytest.fixture(scope="module")
def rows():
    return R.iso_rows(N, SEED)


@pytest.fixture(scope="module")
def query_sets(rows):
    fresh = R.iso_rows(64, QSEED)
    own = rows[[0, 1, 191, 192, 4095, 4096, 8191, N - 2, N - 1]]
    sets = dict(fresh=fresh, times3=fresh[:9] * np.float32(3.0), times001=fresh[:9] * np.float32(0.01), own=own)
    return {name: (qs, np.stack([exact_distances(rows, q) for q in qs])) for name, qs in sets.items()}


@pytest.fixture(scope="module", params=[False, True], ids=["pq", "lpca"])
def small(request, gpu_ctx, rows, tmp_path_factory):
    import semtools_amd as smt

    c = smt.Corpus(gpu_ctx)
    c.append(rows)
    ix = smt.IvfPq(c, nlist=NLIST, train_iters=4, local_pca=request.param)
    path = tmp_path_factory.mktemp("ivf") / "small.ivf"
    ix.save(path)
    assert ix.list_sizes().max() <= 512
    yield rows, c, ix, R.read_index(path)
    ix.close(); c.close()


def main_sets(n):
    return dict(alternate=G.alternate_blocks(n), scattered=G.scattered_rows(n), empties=G.with_empty_members(n),
                second_row=G.every_second_row(n), none=[(5, 5), (9, 9)])


def nearest_list(f, q):
    return int(R.probe_reference(q, f["centroids"], 1)[0][0])


def border_sets(f, q):
    """borders_at of the query's nearest list over (p0, p1) in {0, 1, 63, 64, 65} x {64, 65, 127, 128, size - 1, size}, p0 < p1."""
    l = nearest_list(f, q)
    size = int(f["offsets"][l + 1] - f["offsets"][l])
    assert size > 130, size
    return {f"border{p0}-{p1}": G.borders_at(f, l, p0, p1)
            for p0 in (0, 1, 63, 64, 65) for p1 in sorted({64, 65, 127, 128, size - 1, size}) if p0 < p1 <= size}


def few_rows_set(f, q):
    """Three single rows of the query's nearest list: fewer than top_k = 10 or 56 rows of any probe that holds that list."""
    l = nearest_list(f, q)
    ids = np.sort(f["ids"][int(f["offsets"][l]):int(f["offsets"][l + 1])][[0, 7, 70]].astype(np.int64))
    return [(int(r), int(r) + 1) for r in ids]


_PROBE = {}


def candidates(f, tag, qs, nprobe):
    """Per query the rows of the float64 probe's lists, or None when the probe is undecided (computed once per index and set)."""
    key = (f["kind"], tag, nprobe)
    if key not in _PROBE:
        out = []
        for q in qs:
            lists, decided = R.probe_reference(q, f["centroids"], nprobe)
            out.append(probed_rows(f, lists) if decided else None)
        _PROBE[key] = out
    return _PROBE[key]


def expect(cand, dist_all, ranges, top_k):
    inside = G.in_ranges(np.arange(dist_all.shape[1]), ranges)
    out = []
    for c, d in zip(cand, dist_all):
        if c is None:
            out.append(None)
            continue
        c = c[inside[c]]
        out.append(top_rows(c, d[c], top_k))
    return out


def check(got, want, row_base, where):
    for qi, ((gr, gd), w) in enumerate(zip(got, want)):
        if w is None:
            continue
        assert np.array_equal(gr, (w[0] + row_base).astype(np.uint64)), (where, qi, gr, w[0])
        assert gd.tobytes() == w[1].tobytes(), (where, qi)


# ================================================================================================ 1. no filter is no change
@pytest.mark.parametrize("entry", ["host", "device"])
def test_no_filter_is_no_change(small, gpu_ctx, query_sets, entry):
    x, c, ix, f = small
    qs = query_sets["fresh"][0][:9]
    for rerank in (16, 512):
        for nprobe in (1, 7, 64):
            for top_k in (1, 56):
                plain = search(ix, gpu_ctx, entry, qs, top_k, nprobe, rerank)
                assert same(plain, search(ix, gpu_ctx, entry, qs, top_k, nprobe, rerank, ranges=[])), (rerank, nprobe, top_k)
                assert same(plain, search(ix, gpu_ctx, entry, qs, top_k, nprobe, rerank, ranges=[(0, N)])), (rerank, nprobe, top_k)


# ================================================================================================ 2. the lossless regime
@pytest.mark.parametrize("row_base", [0, (1 << 33) + 5])
@pytest.mark.parametrize("entry", ["host", "device"])
def test_lossless_regime_is_fully_determined(small, gpu_ctx, query_sets, entry, row_base):
    """rerank 512, lists <= 512 rows: the answer is the exact top-k over (rows of the float64 probe's lists) n ranges -- rows equal,
    distances bit-equal; short counts and padding where the ranges leave fewer than top_k rows.  The border sets cut the nearest
    list of the FIRST fresh query at the positions where a wave's 64-code groups begin and end; they run with the fresh queries."""
    import semtools_amd as smt

    x, c, ix, f = small
    for name, (qs, dist_all) in query_sets.items():
        sets = main_sets(N)
        if name == "fresh":
            sets.update(border_sets(f, qs[0]))
            sets["few"] = few_rows_set(f, qs[0])
        for nprobe in (1, 7, 64):
            cand = candidates(f, name, qs, nprobe)
            aside = sum(w is None for w in cand)
            assert aside <= len(qs) // 10, (name, nprobe, aside)
            for sname, ranges in sets.items():
                want56 = expect(cand, dist_all, ranges, 56)
                packed = smt.PackedRanges(ranges)
                for top_k in (1, 10, 56):
                    want = [None if w is None else (w[0][:top_k], w[1][:top_k]) for w in want56]
                    for nq in ((1, 9, 64) if name == "fresh" else (9,)):
                        got = search(ix, gpu_ctx, entry, qs[:nq], top_k, nprobe, 512, row_base, packed)
                        assert len(got) == nq
                        check(got, want, row_base, (name, sname, nprobe, top_k, nq))
                if sname == "none":
                    assert all(w is None or len(w[0]) == 0 for w in want56)
                if sname == "few":
                    assert want56[0] is None or len(want56[0][0]) == 3


# ================================================================================================ 3. every list probed
_EXACT = {}


@pytest.mark.parametrize("entry", ["host", "device"])
def test_probing_every_list_equals_the_exact_filtered_search(small, gpu_ctx, query_sets, entry):
    """(The exact filtered answers are computed once per coding and shared by the two entries.)"""
    x, c, ix, f = small
    qs = query_sets["fresh"][0]
    sets = main_sets(N)
    sets.update(border_sets(f, qs[0]))
    sets["few"] = few_rows_set(f, qs[0])
    for name, (qs, _) in query_sets.items():
        for sname, ranges in sets.items():
            for top_k in (1, 10, 56):
                key = (f["kind"], name, sname, top_k)
                if key not in _EXACT:
                    _EXACT[key] = c.search(qs, top_k=top_k, ranges=ranges)
                got = search(ix, gpu_ctx, entry, qs, top_k, NLIST, 512, 0, ranges)
                assert same(got, _EXACT[key]), (name, sname, top_k)


# ================================================================================================ 4. where the shortlist bites
@pytest.fixture(scope="module", params=["segmented", "one-long-list"])
def long_corpus(request, gpu_ctx):
    import semtools_amd as smt

    x, nlist, sizes = _corpus(request.param)
    c = smt.Corpus(gpu_ctx)
    c.append(x)
    yield request.param, x, nlist, sizes, c
    c.close()


@pytest.fixture(scope="module", params=[False, True], ids=["pq", "lpca"])
def biting(request, long_corpus, tmp_path_factory):
    import semtools_amd as smt

    name, x, nlist, sizes, c = long_corpus
    ix = smt.IvfPq(c, nlist=nlist, train_iters=4, local_pca=request.param)
    path = tmp_path_factory.mktemp("ivf") / "biting.ivf"
    ix.save(path)
    assert np.array_equal(ix.list_sizes(), np.array(sizes, dtype=np.uint64)), ix.list_sizes()
    yield name, x, c, ix, R.read_index(path)
    ix.close()


def segments(f, nprobe):
    """(n_seg, segment of a list position) as smt_ivfpq_search documents them: a typical list (1.5 x the mean) is cut into 8192-code
    segments, the last one takes the rest of a longer list.  (nprobe 2 leaves every list the segments it wants.)"""
    typical = (f["n_rows"] // f["nlist"]) * 3 // 2
    n_seg = max(1, -(-typical // SEGMENT))
    assert n_seg <= 512 // nprobe
    return n_seg, lambda p: min(p // SEGMENT, n_seg - 1)


def check_partial_oracle_in_ranges(x, f, qs, got, nprobe, top_k, rerank, ranges):
    """check_partial_oracle of the contract test with the mask applied: every returned row lies in the ranges and in a probed list,
    every returned distance is the exact one, and every CERTAIN row of the exact top-k over (probed rows n ranges) is returned --
    certain: fewer than ceil(rerank / 8) IN-RANGE rows of its list SEGMENT may have an ADC distance <= its own * (1 + 2^-7), f32
    bounds of the ADC sums included.  Returns (certain rows seen, queries set aside)."""
    list_of, pos_of = R.list_of_rows(f)
    off = f["offsets"].astype(np.int64)
    need = -(-rerank // 8)
    n_seg, seg_of = segments(f, nprobe)
    inside = G.in_ranges(np.arange(f["n_rows"]), ranges)
    n_certain = aside = 0
    for qi, (q, (gr, gd)) in enumerate(zip(qs, got)):
        gr = gr.astype(np.int64)
        assert len(set(gr.tolist())) == len(gr) and (np.diff(gd) >= 0).all()
        assert inside[gr].all(), (qi, "a returned row lies outside the ranges", gr[~inside[gr]])
        for r, d in zip(gr, gd):
            assert d == orc.cosine(q, x[r], accurate=True), (qi, r)
        lists, decided = R.probe_reference(q, f["centroids"], nprobe)
        if not decided:
            aside += 1
            continue
        assert np.isin(list_of[gr], lists).all(), (qi, "a returned row lies outside the probed lists")
        cand = probed_rows(f, lists)
        cand = cand[inside[cand]]
        best = top_rows(cand, exact_distances(x[cand], q), top_k)[0]
        adc = {int(l): R.adc_distance(q, f, int(l)) for l in lists}
        for r in best.tolist():
            l = int(list_of[r])
            d, err = adc[l]
            p = int(pos_of[r] - off[l])
            rival = inside[f["ids"][off[l]:off[l + 1]].astype(np.int64)] & (np.minimum(np.arange(len(d)) // SEGMENT, n_seg - 1) == seg_of(p))
            certain = int((rival & ((d - err) <= (d[p] + err[p]) * (1 + 2.0 ** -7))).sum()) < need
            n_certain += certain
            if certain:
                assert r in gr, (qi, f"row {r} (list {l}, position {p}) is certain to be re-scored and in the exact top-{top_k}, but missing")
    return n_certain, aside


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("rerank", [16, 64, 256])
def test_certain_in_range_rows_are_returned(biting, gpu_ctx, rerank, entry):
    """Lists longer than 8192 codes, range borders at list positions 8191 / 8192 / 8193 of the long list (from either side) and
    alternate blocks; self-queries of in-range rows of the long list at those positions, nprobe 2."""
    name, x, c, ix, f = biting
    off = f["offsets"].astype(np.int64)
    size = int(off[1] - off[0])
    assert size > SEGMENT + 1000
    sets = {f"0-{p}": G.borders_at(f, 0, 0, p) for p in (8191, 8192, 8193)}
    sets.update({f"{p}-end": G.borders_at(f, 0, p, size) for p in (8191, 8192, 8193)})
    sets["alternate"] = G.alternate_blocks(f["n_rows"])
    total = 0
    for sname, ranges in sets.items():
        # the positions where the scan changes path, then a run of ordinary ones (so that every set keeps a few): the in-range ones
        own = np.array([int(f["ids"][off[0] + p]) for p in (0, 1, 63, 64, 8190, 8191, 8192, 8193, size - 2, size - 1) + tuple(range(100, 140))])
        own = own[G.in_ranges(own, ranges)][:12]
        assert len(own) >= 3, sname
        got = search(ix, gpu_ctx, entry, x[own], 10, 2, rerank, 0, ranges)
        n_certain, aside = check_partial_oracle_in_ranges(x, f, x[own], got, 2, 10, rerank, ranges)
        assert aside <= len(own) // 10, (sname, aside)
        total += n_certain
    print(f"{name} kind {f['kind']} rerank {rerank}: certain rows checked {total}")
    assert total > 0           # (data condition: the check must have looked at something)


# ================================================================================================ 5. append
@pytest.mark.parametrize("local_pca", [False, True], ids=["pq", "lpca"])
def test_rows_not_yet_appended_to_the_index_are_never_returned(gpu_ctx, rows, query_sets, tmp_path, local_pca):
    import semtools_amd as smt

    qs, dist_all = query_sets["fresh"]
    c = smt.Corpus(gpu_ctx)
    c.append(rows[:8192])
    ix = smt.IvfPq(c, nlist=NLIST, train_iters=4, local_pca=local_pca)
    c.append(rows[8192:])                            # the corpus holds all N rows, the index its first 8192
    ranges = [(8000, 8400), (9000, N)]
    for nprobe in (7, 64):
        for gr, _ in ix.search(qs, top_k=56, nprobe=nprobe, rerank=512, ranges=ranges):
            assert ((gr >= 8000) & (gr < 8192)).all(), gr
    assert ix.append() == N - 8192
    ix.save(tmp_path / "appended.ivf")
    f = R.read_index(tmp_path / "appended.ivf")
    assert ix.list_sizes().max() <= 512
    for nprobe in (1, 7, 64):
        cand = [probed_rows(f, R.probe_reference(q, f["centroids"], nprobe)[0]) if R.probe_reference(q, f["centroids"], nprobe)[1] else None
                for q in qs]
        assert sum(w is None for w in cand) <= len(qs) // 10
        check(ix.search(qs, top_k=56, nprobe=nprobe, rerank=512, ranges=ranges), expect(cand, dist_all, ranges, 56), 0, ("appended", nprobe))
    ix.close(); c.close()


# ================================================================================================ 6. argument errors
BAD = dict(unsorted=[(100, 200), (0, 50)], overlapping=[(0, 100), (99, 200)], past_the_end=[(0, N + 1)], begin_after_end=[(10, 9)])


def test_invalid_ranges_are_refused_before_anything_runs(small, gpu_ctx, query_sets):
    import torch

    import semtools_amd as smt
    from semtools_amd import _lib as L

    x, c, ix, f = small
    qs = np.ascontiguousarray(query_sets["fresh"][0][:4])
    lib = L.lib()
    out_r, out_d, cnt = np.empty((4, 10), np.uint64), np.empty((4, 10)), np.zeros(4, np.uint64)
    qd = torch.from_numpy(qs).cuda()
    dr = torch.empty((4, 10), dtype=torch.int64, device="cuda")
    dd = torch.empty((4, 10), dtype=torch.float64, device="cuda")
    group = smt.Group.logical(0, 1)
    sc = smt.ShardedCorpus(group, rows=x)
    six = smt.ShardedIvfPq(sc, nlist=NLIST, train_iters=4, local_pca=False)
    good = [(0, 6000)]
    want = c.search(qs, top_k=10, ranges=good)

    def calls(rng, n):
        p = C.cast(rng, C.c_void_p) if rng is not None else None
        yield lib.smt_ivfpq_search_ranges(ix._h, L.np_ptr(qs), 4, 10, NLIST, 512, p, n, 0, L.np_ptr(out_r), L.np_ptr(out_d), L.np_ptr(cnt), 10)
        yield lib.smt_ivfpq_search_ranges_device(ix._h, C.c_void_p(qd.data_ptr()), 4, 10, NLIST, 512, p, n, 0, C.c_void_p(dr.data_ptr()),
                                                 C.c_void_p(dd.data_ptr()))
        yield lib.smt_sharded_ivfpq_search_ranges(six._h, L.np_ptr(qs), 4, 10, NLIST, 512, p, n, L.np_ptr(out_r), L.np_ptr(out_d),
                                                  L.np_ptr(cnt), 10)

    for name, ranges in BAD.items():
        rng = (L.SmtRange * len(ranges))(*[L.SmtRange(b, e) for b, e in ranges])
        assert list(calls(rng, len(ranges))) == [L.SMT_E_INVALID] * 3, name
    assert list(calls(None, 2)) == [L.SMT_E_INVALID] * 3
    gpu_ctx.synchronize()
    assert same(ix.search(qs, top_k=10, nprobe=NLIST, rerank=512, ranges=good), want)
    assert same(search(ix, gpu_ctx, "device", qs, 10, NLIST, 512, 0, good), want)
    assert same(six.search(qs, top_k=10, nprobe=NLIST, rerank=512, ranges=good), want)
    six.close(); sc.close(); group.close()


# ================================================================================================ 7. three logical shards
def test_three_shards_equal_the_sharded_exact_filtered_search(rows, query_sets):
    import semtools_amd as smt

    qs = query_sets["fresh"][0][:9]
    group = smt.Group.logical(0, 3)
    sc = smt.ShardedCorpus(group, rows=rows)
    six = smt.ShardedIvfPq(sc, nlist=NLIST, train_iters=4, local_pca=True)
    b1 = int(sc.rank_rows()[0])                                   # first row of shard 1
    for i in range(3):
        assert six.shard_list_sizes(i, NLIST).max() <= 512
    sets = dict(alternate=G.alternate_blocks(N), straddle=[(b1 - 150, b1 + 150)], inside_shard0=[(10, b1 - 10)],
                nothing=[(7, 7)], no_filter=[])
    for sname, ranges in sets.items():
        for top_k in (1, 10, 56):
            got = six.search(qs, top_k=top_k, nprobe=NLIST, rerank=512, ranges=ranges)
            want = sc.search(qs, top_k=top_k, ranges=ranges if ranges else None)
            assert same(got, want), (sname, top_k)
            if sname == "inside_shard0":
                assert all((gr < b1).all() and len(gr) == top_k for gr, _ in got)
            if sname == "nothing":
                assert all(len(gr) == 0 for gr, _ in got)
    six.close(); sc.close(); group.close()
