"""GPU: what smt_ivfpq_search must return.  The header promises exact distances and approximate membership; these tests pin down
the part of membership that is NOT allowed to be approximate.

(a) Lossless regime: every list fits one block's shortlists (<= 512 rows, rerank 512), so every row of a probed list is re-scored
    and the answer is fully determined: the exact top-k over the rows of the nprobe nearest lists.  Rows equal, distances bit-equal.
(b) Where the shortlist bites (rerank 16 / 64 / 256, lists of 20 000 rows): a row is CERTAIN to be re-scored when fewer than
    ceil(rerank / 8) rows of its list have an ADC distance <= its own * (1 + 2^-7) (+ the f32 bound of the ADC sum): shortlists are
    per wave, rerank / waves each with waves in {4, 8} (ivfpq_search.hip, `adc_waves` / `shortlist` in ivfpq_search_core, `ks` in
    ivf_adc_kernel), and the selection keeps the top 16 bits of the f32 distance (`kd[r] >> 16` in ivf_adc_kernel: sign, 8 exponent
    and 7 mantissa bits, a relative step of 2^-7).  Every certain row of the exact top-k over the probed rows must be returned,
    every returned row lies in a probed list, every returned distance is the exact one.

The probe's choice is taken from a float64 reference; a query whose nprobe-th and (nprobe+1)-th lists lie within the derived f32
bound of each other (tests/ivf_ref.py probe_reference) is set aside, at most 10 % of a query set."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from oracle import oracle as orc
from tests import ivf_ref as R

pytestmark = pytest.mark.gpu

N, NLIST, SEED, QSEED = R.GPU_N, R.GPU_NLIST, R.GPU_SEED, R.GPU_QSEED

_RES = np.dtype([("doc", "<u8"), ("line", "<u8"), ("start", "<u8"), ("end", "<u8"), ("distance", "<f8")])


def exact_distances(emb, q):
    """The oracle's accurate (f64-accumulating) cosine distance of every row of emb to q -- orc.cosine(q, row, accurate=True) for
    all rows in one call."""
    emb = np.ascontiguousarray(emb, dtype=np.float32)
    q = np.ascontiguousarray(q, dtype=np.float32)
    n = len(emb)
    counts = np.array([n], dtype=np.uint64)
    out = (orc.OrcResult * n)()
    got = orc.lib().orc_search_documents(orc._p(emb, C.c_float), orc._p(counts, C.c_uint64), 1, 256, orc._p(q, C.c_float), 0, n, 0, 0.0, 1, out, n)
    assert got == n
    res = np.frombuffer(out, dtype=_RES, count=n)
    d = np.empty(n)
    d[res["line"].astype(np.int64)] = res["distance"]
    return d


def top_rows(rows, dist, k):
    """The k best of (rows, dist): distance ascending, ties by row."""
    order = np.lexsort((rows, dist))[:k]
    return rows[order], dist[order]


def probed_rows(f, lists):
    off = f["offsets"].astype(np.int64)
    return np.concatenate([f["ids"][off[l]:off[l + 1]] for l in lists]).astype(np.int64)


def search(ix, ctx, entry, qs, top_k, nprobe, rerank, row_base):
    """[(rows, dist)] per query through the host entry point or smt_ivfpq_search_device."""
    if entry == "host":
        return ix.search(qs, top_k=top_k, nprobe=nprobe, rerank=rerank, row_base=row_base)
    import torch

    nq = len(qs)
    qd = torch.from_numpy(np.ascontiguousarray(qs, dtype=np.float32)).cuda()
    rows = torch.empty((nq, top_k), dtype=torch.int64, device="cuda")
    dist = torch.empty((nq, top_k), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ix.search_device(qd.data_ptr(), nq, top_k, nprobe, rerank, row_base, rows.data_ptr(), dist.data_ptr())
    ctx.synchronize()
    r, d = rows.cpu().numpy().view(np.uint64), dist.cpu().numpy()
    out = []
    for i in range(nq):
        keep = r[i] != np.uint64(0xFFFFFFFFFFFFFFFF)
        out.append((r[i][keep], d[i][keep]))
    return out


# ================================================================================================ (a) the lossless regime
@pytest.fixture(scope="module")
def rows():
    return R.iso_rows(N, SEED)


@pytest.fixture(scope="module")
def query_sets(rows):
    """Query sets and, computed once, the exact distance of every corpus row to every query."""
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
    yield rows, c, ix, R.read_index(path)
    ix.close(); c.close()


def lossless_expectation(f, qs, dist_all, nprobe):
    """Per query: (rows, dist) of the exact top-56 over the rows of the float64 probe's lists, or None when the probe is undecided."""
    out = []
    for q, d in zip(qs, dist_all):
        lists, decided = R.probe_reference(q, f["centroids"], nprobe)
        cand = probed_rows(f, lists)
        out.append(top_rows(cand, d[cand], 56) if decided else None)
    return out


@pytest.mark.parametrize("row_base", [0, (1 << 33) + 5])
@pytest.mark.parametrize("entry", ["host", "device"])
def test_lossless_regime_is_fully_determined(small, gpu_ctx, query_sets, entry, row_base):
    """Lists <= 512 rows and rerank = 512: rows equal and distances bit-equal to the exact top-k over the probed lists, for
    nprobe in {1, 2, 7, 32, 64} x top_k in {1, 10, 56} x nq in {1, 7, 8, 9, 64} (the ADC grid deals queries to XCDs in groups of
    eight; the last group may be short), fresh unit queries, the same scaled by 3.0 and by 0.01 (the probe normalises: the lists
    must not move), and corpus rows themselves.  Observed share of queries set aside: 0."""
    x, c, ix, f = small
    assert ix.list_sizes().max() <= 512
    for name, (qs, dist_all) in query_sets.items():
        for nprobe in (1, 2, 7, 32, 64):
            want = lossless_expectation(f, qs, dist_all, nprobe)
            aside = sum(w is None for w in want)
            assert aside <= len(qs) // 10, (name, nprobe, aside)
            for top_k in (1, 10, 56):
                for nq in ((1, 7, 8, 9, 64) if name == "fresh" else (9,)):
                    got = search(ix, gpu_ctx, entry, qs[:nq], top_k, nprobe, 512, row_base)
                    assert len(got) == nq
                    for qi, ((gr, gd), w) in enumerate(zip(got, want)):
                        if w is None:
                            continue
                        where = (name, nprobe, top_k, nq, qi)
                        assert np.array_equal(gr, (w[0][:top_k] + row_base).astype(np.uint64)), where
                        assert gd.tobytes() == w[1][:top_k].tobytes(), where


def test_probing_every_list_equals_the_exact_search(small, query_sets):
    x, c, ix, f = small
    for name, (qs, _) in query_sets.items():
        for top_k in (1, 10, 56):
            for (gr, gd), (er, ed) in zip(ix.search(qs, top_k=top_k, nprobe=NLIST, rerank=512), c.search(qs, top_k=top_k)):
                assert np.array_equal(gr, er) and gd.tobytes() == ed.tobytes(), (name, top_k)


# ================================================================================================ (b) where the shortlist bites
def topic_rows(sizes, seed, latent=32, spread=0.25, noise=0.35):
    """Clustered unit rows, topic t with sizes[t] rows: row = centre_t + spread * z . B_t + noise * g, normalised, with z ~ N(0, I_32)
    in the topic's own 32-d subspace B_t and g isotropic in all 256 dims.  Inside a topic the rows lie about equally far from each
    other in both parts, so a row queried as itself is the clear ADC best of its list under either coding: the isotropic part is
    what the global codebooks of kind 0 tell apart, the 32-d part is what the 32 per-list directions of kind 1 keep.
    The rows are shuffled, except that the build's starting row of list l (ivf_ref.build_sample) is a row of topic l.  The topics
    are far apart, so k-means keeps list l == topic l and the list sizes are the topic sizes: that is how a list of a chosen
    length is made."""
    rng = np.random.default_rng(seed)
    n, nt = int(sum(sizes)), len(sizes)
    centers = rng.standard_normal((nt, 256)).astype(np.float32)
    centers /= np.linalg.norm(centers, axis=1, keepdims=True)
    basis = rng.standard_normal((nt, latent, 256)).astype(np.float32) / np.float32(16.0)
    which = rng.permutation(np.repeat(np.arange(nt), sizes))
    _, start = R.build_sample(n, nt)
    for t in range(nt):                                         # swap a row of topic t into the starting position of list t
        if which[start[t]] != t:
            other = np.nonzero(which == t)[0]
            other = other[~np.isin(other, start)][0]
            which[other], which[start[t]] = which[start[t]], t
    x = np.empty((n, 256), dtype=np.float32)
    for b in range(0, n, 32768):
        w = which[b:b + 32768]
        z = rng.standard_normal((len(w), latent), dtype=np.float32) * np.float32(spread / np.sqrt(latent))
        xs = centers[w] + np.float32(noise / 16.0) * rng.standard_normal((len(w), 256), dtype=np.float32)
        for t in np.unique(w):
            xs[w == t] += z[w == t] @ basis[t]
        x[b:b + 32768] = xs / np.linalg.norm(xs, axis=1, keepdims=True)
    return x, which


def _corpus(name):
    if name == "balanced":        # lists of ~190 rows: one segment, four waves that each see a few dozen codes
        return R.iso_rows(N, SEED), NLIST, None
    if name == "tiny-lists":      # lists of <= 64 rows: ALL codes of a list go to wave 0, which keeps rerank / waves of them; + zero rows
        x = R.iso_rows(2048, SEED + 1)
        x[[5, 100, 2047]] = 0.0
        return x, 64, None
    if name == "segmented":       # 5504 rows per list on average: 1.5 x that > 8192 => two segments per probed list; list 0 holds 20 000
        sizes = [20000] + [5036] * 30 + [5048]                 # rows: its last segment takes 11 808 codes ("takes the rest" with n_seg = 2)
        return topic_rows(sizes, 31)[0], 32, sizes
    if name == "one-long-list":   # typical list 1280 rows => ONE segment; list 0 holds 10 000 > 8192: "takes the rest" with n_seg = 1
        sizes = [10000] + [998] * 30 + [1020]
        return topic_rows(sizes, 32)[0], 32, sizes
    raise KeyError(name)


@pytest.fixture(scope="module", params=["balanced", "tiny-lists", "segmented", "one-long-list"])
def corpus(request, gpu_ctx):
    import semtools_amd as smt

    x, nlist, sizes = _corpus(request.param)
    c = smt.Corpus(gpu_ctx)
    c.append(x)
    yield request.param, x, nlist, sizes, c
    c.close()


@pytest.fixture(scope="module", params=[False, True], ids=["pq", "lpca"])
def biting(request, corpus, tmp_path_factory):
    import semtools_amd as smt

    name, x, nlist, sizes, c = corpus
    ix = smt.IvfPq(c, nlist=nlist, train_iters=4, local_pca=request.param)
    path = tmp_path_factory.mktemp("ivf") / "biting.ivf"
    ix.save(path)
    f = R.read_index(path)
    if sizes is not None:                                       # the corpus was made to give these list lengths
        assert np.array_equal(ix.list_sizes(), np.array(sizes, dtype=np.uint64)), ix.list_sizes()
    if name == "tiny-lists":                                    # every list inside ONE 64-code group, i.e. one wave
        assert ix.list_sizes().max() <= 64, ix.list_sizes().max()
    yield name, x, c, ix, f
    ix.close()


_BEST = {}
POSITIONS = (0, 1, 63, 64, 255, 256, 8191, 8192, 8193, -2, -1)


def check_partial_oracle(x, f, qs, got, nprobe, top_k, rerank, own=None):
    """The three assertions of (b) for one call; returns (own rows that are certain, own rows looked at, queries set aside)."""
    list_of, pos_of = R.list_of_rows(f)
    off = f["offsets"].astype(np.int64)
    need = -(-rerank // 8)
    n_certain = n_own = aside = 0
    index_id = (f["kind"], hashlib.sha1(f["ids"].tobytes() + f["offsets"].tobytes()).digest())
    for qi, (q, (gr, gd)) in enumerate(zip(qs, got)):
        gr = gr.astype(np.int64)
        assert len(set(gr.tolist())) == len(gr) and (np.diff(gd) >= 0).all()
        for r, d in zip(gr, gd):                                                   # every returned distance is the exact one
            assert d == orc.cosine(q, x[r], accurate=True), (qi, r)
        lists, decided = R.probe_reference(q, f["centroids"], nprobe)
        if not decided:
            aside += 1
            continue
        assert np.isin(list_of[gr], lists).all(), (qi, "a returned row lies outside the probed lists")
        key = (index_id, q.tobytes(), tuple(lists.tolist()), top_k)
        if key not in _BEST:                                                       # (the same for every rerank on one index)
            cand = probed_rows(f, lists)
            _BEST[key] = top_rows(cand, exact_distances(x[cand], q), top_k)[0]
        best = _BEST[key]
        adc = {int(l): R.adc_distance(q, f, int(l)) for l in lists}
        for r in set(best.tolist()) | ({int(own[qi])} if own is not None else set()):
            l = int(list_of[r])
            if l not in adc:
                continue
            d, err = adc[l]
            p = int(pos_of[r] - off[l])
            certain = int(((d - err) <= (d[p] + err[p]) * (1 + 2.0 ** -7)).sum()) < need
            if own is not None and r == int(own[qi]):
                n_own += 1
                n_certain += certain
            if certain and r in best:
                assert r in gr, (qi, f"row {r} (list {l}, position {p}) is certain to be re-scored and in the exact top-{top_k}, but missing")
    return n_certain, n_own, aside


@pytest.mark.parametrize("rerank", [16, 64, 256])
def test_certain_rows_are_returned(biting, rerank):
    """Self-queries at the list positions where the scan changes path (wave and pass borders, the 8192-code segment border, the
    tail of a list that is longer than its segments) with nprobe 2, and 64 fresh queries.
    Data condition, for every (corpus, kind, rerank): at least 90 % of the self-queries' own rows are certain (it depends on the
    codebooks the GPU build produces; if it fails the data is wrong, not the kernel).  At rerank 16 only the single ADC-best row
    of a list is certain.  Observed share of certain own rows, the same at
    rerank 16, 64 and 256 and for both kinds: balanced 12 of 12, tiny-lists 6 of 6, segmented 19 of 19, one-long-list 19 of 19;
    no query set aside."""
    name, x, c, ix, f = biting
    off = f["offsets"].astype(np.int64)
    sizes = np.diff(off)
    own = []
    for l in sorted({int(np.argmax(sizes)), int(np.argsort(sizes)[len(sizes) // 2])}):
        for p in POSITIONS:
            p = p + sizes[l] if p < 0 else p
            if 0 <= p < sizes[l]:
                own.append(int(f["ids"][off[l] + p]))
    own = np.array(sorted(set(own)))
    own = own[np.abs(x[own]).sum(axis=1) > 0]
    got = ix.search(x[own], top_k=10, nprobe=2, rerank=rerank)
    n_certain, n_own, aside = check_partial_oracle(x, f, x[own], got, 2, 10, rerank, own=own)
    print(f"{name} kind {f['kind']} rerank {rerank}: own rows certain {n_certain} of {n_own}, set aside {aside} of {len(own)}")
    assert aside <= len(own) // 10, aside
    assert n_certain >= 0.9 * n_own, (n_certain, n_own)
    fresh = R.iso_rows(64, QSEED + 1)
    if name in ("segmented", "one-long-list"):                   # (clustered rows: a fresh unit vector is far from every topic)
        fresh = x[np.random.default_rng(9).choice(len(x), 64, replace=False)] + np.float32(0.02) * fresh
    got = ix.search(fresh, top_k=10, nprobe=2, rerank=rerank)
    _, _, aside = check_partial_oracle(x, f, fresh, got, 2, 10, rerank)
    assert aside <= 6, aside


@pytest.mark.parametrize("local_pca", [False, True], ids=["pq", "lpca"])
def test_zero_query_and_zero_rows(gpu_ctx, tmp_path, local_pca):
    """A zero query and zero corpus rows: the call succeeds and the returned pairs are exact."""
    import semtools_amd as smt

    x, nlist, _ = _corpus("tiny-lists")
    assert (np.abs(x).sum(axis=1) == 0).sum() == 3
    c = smt.Corpus(gpu_ctx)
    c.append(x)
    ix = smt.IvfPq(c, nlist=nlist, train_iters=4, local_pca=local_pca)
    ix.save(tmp_path / "zero.ivf")
    f = R.read_index(tmp_path / "zero.ivf")
    qs = np.stack([np.zeros(256, dtype=np.float32), R.iso_rows(1, 77)[0], x[6]])
    for nprobe, rerank in ((64, 512), (3, 64)):
        got = ix.search(qs, top_k=10, nprobe=nprobe, rerank=rerank)
        check_partial_oracle(x, f, qs, got, nprobe, 10, rerank)
        assert all(len(gr) == 10 for gr, _ in got)
    assert ix.list_sizes().max() <= 512
    every = ix.search(qs, top_k=56, nprobe=64, rerank=512)          # lists <= 512 rows: lossless, so this IS the exact search
    for (gr, gd), (er, ed) in zip(every, c.search(qs, top_k=56)):
        assert np.array_equal(gr, er) and gd.tobytes() == ed.tobytes()
    ix.close(); c.close()
