"""CPU: pins tests/ivf_ref.py (the parser, the float64 reference and the bounds the GPU tests of the IVF index rely on) without a
GPU: a tiny index is built entirely in NumPy, written in the file format, read back, and every reference function is compared
with brute force written out coordinate by coordinate.  Also the data preconditions of the GPU tests that depend on the corpus
alone (near-tie shares under the derived bounds) are checked here, on centroids from a NumPy k-means."""
import functools

import numpy as np
import pytest

from tests import ivf_ref as R

N, NLIST = 2000, 32


@functools.lru_cache(maxsize=None)
def _tiny_index(kind):
    x = R.iso_rows(N, seed=7)
    x64 = x.astype(np.float64)
    cent = R.numpy_kmeans(x, NLIST, 3).astype(np.float32)
    a = np.argmax(R.assign_scores(x, cent), axis=1)
    ids = np.argsort(a, kind="stable").astype(np.uint32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=NLIST))]).astype(np.uint64)
    resid = x64[ids] - cent.astype(np.float64)[a[ids]]
    ix = dict(nlist=NLIST, n_rows=N, kind=kind, centroids=cent,
              cnorm_half=(0.5 * np.sum(cent.astype(np.float64) ** 2, axis=1)).astype(np.float32), offsets=offsets, ids=ids)
    rng = np.random.default_rng(3)
    cb = np.zeros((R.PQ_M, R.PQ_K, R.PQ_DSUB), dtype=np.float32)
    if kind == 0:
        r = resid.reshape(N, R.PQ_M, R.PQ_DSUB)
        cb = r[rng.choice(N, R.PQ_K, replace=False)].transpose(1, 0, 2).copy()          # start: residuals of 256 rows
        for _ in range(2):                                                                # hand-rolled PQ k-means
            code = np.argmin(R.pq_nearest(resid, cb), axis=2)
            for s in range(R.PQ_M):
                for k in np.unique(code[:, s]):
                    cb[s, k] = r[code[:, s] == k, s].mean(axis=0)
        cb = cb.astype(np.float32)
        ix["codes"] = np.argmin(R.pq_nearest(resid, cb), axis=2).astype(np.uint8)
    else:
        basis = np.zeros((NLIST, R.LP_DIMS, R.DIM), dtype=np.float32)
        lscale = np.ones((NLIST, R.LP_DIMS), dtype=np.float32)
        for l in range(NLIST):
            rl = resid[int(offsets[l]):int(offsets[l + 1])]
            _, sv, vt = np.linalg.svd(rl, full_matrices=False)
            basis[l] = vt[:R.LP_DIMS]
            lscale[l] = np.maximum(4.0 * sv[:R.LP_DIMS] / np.sqrt(len(rl)), 1e-12) / 127.0
        ix["basis"], ix["lscale"] = basis, lscale
        ix["codes"] = R.lpca_codes(x[ids], a[ids], ix).astype(np.int8).view(np.uint8)
    ix["codebooks"] = cb
    return x, ix


@pytest.fixture(scope="module", params=[0, 1])
def tiny(request, tmp_path_factory):
    x, ix = _tiny_index(request.param)
    path = tmp_path_factory.mktemp("ivf") / f"tiny{request.param}.ivf"
    R.write_index(path, ix)
    return x, ix, path


def test_file_round_trip_and_refusals(tiny, tmp_path):
    x, ix, path = tiny
    back = R.read_index(path)
    assert path.stat().st_size == R.index_file_size(NLIST, N, ix["kind"])
    for key, val in ix.items():
        assert np.array_equal(back[key], val), key
    assert back["centroids"].dtype == np.float32 and back["offsets"].dtype == np.uint64 and back["codes"].shape == (N, 32)
    blob = path.read_bytes()
    for name, bad in (("magic", b"NOTANIDX" + blob[8:]), ("short", blob[:-1]), ("long", blob + b"\0"),
                      ("dim", blob[:20] + (128).to_bytes(4, "little") + blob[24:]),
                      ("nlist", blob[:8] + (40).to_bytes(4, "little") + blob[12:]),
                      ("rows", blob[:24] + (N + 1).to_bytes(8, "little") + blob[32:])):
        (tmp_path / name).write_bytes(bad)
        with pytest.raises(ValueError):
            R.read_index(tmp_path / name)
    list_of, pos_of = R.list_of_rows(back)
    for row in (0, 1, 999, N - 1):
        p = int(np.nonzero(back["ids"] == row)[0][0])
        assert pos_of[row] == p and back["offsets"][list_of[row]] <= p < back["offsets"][list_of[row] + 1]


def test_assign_scores_and_dot_bound_against_brute_force(tiny):
    x, ix, _ = tiny
    s = R.assign_scores(x[:5], ix["centroids"])
    for i in range(5):
        for l in (0, 7, NLIST - 1):
            c = [float(v) for v in ix["centroids"][l]]
            want = sum(float(a) * b for a, b in zip(x[i], c)) - 0.5 * sum(b * b for b in c)
            assert abs(s[i, l] - want) < 1e-14
    # every row of the NumPy index sits in its float64 arg-max list
    list_of, _ = R.list_of_rows(ix)
    assert np.array_equal(list_of, np.argmax(R.assign_scores(x, ix["centroids"]), axis=1))
    a, b = x[3], ix["centroids"][4]
    g = 256 * 2.0 ** -24 / (1 - 256 * 2.0 ** -24)
    assert R.dot_bound(a, b) == pytest.approx(g * sum(abs(float(p) * float(q)) for p, q in zip(a, b)), rel=1e-12)
    assert R.dot_bound(x[:4], ix["centroids"][:4]).shape == (4,)
    assert np.allclose(R.pair_abs(x[:4], ix["centroids"])[2, 5] * g, R.dot_bound(x[2], ix["centroids"][5]), rtol=1e-12)
    # the bound really bounds f32 arithmetic: a sequential f32 dot product against the float64 one
    f32 = np.float32(0)
    for p, q in zip(a, b):
        f32 = np.float32(f32 + np.float32(p * q))
    assert abs(float(f32) - float(a.astype(np.float64) @ b.astype(np.float64))) <= R.dot_bound(a, b)
    assert R.BF16X3_COEF > R.F32_COEF and 9.0e-5 < R.BF16X3_COEF < 9.5e-5


def test_pq_nearest_and_code_slack():
    x, ix = _tiny_index(0)
    list_of, _ = R.list_of_rows(ix)
    rows = ix["ids"].astype(np.int64)
    resid = x[rows].astype(np.float64) - ix["centroids"].astype(np.float64)[list_of[rows]]
    d = R.pq_nearest(resid[:3], ix["codebooks"])
    assert d.shape == (3, 32, 256)
    for i, s, k in ((0, 0, 0), (1, 31, 255), (2, 13, 77)):
        want = sum((resid[i, s * 8 + j] - float(ix["codebooks"][s, k, j])) ** 2 for j in range(8))
        assert abs(d[i, s, k] - want) < 1e-15
    slack, bound = R.pq_code_slack(resid, ix["codebooks"], ix["codes"])
    assert (slack == 0).all() and (bound > 0).all() and bound.max() < 1e-6
    wrong = ix["codes"].copy()
    wrong[17, 5] ^= 1                                              # one code of one row is not the nearest codeword
    slack, bound = R.pq_code_slack(resid, ix["codebooks"], wrong)
    assert ((slack > bound) == (np.arange(N)[:, None] == 17) & (np.arange(32)[None, :] == 5)).all()
    unwritten = ix["codes"].copy()
    unwritten[1000:] = 0                                           # rows an encoder never reached
    slack, bound = R.pq_code_slack(resid, ix["codebooks"], unwritten)
    assert (slack > bound)[1000:].any(axis=1).all()


def test_adc_distance_against_brute_force(tiny):
    x, ix, _ = tiny
    q = R.iso_rows(2, seed=11)[1] * np.float32(3.0)
    qh = [float(v) for v in q.astype(np.float64) / np.linalg.norm(q.astype(np.float64))]
    for l in (0, 5, NLIST - 1):
        d, err = R.adc_distance(q, ix, l)
        b, e = int(ix["offsets"][l]), int(ix["offsets"][l + 1])
        assert d.shape == err.shape == (e - b,) and (err > 0).all() and err.max() < 2e-3      # (far below the 2^-7 d of the 16-bit selection)
        c = ix["centroids"][l]
        for p in (b, e - 1):
            score = sum(a * float(v) for a, v in zip(qh, c))
            for s in range(32):
                code = int(ix["codes"][p, s])
                if ix["kind"] == 0:
                    score += sum(qh[8 * s + j] * float(ix["codebooks"][s, code, j]) for j in range(8))
                else:
                    proj = sum(a * float(v) for a, v in zip(qh, ix["basis"][l, s]))
                    score += float(ix["lscale"][l, s]) * proj * (code - 256 if code > 127 else code)
            assert abs(d[p - b] - max(1.0 - score, 0.0)) < 1e-13
    # the ADC distance approximates the true one (the codes describe the rows): rank correlation inside a list
    l = 3
    d, _ = R.adc_distance(q, ix, l)
    rows = ix["ids"][int(ix["offsets"][l]):int(ix["offsets"][l + 1])]
    true = 1.0 - x[rows].astype(np.float64) @ np.array(qh)
    assert np.corrcoef(d, true)[0, 1] > (0.5 if ix["kind"] == 0 else 0.3)


def test_lpca_codes_formula():
    x, ix = _tiny_index(1)
    list_of, _ = R.list_of_rows(ix)
    for p in (0, 555, N - 1):
        row, l = int(ix["ids"][p]), int(list_of[ix["ids"][p]])
        r = x[row].astype(np.float64) - ix["centroids"][l].astype(np.float64)
        for k in (0, 9, 31):
            y = sum(float(a) * b for a, b in zip(ix["basis"][l, k], r)) / float(ix["lscale"][l, k])
            want = int(min(max(round(y), -127), 127))               # (Python's round is half-to-even too)
            assert int(ix["codes"].view(np.int8)[p, k]) == want


def test_probe_reference(tiny):
    x, ix, _ = tiny
    q = R.iso_rows(3, seed=12)[2]
    c = ix["centroids"].astype(np.float64)
    score = np.array([0.5 * sum(v * v for v in cl) - sum(a * b for a, b in zip(cl, q.astype(np.float64) / np.linalg.norm(q.astype(np.float64))))
                      for cl in c])
    for nprobe in (1, 5, NLIST):
        lists, decided = R.probe_reference(q, ix["centroids"], nprobe)
        assert sorted(lists.tolist()) == sorted(np.argsort(score, kind="stable")[:nprobe].tolist())
    assert R.probe_reference(q, ix["centroids"], NLIST)[1] is True
    twin = ix["centroids"].copy()
    order = np.argsort(score)
    twin[order[1]] = twin[order[0]]                                  # two equal centroids: ties go to the smaller list id ...
    lists, decided = R.probe_reference(q, twin, 1)
    assert lists.tolist() == [min(int(order[0]), int(order[1]))] and decided is False       # ... and the choice is not decided
    assert R.probe_reference(q * np.float32(0.01), ix["centroids"], 5)[0].tolist() == R.probe_reference(q, ix["centroids"], 5)[0].tolist()


# ------------------------------------------------------------------------------------------------ data preconditions of the GPU tests
GPU_N, GPU_NLIST, GPU_SEED, GPU_QSEED = R.GPU_N, R.GPU_NLIST, R.GPU_SEED, R.GPU_QSEED


@pytest.fixture(scope="module")
def gpu_corpus():
    x = R.iso_rows(GPU_N, GPU_SEED)
    return x, R.numpy_kmeans(x, GPU_NLIST, 4)


def test_gpu_corpus_lists_are_balanced(gpu_corpus):
    """The lossless regime of the search contract needs every list to fit one block's shortlists (512 rows)."""
    x, cent = gpu_corpus
    sizes = np.bincount(np.argmax(R.assign_scores(x, cent), axis=1), minlength=GPU_NLIST)
    assert sizes.min() >= 64 and sizes.max() <= 384, (sizes.min(), sizes.max())


def test_gpu_queries_are_rarely_near_ties_of_the_probe(gpu_corpus):
    """At most 10 % of the queries may be set aside because their nprobe-th and (nprobe+1)-th lists lie within the f32 bound.
    Observed on these centroids: 0 of 64 at every nprobe."""
    x, cent = gpu_corpus
    qs = R.iso_rows(64, GPU_QSEED)
    for nprobe in (1, 2, 7, 32, 64):
        aside = sum(not R.probe_reference(q, cent.astype(np.float32), nprobe)[1] for q in qs)
        assert aside <= 6, (nprobe, aside)


def test_one_kmeans_step_near_ties(gpu_corpus):
    """One k-means step from the documented starting rows (train_sample = N).  Under the bf16 x 3 bound of the build's assignment
    70 of 12 288 rows are near-ties and they touch 55 of the 64 lists (even the f32 bound leaves 23 lists touched): on isotropic
    rows, leaving out every list with a near-tie member would leave out almost all of them.  The GPU test therefore checks such a
    list too -- against every way of dealing its few near-tie rows -- and leaves a list out only when it has more than
    MAX_AMBIGUOUS of them; that share is what stays under the 10 % cap (observed: 0 lists)."""
    x, _ = gpu_corpus
    _, start = R.build_sample(GPU_N, GPU_NLIST, GPU_N)
    con = R.contenders(x, x[start], R.BF16X3_COEF)
    amb = con.sum(axis=1) > 1
    per_list = con[amb].sum(axis=0)
    assert 0 < amb.sum() < 200 and per_list.max() <= 8 and (per_list > 8).sum() <= GPU_NLIST // 10, (amb.sum(), per_list.max())
    assert con[np.arange(GPU_N), np.argmax(R.assign_scores(x, x[start]), axis=1)].all()
    assert con[start, np.arange(GPU_NLIST)].all()                   # no list can come out empty: a starting row is its own nearest
