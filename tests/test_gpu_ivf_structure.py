"""GPU: what smt_ivfpq_build / smt_ivfpq_append WROTE, array by array.  The index is built on the GPU, saved (smt_ivfpq_save keeps
every device array), parsed with NumPy (tests/ivf_ref.py) and compared with a float64 reference computed from the corpus rows.
Recall thresholds pass with rows that were never encoded or sit in the wrong list; these checks do not.  Every tolerance is a
derived forward error bound of the format the kernel computes in (ivf_ref.py), none is measured."""
import itertools

import numpy as np
import pytest

from tests import ivf_ref as R

pytestmark = pytest.mark.gpu

N, NLIST, SEED = R.GPU_N, R.GPU_NLIST, R.GPU_SEED

MAX_AMBIGUOUS = 8          # near-tie rows of one list whose dealings the one-step test still enumerates (2^8 subsets)


@pytest.fixture(scope="module")
def rows():
    return R.iso_rows(N, SEED)


@pytest.fixture(scope="module", params=[False, True], ids=["pq", "lpca"])
def built(request, gpu_ctx, rows, tmp_path_factory):
    import semtools_amd as smt

    c = smt.Corpus(gpu_ctx)
    c.append(rows)
    ix = smt.IvfPq(c, nlist=NLIST, train_iters=4, local_pca=request.param)
    path = tmp_path_factory.mktemp("ivf") / "index.ivf"
    ix.save(path)
    yield rows, ix, R.read_index(path)
    ix.close(); c.close()


def check_lists(f, n_rows):
    off, ids = f["offsets"].astype(np.int64), f["ids"].astype(np.int64)
    assert f["n_rows"] == n_rows and off[0] == 0 and off[-1] == n_rows and (np.diff(off) >= 0).all()
    assert np.array_equal(np.sort(ids), np.arange(n_rows))                         # a permutation: every row exactly once
    inside = np.ones(n_rows, dtype=bool)
    inside[off[1:-1][off[1:-1] < n_rows]] = False                                  # (positions where a new list starts)
    assert (np.diff(ids)[inside[1:]] > 0).all()                                    # ascending inside every list


def check_assignment(x, list_of, f, coef):
    """Every row sits in a list whose float64 score is within the derived bound of the best one; returns how many are not in the
    float64 arg-max itself."""
    con = R.contenders(x, f["centroids"], coef)
    bad = np.nonzero(~con[np.arange(len(x)), list_of])[0]
    assert bad.size == 0, f"{bad.size} rows sit in a list that is not their nearest (first: row {bad[:5]})"
    return int((list_of != np.argmax(R.assign_scores(x, f["centroids"]), axis=1)).sum())


def check_codes(x, rows_idx, list_of, pos_of, f):
    """The code checks of either kind for the corpus rows `rows_idx`."""
    lists, codes = list_of[rows_idx], f["codes"][pos_of[rows_idx]]
    if f["kind"] == 0:
        resid = x[rows_idx].astype(np.float64) - f["centroids"].astype(np.float64)[lists]
        slack, bound = R.pq_code_slack(resid, f["codebooks"], codes)
        bad = np.argwhere(slack > bound)
        assert bad.size == 0, f"{len(bad)} (row, subspace) codes are not the nearest codeword (first: {bad[:3].tolist()})"
        return float((slack > 0).mean())
    want = R.lpca_codes(x[rows_idx], lists, f)
    diff = np.abs(codes.view(np.int8).astype(np.int64) - want)
    assert diff.max() <= 1, f"a code byte is off by {diff.max()}"
    share = float((diff != 0).mean())
    assert share < 0.01, share
    return share


def test_lists_partition_the_rows_in_order(built):
    x, ix, f = built
    check_lists(f, N)
    assert f["nlist"] == NLIST and np.array_equal(ix.list_sizes(), np.diff(f["offsets"]))


def test_every_row_sits_in_its_nearest_list(built):
    """Against the FINAL centroids of the file (the build assigns all rows after the last update), no exclusions.  The build's
    assignment multiplies bf16 x 3 split products (tuning key gemm_bf16x3, the default), so the bound takes its constants from that
    format (ivf_ref.BF16X3_COEF), not from f32.  Observed: 0 rows outside the float64 arg-max."""
    x, ix, f = built
    list_of, _ = R.list_of_rows(f)
    print("rows outside the float64 arg-max:", check_assignment(x, list_of, f, R.BF16X3_COEF))


def test_cnorm_half(built):
    x, ix, f = built
    c = f["centroids"].astype(np.float64)
    want = 0.5 * np.sum(c * c, axis=1)
    assert (np.abs(f["cnorm_half"].astype(np.float64) - want) <= R.gamma(R.DIM) * want + R.U32 * want).all()


def test_f32_assignment_meets_the_f32_bound(rows, tmp_path):
    """The same with the assignment on f32 MFMAs (gemm_bf16x3 = 0): plain f32 products, so dot_bound's gamma_256 with u = 2^-24.
    On a context of its own: the tuning of the shared one stays as it is."""
    import semtools_amd as smt

    ctx = smt.Context(0)
    ctx.set_tuning("gemm_bf16x3", 0)
    c = smt.Corpus(ctx)
    c.append(rows)
    ix = smt.IvfPq(c, nlist=NLIST, train_iters=4, local_pca=True)
    ix.save(tmp_path / "f32.ivf")
    f = R.read_index(tmp_path / "f32.ivf")
    ix.close(); c.close(); ctx.close()
    check_lists(f, N)
    check_assignment(rows, R.list_of_rows(f)[0], f, R.F32_COEF)


def test_codes(built):
    """Kind 0 (pq_assign_kernel): for every row and each of the 32 subspaces the stored code's float64 distance to the residual
    x - c_list is within the derived f32 bound of the minimum over the 256 codewords -- a row whose code was never written fails.
    Observed share of codes that are not the float64 arg-min itself: 0.

    Kind 1 (lpca_encode_kernel): code_k = clamp(rint((Q_l[k] . (x - c_l)) / scale_l[k]), -127, 127) as a signed byte, rint = round
    half to even, Q_l / scale_l the list's basis and scales from the file.  Every stored byte is within +-1 of that formula's float64
    value (f32 rounding at a .5 boundary) and fewer than 1 % of the bytes differ at all.  Observed share that differs: 0."""
    x, ix, f = built
    list_of, pos_of = R.list_of_rows(f)
    print("kind", f["kind"], "share of codes that differ from the float64 choice:", check_codes(x, np.arange(N), list_of, pos_of, f))


@pytest.mark.parametrize("local_pca", [False, True], ids=["pq", "lpca"])
def test_one_kmeans_step(gpu_ctx, rows, tmp_path, local_pca):
    """train_iters = 1 over the whole corpus as the sample: the file's centroids are ONE Lloyd step away from the documented
    starting rows (row l * (N / nlist): gather_rows_kernel with stride * (S / nlist)).  The float64 assignment to those rows says
    which rows a list certainly has; a near-tie row (under the bf16 x 3 bound) may be in any of its contending lists.  The file's
    centroid must equal the float64 mean of the certain members plus SOME dealing of the list's near-tie rows, within
    count * 2^-32 + u |mean| per component (fixed-point accumulation, one f32 rounding).  A list with more than MAX_AMBIGUOUS
    near-tie rows is left out, at most 10 % of the lists (observed: none; tests/test_ivf_ref_cpu.py checks the seed).  No list can
    come out empty here (a starting row is its own nearest): test_empty_list_keeps_its_centroid makes one."""
    import semtools_amd as smt

    c = smt.Corpus(gpu_ctx)
    c.append(rows)
    ix = smt.IvfPq(c, nlist=NLIST, train_iters=1, train_sample=N, local_pca=local_pca)
    ix.save(tmp_path / "one.ivf")
    f = R.read_index(tmp_path / "one.ivf")
    ix.close(); c.close()
    _, start = R.build_sample(N, NLIST, N)
    assert np.array_equal(start, np.arange(NLIST) * (N // NLIST))
    x64 = rows.astype(np.float64)
    con = R.contenders(rows, rows[start], R.BF16X3_COEF)
    decided = con.sum(axis=1) == 1
    left_out = 0
    for l in range(NLIST):
        sure = np.nonzero(decided & con[:, l])[0]
        maybe = np.nonzero(~decided & con[:, l])[0]
        if len(maybe) > MAX_AMBIGUOUS:
            left_out += 1
            continue
        got = f["centroids"][l].astype(np.float64)
        base = x64[sure].sum(axis=0)
        ok = False
        for take in itertools.product((False, True), repeat=len(maybe)):
            members = maybe[np.array(take, dtype=bool)] if len(maybe) else maybe
            count = len(sure) + len(members)
            mean = (base + x64[members].sum(axis=0)) / count
            ok = ok or bool((np.abs(got - mean) <= count * 2.0 ** -32 + R.U32 * np.abs(mean)).all())
        assert ok, f"list {l}: the centroid is not the mean of its members ({len(sure)} certain, {len(maybe)} near-tie rows)"
    assert left_out <= NLIST // 10, left_out


def test_empty_list_keeps_its_centroid(gpu_ctx, rows, tmp_path):
    """ivf_finalize_kernel writes a centroid only when its count is non-zero: "empty cluster keeps its centroid".  The starting row of
    list 1 is made a copy of list 0's: both centroids score every row alike, ties go to the smaller list id, so the one k-means step
    gives list 1 no member and its centroid stays the starting row, bit for bit, while list 0's moves to the mean of its members."""
    import semtools_amd as smt

    x = rows.copy()
    _, start = R.build_sample(N, NLIST, N)
    x[start[1]] = x[start[0]]
    c = smt.Corpus(gpu_ctx)
    c.append(x)
    ix = smt.IvfPq(c, nlist=NLIST, train_iters=1, train_sample=N, local_pca=True)
    ix.save(tmp_path / "empty.ivf")
    f = R.read_index(tmp_path / "empty.ivf")
    ix.close(); c.close()
    assert f["centroids"][1].tobytes() == x[start[1]].tobytes()
    assert np.linalg.norm(f["centroids"][0].astype(np.float64)) < 0.5          # a mean of ~200 unit rows, no longer the unit starting row
    assert (np.abs(np.linalg.norm(f["centroids"][2:].astype(np.float64), axis=1)) < 0.5).all()


@pytest.mark.parametrize("local_pca", [False, True], ids=["pq", "lpca"])
def test_append_keeps_old_rows_and_places_new_ones(gpu_ctx, rows, tmp_path, local_pca):
    import semtools_amd as smt

    n_old = 10000
    c = smt.Corpus(gpu_ctx)
    c.append(rows[:n_old])
    ix = smt.IvfPq(c, nlist=NLIST, train_iters=4, local_pca=local_pca)
    ix.save(tmp_path / "before.ivf")
    c.append(rows[n_old:])
    assert ix.append() == N - n_old
    ix.save(tmp_path / "after.ivf")
    a, b = R.read_index(tmp_path / "before.ivf"), R.read_index(tmp_path / "after.ivf")
    assert np.array_equal(ix.list_sizes(), np.diff(b["offsets"]))
    ix.close(); c.close()
    check_lists(a, n_old)
    check_lists(b, N)                                                              # ids still ascend inside every list
    for key in ("centroids", "cnorm_half", "codebooks") + (("basis", "lscale") if local_pca else ()):
        assert a[key].tobytes() == b[key].tobytes(), key                          # no retraining
    la, pa = R.list_of_rows(a)
    lb, pb = R.list_of_rows(b)
    assert np.array_equal(lb[:n_old], la)                                          # every old row keeps its list ...
    assert np.array_equal(b["codes"][pb[:n_old]], a["codes"][pa])                  # ... and its 32 code bytes
    new = np.arange(n_old, N)
    check_assignment(rows[new], lb[new], b, R.BF16X3_COEF)
    check_codes(rows, new, lb, pb, b)


def test_sharded_build_shares_its_centroids(rows, tmp_path):
    """Three logical ranks on one GPU, shared_centroids: the centroid block of every shard's file is bit-identical, and each
    shard's lists partition ITS rows, every row in its nearest list."""
    import semtools_amd as smt

    g = smt.Group.logical(0, 3)
    sc = smt.ShardedCorpus(g, rows=rows)
    six = smt.ShardedIvfPq(sc, nlist=NLIST, train_iters=4, local_pca=False, shared_centroids=True)
    six.save(tmp_path / "sharded.ivf")
    counts = [int(v) for v in sc.rank_rows()]
    sizes = [six.shard_list_sizes(r, NLIST) for r in range(3)]
    six.close(); sc.close(); g.close()
    assert sum(counts) == N
    files = [R.read_index(f"{tmp_path / 'sharded.ivf'}.r{r}of3") for r in range(3)]
    first = 0
    for r, f in enumerate(files):
        assert f["centroids"].tobytes() == files[0]["centroids"].tobytes() and f["cnorm_half"].tobytes() == files[0]["cnorm_half"].tobytes()
        check_lists(f, counts[r])
        assert np.array_equal(sizes[r], np.diff(f["offsets"]))
        mine = rows[first:first + counts[r]]                                      # (made in one go: contiguous row ranges)
        list_of, pos_of = R.list_of_rows(f)
        check_assignment(mine, list_of, f, R.BF16X3_COEF)
        check_codes(mine, np.arange(counts[r]), list_of, pos_of, f)
        first += counts[r]
