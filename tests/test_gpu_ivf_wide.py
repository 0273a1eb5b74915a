"""GPU: the wide IVF searches (smt_ivfpq_search_wide, its device form, smt_sharded_ivfpq_search_wide): top_k 57 ... 1024 answered
from a per-query candidate pool.

The header defines the answer: with C the rows the scan re-scores (the set the narrow route draws from), S the
kg = min(|C|, top_k + max(64, top_k / 16)) rows of C with the smallest (f32 distance, row) keys, it is the top_k best of S by
(exact f64 distance, row).  Where every list is re-scored entirely (lists <= 512 rows, rerank 512) C is the rows of the probed lists
and the answer is their exact top_k: rows equal, distances bit-equal -- for S to lose a row of the exact top_k, f32 (error bound
F32_ERR_SCAN = 4e-6) would have to misplace it by more than the guard of at least 64 positions.
The corpus, seeds, query sets and the float64 probe reference are those of tests/test_gpu_ivf_search_contract.py."""
import ctypes as C

import numpy as np
import pytest

from tests import ivf_ranges_ref as G
from tests import ivf_ref as R
from tests.test_gpu_ivf_search_contract import (biting, check_partial_oracle, corpus, exact_distances, probed_rows,  # noqa: F401
                                                _corpus, top_rows)

pytestmark = pytest.mark.gpu

N, NLIST, SEED, QSEED = R.GPU_N, R.GPU_NLIST, R.GPU_SEED, R.GPU_QSEED
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
WIDE_K = (57, 64, 100, 512, 1024)


def search(ix, ctx, entry, qs, top_k, nprobe, rerank, row_base=0, ranges=None, wide=True):
    """[(rows, dist)] per query through the host entry point or the device one (whose padding is checked here)."""
    if entry == "host":
        return ix.search(qs, top_k=top_k, nprobe=nprobe, rerank=rerank, row_base=row_base, ranges=ranges, wide=wide)
    import torch

    nq = len(qs)
    qd = torch.from_numpy(np.ascontiguousarray(qs, dtype=np.float32)).cuda()
    rows = torch.zeros((nq, top_k), dtype=torch.int64, device="cuda")
    dist = torch.zeros((nq, top_k), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ix.search_device(qd.data_ptr(), nq, top_k, nprobe, rerank, row_base, rows.data_ptr(), dist.data_ptr(), ranges=ranges, wide=wide)
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


def head(a, k):
    return [(r[:k], d[:k]) for r, d in a]


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
    assert ix.list_sizes().max() <= 512
    yield rows, c, ix, R.read_index(path)
    ix.close(); c.close()


_CAND = {}


def candidates(f, tag, qs, nprobe):
    """Per query the rows of the float64 probe's lists, or None when the probe is undecided (once per index kind, set and nprobe)."""
    key = (f["kind"], tag, nprobe)
    if key not in _CAND:
        out = []
        for q in qs:
            lists, decided = R.probe_reference(q, f["centroids"], nprobe)
            out.append(probed_rows(f, lists) if decided else None)
        aside = sum(c is None for c in out)
        assert aside <= len(qs) // 10, (tag, nprobe, aside)
        _CAND[key] = out
    return _CAND[key]


def expect(cand, dist_all, top_k, ranges=None):
    inside = G.in_ranges(np.arange(dist_all.shape[1]), ranges) if ranges is not None else None
    out = []
    for c, d in zip(cand, dist_all):
        if c is None:
            out.append(None)
            continue
        if inside is not None:
            c = c[inside[c]]
        out.append(top_rows(c, d[c], top_k))
    return out


def check(got, want, row_base, where):
    assert len(got) <= len(want)
    for qi, ((gr, gd), w) in enumerate(zip(got, want)):
        if w is None:
            continue
        assert np.array_equal(gr, (w[0] + row_base).astype(np.uint64)), (where, qi, len(gr), len(w[0]))
        assert gd.tobytes() == w[1].tobytes(), (where, qi)


# ================================================================================================ 1. the lossless regime
@pytest.mark.parametrize("row_base", [0, (1 << 33) + 5])
@pytest.mark.parametrize("entry", ["host", "device"])
def test_lossless_regime_is_the_exact_top_k_of_the_probed_lists(small, gpu_ctx, query_sets, entry, row_base):
    """Lists <= 512 rows and rerank = 512: rows equal and distance bytes equal to the exact top-k over the rows of the float64
    probe's lists.  nprobe 1 holds fewer rows than k (a short answer and its padding), 2 gives a pool of 2 x 512 slots (the direct
    path of the finish), 7 and above the radix select; nq around the groups of eight of the ADC grid."""
    x, c, ix, f = small
    short = direct = radix = 0
    for name, (qs, dist_all) in query_sets.items():
        for nprobe in (1, 2, 7, 32, 64):
            cand = candidates(f, name, qs, nprobe)
            for top_k in WIDE_K:
                want = expect(cand, dist_all, top_k)
                for nq in ((1, 7, 8, 9, 64) if name == "fresh" else (9,)):
                    got = search(ix, gpu_ctx, entry, qs[:nq], top_k, nprobe, 512, row_base)
                    assert len(got) == nq
                    check(got, want, row_base, (name, nprobe, top_k, nq))
                short += sum(w is not None and len(w[0]) < top_k for w in want)
            sizes = [len(cd) for cd in cand if cd is not None]
            direct += sum(s <= 2048 for s in sizes)
            radix += sum(s > 2048 for s in sizes)
    assert short and direct and radix, (short, direct, radix)     # every path of the finish was taken


def test_probing_every_list_equals_the_exact_large_k_search(small, query_sets):
    x, c, ix, f = small
    for name, (qs, _) in query_sets.items():
        for top_k in WIDE_K:
            assert same(ix.search(qs, top_k=top_k, nprobe=NLIST, rerank=512, wide=True), c.search(qs, top_k=top_k)), (name, top_k)


# ================================================================================================ 2. narrow and wide agree
@pytest.mark.parametrize("entry", ["host", "device"])
def test_wide_up_to_56_is_the_narrow_call(small, gpu_ctx, query_sets, entry):
    x, c, ix, f = small
    qs = query_sets["fresh"][0][:9]
    for rerank in (16, 512):
        for nprobe in (1, 7, 64):
            for top_k in (1, 10, 56):
                narrow = search(ix, gpu_ctx, entry, qs, top_k, nprobe, rerank, wide=False)
                assert same(narrow, search(ix, gpu_ctx, entry, qs, top_k, nprobe, rerank, wide=True)), (rerank, nprobe, top_k)
                ranged = search(ix, gpu_ctx, entry, qs, top_k, nprobe, rerank, ranges=[(100, 9000)], wide=False)
                assert same(ranged, search(ix, gpu_ctx, entry, qs, top_k, nprobe, rerank, ranges=[(100, 9000)], wide=True))


def test_first_56_of_a_wide_answer_are_the_narrow_answer_lossless(small, query_sets):
    x, c, ix, f = small
    qs = query_sets["fresh"][0]
    for nprobe in (2, 32):
        narrow = ix.search(qs, top_k=56, nprobe=nprobe, rerank=512)
        for top_k in (57, 300):
            assert same(head(ix.search(qs, top_k=top_k, nprobe=nprobe, rerank=512, wide=True), 56), narrow), (nprobe, top_k)


def _biting_queries(name, x):
    fresh = R.iso_rows(16, QSEED + 1)
    if name in ("segmented", "one-long-list"):                  # (clustered rows: a fresh unit vector is far from every topic)
        fresh = x[np.random.default_rng(9).choice(len(x), 16, replace=False)] + np.float32(0.02) * fresh
    return fresh


@pytest.mark.parametrize("rerank", [16, 64, 256])
def test_first_56_of_a_wide_answer_are_the_narrow_answer_where_the_shortlist_bites(biting, rerank):
    """Both routes draw from the same re-scored rows C.  The narrow route keeps the 64 best of a block by f32 and ranks 56 exactly;
    the wide one keeps the k + guard best of all blocks.  A difference in the first 56 would need nine f32 misorderings in one block."""
    name, x, c, ix, f = biting
    qs = _biting_queries(name, x)
    narrow = ix.search(qs, top_k=56, nprobe=2, rerank=rerank)
    for top_k in (57, 300):
        wide = ix.search(qs, top_k=top_k, nprobe=2, rerank=rerank, wide=True)
        assert same(head(wide, 56), narrow), (name, rerank, top_k)


@pytest.mark.parametrize("rerank", [16, 64, 256])
def test_partial_oracle_guarantees_hold_at_100(biting, rerank):
    """check_partial_oracle at top_k = 100: certain rows are returned, every returned row lies in a probed list, every distance is
    exact, the list is sorted and free of duplicates; ties in distance come in row order."""
    name, x, c, ix, f = biting
    qs = _biting_queries(name, x)
    got = ix.search(qs, top_k=100, nprobe=2, rerank=rerank, wide=True)
    _, _, aside = check_partial_oracle(x, f, qs, got, 2, 100, rerank)
    assert aside <= len(qs) // 10, aside
    for gr, gd in got:
        tie = np.diff(gd) == 0
        assert (np.diff(gr.astype(np.int64))[tie] > 0).all()


# ================================================================================================ 3. inside ranges
@pytest.mark.parametrize("entry", ["host", "device"])
def test_ranges_lossless_and_in_range_only(small, gpu_ctx, query_sets, entry):
    x, c, ix, f = small
    qs, dist_all = query_sets["fresh"]
    qs, dist_all = qs[:9], dist_all[:9]
    sets = dict(alternate=G.alternate_blocks(N), scattered=G.scattered_rows(N), empties=G.with_empty_members(N), whole=[(0, N)])
    for sname, ranges in sets.items():
        for nprobe in (2, 32, 64):
            want = expect(candidates(f, "fresh9", qs, nprobe), dist_all, 100, ranges)
            got = search(ix, gpu_ctx, entry, qs, 100, nprobe, 512, ranges=ranges)
            check(got, want, 0, (sname, nprobe))
            for gr, _ in got:
                assert G.in_ranges(gr.astype(np.int64), ranges).all(), (sname, nprobe)
    for empty in ([], [(5, 5), (9, 9)]):                          # an empty filter: an empty answer
        assert all(len(gr) == 0 for gr, _ in search(ix, gpu_ctx, entry, qs, 100, 7, 512, ranges=empty))


@pytest.mark.parametrize("local_pca", [False, True], ids=["pq", "lpca"])
def test_decoys_outside_both_ends_of_the_ranges_are_never_returned(gpu_ctx, rows, query_sets, local_pca):
    """Copies of the nine queries themselves (distance 0: each wins its query) sit in the nine rows before the range and the nine
    rows behind it.  Every list is probed and re-scored entirely, so the answer is the exact filtered top-100 -- without a decoy."""
    import semtools_amd as smt

    qs = query_sets["fresh"][0][:9]
    a, b = 3000, 9000
    x = rows.copy()
    x[a - 9:a] = qs
    x[b:b + 9] = qs
    c = smt.Corpus(gpu_ctx)
    c.append(x)
    ix = smt.IvfPq(c, nlist=NLIST, train_iters=4, local_pca=local_pca)
    assert ix.list_sizes().max() <= 512
    for qi, (gr, _) in enumerate(ix.search(qs, top_k=100, nprobe=NLIST, rerank=512, wide=True)):      # (unfiltered, the decoys do win)
        assert gr[:2].tolist() == [a - 9 + qi, b + qi], (qi, gr[:2])
    for entry in ("host", "device"):
        got = search(ix, gpu_ctx, entry, qs, 100, NLIST, 512, ranges=[(a, b)])
        assert same(got, c.search(qs, top_k=100, ranges=[(a, b)])), entry
        for gr, gd in got:
            assert len(gr) == 100 and ((gr >= a) & (gr < b)).all()
    ix.close(); c.close()


# ================================================================================================ 4. duplicates, degenerate inputs
@pytest.mark.parametrize("local_pca", [False, True], ids=["pq", "lpca"])
def test_rows_stored_three_times_come_back_in_row_order(gpu_ctx, local_pca):
    import semtools_amd as smt

    x = R.iso_rows(4096, SEED + 2)
    dup = np.arange(64) * 50
    x[1000:1064] = x[dup]
    x[3000:3064] = x[dup]
    c = smt.Corpus(gpu_ctx)
    c.append(x)
    ix = smt.IvfPq(c, nlist=32, train_iters=4, local_pca=local_pca)
    assert ix.list_sizes().max() <= 512, ix.list_sizes().max()
    qs = x[dup[:9]]
    for top_k in (57, 100, 1024):
        got = ix.search(qs, top_k=top_k, nprobe=32, rerank=512, wide=True)
        assert same(got, c.search(qs, top_k=top_k)), top_k
        for qi, (gr, gd) in enumerate(got):
            assert gr[:3].tolist() == [dup[qi], 1000 + qi, 3000 + qi] and gd[0] == gd[1] == gd[2]
    ix.close(); c.close()


@pytest.mark.parametrize("local_pca", [False, True], ids=["pq", "lpca"])
def test_zero_query_and_zero_rows_at_100(gpu_ctx, tmp_path, local_pca):
    """As test_zero_query_and_zero_rows of the contract test, at top_k = 100: the call succeeds and the returned pairs are exact."""
    import semtools_amd as smt

    x, nlist, _ = _corpus("tiny-lists")
    assert (np.abs(x).sum(axis=1) == 0).sum() == 3
    c = smt.Corpus(gpu_ctx)
    c.append(x)
    ix = smt.IvfPq(c, nlist=nlist, train_iters=4, local_pca=local_pca)
    ix.save(tmp_path / "zero.ivf")
    f = R.read_index(tmp_path / "zero.ivf")
    qs = np.stack([np.zeros(256, dtype=np.float32), R.iso_rows(1, 77)[0], x[6]])
    for nprobe, rerank in ((64, 512), (8, 64)):
        got = ix.search(qs, top_k=100, nprobe=nprobe, rerank=rerank, wide=True)
        check_partial_oracle(x, f, qs, got, nprobe, 100, rerank)
        assert all(len(gr) == 100 for gr, _ in got)
    assert ix.list_sizes().max() <= 512
    assert same(ix.search(qs, top_k=100, nprobe=64, rerank=512, wide=True), c.search(qs, top_k=100))
    ix.close(); c.close()


# ================================================================================================ 5. arguments
def test_argument_validation(small, gpu_ctx, query_sets):
    import torch

    import semtools_amd as smt
    from semtools_amd import _lib as L

    x, c, ix, f = small
    qs = np.ascontiguousarray(query_sets["fresh"][0][:4])
    lib = L.lib()
    out_r, out_d, cnt = np.empty((4, 1025), np.uint64), np.empty((4, 1025)), np.zeros(4, np.uint64)
    qd = torch.from_numpy(qs).cuda()
    dr = torch.empty((4, 1025), dtype=torch.int64, device="cuda")
    dd = torch.empty((4, 1025), dtype=torch.float64, device="cuda")
    g1 = smt.Group.logical(0, 1)
    sc1 = smt.ShardedCorpus(g1, rows=x)
    six1 = smt.ShardedIvfPq(sc1, nlist=NLIST, train_iters=4, local_pca=False)
    g3 = smt.Group.logical(0, 3)
    sc3 = smt.ShardedCorpus(g3, rows=x)
    six3 = smt.ShardedIvfPq(sc3, nlist=NLIST, train_iters=4, local_pca=False)

    def calls(top_k, nprobe):
        yield lib.smt_ivfpq_search_wide(ix._h, L.np_ptr(qs), 4, top_k, nprobe, 512, None, 0, 0, L.np_ptr(out_r), L.np_ptr(out_d),
                                        L.np_ptr(cnt), 1025)
        yield lib.smt_ivfpq_search_wide_device(ix._h, C.c_void_p(qd.data_ptr()), 4, top_k, nprobe, 512, None, 0, 0,
                                               C.c_void_p(dr.data_ptr()), C.c_void_p(dd.data_ptr()))
        for six in (six1, six3):
            yield lib.smt_sharded_ivfpq_search_wide(six._h, L.np_ptr(qs), 4, top_k, nprobe, 512, None, 0, L.np_ptr(out_r),
                                                    L.np_ptr(out_d), L.np_ptr(cnt), 1025)

    assert list(calls(1025, 4)) == [L.SMT_E_INVALID] * 4
    assert list(calls(100, 0)) == [L.SMT_E_INVALID] * 4
    assert list(calls(100, NLIST + 1)) == [L.SMT_E_INVALID] * 4
    # a range past the corpus is refused, as in smt_ivfpq_search_ranges
    bad = (L.SmtRange * 1)(L.SmtRange(10, N + 1))
    assert lib.smt_ivfpq_search_wide(ix._h, L.np_ptr(qs), 4, 100, 4, 512, C.cast(bad, C.c_void_p), 1, 0, L.np_ptr(out_r), L.np_ptr(out_d),
                                     L.np_ptr(cnt), 1025) == L.SMT_E_INVALID
    # the sharded form: n_ranks x top_k <= 8192, found before anything is enqueued (9 ranks x 1024)
    g9 = smt.Group.logical(0, 9)
    sc9 = smt.ShardedCorpus(g9, rows=x)
    six9 = smt.ShardedIvfPq(sc9, nlist=32, train_iters=2, local_pca=False)
    assert lib.smt_sharded_ivfpq_search_wide(six9._h, L.np_ptr(qs), 4, 1024, 4, 512, None, 0, L.np_ptr(out_r), L.np_ptr(out_d),
                                             L.np_ptr(cnt), 1025) == L.SMT_E_INVALID
    assert "8192" in L.lib().smt_last_error().decode()
    assert same(six9.search(qs, top_k=100, nprobe=32, rerank=512, wide=True), c.search(qs, top_k=100))   # ... and the group still answers
    six9.close(); sc9.close(); g9.close()
    # the host form takes top_k = 0
    assert lib.smt_ivfpq_search_wide(ix._h, L.np_ptr(qs), 4, 0, 4, 512, None, 0, 0, L.np_ptr(out_r), L.np_ptr(out_d), L.np_ptr(cnt), 1025) == 0
    assert (cnt == 0).all()
    # without `wide` 57 is still refused, and the refusals left everything usable
    with pytest.raises(L.SmtError):
        ix.search(x[:1], top_k=57, nprobe=4)
    with pytest.raises(L.SmtError):
        six3.search(x[:1], top_k=57, nprobe=4)
    gpu_ctx.synchronize()
    want = c.search(qs, top_k=100)
    assert same(ix.search(qs, top_k=100, nprobe=NLIST, rerank=512, wide=True), want)
    assert same(six1.search(qs, top_k=100, nprobe=NLIST, rerank=512, wide=True), want)
    assert same(six3.search(qs, top_k=100, nprobe=NLIST, rerank=512, wide=True), want)
    for o in (six1, sc1, g1, six3, sc3, g3):
        o.close()


# ================================================================================================ 6. sharded
@pytest.mark.parametrize("transport", ["peer", "copy"])
@pytest.mark.parametrize("n_shards", [2, 3])
def test_logical_shards_equal_the_unsharded_wide_answer_and_the_exact_search(small, rows, query_sets, n_shards, transport):
    import semtools_amd as smt

    x, c, ix, f = small
    qs = query_sets["fresh"][0][:9]
    group = smt.Group.logical(0, n_shards)
    group.set_transport(transport)
    sc = smt.ShardedCorpus(group, rows=rows)
    six = smt.ShardedIvfPq(sc, nlist=NLIST, train_iters=4, local_pca=f["kind"] == 1)
    for i in range(n_shards):
        assert six.shard_list_sizes(i, NLIST).max() <= 512
    b1 = int(sc.rank_rows()[0])
    for top_k in (57, 100, 1024):
        got = six.search(qs, top_k=top_k, nprobe=NLIST, rerank=512, wide=True)
        assert same(got, ix.search(qs, top_k=top_k, nprobe=NLIST, rerank=512, wide=True)), top_k
        assert same(got, c.search(qs, top_k=top_k)), top_k
    for ranges in ([(b1 - 150, b1 + 150)], G.alternate_blocks(N), [(7, 7)], []):
        got = six.search(qs, top_k=100, nprobe=NLIST, rerank=512, ranges=ranges, wide=True)
        if sum(e - b for b, e in ranges) == 0:
            assert all(len(gr) == 0 for gr, _ in got)
        else:
            assert same(got, c.search(qs, top_k=100, ranges=ranges)), ranges[:2]
    assert same(six.search(qs, top_k=10, nprobe=7, rerank=64, wide=True), six.search(qs, top_k=10, nprobe=7, rerank=64))
    six.close(); sc.close(); group.close()


# ================================================================================================ 7. the workspace store
def test_store_answers_100_hits_through_the_index(gpu_ctx, tmp_path, monkeypatch, capfd):
    """SEMTOOLS_INDEX_MAX_TOP_K: a whole-workspace search at top_k = 100 goes through the index (it gets built) and, with every
    list probed and every row re-scored, prints what the exact scan prints; without the variable the same call takes the exact
    route, as before (no index appears)."""
    from safetensors.numpy import save_file

    import json

    from semtools_amd import host
    from tests import synth

    V = 20000
    d = tmp_path / "model"
    d.mkdir()
    save_file({"embeddings": synth.table(V, seed=2)}, str(d / "model.safetensors"))
    (d / "vocab.txt").write_text("".join(f"w{i}\n" for i in range(V - 1)) + "[UNK]\n")
    (d / "config.json").write_text(json.dumps({"normalize": True, "unk_token": "[UNK]"}))
    model = host.StaticModel(gpu_ctx, model_dir=d)
    monkeypatch.setenv("HOME", str(tmp_path))
    monkeypatch.delenv("SEMTOOLS_WORKSPACE", raising=False)
    monkeypatch.delenv("SEMTOOLS_INDEX_MAX_TOP_K", raising=False)
    files = []
    for i in range(6):
        p = tmp_path / f"big{i}.txt"
        p.write_text("\n".join(synth.pseudo_prose(1000, vocab_size=V - 1, seed=100 + i)) + "\n")
        files.append(str(p))
    query = synth.pseudo_prose(1, vocab_size=V - 1, seed=103)[0]
    try:
        host.workspace_use(None, "wide")
        root = tmp_path / ".semtools" / "workspaces" / "wide"
        monkeypatch.setenv("SEMTOOLS_INDEX_MIN_ROWS", "1000000000")
        exact = host.search_with_workspace(model, query, files, workspace_name="wide", n_lines=0, top_k=100)
        exact_sub = host.search_with_workspace(model, query, files[:5], workspace_name="wide", n_lines=0, top_k=100)
        monkeypatch.setenv("SEMTOOLS_INDEX_MIN_ROWS", "4000")
        monkeypatch.setenv("SEMTOOLS_INDEX_NPROBE", "512")
        assert host.search_with_workspace(model, query, files, workspace_name="wide", n_lines=0, top_k=100) == exact
        assert not (root / "line_index.ivf").exists()                 # top_k = 100 > 24 without the variable: the exact route
        monkeypatch.setenv("SEMTOOLS_INDEX_MAX_TOP_K", "200")
        assert host.search_with_workspace(model, query, files, workspace_name="wide", n_lines=0, top_k=100) == exact
        assert (root / "line_index.ivf").exists()                     # ... with it: the index was built and answered
        assert host.search_with_workspace(model, query, files[:5], workspace_name="wide", n_lines=0, top_k=100) == exact_sub
        assert len(exact) > 0
    finally:
        capfd.readouterr()
        model.close()
