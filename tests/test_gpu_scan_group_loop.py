"""The group reducer of scan_pair_kernel: the queries of a group are reduced together, and ONE distance, ONE compare and ONE ballot
serve the sixteen (row, query) pairs of a chunk -- lane 16 g + j takes query g and row j, against its own query's threshold, and
bits 16 g .. 16 g + 3 of the ballot go to list g (row g of the wave, not quad g: wave_sum4 leaves other roundings in the other quads
of a row, which seeds 56 and 57 of the near-tie test show as other rows in an UNCERTAIN answer).  Its arithmetic is that of the one-query scan, bit for bit: every series here is
compared byte for byte (rows, f64 distances, status words) with its scan_pair = 0 run, which the one-query kernel serves, and where
the answers are PROVED also with the oracle's accurate form.

Set up like tests/test_gpu_scan_groups.py: the series runner of tests/test_gpu_scan_pairing.py, a context of its own on a torch
stream that can pair, scan_pair_wait_us = 2000 so that corpora which scan faster than the host issues calls still group."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import synth
from tests.test_gpu_scan_pairing import _same, _series

pytestmark = pytest.mark.gpu

CALLS = 24
N_PLANT = 4099                      # 1025 chunks, the last of 3 rows: not a multiple of the 8 waves of a block either
TINY = (1, 2, 3, 4, 5, 7, 33)
ADV_SEEDS = (55, 56, 57)
ZERO_ROWS = (40, 81, 122, 163)      # one at each residue mod 4
DUP_ROWS = (7, 1031, 2050)          # the same vector in three chunks, residues 3, 3, 2


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _unit(v):
    return v / np.linalg.norm(v)


def _planted():
    """4099 unit rows and four unit queries with disjoint planted neighbours at cosines 0.95 .. 0.90 (built as tests/decoys.py
    builds its queries around a centre: q + tan(acos(cos)) u, u orthogonal to q).  Query g owns row g of chunk 0 -- that chunk holds
    a winner of every query, one per row -- a whole chunk of its own (four winners of one list from one ballot), and one of the last
    four rows: 4095 closes a full chunk, 4096 .. 4098 are the ragged last chunk."""
    rng = np.random.default_rng(9100)
    emb = synth.unit_rows(N_PLANT, seed=9101, dup_frac=0.0, zero_frac=0.0)
    qs = np.stack([_unit(rng.standard_normal(256)) for _ in range(4)])
    owned = []
    for g in range(4):
        quad = 4 * (250 + 10 * g)
        rows = [g, quad, quad + 1, quad + 2, quad + 3, 4095 + g]
        for r, cos in zip(rows, np.linspace(0.95, 0.90, len(rows))[rng.permutation(len(rows))]):
            u = rng.standard_normal(256)
            u -= (u @ qs[g]) * qs[g]
            emb[r] = _unit(qs[g] + math.tan(math.acos(cos)) * _unit(u)).astype(np.float32)
        owned.append(rows)
    return np.ascontiguousarray(emb), np.ascontiguousarray(qs, dtype=np.float32), owned


class _Setup:
    pass


@pytest.fixture(scope="module")
def S():
    import torch
    import semtools_amd as smt
    from tests.test_gpu_nearties import adversarial_corpus

    s = _Setup()
    s.torch = torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(59)
    s.x = torch.randn(N_PLANT, 256, device=dev, generator=g)
    s.x /= s.x.norm(dim=1, keepdim=True)
    s.qs = torch.randn(64, 256, device=dev, generator=g)
    s.qs /= s.qs.norm(dim=1, keepdim=True)
    s.xz = s.x.clone()
    for r in ZERO_ROWS:
        s.xz[r] = 0.0
    for r in DUP_ROWS[1:]:
        s.xz[r] = s.xz[DUP_ROWS[0]]
    s.qs_zero = s.qs[:4].clone()
    s.qs_zero[0] = 0.0                                             # the zero query,
    s.qs_zero[1] = s.xz[DUP_ROWS[0]]                               # a query that IS a (duplicated) row, and two random ones
    s.emb_plant, qs_plant, s.owned = _planted()
    s.qs_plant_np = qs_plant
    s.qs_plant = torch.from_numpy(qs_plant).to(dev)
    s.x_plant = torch.from_numpy(s.emb_plant).to(dev)
    s.adv = {seed: adversarial_corpus(seed=seed) for seed in ADV_SEEDS}
    s.q_adv = None
    torch.cuda.synchronize()
    # (a context whose stream cannot pair at all is given up for one on the next stream: tests/test_gpu_scan_groups.py says why)
    for attempt in range(6):
        s.stream = torch.cuda.Stream(dev)
        s.ctx = smt.Context(0, stream=s.stream.cuda_stream)
        s.corpora = {n: smt.Corpus(s.ctx, device_ptr=s.x.data_ptr(), rows=n) for n in TINY + (1000,)}
        s.ctx.set_tuning("async_select", 1)
        if _series(s, (1000,), 8, (10,), 1)[1][0] > 0 or attempt == 5:
            break
        for c in s.corpora.values():
            c.close()
        s.ctx.close()
    s.corpora["plant"] = smt.Corpus(s.ctx, device_ptr=s.x_plant.data_ptr(), rows=N_PLANT)
    s.corpora["zero"] = smt.Corpus(s.ctx, device_ptr=s.xz.data_ptr(), rows=N_PLANT)
    for seed, (_, emb, _) in s.adv.items():
        c = smt.Corpus(s.ctx)
        c.append(emb)
        s.corpora[("adv", seed)] = c
    s.ctx.set_tuning("async_select", 1)
    yield s
    for c in s.corpora.values():
        c.close()
    s.ctx.close()


def _with_queries(s, qs):
    """The setup with another query block (the series runner reads s.qs)."""
    v = _Setup()
    v.__dict__.update(s.__dict__)
    v.qs = qs
    return v


def _grouped(s, *args, pair=3, **kw):
    before = s.ctx.scan_groups()
    got, counts = _series(s, *args, pair=pair, **kw)
    by_size = tuple(int(b - a) for a, b in zip(before, s.ctx.scan_groups()))
    print("  by_size", by_size)
    assert sum((n + 1) * v for n, v in enumerate(by_size)) == CALLS, (by_size, counts)
    return got, by_size


def _alone(s, *args, **kw):
    got, counts = _series(s, *args, pair=0, **kw)
    assert counts == (0, 0, 0), counts
    return got


def _four_per_group(i):
    return (i // 2) % 4                                            # steps i, i + 2, i + 4, i + 6 carry four different queries


@pytest.mark.parametrize("seed", ADV_SEEDS)
def test_near_ties_in_groups_of_three_and_four(S, seed):
    """40 near-ties around the 10th place: which of them the f32 scan nominates decides the rows of an UNCERTAIN answer, so one
    rounding that differs from the one-query kernel's shows as a byte that differs."""
    s = _with_queries(S, S.qs)
    s.q_adv = S.torch.from_numpy(S.adv[seed][0]).to(S.qs.device)
    name = ("adv", seed)
    three_or_more = 0
    for k in (3, 10, 20):
        want = _alone(s, (name,), CALLS, (k,), adv_query=True)
        print("seed", seed, "k", k, "status words of the scan_pair = 0 run:", sorted(set(want[2].tolist())))
        if seed == 55 and k == 10:
            assert (want[2] == 1).all()                            # SMT_STATUS_UNCERTAIN (tests/test_gpu_scan_pairing.py relies on it too)
        for pair in (2, 3):
            got, by_size = _grouped(s, (name,), CALLS, (k,), pair=pair, adv_query=True)
            _same(got, want)                                       # (status words included: UNCERTAIN where the lone run says so)
            assert by_size[3] == 0 or pair == 3, by_size
            three_or_more += by_size[2] + by_size[3]
    assert three_or_more > 0                                       # counted over the six grouped series (see test_gpu_scan_groups.py)


@pytest.mark.parametrize("k", [3, 10])
def test_four_different_queries_in_one_group_winners_in_every_slot(S, k):
    from oracle import oracle as orc

    s = _with_queries(S, S.qs_plant)
    want = _alone(s, ("plant",), CALLS, (k,), qsel=_four_per_group)
    assert (want[2] == 0).all()                                    # PROVED: the planted rows are far in front of the random ones
    full = 0
    for _ in range(6):
        got, by_size = _grouped(s, ("plant",), CALLS, (k,), qsel=_four_per_group)
        _same(got, want)
        full += by_size[3]
        if full:
            break
    assert full > 0
    for g in range(4):
        ref = orc.search_documents(S.emb_plant, [N_PLANT], S.qs_plant_np[g], n_lines=0, top_k=k, accurate=True)
        others = {r for h in range(4) if h != g for r in S.owned[h]}
        for i in range(CALLS):
            if _four_per_group(i) != g:
                continue
            assert got[0][i, :k].tolist() == [r["match_line"] for r in ref], (g, i)
            assert np.array_equal(got[1][i, :k], np.array([r["distance"] for r in ref])), (g, i)
            assert not others & set(got[0][i, :k].tolist()), (g, i)        # no other query's winners: lists and lanes not mixed up
            assert set(got[0][i, :min(k, 6)].tolist()) <= set(S.owned[g]), (g, i)


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("rows", TINY)
def test_tiny_and_ragged_corpora_in_groups_of_four(S, rows, k):
    want = _alone(S, (rows,), CALLS, (k,))
    got, by_size = _grouped(S, (rows,), CALLS, (k,))
    _same(got, want)
    assert by_size[1] + by_size[2] + by_size[3] > 0, by_size


def test_zero_query_zero_rows_and_duplicates_inside_a_group(S):
    s = _with_queries(S, S.qs_zero)
    want = _alone(s, ("zero",), CALLS, (10,), qsel=_four_per_group)
    full = 0
    for _ in range(6):
        got, by_size = _grouped(s, ("zero",), CALLS, (10,), qsel=_four_per_group)
        _same(got, want)
        full += by_size[3]
        if full:
            break
    assert full > 0
    for i in range(CALLS):
        if _four_per_group(i) == 0:                                # zero query: the zero rows at distance 0, then distance 1 in row order
            assert got[0][i, :10].tolist() == list(ZERO_ROWS) + [0, 1, 2, 3, 4, 5], i
            assert got[1][i, :10].tolist() == [0.0] * 4 + [1.0] * 6, i
        if _four_per_group(i) == 1:                                # the three copies of the query's row, in row order
            assert got[0][i, :3].tolist() == list(DUP_ROWS), i
            assert got[1][i, 0] == got[1][i, 1] == got[1][i, 2], i


def test_interleaved_trees_equal_the_lone_tree_bit_for_bit():
    """tools/micro/wave_sum4_multi: wave_sum4_multi<3>, and <2> in its head / tail halves, against wave_sum4 on 64 rounds of inputs
    whose sums depend on the order of the additions."""
    exe = os.path.join(ROOT, "tools", "micro", "wave_sum4_multi")
    if not os.path.exists(exe):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                               exe + ".hip", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS wave_sum4_multi" in r.stdout, r.stdout + r.stderr
