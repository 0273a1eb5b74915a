"""tests/pipeline_life.py on the CPU: every script the GPU test performs obeys the visibility rule and the PROVED gap (so the GPU test
needs no list of exemptions), check_script fails on scripts that break either, and the model's pieces agree with numpy and with the
oracle on all rows."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import pipeline_life as pl


@pytest.mark.parametrize("script_id,build", pl.all_scripts(), ids=[x[0] for x in pl.all_scripts()])
def test_check_script_passes(script_id, build):
    script = build()
    exp = pl.check_script(script)
    searches = script.searches()
    assert len(exp.answers) == len(script.steps) and len(searches) >= 60
    assert exp.mutations, "a script without a change of contents tests nothing"
    for i in searches:
        rows, dist = exp.answers[i]
        assert len(rows) == script.steps[i][3] and (rows >= pl.row_base(i)).all()
    if script_id.startswith("random_life"):
        ops = len(script.steps) - len(searches)
        assert len(script.steps) >= 150 and 0.65 <= len(searches) / len(script.steps) <= 0.75, (len(script.steps), ops)
    else:
        # sixteen queries through the places of a group, every k of the issue somewhere in the scripted set
        assert {s[3] for s in script.steps if s[0] == "search"} <= set(pl.KS)
        assert 64 <= len(script.steps) <= 128


def test_every_k_and_every_query_is_used():
    ks, qis = set(), set()
    for _, build in pl.all_scripts()[:2]:
        for s in build().steps:
            if s[0] == "search":
                ks.add(s[3])
                qis.add(s[2])
    assert ks == set(pl.KS) and qis == set(range(pl.NQ))


def _small(seed=1):
    return pl.Builder("bad", seed, {"a": ("owned", 1000, 400)})


def test_check_script_fails_on_a_mutation_that_moves_no_winner():
    """The test of the test: fresh rows over rows that hold no copy leave every top-1 where it was."""
    b = _small()
    b.run("a", 10, 1)
    b.op("write_rows", "a", 900, b.fresh(16))
    b.run("a", 10, 1)
    with pytest.raises(AssertionError, match="does not move the winner"):
        pl.check_script(b.script())
    b = _small()                                                     # ... while the same script with the copies moved passes
    b.run("a", 10, 1)
    b.replant("a")
    b.run("a", 10, 1)
    pl.check_script(b.script())


def test_check_script_fails_where_a_later_step_undoes_a_mutation():
    """The copies go and come back to their rows before query 15 is searched again: a stale answer would pass for a fresh one."""
    b = _small()
    b.run("a", 10, 10)
    b.op("write_rows", "a", 400, b.fresh(16))
    b.run("a", 10, 10)                                               # (queries 5 .. 9)
    b.op("write_rows", "a", 400, pl.QUERIES.copy())
    b.run("a", 32, 10)
    with pytest.raises(AssertionError, match="does not move the winner"):
        pl.check_script(b.script())


def test_check_script_fails_on_a_gap_too_narrow_to_prove():
    b = _small()
    fifth = int(pl.oracle_topk(b.model["a"], pl.QUERIES[0], 5)[0][4])
    near = b.model["a"][fifth].copy()
    near[:2] += np.float32(1e-4)                                     # a second row some 1e-8 from the one on place 5 of query 0
    b.op("write_rows", "a", 900, near[None])
    rows, dist = pl.oracle_topk(b.model["a"], pl.QUERIES[0], 6)
    assert sorted(rows[4:].tolist()) == sorted([fifth, 900]) and 0 < dist[5] - dist[4] < pl.PROVED_GAP
    b.steps.clear()
    b.initial["a"] = ("owned", b.model["a"].copy())
    b.search("a", 0, 10)                                             # both rows inside the top ten: proved
    pl.check_script(b.script())
    b.search("a", 0, 5)                                              # the k-th place between them: not
    with pytest.raises(AssertionError, match="apart"):
        pl.check_script(b.script())


def test_the_subset_shortcut_is_the_oracle_on_all_rows():
    rows = pl.unit_rows(np.random.default_rng(3), pl.SIZES[1])
    rows[70:70 + pl.NQ] = pl.QUERIES
    approx = pl.approx_distances(rows, pl.QUERIES)
    for qi in range(pl.NQ):
        want = orc.search_documents(rows, [len(rows)], pl.QUERIES[qi], n_lines=0, top_k=pl.KTOP, accurate=True)
        got = pl.oracle_topk(rows, pl.QUERIES[qi], pl.KTOP, approx=approx[:, qi])
        assert got[0].tolist() == [r["match_line"] for r in want] and got[0][0] == 70 + qi
        assert got[1].tolist() == [r["distance"] for r in want] and 0.0 <= got[1][0] < 1e-12 and not np.signbit(got[1][0])
        for k in pl.KS:                                              # a top-k is the head of the top-(k + 1)
            short = orc.search_documents(rows, [len(rows)], pl.QUERIES[qi], n_lines=0, top_k=k, accurate=True)
            assert [r["match_line"] for r in short] == got[0][:k].tolist() and [r["distance"] for r in short] == got[1][:k].tolist()
    elig = pl.kept_index([(0, 100), (5000, 60_000)])
    want = orc.search_documents(rows[elig], [len(elig)], pl.QUERIES[2], n_lines=0, top_k=10, max_distance=0.8, accurate=True)
    got = pl.oracle_topk(rows, pl.QUERIES[2], 10, eligible=elig, max_distance=0.8)
    assert got[0].tolist() == elig[[r["match_line"] for r in want]].tolist() and got[1].tolist() == [r["distance"] for r in want]
    assert len(got[0]) > 10                                          # (documents mode: every row below the threshold)


def test_the_model_applies_ops_as_numpy_would():
    rng = np.random.default_rng(4)
    x = pl.unit_rows(rng, 50)
    model = {"a": x.copy()}
    pl.apply_op(model, "write_rows", ("a", 48, x[:2]))
    assert np.array_equal(model["a"][48:], x[:2]) and np.array_equal(model["a"][:48], x[:48])
    pl.apply_op(model, "truncate", ("a", 40))
    pl.apply_op(model, "append", ("a", x[10:13]))
    assert np.array_equal(model["a"], np.concatenate([x[:40], x[10:13]]))
    assert not pl.mutates(model, "compact", ("a", [(0, 43)])) and pl.mutates(model, "compact", ("a", [(0, 42)]))
    pl.apply_op(model, "compact", ("a", [(1, 3), (40, 43)]))
    assert np.array_equal(model["a"], np.concatenate([x[1:3], x[10:13]]))
    table = pl.embed_table()
    pl.apply_op(model, "embed", ("a", np.array([3, 20, 21], np.uint32), np.array([0, 1, 3], np.uint64)), table)
    assert len(model["a"]) == 7
    assert pl.oracle_topk(model["a"], pl.QUERIES[3], 1)[0].tolist() == [5]   # the line of token 3 alone IS query 3 (to an ulp)
    pl.apply_op(model, "set_tuning", ("scan_blocks", 2))
    pl.apply_op(model, "close", ("a",))
    assert model["a"] is None
    with pytest.raises(AssertionError):
        pl.apply_op(model, "no_such_op", ())


def _as_run(script, exp):
    """what a run that answers every search as the model does would leave behind (scripts of searches and writes only)"""
    from tests import test_gpu_pipeline_life as gpu

    n = len(script.steps)
    run = gpu._Run()
    run.rows = np.full((n, gpu.KMAX + 2 * gpu.GUARD), -7, dtype=np.int64)
    run.dist = np.full((n, gpu.KMAX + 2 * gpu.GUARD), -7.0)
    run.status = np.full(n, 7, dtype=np.int32)
    run.answers, run.held = [None] * n, {}
    for i in script.searches():
        rows, dist = exp.answers[i]
        run.rows[i, gpu.GUARD:gpu.GUARD + len(rows)] = rows
        run.dist[i, gpu.GUARD:gpu.GUARD + len(rows)] = dist
        run.status[i] = 0
    return run


def test_the_gpu_tests_comparison_catches_one_stale_answer():
    """The comparison of tests/test_gpu_pipeline_life.py on made-up runs: the model's own answers pass; ONE search behind a write
    answered from the rows as they were before it -- by the run and by its twin alike -- does not, and neither does a touched
    guard word, a status word other than PROVED, or a twin that differs in one distance bit."""
    from tests import test_gpu_pipeline_life as gpu

    script = pl.write_rows_script(pl.SIZES[0])
    exp = pl.expected(script)
    gpu.check_answers(script, exp, _as_run(script, exp), _as_run(script, exp), "made up")
    m = exp.mutations[0]
    j = next(i for i in script.searches() if i > m)
    _, c, qi, k = script.steps[j]
    before = pl.oracle_topk(script.corpora[c][1], pl.QUERIES[qi], k)
    stale = []
    for _ in range(2):
        run = _as_run(script, exp)
        run.rows[j, gpu.GUARD:gpu.GUARD + k] = before[0] + pl.row_base(j)
        run.dist[j, gpu.GUARD:gpu.GUARD + k] = before[1]
        stale.append(run)
    with pytest.raises(AssertionError, match="step %d" % j):
        gpu.check_answers(script, exp, stale[0], stale[1], "made up")
    for spoil in ("guard", "status", "twin"):
        run, twin = _as_run(script, exp), _as_run(script, exp)
        if spoil == "guard":
            run.rows[j, gpu.GUARD + k] = 0
        elif spoil == "status":
            twin.status[j] = 1
        else:
            twin.dist[j, gpu.GUARD] = np.nextafter(twin.dist[j, gpu.GUARD], 1.0)
        with pytest.raises(AssertionError, match="step %d" % j):
            gpu.check_answers(script, exp, run, twin, "made up")
