"""The queued one-query pipeline with OTHER entry points between the queued calls (tests/pipeline_life.py has the scripts, the host
model and the rules the scripts obey).  A script runs with no synchronise of its own but the one at its end, grouping live
(async_select = 1, scan_deep = 15, select_group = 1, ov_skip_ready = 1: the defaults; scan_pair_wait_us = 2000 so that corpora which
scan faster than the host issues calls still group), and

 1. every search equals the oracle on the model's contents at its step: rows equal, distances the same bytes;
 2. rows, distances and status words are byte for byte those of the same script at async_select = 0 on fresh corpora (the twin; it
    makes the guard_band switches too, since a status word may depend on the band), every search PROVED in both, the guard words
    around every output list untouched;
 3. grouping happened around the op: the counters are read right behind every op that drains the pipeline itself (the read adds
    nothing there; behind an op that does NOT drain -- truncate, the plain tuning keys, a compaction that keeps everything,
    prof_enable, a merge on the aux stream -- they are not read, so that the calls on both sides of it stay queued together).  Every
    stretch between two reads that holds eight searches in a row of one corpus and one k, each of them made while grouping was
    switched on (whatever was switched before or behind that run), has paired > 0, and, where select_group was on for all its
    searches, a select launch in it that served two calls or more.  This is a condition of the run, not a measurement:
    a run that misses it is repeated on a context on the next stream (up to six), as the fixture does, its answers checked all
    the same; if no stream groups, the test fails and says so.

A drain in mid-series lets the current leader's 2 ms wait run out; that ends the group and is no error, as at the end of every
series of the other pipeline tests.

The caller's stream stays EMPTY ahead of a segment.  Work queued there (a "stall") would not let the host run ahead of calls that
can be taken: a call is published as absorbable only when the caller's stream was empty at the call (overlap_prologue), so behind
a stall nothing groups until it has run out.  Measured with `perform(..., stall=40)`, about 4 ms of torch.mul ahead of every
segment of the write_rows script, twice each way: every segment (paired, alone, absorbed) = (0, 10, 0) behind the stall,
(2, 0, 8) without it -- two leaders that took four calls along each.  The leader's wait is what keeps the pipeline live while the
host issues the op.

SMT_PIPELINE_LIFE_PROFILE=<path>: the group histograms seen, per script and attempt, as JSON (profiles/pipeline_life.json)."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import pipeline_life as pl

pytestmark = pytest.mark.gpu

GUARD = pl.GUARD
KMAX = max(pl.KS)
DRAINING_KEYS = {"scan_deep", "select_group", "scan_pair_ring", "scan_overlap", "async_select", "merge_on_aux", "scan_pair", "scan_take"}
TWIN_KEYS = {"guard_band", "compact_bounce_rows"}          # the switches the twin makes too
DEFAULTS = {"scan_deep": 15, "scan_overlap": 1, "async_select": 1, "scan_unroll": 4, "merge_on_aux": 0, "select_group": 1, "prof_every": 1}
ATTEMPTS = 6


class _Setup:
    pass


def _new_context(s):
    import semtools_amd as smt

    s.stream = s.torch.cuda.Stream(s.dev)
    s.ctx = smt.Context(0, stream=s.stream.cuda_stream)
    s.attempt += 1


def _next_stream(s):
    s.ctx.close()
    _new_context(s)


def _probe(s):
    """eight queued calls over 1000 rows: how many launches took a later call along"""
    import semtools_amd as smt

    torch, ctx = s.torch, s.ctx
    ctx.set_tuning("async_select", 1)
    ctx.set_tuning("scan_pair_wait_us", 2000)
    with torch.cuda.stream(s.stream):
        x = torch.from_numpy(pl.unit_rows(np.random.default_rng(5), 1000)).to(s.dev)
        rows = torch.full((8, 10), -7, dtype=torch.int64, device=s.dev)
        dist = torch.full((8, 10), -7.0, dtype=torch.float64, device=s.dev)
    s.stream.synchronize()
    c = smt.Corpus(ctx, device_ptr=x.data_ptr(), rows=1000)
    before = ctx.scan_pairs()
    for i in range(8):
        c.search_topk_device(s.qd[i].data_ptr(), 1, 10, 0, rows[i].data_ptr(), dist[i].data_ptr())
    ctx.synchronize()
    paired = ctx.scan_pairs()[0] - before[0]
    c.close()
    return paired


@pytest.fixture(scope="module")
def S():
    import torch

    s = _Setup()
    s.torch = torch
    s.dev = torch.device("cuda:0")
    s.qd = torch.from_numpy(pl.QUERIES).to(s.dev)
    torch.cuda.synchronize()
    s.attempt = -1
    s.profile = {}
    # (why a context that cannot take anything along is given up for one on the next stream: tests/test_gpu_scan_groups.py)
    for attempt in range(ATTEMPTS):
        _new_context(s)
        if _probe(s) > 0 or attempt == ATTEMPTS - 1:       # (the last one stays: the tests then say what is wrong)
            break
        s.ctx.close()
    yield s
    s.ctx.close()
    path = os.environ.get("SMT_PIPELINE_LIFE_PROFILE")
    if path:
        with open(path, "w") as f:                           # one line per script
            f.write("{\n" + ",\n".join(' "%s": %s' % (k, json.dumps(v, sort_keys=True)) for k, v in sorted(s.profile.items())) + "\n}\n")


class _Run:
    pass


def _counters(ctx):
    return ctx.scan_pairs(), ctx.scan_groups_deep(), ctx.select_groups()


def _delta(now, then):
    return tuple(tuple(int(b - a) for a, b in zip(x, y)) for x, y in zip(then, now))


def _merge_input(seed):
    """three sorted lists of eight (row, distance) pairs for one query, packed [3][1][2][8]"""
    rng = np.random.default_rng(50 + seed)
    d = np.sort(rng.random((3, 8)), axis=1)
    r = rng.permutation(1000)[:24].reshape(3, 8).astype(np.int64)
    return np.ascontiguousarray(np.stack([r, d.view(np.int64)], axis=1)[:, None])


def perform(s, script, twin=False, stall=0):
    """Performs `script` on fresh corpora of the fixture's context; no synchronise but the ops' own and one at the end."""
    import semtools_amd as smt

    torch, ctx, stream, dev = s.torch, s.ctx, s.stream, s.dev
    steps = script.steps
    n = len(steps)
    run = _Run()
    run.answers = [None] * n
    run.segments = []                                              # (longest run of searches of one corpus and k made with grouping on, counters)
    tune = dict(DEFAULTS)
    ctx.set_tuning("async_select", 0 if twin else 1)
    ctx.set_tuning("scan_pair_wait_us", 0 if twin else 2000)
    if twin:
        tune["async_select"] = 0
    held = {}                                                      # per step: the device buffers of an op that answers on the device
    with torch.cuda.stream(stream):
        rows = torch.full((n, KMAX + 2 * GUARD), -7, dtype=torch.int64, device=dev)
        dist = torch.full((n, KMAX + 2 * GUARD), -7.0, dtype=torch.float64, device=dev)
        status = torch.full((n,), 7, dtype=torch.int32, device=dev)
        tens = {c: torch.from_numpy(r0).to(dev) for c, (kind, r0) in script.corpora.items() if kind == "adopted"}
        for i, st in enumerate(steps):
            if st[0] != "op":
                continue
            if st[1] == "search_device":
                _, qis, k = st[2]
                held[i] = (torch.from_numpy(pl.QUERIES[qis]).to(dev), torch.full((len(qis), k), -7, dtype=torch.int64, device=dev),
                           torch.full((len(qis), k), -7.0, dtype=torch.float64, device=dev),
                           torch.full((len(qis),), 7, dtype=torch.int32, device=dev))
            elif st[1] == "group_search":
                k = st[2][2]
                held[i] = (torch.full((1, 2, k), -7, dtype=torch.int64, device=dev), torch.full((1,), 7, dtype=torch.int32, device=dev))
            elif st[1] == "merge_packed":
                held[i] = (torch.from_numpy(_merge_input(st[2][0])).to(dev), torch.full((1, 2, 8), -7, dtype=torch.int64, device=dev))
        if stall:
            big_in = torch.ones(64 << 20, dtype=torch.float32, device=dev)
            big_out = torch.empty_like(big_in)
    torch.cuda.synchronize()
    corp, ivf, sharded, extra = {}, {}, {}, []
    try:
        for c, (kind, r0) in script.corpora.items():
            if kind == "adopted":
                corp[c] = smt.Corpus(ctx, device_ptr=tens[c].data_ptr(), rows=len(r0))
            else:
                corp[c] = smt.Corpus(ctx)
                corp[c].append(r0)
        model = smt.Model(ctx, script.table, normalize=True) if script.table is not None else None
        if model is not None:
            extra.append(model)
        if any(st[0] == "op" and st[1] == "group_search" for st in steps):
            group = smt.Group.from_ctx(ctx)
            for c in tens:
                sharded[c] = smt.ShardedCorpus(group, device_ptrs=[tens[c].data_ptr()], shard_rows=[len(script.corpora[c][1])])
            extra.insert(0, group)
        ctx.synchronize()
        ctx.uncertain_count(reset=True)
        base = _counters(ctx)
        longest, streak, last, sel_on = 0, 0, None, True
        prof_on = False

        def can_group():
            # (plan_scan's conditions; and a launch bracketed by profiling events neither takes a call nor is taken)
            return (tune["scan_deep"] > 0 and tune["scan_overlap"] == 1 and tune["async_select"] == 1 and tune["scan_unroll"] == 4
                    and not (prof_on and tune["prof_every"] <= 1))

        def close_segment(at):
            nonlocal base, longest, streak, last, sel_on
            now = _counters(ctx)
            run.segments.append(dict(ends_at=at, longest_run=longest, select_group=sel_on, counters=_delta(now, base)))
            base, longest, streak, last, sel_on = now, 0, 0, None, True

        def stall_now():
            if stall:
                with torch.cuda.stream(stream):
                    for _ in range(stall):
                        torch.mul(big_in, 1.0, out=big_out)

        stall_now()
        for i, st in enumerate(steps):
            if st[0] == "search":
                _, c, qi, k = st
                corp[c].search_topk_device(s.qd[qi].data_ptr(), 1, k, pl.row_base(i), rows[i, GUARD:].data_ptr(),
                                           dist[i, GUARD:].data_ptr(), out_status_ptr=status[i:].data_ptr())
                if can_group():                                    # (decided per search: a switch in front of or behind a run does not count)
                    streak = streak + 1 if last == (c, k) else 1
                    last = (c, k)
                    longest = max(longest, streak)
                else:
                    streak, last = 0, None
                sel_on = sel_on and tune["select_group"] == 1
                continue
            _, name, args = st
            drains = True
            last = None                                            # (a run of searches ends at every op)
            if name == "write_rows":
                corp[args[0]].write_rows(args[1], args[2])
            elif name == "truncate":
                corp[args[0]].truncate(args[1])
                drains = False
            elif name == "append":
                corp[args[0]].append(args[1])
            elif name == "compact":
                drains = len(pl.kept_index(args[1])) != corp[args[0]].rows
                corp[args[0]].compact(args[1])
            elif name == "prepack":
                corp[args[0]].prepack(args[1])
            elif name == "embed":
                model.embed(args[1], args[2], append_to=corp[args[0]], want_host=False)
            elif name == "search_host":
                run.answers[i] = corp[args[0]].search(pl.QUERIES[args[1]], **args[2])
            elif name == "search_device":
                q, o_rows, o_dist, o_status = held[i]
                corp[args[0]].search_topk_device(q.data_ptr(), len(args[1]), args[2], 0, o_rows.data_ptr(), o_dist.data_ptr(),
                                                 out_status_ptr=o_status.data_ptr())
                drains = not (len(args[1]) == 1 and args[2] <= 56)
            elif name == "group_search":
                out, o_status = held[i]
                sharded[args[0]].search_topk_device([s.qd[args[1]].data_ptr()], 1, args[2], [out.data_ptr()], [o_status.data_ptr()])
                drains = False
            elif name == "ivf_build":
                ivf[args[0]] = smt.IvfPq(corp[args[0]], nlist=32, train_iters=5)
            elif name == "ivf_search":
                run.answers[i] = ivf[args[0]].search(pl.QUERIES[args[1]], top_k=args[2], nprobe=32)
            elif name == "ivf_close":
                ivf.pop(args[0]).close()
                drains = False
            elif name == "set_tuning":
                key, value = args
                if not twin or key in TWIN_KEYS:
                    ctx.set_tuning(key, value)
                    if key in tune:
                        tune[key] = value
                drains = key in DRAINING_KEYS and not twin
            elif name == "uncertain_count":
                run.answers[i] = ctx.uncertain_count(reset=True)
            elif name == "prof":
                ctx.prof_enable(args[0])
                prof_on = bool(args[0])
                drains = False
            elif name == "merge_packed":
                packed, out = held[i]
                ctx.merge_topk_packed_device(packed.data_ptr(), 3, 1, 8, 8, out.data_ptr())
                drains = not tune["merge_on_aux"]
            elif name == "readopt":
                c, new_rows = args
                corp[c].close()
                with torch.cuda.stream(stream):
                    tens[c].copy_(torch.from_numpy(new_rows))
                corp[c] = smt.Corpus(ctx, device_ptr=tens[c].data_ptr(), rows=len(new_rows))
            elif name == "torch_write":
                c, first, new_rows = args
                with torch.cuda.stream(stream):
                    tens[c][first:first + len(new_rows)].copy_(torch.from_numpy(new_rows))
                drains = False                                     # (its script synchronised in the step before)
            elif name == "close":
                corp.pop(args[0]).close()
            elif name == "synchronize":
                ctx.synchronize()
            else:
                raise AssertionError(name)
            if drains:
                close_segment(i)
                stall_now()
        ctx.synchronize()
        close_segment(n)
        run.rows, run.dist, run.status = rows.cpu().numpy(), dist.cpu().numpy(), status.cpu().numpy()
        run.held = {i: tuple(t.cpu().numpy() for t in v) for i, v in held.items()}
    finally:
        for key, value in list(DEFAULTS.items()) + [("guard_band", 8), ("scan_blocks", 0), ("scan_threads", 512), ("direct_delivery", 1),
                                                    ("scan_pair_ring", 4096), ("select_group", 1), ("prof_every", 1),
                                                    ("compact_bounce_rows", 65536), ("scan_pair_wait_us", 0)]:
            ctx.set_tuning(key, value)
        ctx.prof_enable(False)
        for x in list(ivf.values()) + list(sharded.values()) + list(corp.values()):
            x.close()
        for x in extra:
            x.close()
    return run


def check_answers(script, exp, run, twin, tag):
    """Points 1 and 2 of the module's text.  `tag` goes into every message."""
    steps = script.steps
    for i, st in enumerate(steps):
        what = "%s step %d %r" % (tag, i, st[:2] if st[0] == "op" else st)
        if st[0] == "search":
            k = st[3]
            for r in (run, twin):
                assert (r.rows[i, :GUARD] == -7).all() and (r.rows[i, GUARD + k:] == -7).all(), what
                assert (r.dist[i, :GUARD] == -7.0).all() and (r.dist[i, GUARD + k:] == -7.0).all(), what
                assert r.status[i] == 0, (what, int(r.status[i]))                  # PROVED
            want_rows, want_dist = exp.answers[i]
            got_rows, got_dist = run.rows[i, GUARD:GUARD + k], run.dist[i, GUARD:GUARD + k]
            assert got_rows.tolist() == want_rows.tolist(), (what, got_rows.tolist(), want_rows.tolist())
            assert got_dist.tobytes() == want_dist.tobytes(), (what, got_dist.tolist(), want_dist.tolist())
            assert run.rows[i].tobytes() == twin.rows[i].tobytes() and run.dist[i].tobytes() == twin.dist[i].tobytes(), what
            continue
        name, args = st[1], st[2]
        want = exp.answers[i]
        if name == "search_host":
            for r in (run, twin):
                for (got_rows, got_dist), (want_rows, want_dist) in zip(r.answers[i], want):
                    assert got_rows.tolist() == want_rows.tolist(), (what, got_rows.tolist(), want_rows.tolist())
                    assert got_dist.tobytes() == want_dist.tobytes(), what
        elif name == "search_device":
            for r in (run, twin):
                _, o_rows, o_dist, o_status = r.held[i]
                assert (o_status == 0).all(), (what, o_status.tolist())
                for j, (want_rows, want_dist) in enumerate(want):
                    assert o_rows[j].tolist() == want_rows.tolist(), (what, j)
                    assert o_dist[j].tobytes() == want_dist.tobytes(), (what, j)
        elif name == "group_search":
            for r in (run, twin):
                out, o_status = r.held[i]
                assert o_status.tolist() == [0], (what, o_status.tolist())
                assert out[0, 0].tolist() == want[0].tolist(), (what, out[0, 0].tolist(), want[0].tolist())
                assert out[0, 1].tobytes() == want[1].tobytes(), what
        elif name == "ivf_search":
            model_rows = exp.snapshots[i]
            for r in (run, twin):
                for qi, (got_rows, got_dist) in zip(args[1], r.answers[i]):
                    assert len(got_rows) == args[2] and len(set(got_rows.tolist())) == args[2], what
                    for row, d in zip(got_rows.tolist(), got_dist.tolist()):   # every returned pair is the row's exact distance
                        assert d == orc.cosine(pl.QUERIES[qi], model_rows[row], accurate=True), (what, qi, row)
        elif name == "uncertain_count":
            assert run.answers[i] == 0 and twin.answers[i] == 0, (what, run.answers[i], twin.answers[i])
        elif name == "merge_packed":
            packed = _merge_input(args[0])
            pairs = sorted(zip(packed[:, 0, 1].view(np.float64).ravel().tolist(), packed[:, 0, 0].ravel().tolist()))[:8]
            for r in (run, twin):
                out = r.held[i][1]
                assert out[0, 0].tolist() == [p[1] for p in pairs], what
                assert out[0, 1].view(np.float64).tolist() == [p[0] for p in pairs], what


def grouped(run):
    """Point 3: (it holds, why not)"""
    checked = 0
    for seg in run.segments:
        (paired, alone, absorbed), deep, sel = seg["counters"]
        if seg["longest_run"] < 8:
            continue
        checked += 1
        if paired == 0:
            return False, "the segment that ends at step %d (%d searches in a row) grouped nothing: %s" % (
                seg["ends_at"], seg["longest_run"], seg["counters"])
        if seg["select_group"] and sum(sel[2:]) == 0:
            return False, "the segment that ends at step %d: no select launch served two calls: %s" % (seg["ends_at"], seg["counters"])
    if checked == 0:
        return False, "no segment holds eight searches in a row"
    return True, ""


def life(s, script_id, build, stall=0):
    script = build()
    exp = pl.expected(script)                                      # the model's answers, computed once and never changed
    twin = perform(s, script, twin=True)
    tries = []
    for attempt in range(ATTEMPTS):
        run = perform(s, script, stall=stall)
        tag = "%s (context %d)" % (script.name, s.attempt)
        check_answers(script, exp, run, twin, tag)
        ok, why = grouped(run)
        tries.append(dict(context=s.attempt, grouped=ok, why=why,
                          segments=[dict(ends_at=g["ends_at"], longest_run=g["longest_run"], select_group=g["select_group"],
                                         pairs=g["counters"][0], deep=g["counters"][1], select=g["counters"][2]) for g in run.segments]))
        s.profile[script_id] = dict(attempts=len(tries), grouped_on_context=s.attempt if ok else None, retried=[t["why"] for t in tries[:-1]],
                                    segments=tries[-1]["segments"])
        print(tag, "grouped" if ok else "NOT grouped: " + why, [(g["longest_run"], g["counters"][0]) for g in run.segments])
        if ok:
            return
        _next_stream(s)
    pytest.fail("%s: no stream of %d grouped: %s" % (script.name, ATTEMPTS, [t["why"] for t in tries]))


@pytest.mark.parametrize("n", pl.SIZES)
@pytest.mark.parametrize("name", list(pl.SCRIPTED))
def test_scripted_life(S, name, n):
    life(S, "%s-%d" % (name, n), lambda: pl.SCRIPTED[name](n))


@pytest.mark.parametrize("seed", pl.RANDOM_SEEDS)
def test_random_life(S, seed):
    """150 steps, 70 % searches, the ops drawn from the scripted ones; the seed (in the script's name) and the step are in every
    assertion message."""
    life(S, "random_life-%d" % seed, lambda: pl.random_life_script(seed))
