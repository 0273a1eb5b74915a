"""GPU: the three kernels of csrc/merge.hip -- every sharded answer leaves the library through them -- against a NumPy merge
(tests/merge_ref.py), bit for bit: rows as uint64, distances by their 64-bit patterns, no tolerance anywhere.

Every case of merge_ref.cases() goes through every device form: the plain layout (smt_merge_topk_device), the packed layout
(smt_merge_topk_packed_device, on the context's stream and, with the tuning key merge_on_aux, on its aux stream), the packed layout
with a list stride as the copy and RCCL transports launch it (smt_debug_merge_packed_strided; the gap holds words that are not
padding, so a stride error reads them as candidates) and the in-place merge of the peer transport (smt_debug_merge_sources; every
list in a buffer of its own).  The output is poisoned first, guard words lie around it, and the input is read back afterwards.
tests/test_merge_ref_cpu.py shows, without a GPU, that these cases tell a subtly wrong merge from the right one."""
import functools

import numpy as np
import pytest

from tests import merge_ref as mr

pytestmark = pytest.mark.gpu

NAMES = mr.case_names()
FORMS = ["plain", "packed", "packed_on_aux", "strided_dense", "strided_status_words", "strided_plus_7", "in_place"]
POISON, GUARD, FOREIGN = np.uint64(0xA5A5A5A5A5A5A5A5), np.uint64(0xC3C3C3C3C3C3C3C3), np.uint64(3)
POISON32, GUARD32 = np.uint32(0xA5A5A5A5), np.uint32(0xC3C3C3C3)
G = 64            # guard words on either side of an output
INF_BITS = np.uint64(0x7FF0000000000000)


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401  (first: the library binds to the HIP runtime torch loaded)
    import semtools_amd as smt

    c = smt.Context(0)
    c.aux_stream()       # the aux stream exists, so that merge_on_aux = 1 has somewhere to go
    yield c
    c.close()


def _dev(words):
    """A device tensor holding a copy of a uint64 array."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64).copy()).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64 if t.element_size() == 8 else np.uint32)


class _Guarded:
    """n poisoned words on the device (8 bytes each, or 4) with G guard words in front of them and G behind."""

    def __init__(self, n, bytes_per_word=8):
        import torch

        dt, poison, guard = (np.uint64, POISON, GUARD) if bytes_per_word == 8 else (np.uint32, POISON32, GUARD32)
        h = np.full(G + n + G, poison, dtype=dt)
        h[:G] = guard
        h[G + n:] = guard
        self.n, self.guard = n, guard
        self.t = torch.from_numpy(h.view(np.int64 if bytes_per_word == 8 else np.int32)).cuda()
        self.ptr = self.t.data_ptr() + G * bytes_per_word

    def read(self):
        h = _host(self.t)
        assert (h[:G] == self.guard).all(), "words in front of the output were written"
        assert (h[G + self.n:] == self.guard).all(), "words behind the output were written"
        return h[G:G + self.n].copy()

    def untouched(self):
        h = self.read()
        return bool((h == (POISON if h.dtype == np.uint64 else POISON32)).all())


def _strided(packed, stride):
    """The lists of packed [n][nq][2][k] laid stride words apart, the gaps filled with words that are not padding."""
    n = packed.shape[0]
    flat = np.full(max(n * stride, 1), FOREIGN, dtype=np.uint64)
    for l in range(n):
        flat[l * stride:l * stride + packed[l].size] = packed[l].reshape(-1)
    return flat


def _launch(ctx, form, rows, dist, k_out, passed=None):
    """Prepares one merge of form `form`: (the call, the inputs as (device tensor, host copy) pairs, the guarded outputs, a reader of
    the answer as (rows, dist)).  passed: n_lists / nq / k_out as the library is to hear them, where they are not the arrays'
    (the buffers keep the arrays' sizes: what such a call reads or writes, if it wrongly does, is memory that is there)."""
    import torch

    n, nq, k_in = rows.shape
    passed = passed or {}
    a_n, a_nq, a_k = passed.get("n_lists", n), passed.get("nq", nq), passed.get("k_out", k_out)
    if form == "plain":
        host = [np.array(rows).reshape(-1), np.array(dist).view(np.uint64).reshape(-1)]
        ins = [_dev(h) for h in host]
        o_r, o_d = _Guarded(nq * k_out), _Guarded(nq * k_out)
        torch.cuda.synchronize()
        call = lambda: ctx.merge_topk_device(ins[0].data_ptr(), ins[1].data_ptr(), a_n, a_nq, k_in, a_k, o_r.ptr, o_d.ptr)
        read = lambda: (o_r.read().reshape(nq, k_out), o_d.read().reshape(nq, k_out).view(np.float64))
        return call, list(zip(ins, host)), [o_r, o_d], read
    packed = mr.pack(rows, dist)
    out = _Guarded(nq * 2 * k_out)
    read = lambda: mr.unpack(out.read().reshape(nq, 2, k_out))
    if form in ("packed", "packed_on_aux"):
        host = [packed.reshape(-1)]
        ins = [_dev(host[0])]
        call = lambda: ctx.merge_topk_packed_device(ins[0].data_ptr(), a_n, a_nq, k_in, a_k, out.ptr)
    elif form.startswith("strided"):
        stride = nq * 2 * k_in + _gap(form, nq)
        host = [_strided(packed, stride)]
        ins = [_dev(host[0])]
        call = lambda: ctx.debug_merge_packed_strided(ins[0].data_ptr(), stride, a_n, a_nq, k_in, a_k, out.ptr)
    else:
        assert form == "in_place"
        host = [packed[l].reshape(-1) for l in range(n)]
        ins = [_dev(h) for h in host]     # one allocation per list
        call = lambda: ctx.debug_merge_sources([t.data_ptr() for t in ins], a_nq, k_in, a_k, out.ptr, n_lists=a_n)
    torch.cuda.synchronize()
    return call, list(zip(ins, host)), [out], read


def _gap(form, nq):
    """Words between two lists: none, a rank's status words (nq verdicts and one more), or seven."""
    return {"strided_dense": 0, "strided_status_words": nq + 1, "strided_plus_7": 7}[form]


def _on_stream_of(ctx, form, call):
    """Runs `call` with merge_on_aux set as the form wants it and drains the context (its aux stream too)."""
    ctx.set_tuning("merge_on_aux", 1 if form == "packed_on_aux" else 0)
    try:
        call()
        ctx.synchronize()
    finally:
        ctx.set_tuning("merge_on_aux", 0)


def _run(ctx, form, rows, dist, k_out):
    call, ins, outs, read = _launch(ctx, form, rows, dist, k_out)
    _on_stream_of(ctx, form, call)
    got = read()
    for t, h in ins:
        assert np.array_equal(_host(t)[:h.size], h), "the merge wrote into its input"
    return got


@functools.lru_cache(maxsize=None)
def _reference(name):
    rows, dist, k_out = mr.case(name)
    return mr.merge_lists(rows, dist, k_out)


def _assert_same(got, want, what):
    (g_r, g_d), (w_r, w_d) = got, want[:2]
    bad = np.argwhere((g_r != w_r) | (np.ascontiguousarray(g_d).view(np.uint64) != np.ascontiguousarray(w_d).view(np.uint64)))
    if len(bad):
        q, i = (int(v) for v in bad[0])
        raise AssertionError("%s: %d of %d slots differ; first at query %d slot %d: got (%d, %r), expected (%d, %r)"
                             % (what, len(bad), g_r.size, q, i, g_r[q, i], g_d[q, i], w_r[q, i], w_d[q, i]))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_merge_equals_the_numpy_merge(ctx, name, form):
    rows, dist, k_out = mr.case(name)
    _assert_same(_run(ctx, form, rows, dist, k_out), _reference(name), "%s / %s" % (name, form))


# ------------------------------------------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize("form", [f for f in FORMS if f != "in_place"])
@pytest.mark.parametrize("aliased", [False, True], ids=["out_apart", "out_is_in"])
def test_no_lists_write_padding(ctx, form, aliased):
    """n_lists == 0: k_out padding entries per query -- also with the output given as the input, as search.cpp and topk_large.hip
    pad the lists of an empty corpus (n_lists 0, k_in 1).  (The in-place form refuses n_lists == 0, below.)"""
    import torch

    nq, k_out = 3, 300
    outs = [_Guarded(nq * k_out), _Guarded(nq * k_out)] if form == "plain" else [_Guarded(nq * 2 * k_out)]
    other = _dev(np.full(nq * 2 * k_out, FOREIGN, dtype=np.uint64))
    src = [o.ptr for o in outs] if aliased else [other.data_ptr(), other.data_ptr()]
    torch.cuda.synchronize()
    if form == "plain":
        call = lambda: ctx.merge_topk_device(src[0], src[1], 0, nq, 1, k_out, outs[0].ptr, outs[1].ptr)
    elif form in ("packed", "packed_on_aux"):
        call = lambda: ctx.merge_topk_packed_device(src[0], 0, nq, 1, k_out, outs[0].ptr)
    else:
        call = lambda: ctx.debug_merge_packed_strided(src[0], 2 * nq + _gap(form, nq), 0, nq, 1, k_out, outs[0].ptr)
    _on_stream_of(ctx, form, call)
    if form == "plain":
        got_r, got_d = outs[0].read(), outs[1].read()
    else:
        w = outs[0].read().reshape(nq, 2, k_out)
        got_r, got_d = w[:, 0, :], w[:, 1, :]
    assert (got_r == mr.PAD).all() and (got_d == INF_BITS).all()
    assert (_host(other) == FOREIGN).all()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("passed", [dict(nq=0), dict(k_out=0)], ids=["no_query", "k_out_0"])
def test_nothing_to_do_is_ok_and_touches_nothing(ctx, form, passed):
    rows, dist, k_out = mr.case("dealt-3x6_to_6_nq3")
    call, ins, outs, _ = _launch(ctx, form, rows, dist, k_out, passed=passed)
    _on_stream_of(ctx, form, call)           # SMT_OK: anything else raises
    assert all(o.untouched() for o in outs)


# --------------------------------------------------------------------------------------------------------------------- refusals
def _refused(ctx, form, n_lists, k_in, n_alloc=None):
    """The call of `form` over n_lists x k_in candidates per query is SMT_E_INVALID and leaves the poisoned output alone.  The
    lists it names exist (n_alloc of them where the in-place form would need more buffers than it may ever read: its pointer
    table has 64 entries)."""
    from semtools_amd import _lib as L

    nq, k_out = 1, 8
    n_alloc = n_lists if n_alloc is None else n_alloc
    rows = np.arange(n_alloc * nq * k_in, dtype=np.uint64).reshape(n_alloc, nq, k_in)
    dist = np.linspace(0.0, 1.0, rows.size).reshape(rows.shape)
    call, _, outs, _ = _launch(ctx, form, rows, dist, k_out, passed=dict(n_lists=n_lists))
    with pytest.raises(L.SmtError) as e:
        _on_stream_of(ctx, form, call)
    ctx.synchronize()
    assert e.value.code == L.SMT_E_INVALID, e.value
    assert all(o.untouched() for o in outs)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n_lists,k_in", [(8193, 1), (3, 2731), (9, 911)])
def test_more_than_8192_candidates_are_refused(ctx, form, n_lists, k_in):
    assert n_lists * k_in > 8192 and (n_lists * k_in == 8193 or n_lists == 9)
    _refused(ctx, form, n_lists, k_in, n_alloc=min(n_lists, 65) if form == "in_place" else None)


def test_in_place_merge_refuses_65_lists_and_no_list(ctx):
    _refused(ctx, "in_place", 65, 1)
    _refused(ctx, "in_place", 0, 4, n_alloc=1)


# --------------------------------------------------------------------------------------------------------------- status combine
def _status_patterns(n, nq, seed):
    rng = np.random.default_rng(seed)
    drawn = rng.integers(0, 4, size=(n, nq)).astype(np.uint64)
    last_only = np.zeros((n, nq), dtype=np.uint64)
    last_only[-1] = rng.integers(1, 4, size=nq)
    different = ((np.arange(n)[:, None] + np.arange(nq)[None, :]) % n + 1).astype(np.uint64)     # every source another code
    return {"drawn": drawn, "last_only": last_only, "all_different": different}


@pytest.mark.parametrize("nq", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("n", [1, 2, 9, 64])
def test_status_combine_equals_the_maximum(ctx, n, nq):
    import torch

    for pattern, words in _status_patterns(n, nq, seed=1000 * n + nq).items():
        want = mr.combine_status(words)
        # by pointer: every source's words in a buffer of its own (the peer transport)
        srcs = [_dev(words[j]) for j in range(n)]
        out = _Guarded(nq, 4)
        torch.cuda.synchronize()
        ctx.debug_combine_status(n, nq, out.ptr, word_ptrs=[t.data_ptr() for t in srcs])
        ctx.synchronize()
        assert np.array_equal(out.read(), want), (pattern, "pointers")      # (read() looks at the words behind out[nq - 1] too)
        assert all(np.array_equal(_host(t), words[j]) for j, t in enumerate(srcs))
        # strided: blocks of nq words, stride > nq apart behind one base, foreign words in the gaps (the gathered buffer)
        stride = nq + 5
        flat = np.full(n * stride, np.uint64(0xFFFF), dtype=np.uint64)
        for j in range(n):
            flat[j * stride:j * stride + nq] = words[j]
        base = _dev(flat)
        out = _Guarded(nq, 4)
        torch.cuda.synchronize()
        ctx.debug_combine_status(n, nq, out.ptr, base_ptr=base.data_ptr(), stride_words=stride)
        ctx.synchronize()
        assert np.array_equal(out.read(), want), (pattern, "strided")
        assert np.array_equal(_host(base), flat)


def test_status_combine_wants_exactly_one_kind_of_source(ctx):
    import torch
    from semtools_amd import _lib as L

    n, nq = 2, 10
    words = _status_patterns(n, nq, seed=3)["drawn"]
    srcs = [_dev(words[j]) for j in range(n)]
    base = _dev(words.reshape(-1))
    out = _Guarded(nq, 4)
    torch.cuda.synchronize()
    for kw in (dict(word_ptrs=[t.data_ptr() for t in srcs], base_ptr=base.data_ptr(), stride_words=nq), dict()):
        with pytest.raises(L.SmtError) as e:
            ctx.debug_combine_status(n, nq, out.ptr, **kw)
        assert e.value.code == L.SMT_E_INVALID
    ctx.synchronize()
    assert out.untouched()


