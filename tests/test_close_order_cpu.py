"""CPU: a sharded corpus or model whose group is already destroyed is not destroyed natively.

smt_sharded_corpus_destroy reads the group and its contexts (group_bind, the shards' streams), smt_sharded_model_destroy the contexts.
The cycle collector finalises a dropped set of objects in any order -- what a failed test leaves behind goes that way, group first --
so the wrappers ask the owner before they destroy.  No library here: the native calls are recorded by a stand-in."""
import ctypes as C
import gc

import pytest

from semtools_amd import _lib as L
from semtools_amd import core


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a: self.calls.append(name)


def _make(cls, **attrs):
    o = object.__new__(cls)
    o._h = C.c_void_p(0x1000)
    o.__dict__.update(attrs)
    return o


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: r)
    return r


@pytest.mark.parametrize("cls,destroy", [(core.ShardedCorpus, "smt_sharded_corpus_destroy"), (core.ShardedModel, "smt_sharded_model_destroy")])
def test_dependent_closed_after_its_group_skips_the_native_destroy(rec, cls, destroy):
    g = _make(core.Group)
    first, second = _make(cls, group=g), _make(cls, group=g)
    first.close()
    g.close()
    second.close()
    second.close()
    assert rec.calls == [destroy, "smt_group_destroy"]
    assert first._h is None and second._h is None and g._h is None


def test_collected_cycle_destroys_each_handle_at_most_once_and_never_behind_the_group(rec):
    def leave_a_cycle():
        g = _make(core.Group)
        sc = _make(core.ShardedCorpus, group=g)
        frame = {"g": g, "sc": sc}
        frame["self"] = frame

    gc.collect()
    leave_a_cycle()
    gc.collect()
    assert rec.calls.count("smt_group_destroy") == 1
    assert rec.calls.count("smt_sharded_corpus_destroy") <= 1
    if "smt_sharded_corpus_destroy" in rec.calls:
        assert rec.calls.index("smt_sharded_corpus_destroy") < rec.calls.index("smt_group_destroy")
