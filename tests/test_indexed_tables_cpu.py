"""Indexed model tables (mapping + per-token weights), the parts that need no GPU: the header declares the new entry points and the
library exports them, the binding refuses malformed token arrays before it touches the device, hf.py reads a three-tensor
directory into (table as stored, u32 mapping, f32 weights)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["smt_model_create_indexed", "smt_model_create_from_file_indexed", "smt_model_create_from_device_indexed", "smt_model_token_info",
       "smt_sharded_model_create_indexed", "smt_sharded_model_create_from_file_indexed", "smt_sharded_model_token_info"]


def test_header_declares_and_library_exports_the_new_functions():
    from semtools_amd import _lib as L

    hdr = open(os.path.join(ROOT, "include", "semtools_hip.h")).read()
    host_hdr = open(os.path.join(ROOT, "include", "semtools_host.h")).read()
    lib = L.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in L.EXPORTS and hasattr(lib, name), name
    assert re.search(r"\bint\s+smt_host_model_token_info\s*\(", host_hdr)
    assert "smt_host_model_token_info" in L.HOST_EXPORTS and hasattr(lib, "smt_host_model_token_info")


class _NoDevice:
    """A context whose handle must never be read: the checks below happen before the library is called."""

    @property
    def _h(self):
        raise AssertionError("the binding touched the device before refusing its arguments")


def test_binding_refuses_malformed_token_arrays_before_touching_the_device():
    import semtools_amd as smt

    table = np.zeros((40, 256), np.int8)
    good = np.arange(300) % 40
    bad_neg = good.astype(np.int64)
    bad_neg[17] = -1
    w = np.ones(300, np.float32)
    for make in (lambda **kw: smt.Model(_NoDevice(), table, **kw),
                 lambda **kw: smt.Model.from_file(_NoDevice(), "/nonexistent", 0, 40, dtype=np.int8, **kw),
                 lambda **kw: smt.ShardedModel(_NoDevice(), table, **kw)):
        with pytest.raises(ValueError, match="negative.*token 17"):
            make(mapping=bad_neg, weights=w)
        with pytest.raises(ValueError, match="one per token"):
            make(mapping=good, weights=w[:299])
        with pytest.raises(ValueError, match="one entry per table row"):
            make(weights=w)                                  # 300 weights, 40 rows, no mapping
        with pytest.raises(ValueError):
            make(mapping=good.astype(np.float32))            # not an integer array
        with pytest.raises(ValueError):
            make(mapping=good.reshape(3, 100))
        with pytest.raises(ValueError):
            make(mapping=np.zeros(0, np.int64))


def test_token_arrays_are_converted_by_value():
    from semtools_amd import _lib as L

    m, w, n = L.token_arrays(np.array([3, 0, 2], np.int64), np.array([0.5, 2.0 ** -130, -0.0], np.float64), 4)
    assert m.dtype == np.uint32 and m.tolist() == [3, 0, 2] and n == 3
    assert w.dtype == np.float32 and w[0] == 0.5 and w[1] == np.float32(2.0 ** -130) and np.signbit(w[2])
    assert L.token_arrays(None, None, 7) == (None, None, 7)


def test_hf_reads_a_three_tensor_directory(tmp_path):
    from safetensors.numpy import save_file
    from semtools_amd import hf

    rng = np.random.default_rng(5)
    table = rng.integers(-128, 128, size=(40, 256)).astype(np.int8)
    mapping = rng.integers(0, 40, size=300).astype(np.int64)
    weights = rng.uniform(0.25, 4, size=300)                 # float64
    save_file({"embeddings": table, "mapping": mapping, "weights": weights}, str(tmp_path / "model.safetensors"))
    t, m, w = hf.read_model_tensors(str(tmp_path))
    assert t.dtype == np.int8 and np.array_equal(t, table)
    assert m.dtype == np.uint32 and np.array_equal(m, mapping)
    assert w.dtype == np.float32 and np.array_equal(w, weights.astype(np.float32))
    # float16 weights, int32 mapping; a plain directory gives (table, None, None)
    save_file({"embeddings": table.astype(np.float16), "mapping": mapping.astype(np.int32), "weights": weights.astype(np.float16)},
              str(tmp_path / "model.safetensors"))
    t, m, w = hf.read_model_tensors(str(tmp_path))
    assert t.dtype == np.float16 and m.dtype == np.uint32 and np.array_equal(w, weights.astype(np.float16).astype(np.float32))
    save_file({"embeddings": table}, str(tmp_path / "model.safetensors"))
    t, m, w = hf.read_model_tensors(str(tmp_path))
    assert m is None and w is None and t.dtype == np.int8
    mapping[5] = -3
    save_file({"embeddings": table, "mapping": mapping}, str(tmp_path / "model.safetensors"))
    with pytest.raises(ValueError, match="negative"):
        hf.read_model_tensors(str(tmp_path))
