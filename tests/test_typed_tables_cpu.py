"""CPU: the typed-table surface of the C ABI is in the header and in the library, and the Python binding does not convert a table
of an unsupported dtype silently."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "semtools_hip.h")
NEW = ["smt_model_create_typed", "smt_model_create_from_file_typed", "smt_model_create_from_device_typed", "smt_model_info",
       "smt_sharded_model_create_typed", "smt_sharded_model_create_from_file_typed", "smt_sharded_model_info", "smt_host_model_table_info"]


def test_header_declares_the_constants_and_functions():
    hdr = open(HEADER).read() + open(os.path.join(ROOT, "include", "semtools_host.h")).read()
    for name, val in (("SMT_TABLE_F32", 0), ("SMT_TABLE_F16", 1), ("SMT_TABLE_I8", 2)):
        assert re.search(rf"#define\s+{name}\s+{val}\b", hdr), name
    for fn in NEW:
        assert re.search(rf"\bint\s+{fn}\s*\(", hdr), fn


def test_library_exports_the_new_symbols():
    from semtools_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [fn for fn in NEW if fn not in exported]
    assert all(fn in _lib.EXPORTS + _lib.HOST_EXPORTS for fn in NEW)
    assert (_lib.TABLE_F32, _lib.TABLE_F16, _lib.TABLE_I8) == (0, 1, 2)


def test_binding_rejects_a_float64_table_before_touching_the_device():
    import semtools_amd as smt
    from semtools_amd import _lib

    class NoCtx:      # never reached: the dtype is checked first
        _h = None

    for bad in (np.float64, np.int16, np.uint8):
        with pytest.raises(TypeError, match="float32, float16 or int8"):
            smt.Model(NoCtx(), np.zeros((4, 256), dtype=bad))
        with pytest.raises(TypeError, match="float32, float16 or int8"):
            _lib.table_dtype_code(bad)
    assert [_lib.table_dtype_code(t) for t in (np.float32, np.float16, "int8")] == [0, 1, 2]
