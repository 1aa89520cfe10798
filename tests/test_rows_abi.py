"""The output-row entry points of the C ABI (include/siddhi_hip.h): declared, exported, and
SDH_E_INVALID on NULL arguments -- no device needed."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sdh_engine_retain_events", "sdh_engine_poll_rows", "sdh_engine_query_outputs")


def test_declared_and_exported():
    from siddhi_amd.engine import EXPORTS, load_library
    src = open(os.path.join(ROOT, "include", "siddhi_hip.h")).read()
    declared = set(re.findall(r"\b(sdh_\w+)\s*\(", src))
    lib = load_library()
    for s in NEW:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in EXPORTS
    assert "typedef struct sdh_rows" in src and "QuerySelector.java:76-169" in src


def test_null_arguments_are_invalid():
    from siddhi_amd.engine import SdhRows, load_library
    lib = load_library()
    r = SdhRows()
    n = ctypes.c_int32()
    assert lib.sdh_engine_retain_events(None, 1024) == -1
    assert lib.sdh_engine_poll_rows(None, 0, ctypes.byref(r)) == -1
    assert lib.sdh_engine_poll_rows(None, 0, None) == -1
    assert lib.sdh_engine_query_outputs(None, 0, ctypes.byref(n), None, 0) == -1


def test_rows_struct_layout():
    """SdhRows mirrors sdh_rows field by field (LP64: 8 + 4 + 4 + 5 pointers)."""
    from siddhi_amd.engine import SdhRows
    assert ctypes.sizeof(SdhRows) == 56
    assert [f[0] for f in SdhRows._fields_] == ["n", "width", "flags", "query", "ts", "seq", "cells", "nulls"]
