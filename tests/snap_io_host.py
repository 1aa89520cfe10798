"""ctypes wrapper of tests/native/libsnap_io_host.so: the snapshot blob's cursors
(siddhi_amd/csrc/snap_io.h) and their checks compiled for the host (test infrastructure only; see
tests/native/snap_io_host.cpp)."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "snap_io_host.cpp")
SO = os.path.join(HERE, "native", "libsnap_io_host.so")
HEADER = os.path.join(os.path.dirname(HERE), "siddhi_amd", "csrc", "snap_io.h")
CHECKS = ("roundtrip", "truncated", "huge_counts", "need")
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in (SRC, HEADER)):
            subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-Wall", "-shared",
                                   "-o", SO, SRC])
        _lib = ctypes.CDLL(SO)
    return _lib


def run(check):
    """(0, "") or (the failing line, the reason) of one check."""
    msg = ctypes.create_string_buffer(256)
    rc = getattr(lib(), "sih_" + check)(msg, ctypes.c_size_t(len(msg)))
    return rc, msg.value.decode()
