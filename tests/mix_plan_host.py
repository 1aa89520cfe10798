"""ctypes wrapper of tests/native/libmix_plan_host.so: the eligibility of an interleaved push
(siddhi_amd/csrc/mix_plan.h) compiled for the host (test infrastructure only; see
tests/native/mix_plan_host.cpp)."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "mix_plan_host.cpp")
SO = os.path.join(HERE, "native", "libmix_plan_host.so")
HEADER = os.path.join(os.path.dirname(HERE), "siddhi_amd", "csrc", "mix_plan.h")
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in (SRC, HEADER)):
            subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-Wall", "-shared",
                                   "-o", SO, SRC])
        L = ctypes.CDLL(SO)
        L.mph_why_split.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
        L.mph_kind.argtypes = [ctypes.c_char_p]
        L.mph_kind.restype = ctypes.c_uint
        _lib = L
    return _lib


def kind(names):
    """The consumer bitmask of a stream read by the named plans ("chain gen")."""
    m = 0
    for n in names.split():
        k = lib().mph_kind(n.encode())
        assert k, n
        m |= k
    return m


def why_split(parts, total=100, knob=False, comm=False, timed=False):
    """None for a native call, else the reason; parts: per named stream the plans that read it."""
    arr = (ctypes.c_uint32 * max(1, len(parts)))(*[kind(p) for p in parts])
    why = ctypes.create_string_buffer(128)
    rc = lib().mph_why_split(len(parts), arr, total, int(knob), int(comm), int(timed), why, len(why))
    assert (rc == 0) == (why.value == b"")
    return why.value.decode() if rc else None
