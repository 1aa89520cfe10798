"""ctypes wrapper of tests/native/librec_rows_host.so: siddhi_amd/csrc/rec_rows.h -- the row location,
the rec4 side-run expansion and the flat / K_chain record match sources of sdh_engine_records_rows --
compiled for the host (test infrastructure only; see tests/native/rec_rows_host.cpp)."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "rec_rows_host.cpp")
SO = os.path.join(HERE, "native", "librec_rows_host.so")
CSRC = os.path.join(os.path.dirname(HERE), "siddhi_amd", "csrc")
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(CSRC, h) for h in ("rec_rows.h", "select_body.h", "kgen.h")]
        if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
            subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-Wall",
                                   "-Wno-maybe-uninitialized", "-shared", "-o", SO, SRC])
        L = ctypes.CDLL(SO)
        LL, VP, I = ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int
        LLP = ctypes.POINTER(LL)
        L.rrh_locate.argtypes = [VP, LL, LL]
        L.rrh_locate.restype = LL
        L.rrh_part_of.argtypes = [LL, LL, LL, LL, LLP]
        L.rrh_part_window.argtypes = [LL, LL, LL, I, LL, LL, LLP]
        L.rrh_part_window.restype = LL
        L.rrh_pairs.argtypes = [VP, LL, I, I, I, I, LL, VP]
        L.rrh_side_of.argtypes = [VP, LL, I, I]
        L.rrh_walk.argtypes = [VP, LL, LL, VP, VP, VP, LL, VP, LL, LLP]
        L.rrh_walk.restype = LL
        L.rrh_flat_event.argtypes = [VP, LL, I, LL]
        L.rrh_flat_event.restype = LL
        L.rrh_chain_event.argtypes = [VP, I, I, LL]
        L.rrh_chain_event.restype = LL
        _lib = L
    return _lib


def locate(off, row):
    off = np.ascontiguousarray(off, np.int64)
    return int(lib().rrh_locate(off.ctypes.data, len(off) - 1, row))


def part_of(parts, row):
    local = ctypes.c_longlong()
    p = lib().rrh_part_of(*parts, row, ctypes.byref(local))
    return p, local.value


def part_window(parts, p, first, n):
    local = ctypes.c_longlong()
    c = lib().rrh_part_window(*parts, p, first, n, ctypes.byref(local))
    return local.value, int(c)


def pairs(blk, fmt, ns, i0, i1, seq_base):
    """Entries [i0, i1) of one block (a uint8 array of the block's bytes) -> int64 [i1 - i0, 3]
    (e1, e2, lane), and the side entries a rec4 run read."""
    blk = np.ascontiguousarray(blk, np.uint8)
    out = np.zeros((max(0, i1 - i0), 3), np.int64)
    read = lib().rrh_pairs(blk.ctypes.data, blk.nbytes, fmt, ns, i0, i1, seq_base, out.ctypes.data)
    return out, read


def side_of(blk, ns, i):
    blk = np.ascontiguousarray(blk, np.uint8)
    return lib().rrh_side_of(blk.ctypes.data, blk.nbytes, ns, i)


def walk(words, seq_base):
    """A flat record buffer walked and opened -> ([(head, query, trigger seq, own_ts, ts, slot words)], pads)."""
    words = np.ascontiguousarray(words, np.int64)
    n = len(words)
    heads = np.zeros(n + 1, np.int64)
    meta = np.zeros((n + 1, 4), np.int64)
    wlen = np.zeros(n + 1, np.int64)
    out = np.zeros(4 * n + 16, np.int64)
    pads = ctypes.c_longlong()
    nr = lib().rrh_walk(words.ctypes.data, n, seq_base, heads.ctypes.data, meta.ctypes.data, wlen.ctypes.data,
                        len(heads), out.ctypes.data, len(out), ctypes.byref(pads))
    assert nr >= 0, nr
    recs, at = [], 0
    for i in range(nr):
        recs.append((int(heads[i]), int(meta[i, 0]), int(meta[i, 1]), bool(meta[i, 2]), int(meta[i, 3]),
                     tuple(int(x) for x in out[at:at + wlen[i]])))
        at += int(wlen[i])
    return recs, pads.value


NONE = -(1 << 63)


def flat_event(rec, seq_base, slot, idx):
    rec = np.ascontiguousarray(rec, np.int64)
    v = lib().rrh_flat_event(rec.ctypes.data, seq_base, slot, idx)
    return None if v == NONE else int(v)


def chain_event(rec, S, slot, idx):
    rec = np.ascontiguousarray(rec, np.int64)
    v = lib().rrh_chain_event(rec.ctypes.data, S, slot, idx)
    return None if v == NONE else int(v)
