"""ctypes wrapper of tests/native/libpart_lower_host.so: K_part's shape selection (siddhi_amd/csrc/
part_lower.h) and the chain kind's per-partial step (part_chain.h) compiled for the host (test
infrastructure only; see tests/native/part_lower_host.cpp), and what the K_part chain tests share:
the stream, the seeded chain apps and their events."""
import ctypes
import os
import subprocess

import numpy as np

from harness import decode_matches

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "part_lower_host.cpp")
SO = os.path.join(HERE, "native", "libpart_lower_host.so")
CSRC = os.path.join(os.path.dirname(HERE), "siddhi_amd", "csrc")
HEADERS = ("part_lower.h", "part_chain.h", "kgen.h", "gen_lower.h", "nfa_types.h")
CXXFLAGS = ["-O2", "-std=c++17", "-Wall", "-Wno-maybe-uninitialized", "-Wno-unused-function", "-ffp-contract=off",
            "-fno-fast-math"]
PK_OR, PK_AND, PK_COUNT, PK_CHAIN = range(4)
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(CSRC, h) for h in HEADERS]
        if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
            subprocess.check_call([os.environ.get("CXX", "g++")] + CXXFLAGS + ["-fPIC", "-shared", "-o", SO, SRC])
        L = ctypes.CDLL(SO)
        P, I64, VP, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int
        L.plh_create.argtypes = [VP, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
        L.plh_create.restype = P
        L.plh_shape.argtypes = [P, I, VP]
        L.plh_set_tile.argtypes = [P, I]
        L.plh_send.argtypes = [P, I, I64, I64, VP, VP, VP]
        L.plh_live.argtypes = [P]
        L.plh_live.restype = I64
        L.plh_num_matches.argtypes = [P]
        L.plh_num_matches.restype = I64
        L.plh_match_words.argtypes = [P]
        L.plh_match_words.restype = I64
        L.plh_get_matches.argtypes = [P, VP, VP, VP, VP, VP]
        L.plh_clear.argtypes = [P]
        L.plh_error.argtypes = [P]
        L.plh_error.restype = ctypes.c_char_p
        L.plh_destroy.argtypes = [P]
        _lib = L
    return _lib


class Shape:
    """What kpart_shape decided for one query (kind -1: not a K_part shape)."""

    def __init__(self, out):
        self.kind, self.sA, self.sB, self.cmax, self.n_e1, self.n_first, self.n_last = (int(x) for x in out)

    @property
    def kept(self):
        """Which of slots 0, 1, 2 the entry stores captured words for."""
        return tuple(bool(x) for x in (self.n_e1, self.n_first, self.n_last))


class PartHostEngine:
    """The queries of a program blob under part_lower.h; send() runs the chain walk on the host."""

    def __init__(self, blob, tile=64):
        self.lib = lib()
        self._blob = ctypes.create_string_buffer(blob, len(blob))
        why = ctypes.create_string_buffer(256)
        self.h = self.lib.plh_create(self._blob, len(blob), why, 256)
        if not self.h:
            raise RuntimeError("the IR blob did not lower: " + why.value.decode())
        self.lib.plh_set_tile(self.h, tile)
        self.seq = 0

    def shape(self, qi):
        out = np.zeros(7, np.int32)
        self.lib.plh_shape(self.h, qi, out.ctypes.data)
        return Shape(out)

    def send(self, stream, ts, vals, nulls, as_chunk=False):
        ts = np.ascontiguousarray(ts, dtype=np.int64)
        vals = np.ascontiguousarray(vals, dtype=np.int64)
        nl = None if nulls is None else np.ascontiguousarray(nulls, dtype=np.uint8)
        rc = self.lib.plh_send(self.h, stream, len(ts), self.seq, ts.ctypes.data, vals.ctypes.data,
                               None if nl is None else nl.ctypes.data)
        self.seq += len(ts)
        if rc != 0:
            raise RuntimeError(self.lib.plh_error(self.h).decode())

    def live(self):
        return self.lib.plh_live(self.h)

    def take_matches(self, n_slots_of):
        n = self.lib.plh_num_matches(self.h)
        nw = self.lib.plh_match_words(self.h)
        q, k, ts = (np.zeros(n, np.int64) for _ in range(3))
        off = np.zeros(n + 1, np.int64)
        words = np.zeros(max(nw, 1), np.int64)
        self.lib.plh_get_matches(self.h, q.ctypes.data, k.ctypes.data, ts.ctypes.data, off.ctypes.data,
                                 words.ctypes.data)
        self.lib.plh_clear(self.h)
        return decode_matches(n, q, k, ts, off, words, n_slots_of)

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.plh_destroy(self.h)
            self.h = None


# ---- the seeded chain apps the CPU and the GPU tests share ----

STREAM = "define stream S (k int, p float, v int, d double);"
# f_s over the current event and the earlier slots: compares over float / int / double attributes,
# arithmetic, or / not, is null, a function, a double compare over a null-bearing column, and
# event-only filters
F2 = ["p > e1.p", "v < e1.v", "d > e1.d", "p > e1.p * 0.9 + 1", "v > e1.v or p < 10", "not (p > e1.p)",
      "e1.d is null or d > e1.d", "maximum(p, e1.p) == p", "v > 500"]
F3 = ["p > e2.p", "v > e1.v and p < e2.p", "d < e2.d", "p + e1.p > e2.p * 1.5", "not (v > e2.v) or d > e1.d",
      "e2.p is null or p > e1.p", "v < 300", "maximum(p, e1.p) == p"]
F4 = ["p > e3.p", "v > e2.v and v > e1.v", "d > e3.d or p < e1.p", "p - e3.p > e2.p - e1.p", "v > 700",
      "e3.d is null or d < e1.d"]


# No oracle sees a function, so the oracle runs the function-free twin of the one function filter:
# maximum(p, e1.p) == p  ==  p >= e1.p. e1.p is non-null and above the fold's seed (e1 passed
# `p > t`, t >= 10), so the fold is e1.p unless p is non-null and greater, when it is p: p > e1.p gives
# p == p TRUE, p == e1.p gives e1.p == p TRUE, p < e1.p gives e1.p == p FALSE, a null p gives
# e1.p == null FALSE -- the twin's compare in every case (the events hold no NaN).
MAXF, MAXF_TWIN = "maximum(p, e1.p) == p", "p >= e1.p"


def chain_queries(seed, n=24, states=(2, 3, 4), twin=False):
    """n partitioned same-stream chains of 2, 3 and 4 states over one stream (twin: the function-free
    twin of the same app, for the oracle)."""
    rng = np.random.default_rng(seed)
    qs = []
    for i in range(n):
        S = states[i % len(states)]
        t = int(rng.integers(10, 90))
        w = int(rng.choice([-1, 5, 20, 60]))
        within = f" within {w} milliseconds" if w > 0 else ""
        pat = f"every e1=S[p > {t}] -> e2=S[{rng.choice(F2)}]"
        sel = "e1.p as a, e2.v as b"
        if S >= 3:
            pat += f" -> e3=S[{rng.choice(F3)}]"
            sel += ", e3.p as c"
        if S >= 4:
            pat += f" -> e4=S[{rng.choice(F4)}]"
            sel += ", e4.d as e"
        qs.append(f"@info(name='q{i}') from {pat}{within} select {sel} insert into O;")
    src = f"{STREAM} partition with (k of S) begin {' '.join(qs)} end;"
    return src.replace(MAXF, MAXF_TWIN) if twin else src


def chain_events(seed, n, keys, nulls=True, unordered=False):
    rng = np.random.default_rng(seed + 1000)
    ts = np.cumsum(rng.integers(0, 4, n)).astype(np.int64)
    if unordered:
        ts = ts + rng.integers(-8, 9, n)
    k = rng.integers(0, keys, n).astype(np.int32)
    p = (rng.integers(0, 10000, n) / 100.0).astype(np.float32)
    v = rng.integers(0, 1000, n).astype(np.int32)
    d = rng.integers(0, 10000, n) / 100.0
    nl = np.zeros((n, 4), np.uint8)
    if nulls:
        nl[:, 1] = rng.random(n) < 0.03
        nl[:, 3] = rng.random(n) < 0.03
    vals = np.stack([k.astype(np.int64), p.view(np.uint32).astype(np.int64), v.astype(np.int64),
                     d.view(np.int64)], 1)
    return ts, vals, nl
