"""ctypes wrapper of tests/native/libwave_host.so: K_wave's shape selection (siddhi_amd/csrc/wave_lower.h)
and its per-partial step (wave_step.h) compiled for the host (test infrastructure only; see
tests/native/wave_host.cpp), and what the K_wave tests share: the stream, the seeded count apps and
their events."""
import ctypes
import os
import subprocess

import numpy as np

from harness import decode_matches
from part_lower_host import STREAM

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "wave_host.cpp")
SO = os.path.join(HERE, "native", "libwave_host.so")
CSRC = os.path.join(os.path.dirname(HERE), "siddhi_amd", "csrc")
HEADERS = ("wave_lower.h", "wave_step.h", "part_lower.h", "part_chain.h", "kgen.h", "gen_lower.h", "nfa_types.h")
CXXFLAGS = ["-O2", "-std=c++17", "-Wall", "-Wno-maybe-uninitialized", "-Wno-unused-function", "-ffp-contract=off",
            "-fno-fast-math"]
PK_COUNT = 2
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(CSRC, h) for h in HEADERS]
        if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
            subprocess.check_call([os.environ.get("CXX", "g++")] + CXXFLAGS + ["-fPIC", "-shared", "-o", SO, SRC])
        L = ctypes.CDLL(SO)
        P, I64, VP, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int
        L.wvh_create.argtypes = [VP, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
        L.wvh_create.restype = P
        L.wvh_shape.argtypes = [P, I, I, VP]
        L.wvh_why.argtypes = [P, I]
        L.wvh_why.restype = ctypes.c_char_p
        L.wvh_set_tile.argtypes = [P, I]
        L.wvh_send.argtypes = [P, I, I64, I64, VP, VP, VP]
        for f in ("wvh_live", "wvh_seeds", "wvh_entries", "wvh_num_matches", "wvh_match_words"):
            getattr(L, f).argtypes = [P]
            getattr(L, f).restype = I64
        L.wvh_get_matches.argtypes = [P, VP, VP, VP, VP, VP]
        L.wvh_clear.argtypes = [P]
        L.wvh_error.argtypes = [P]
        L.wvh_error.restype = ctypes.c_char_p
        L.wvh_destroy.argtypes = [P]
        _lib = L
    return _lib


class WaveHostEngine:
    """The queries of a program blob under wave_lower.h; send() runs the kernel's walk on the host."""

    def __init__(self, blob, tile=64):
        self.lib = lib()
        self._blob = ctypes.create_string_buffer(blob, len(blob))
        why = ctypes.create_string_buffer(256)
        self.h = self.lib.wvh_create(self._blob, len(blob), why, 256)
        if not self.h:
            raise RuntimeError("the IR blob did not lower: " + why.value.decode())
        self.lib.wvh_set_tile(self.h, tile)
        self.seq = 0

    def shape(self, qi, kpart=False):
        """(kind, sA, sB, cmax, n_e1, n_first, n_last) under wave_shape, or under kpart_shape."""
        out = np.zeros(7, np.int32)
        self.lib.wvh_shape(self.h, qi, int(kpart), out.ctypes.data)
        return tuple(int(x) for x in out)

    def why(self, qi):
        return self.lib.wvh_why(self.h, qi).decode()

    def send(self, stream, ts, vals, nulls, as_chunk=False):
        ts = np.ascontiguousarray(ts, dtype=np.int64)
        vals = np.ascontiguousarray(vals, dtype=np.int64)
        nl = None if nulls is None else np.ascontiguousarray(nulls, dtype=np.uint8)
        rc = self.lib.wvh_send(self.h, stream, len(ts), self.seq, ts.ctypes.data, vals.ctypes.data,
                               None if nl is None else nl.ctypes.data)
        self.seq += len(ts)
        if rc != 0:
            raise RuntimeError(self.lib.wvh_error(self.h).decode())

    def live(self):
        """Pending-list entries of the non-start states: what sdh_stats.live_partials reports."""
        return self.lib.wvh_live(self.h)

    def seeds(self):
        """Start states whose pending list holds its seed (the oracle's live count includes them)."""
        return self.lib.wvh_seeds(self.h)

    def entries(self):
        return self.lib.wvh_entries(self.h)

    def take_matches(self, n_slots_of):
        n = self.lib.wvh_num_matches(self.h)
        nw = self.lib.wvh_match_words(self.h)
        q, k, ts = (np.zeros(n, np.int64) for _ in range(3))
        off = np.zeros(n + 1, np.int64)
        words = np.zeros(max(nw, 1), np.int64)
        self.lib.wvh_get_matches(self.h, q.ctypes.data, k.ctypes.data, ts.ctypes.data, off.ctypes.data,
                                 words.ctypes.data)
        self.lib.wvh_clear(self.h)
        return decode_matches(n, q, k, ts, off, words, n_slots_of)

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.wvh_destroy(self.h)
            self.h = None


# ---- the seeded count apps the CPU and the GPU tests share ----

COUNTS = [(1, 1), (1, 8), (2, 5), (3, 3)]
# f3 by what it reads of the partial: e1, e2[0], e2[last], nothing captured, all three
F3 = {"e1": ["p > e1.p", "v > e1.v or d < e1.d"],
      "first": ["v >= e2[0].v", "p > e2[0].p"],
      "last": ["p > e2[last].p", "d > e2[last].d or e2[last].d is null"],
      "none": ["v > 850", "p < 6 and v < 500"],
      "all": ["p > e1.p and p > e2[last].p and v >= e2[0].v"]}
F3_KEPT = {"e1": (True, False, False), "first": (False, True, False), "last": (False, False, True),
           "none": (False, False, False), "all": (True, True, True)}


def wave_query(i, t1, t2, cnt, f3, within):
    w = f" within {within} milliseconds" if within > 0 else ""
    return (f"@info(name='w{i}') from every e1=S[p > {t1}] -> e2=S[v > {t2}]<{cnt[0]}:{cnt[1]}> -> e3=S[{f3}]{w} "
            f"select e1.p as a, e2[0].p as b, e2[last].p as c, e3.p as d insert into O;")


def wave_queries(seed, n=10, reads=None, counts=None, withins=(-1, 3, 12, 50)):
    """n unpartitioned count patterns over one stream: <min:max> from COUNTS, f3 over e1 / e2[0] /
    e2[last] / nothing captured / all, `within` absent or 3-50 ms."""
    rng = np.random.default_rng(seed)
    kinds = list(F3) if reads is None else list(reads)
    qs = []
    for i in range(n):
        cnt = (counts or COUNTS)[i % len(counts or COUNTS)]
        kind = kinds[(i // len(COUNTS)) % len(kinds)] if reads is None else kinds[i % len(kinds)]
        f3 = F3[kind][int(rng.integers(0, len(F3[kind])))]
        qs.append(wave_query(i, int(rng.integers(55, 95)), int(rng.integers(500, 900)), cnt, f3,
                             int(withins[int(rng.integers(0, len(withins)))])))
    return f"{STREAM} {' '.join(qs)}"


def wave_events(seed, n, nulls=0.3, unordered=False):
    """Random events of STREAM: ts steps of 0-3 ms (unordered: jittered), `nulls` of the captured
    attributes p, v, d null."""
    rng = np.random.default_rng(seed + 7000)
    ts = np.cumsum(rng.integers(0, 4, n)).astype(np.int64)
    if unordered:
        ts = ts + rng.integers(-8, 9, n)
    k = rng.integers(0, 4, n).astype(np.int32)
    p = (rng.integers(0, 10000, n) / 100.0).astype(np.float32)
    v = rng.integers(0, 1000, n).astype(np.int32)
    d = rng.integers(0, 10000, n) / 100.0
    nl = np.zeros((n, 4), np.uint8)
    for c in (1, 2, 3):
        nl[:, c] = rng.random(n) < nulls
    vals = np.stack([k.astype(np.int64), p.view(np.uint32).astype(np.int64), v.astype(np.int64),
                     d.view(np.int64)], 1)
    return ts, vals, nl


def pv_events(p, v=None, ts=None):
    """Events of STREAM with the given p (and v) columns, 1 ms apart, no nulls."""
    n = len(p)
    p = np.asarray(p, np.float32)
    v = np.zeros(n, np.int64) if v is None else np.asarray(v, np.int64)
    ts = np.arange(n, dtype=np.int64) if ts is None else np.asarray(ts, np.int64)
    vals = np.stack([np.zeros(n, np.int64), p.view(np.uint32).astype(np.int64), v, np.zeros(n, np.int64)], 1)
    return ts, vals, np.zeros((n, 4), np.uint8)


# the app that outgrows a K_gen instance's pools (tests/test_gpu_wave.py, tools/wave_bench.py's deep leg)
DEEP_APP = (f"{STREAM} @info(name='deep') from every e1=S[p > 1] -> e2=S[p > 5000]<2:5> -> "
            "e3=S[p > e1.p and p > e2[last].p and v >= e2[0].v] within 1 hour "
            "select e1.p as a, e2[0].p as b, e2[last].p as c, e3.p as d insert into O;")


def deep_events(n=4200, seed=3):
    """n events with p in 2..8 (each opens a partial; none passes f2), then 6000, 6001, 6002, 7000."""
    rng = np.random.default_rng(seed)
    p = np.concatenate([rng.integers(2, 9, n).astype(np.float32), np.array([6000, 6001, 6002, 7000], np.float32)])
    return pv_events(p)
