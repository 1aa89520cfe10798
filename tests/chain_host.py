"""ctypes wrapper of tests/native/libchain_host.so: K_chain's lowering (siddhi_amd/csrc/chain_lower.h)
and the lane body its kernels evaluate residual programs with (chain_pred.h), compiled for the host
(test infrastructure only; see tests/native/chain_host.cpp), and what the K_chain predicate tests share:
the typed stream, its adversarial events and the seeded filters."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "chain_host.cpp")
SO = os.path.join(HERE, "native", "libchain_host.so")
CSRC = os.path.join(os.path.dirname(HERE), "siddhi_amd", "csrc")
HEADERS = ("chain_lower.h", "chain_pred.h", "kgen.h", "gen_lower.h", "nfa_types.h")
CXXFLAGS = ["-O2", "-std=c++17", "-Wall", "-Wno-maybe-uninitialized", "-Wno-unused-function", "-ffp-contract=off",
            "-fno-fast-math"]
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(CSRC, h) for h in HEADERS]
        if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
            subprocess.check_call([os.environ.get("CXX", "g++")] + CXXFLAGS + ["-fPIC", "-shared", "-o", SO, SRC])
        L = ctypes.CDLL(SO)
        P, VP, I, I64 = ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
        L.clh_create.argtypes = [VP, ctypes.c_size_t]
        L.clh_create.restype = P
        L.clh_destroy.argtypes = [P]
        L.clh_lower.argtypes = [P, I, I, VP]
        L.clh_why.argtypes = [P, I, I]
        L.clh_why.restype = ctypes.c_char_p
        L.clh_col.argtypes = [P, I, I, VP]
        L.clh_state_pass.argtypes = [P, I, I, I64, VP, VP, I, VP]
        _lib = L
    return _lib


class Lowering:
    """What chain_lower.h decided for one query."""

    def __init__(self, out, why):
        self.ok = bool(out[0])
        self.why = why
        self.n_col, self.n_cap, self.n_xa, self.n_atoms, self.n_code = (int(x) for x in out[1:6])
        self.ratchet = bool(out[6])
        self.xa_count = [int(out[8 + 4 * s]) for s in range(4)]
        self.tile_atoms = [int(out[9 + 4 * s]) for s in range(4)]
        self.tile_code = [int(out[10 + 4 * s]) for s in range(4)]
        self.partial_code = [int(out[11 + 4 * s]) for s in range(4)]


class HostChain:
    """The queries of a program blob under chain_lower.h."""

    def __init__(self, blob: bytes):
        self.lib = lib()
        self._blob = ctypes.create_string_buffer(blob, len(blob))
        self.h = self.lib.clh_create(self._blob, len(blob))
        if not self.h:
            raise RuntimeError("the IR blob did not read")

    def lower(self, qi: int, allow_residual=True) -> Lowering:
        out = np.zeros(24, np.int32)
        self.lib.clh_lower(self.h, qi, int(allow_residual), out.ctypes.data)
        return Lowering(out, self.lib.clh_why(self.h, qi, int(allow_residual)).decode())

    def columns(self, qi: int, n: int):
        """(attribute, conversion, stream) of the query's first n columns."""
        cols = []
        for c in range(n):
            out = np.zeros(3, np.int32)
            self.lib.clh_col(self.h, qi, c, out.ctypes.data)
            cols.append(tuple(int(x) for x in out))
        return cols

    def state_pass(self, qi: int, s: int, vals, nulls):
        """State s's whole filter (atoms and residuals) over cases: vals / nulls [case][slot][attribute]."""
        vals = np.ascontiguousarray(vals, np.int64)
        nulls = np.ascontiguousarray(nulls, np.uint8)
        n, _, na = vals.shape
        out = np.zeros(n, np.uint8)
        self.lib.clh_state_pass(self.h, qi, s, n, vals.ctypes.data, nulls.ctypes.data, na, out.ctypes.data)
        return out.astype(bool)

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.clh_destroy(self.h)
            self.h = None


TYPED_STREAM = "define stream T (i int, l long, f float, d double, b bool, s string);"
NUMERIC = ["i", "l", "f", "d"]


def typed_events(n=400, seed=3):
    """Adversarial values for Java's typed compares and arithmetic (the generator of
    test_gpu_chain.typed_events): int->float and long->float/double rounding boundaries, signed zeros,
    NaN, infinities, extremes; some nulls."""
    rng = np.random.default_rng(seed)
    ints = [0, 1, -1, 16777216, 16777217, -16777217, 2**31 - 1, -2**31, 123456789, 7]
    longs = [0, 1, -1, 16777217, 2**53, 2**53 + 1, 2**62 + 1, -2**63, 2**63 - 1, 9007199254740993, 7]
    floats = [0.0, -0.0, 1.0, 16777216.0, 16777218.0, float("nan"), float("inf"), -float("inf"),
              3.4028235e38, 1e-45, 7.0, 0.1]
    doubles = [0.0, -0.0, 1.0, 16777217.0, 9007199254740992.0, 9007199254740994.0, float("nan"),
               float("inf"), 0.1, 7.0, 1e300]
    rows = []
    for k in range(n):
        row = [int(rng.choice(ints)), int(rng.choice(longs)), float(np.float32(rng.choice(floats))),
               float(rng.choice(doubles)), bool(rng.integers(2)), str(rng.choice(["a", "b", "c"]))]
        if rng.random() < 0.05:
            row[int(rng.integers(6))] = None
        rows.append(row)
    return rows


def pred_filters():
    """e2 filters over (the current event, e1) that K_chain evaluates through a residual program: each
    arithmetic op over every numeric pair (the events hold zeros: / 0 and % 0), or / not / is null,
    compares of computed values, bare conjuncts beside plain atoms."""
    fs = []
    for k, a in enumerate(NUMERIC):
        for j, b in enumerate(NUMERIC):
            op = "+-*/%"[(k * 4 + j) % 5]
            fs.append(f"{a} {op} e1.{b} > 1")
    for op, (a, b) in zip("+-*/%/%", [("i", "i"), ("l", "l"), ("f", "f"), ("d", "d"), ("l", "i"), ("i", "i"), ("f", "d")]):
        fs.append(f"e1.{a} {op} {b} <= {a}")
    fs += ["(i / e1.i) is null", "(d % e1.f) is null", "not (f > e1.f)", "not (l > e1.i)", "i > e1.i or e2.l is null",
           "e1.d is null or d > e1.d", "e2.s is null or s == e1.s", "not (b == e1.b)", "b or e1.b", "not b and e1.b",
           "i + l > e1.f * d", "i * 2 > e1.i + 1 and f > e1.f", "f > e1.f * 1.05", "i > e1.i or l > 2 * e1.l",
           "s == e1.s and f > e1.f", "s == e1.s and f > e1.f and i != e1.i", "i > 0 and (d > e1.d or e1.b)",
           "e1.s != 'b' and (s == 'a' or s == e1.s)", "(i > e1.i) == (l > e1.l)", "i - e1.i == l - e1.l"]
    return fs
