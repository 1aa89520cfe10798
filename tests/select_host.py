"""ctypes wrapper of tests/native/libselect_host.so: the device selector's lane body
(siddhi_amd/csrc/select_body.h), its lowering and the event store's row layout compiled for the host
(test infrastructure only; see tests/native/select_host.cpp), and what the selector tests share: the
reference rows (siddhi_amd/selector.py project, encoded), the comparison, and the hand-written and
seeded apps."""
import ctypes
import os
import random
import subprocess

import numpy as np

from siddhi_amd.events import EventLog, encode_rows, encode_value
from siddhi_amd.ir import T_DOUBLE, T_FLOAT
from siddhi_amd.selector import evaluate, project

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "select_host.cpp")
SO = os.path.join(HERE, "native", "libselect_host.so")
CSRC = os.path.join(os.path.dirname(HERE), "siddhi_amd", "csrc")
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(CSRC, h) for h in ("select_body.h", "select_lower.h", "kgen.h", "gen_lower.h")]
        if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
            subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-Wall",
                                   "-Wno-maybe-uninitialized", "-ffp-contract=off", "-fno-fast-math", "-shared",
                                   "-o", SO, SRC])
        L = ctypes.CDLL(SO)
        P, I64, VP, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int
        L.slh_create.argtypes = [VP, ctypes.c_size_t]
        L.slh_create.restype = P
        L.slh_destroy.argtypes = [P]
        for f in ("slh_width", "slh_shapes", "slh_row_words"):
            getattr(L, f).argtypes = [P]
        for f in ("slh_shape_of", "slh_n_out"):
            getattr(L, f).argtypes = [P, I]
        for f in ("slh_out_type", "slh_out_direct"):
            getattr(L, f).argtypes = [P, I, I]
        L.slh_store_append.argtypes = [VP, I64, I, I64, I64, VP, VP, VP, I]
        L.slh_project.argtypes = [P, I64, VP, VP, VP, VP, I64, I, I64, VP, VP]
        L.slh_project_pairs.argtypes = [P, I64, VP, I, I64, VP, I64, I, I64, VP, VP]
        _lib = L
    return _lib


class HostSelector:
    """The select lists of a program blob, lowered for the host body."""

    def __init__(self, blob: bytes):
        self.lib = lib()
        self._blob = ctypes.create_string_buffer(blob, len(blob))
        self.h = self.lib.slh_create(self._blob, len(blob))
        if not self.h:
            raise RuntimeError("selector lowering failed")
        self.width = self.lib.slh_width(self.h)
        self.W = self.lib.slh_row_words(self.h)

    def store(self, log: EventLog, cap: int = 0):
        """(rows, cap): the row-major store holding the log's last `cap` events (default: all)."""
        n = len(log)
        if cap <= 0:
            cap = 1
            while cap < max(n, 1):
                cap *= 2
        rows = np.zeros(cap * self.W, np.int64)
        for k in range(n):
            ts = np.array([log.ts[k]], np.int64)
            vals = np.ascontiguousarray(log.vals[k], dtype=np.int64)
            nulls = np.ascontiguousarray(log.nulls[k], dtype=np.uint8)
            self.lib.slh_store_append(rows.ctypes.data, cap, self.W, k, 1, ts.ctypes.data, vals.ctypes.data,
                                      nulls.ctypes.data, len(vals))
        return rows, cap

    def project(self, matches, log: EventLog, cap: int = 0):
        """matches: harness tuples (query, key, ts, slots) -> (cells[width, n], nulls[n], error bits)."""
        rows, cap = self.store(log, cap)
        n = len(matches)
        query = np.array([m[0] for m in matches], np.int64)
        off = np.zeros(n + 1, np.int64)
        words = []
        for i, m in enumerate(matches):
            for s in m[3]:
                words.append(len(s))
                words.extend(s)
            off[i + 1] = len(words)
        words = np.array(words + [0], np.int64)
        cells = np.zeros((max(self.width, 1), max(n, 1)), np.int64)
        nulls = np.zeros(max(n, 1), np.uint64)
        err = self.lib.slh_project(self.h, n, query.ctypes.data, off.ctypes.data, words.ctypes.data, rows.ctypes.data,
                                   cap, self.W, max(0, len(log) - cap), cells.ctypes.data, nulls.ctypes.data)
        return cells[:self.width, :n], nulls[:n], err

    def project_pairs(self, crow, seq_ref, log: EventLog):
        """K_ratchet compact rows [n, cw] -> (cells, nulls, error bits)."""
        rows, cap = self.store(log)
        crow = np.ascontiguousarray(crow, dtype=np.int32)
        n, cw = crow.shape
        cells = np.zeros((max(self.width, 1), max(n, 1)), np.int64)
        nulls = np.zeros(max(n, 1), np.uint64)
        err = self.lib.slh_project_pairs(self.h, n, crow.ctypes.data, cw, seq_ref, rows.ctypes.data, cap, self.W, 0,
                                         cells.ctypes.data, nulls.ctypes.data)
        return cells[:self.width, :n], nulls[:n], err

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.slh_destroy(self.h)
            self.h = None


def reference_cells(app, matches, width):
    """encode_value(selector.project(...)) of every match: (cells[width, n], nulls[n]) -- bit c of a
    null mask is set for a null cell and for every c at or past the query's output count."""
    n = len(matches)
    cells = np.zeros((width, n), np.int64)
    nulls = np.zeros(n, np.uint64)
    for i, m in enumerate(matches):
        q = app.ir.queries[m[0]]
        row = project(q, m[3], app.log, None, app.dictionary, app.ir.strings)
        bits = ((1 << 64) - 1) & ~((1 << len(row)) - 1)
        for c, (v, o) in enumerate(zip(row, q.outputs)):
            raw, isnull = encode_value(v, o.type, app.dictionary)
            if isnull:
                bits |= 1 << c
            else:
                cells[c, i] = np.array([raw & ((1 << 64) - 1)], np.uint64).view(np.int64)[0]
        nulls[i] = bits
    return cells, nulls


def _is_nan(raw, t):
    if t == T_FLOAT:
        return (raw & 0x7F800000) == 0x7F800000 and (raw & 0x007FFFFF) != 0
    return (raw & 0x7FF0000000000000) == 0x7FF0000000000000 and (raw & 0x000FFFFFFFFFFFFF) != 0


def assert_cells_equal(app, matches, cells, nulls, want_cells, want_nulls):
    """Bit for bit on cells and null masks; any NaN equals any NaN of the same type."""
    assert cells.shape == want_cells.shape and len(nulls) == len(want_nulls)
    assert np.array_equal(np.asarray(nulls, np.uint64), want_nulls), "null masks differ"
    if np.array_equal(cells, want_cells):
        return
    for c, i in zip(*np.nonzero(cells != want_cells)):
        t = app.ir.queries[matches[i][0]].outputs[c].type
        a, b = int(cells[c, i]) & ((1 << 64) - 1), int(want_cells[c, i]) & ((1 << 64) - 1)
        assert t in (T_FLOAT, T_DOUBLE) and _is_nan(a, t) and _is_nan(b, t), \
            f"row {i} cell {c}: {a:#x} != {b:#x} (type {t})"


def callback_rows(fx_kind_query: bool, callback: str, app, matches, rows):
    """The decoded rows a fixture's callback sees: a query's own, or the rows arriving on a stream
    (through the inner-stream chains, which stay on the host: selector.stream_rows)."""
    if fx_kind_query:
        qi = app.ir.query_index(callback)
        return [r for m, r in zip(matches, rows) if m[0] == qi]
    by_input = {}
    for c in getattr(app.ir, "chains", []):
        by_input.setdefault(c.input, []).append(c)
    out = []

    def deliver(row, types, target):
        if target == callback:
            out.append(row)
        for c in by_input.get(target, []):
            vals, nulls = encode_rows([row], types, app.dictionary)
            one = EventLog()
            one.append(-1, [0], vals, nulls)
            if not all(evaluate(f, [[0]], one, None, app.dictionary, app.ir.strings) is True for f in c.filters):
                continue
            if c.outputs:
                deliver([evaluate(o.code, [[0]], one, None, app.dictionary, app.ir.strings) for o in c.outputs],
                        [o.type for o in c.outputs], c.output_stream)
            else:
                deliver(list(row), types, c.output_stream)

    for m, r in zip(matches, rows):
        q = app.ir.queries[m[0]]
        deliver(r, [o.type for o in q.outputs], q.output_stream)
    return out


# ---- hand-written apps: (name, app, [(stream, row, ts)]) ----
_NUM = "define stream S (i int, l long, f float, d double, b bool, s string); "
_NUM_EVENTS = [
    ("S", [7, 1 << 40, np.float32(2.5), 0.1, True, "a"], 1000),
    ("S", [0, 0, np.float32(0.0), 0.0, False, "b"], 1001),
    ("S", [-(2 ** 31), -(2 ** 63), np.float32(-0.0), -0.0, True, "a"], 1002),
    ("S", [-1, -1, np.float32("nan"), float("nan"), None, None], 1003),
    ("S", [None, None, None, None, False, "c"], 1004),
    ("S", [2 ** 31 - 1, 2 ** 63 - 1, np.float32(3.4e38), 1.7e308, True, ""], 1005),
    ("S", [3, -5, np.float32(-7.25), 1e-300, None, "a"], 1006),
]


def _arith_app():
    outs = []
    names = "ilfd"
    k = 0
    for x in names:
        for y in names:
            for op in "+-*/%":
                outs.append(f"e1.{x} {op} e2.{y} as o{k}")
                k += 1
    # 80 outputs: four queries of 20
    qs = []
    for j in range(4):
        qs.append(f"@info(name = 'q{j}') from every e1=S -> e2=S select " + ", ".join(outs[20 * j:20 * j + 20]) +
                  f" insert into O{j};")
    return _NUM + " ".join(qs)


HAND_APPS = [
    ("arith_pairs", _arith_app(), _NUM_EVENTS),
    ("null_ops", _NUM + "@info(name = 'q') from every e1=S -> e2=S select e1.i + e2.i as a, e1.i is null as n1, "
     "e2.s is null as n2, e1.i > e2.i as c1, e1.f == e2.d as c2, e1.l != e2.f as c3, e1.b == e2.b as c4, "
     "e1.s == e2.s as c5, not (e1.d < e2.d) as c6, e1.i is null or e2.b as c7, e1.b and e2.b as c8, "
     "(e1.l / e2.i) is null as n3 insert into O;", _NUM_EVENTS),
    ("strings", _NUM + "@info(name = 'q') from every e1=S[s == 'a'] -> e2=S select 'const' as k, e1.s as s1, e2.s as s2, "
     "e2.s == 'a' as eq, 1 as one, 2.5f as fl, 10l as lg, 1.25 as db, true as t insert into O;", _NUM_EVENTS),
    ("count_chain", "define stream A (v int); define stream B (v int); @info(name = 'q') from every e0=B -> e1=A<2:4> -> e2=B "
     "select e1[0].v as v0, e1[1].v as v1, e1[2].v as v2, e1[3].v as v3, e1[last].v as vl, e1[last - 1].v as vl1, "
     "e1[last - 2].v as vl2, e1[last - 3].v as vl3, e2.v as w, e1[2] is null as n2, e1[0].v + e1[last].v as sm "
     "insert into O;",
     [("B", [0], 0), ("A", [1], 1), ("A", [2], 2), ("B", [10], 3), ("A", [3], 4), ("A", [4], 5), ("A", [5], 6), ("B", [11], 7),
      ("A", [6], 8), ("A", [7], 9), ("A", [8], 10), ("A", [9], 11), ("B", [12], 12)]),
    ("logical_or", "define stream A (v int); define stream B (v int); define stream C (v int); @info(name = 'q') "
     "from every e1=A -> e2=B or e3=C select e1.v as a, e2.v as b, e3.v as c, e2 is null as nb, e3 is null as nc, "
     "e2.v + e3.v as s insert into O;",
     [("A", [1], 1), ("B", [2], 2), ("A", [3], 3), ("C", [4], 4), ("A", [5], 5), ("A", [6], 6), ("C", [7], 7)]),
    # a right-nested sum needs 8 stack entries: past the register stack, the indexed one runs it
    ("deep", _NUM + "@info(name = 'q') from every e1=S -> e2=S select e1.i + (e2.i + (e1.l + (e2.l + (e1.f + (e2.f + "
     "(e1.d + e2.d)))))) as deep, e1.i as plain insert into O;", _NUM_EVENTS),
    ("and_not","define stream A (v int); define stream B (v int); define stream C (v int); @info(name = 'q') "
     "from every e1=A -> e2=B and not C select e1.v as a, e2.v as b insert into O;",
     [("A", [1], 1), ("B", [2], 2), ("A", [3], 3), ("C", [4], 4), ("B", [5], 5), ("A", [6], 6), ("B", [7], 7)]),
]

# ---- seeded select lists over one fixed three-state pattern ----
SEEDED_DEFS = "define stream S (i int, l long, f float, d double, b bool, s string); "
SEEDED_FROM = "from every e1=S[not (b == false)] -> e2=S[not (i <= -100)] -> e3=S "  # (null passes both)
_ATTR_T = {"i": "int", "l": "long", "f": "float", "d": "double", "b": "bool", "s": "string"}
_RANK = {"int": 0, "long": 1, "float": 2, "double": 3}


def _gen_expr(rng, depth):
    """(text, type) of a random expression of at most `depth` levels."""
    if depth <= 1 or rng.random() < 0.25:
        if rng.random() < 0.7:
            a = rng.choice("ilfdbs")
            return f"e{rng.randint(1, 3)}.{a}", _ATTR_T[a]
        t = rng.choice(["int", "long", "float", "double", "bool", "string"])
        lit = {"int": lambda: str(rng.randint(-5, 5)), "long": lambda: f"{rng.randint(-3, 3)}l",
               "float": lambda: f"{rng.choice([0.0, 1.5, -2.25])}f", "double": lambda: str(rng.choice([0.0, 0.5, -3.75])),
               "bool": lambda: rng.choice(["true", "false"]), "string": lambda: rng.choice(["'a'", "'zz'"])}[t]()
        return lit, t
    kind = rng.choice(["arith", "arith", "cmp", "logic", "isnull", "not"])
    if kind == "arith":
        for _ in range(20):
            (l, lt), (r, rt) = _gen_expr(rng, depth - 1), _gen_expr(rng, depth - 1)
            if lt in _RANK and rt in _RANK:
                t = max(lt, rt, key=lambda x: _RANK[x])
                return f"({l} {rng.choice('+-*/%')} {r})", t
        return "e1.i + e2.l", "long"
    if kind == "cmp":
        for _ in range(20):
            (l, lt), (r, rt) = _gen_expr(rng, depth - 1), _gen_expr(rng, depth - 1)
            if lt in _RANK and rt in _RANK:
                return f"({l} {rng.choice(['<', '<=', '>', '>=', '==', '!='])} {r})", "bool"
            if lt == rt and lt in ("bool", "string"):
                return f"({l} {rng.choice(['==', '!='])} {r})", "bool"
        return "e1.i < e2.d", "bool"
    if kind == "isnull":
        e, _ = _gen_expr(rng, depth - 1)
        return f"(({e}) is null)", "bool"
    for _ in range(20):
        (l, lt), (r, rt) = _gen_expr(rng, depth - 1), _gen_expr(rng, depth - 1)
        if lt == "bool" and (kind == "not" or rt == "bool"):
            return (f"(not {l})", "bool") if kind == "not" else (f"({l} {rng.choice(['and', 'or'])} {r})", "bool")
    return "(e1.b and e3.b)", "bool"


def seeded_apps(count=30, seed=20250):
    rng = random.Random(seed)
    apps = []
    for k in range(count):
        outs = [f"{_gen_expr(rng, rng.randint(1, 4))[0]} as o{j}" for j in range(rng.randint(1, 6))]
        apps.append((f"seed{k}", SEEDED_DEFS + f"@info(name = 'q') {SEEDED_FROM}select {', '.join(outs)} insert into O;"))
    return apps


def seeded_events(n=24, seed=77):
    rng = random.Random(seed)
    evs = []
    for k in range(n):
        def maybe(v):
            return None if rng.random() < 0.2 else v
        evs.append(("S", [maybe(rng.randint(-4, 4)), maybe(rng.choice([0, 1, -7, 1 << 35])),
                          maybe(np.float32(rng.choice([0.0, -0.0, 1.5, float("nan"), -2.25]))),
                          maybe(rng.choice([0.0, 2.0, float("nan"), -0.5, 1e200])),
                          maybe(rng.random() < 0.7), maybe(rng.choice(["a", "zz", "q"]))], 1000 + k))
    return evs
