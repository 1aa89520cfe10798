"""What the built-in function tests share (tests/test_functions.py on the CPU, tests/test_gpu_functions.py
on the device): the reference's function fixtures, the quirk pins, the seeded expression generator
and the oracle twins. No oracle sees a function: the yardstick for a function-bearing program is
siddhi_amd/selector.py (evaluate / project), restated from the reference's Java."""
import json
import os
import random
import re

import numpy as np

from harness import App, parse_literal
from siddhi_amd.events import encode_value

HERE = os.path.dirname(os.path.abspath(__file__))
KAT = json.load(open(os.path.join(HERE, "golden", "reference_function_kat.json")))
FIXTURES = KAT["fixtures"]
RUNNABLE = [f for f in FIXTURES if not f.get("expect_creation_error")]
SUITES = ("IfThenElseFunctionTestCase", "ConvertFunctionTestCase", "CastFunctionExecutorTestCase",
          "InstanceOfFunctionTestCase", "MaximumFunctionExtensionTestCase", "MinimumFunctionExtensionTestCase",
          "FunctionTestCase")
TS0 = 1_500_000_000_000


# ---- reference fixtures: `from S[f] select L` as the one-state pattern `from every e1=S[f] select L` ----
def _qualify(text, attrs):
    """attribute names -> e1.<name> (outside string literals), the way test_filter_kat.pattern_app does
    for `is null`: in a pattern's select list an unqualified name needs no alias, but before `is null`
    it would resolve as a stream reference."""
    parts = re.split(r"('[^']*')", text)
    rx = re.compile(r"(?<![\w.])(" + "|".join(sorted(attrs, key=len, reverse=True)) + r")\b(?!\s*\()")
    return "".join(p if p.startswith("'") else rx.sub(r"e1.\1", p) for p in parts)


def fixture_app(fx):
    attrs = [a.split()[0] for a in fx["define"].split("(", 1)[1].rsplit(")", 1)[0].split(",")]
    outs = []
    for k, item in enumerate(_split_select(fx["select"])):
        m = re.match(r"(.*?)\s+as\s+(\w+)\s*$", item, re.S)
        expr, name = (m.group(1), m.group(2)) if m else (item, item.strip())
        outs.append(f"{_qualify(expr, attrs)} as {name}")
    flt = f"[{_qualify(fx['filter'], attrs)}]" if fx.get("filter") else ""
    return (f"{fx['define']} @info(name = 'query1') from every e1={fx['stream']}{flt} "
            f"select {', '.join(outs)} insert into OutputStream;")


def _split_select(text):
    out, depth, cur = [], 0, ""
    for ch in text:
        depth += {"(": 1, ")": -1}.get(ch, 0)
        if ch == "," and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += ch
    return [x.strip() for x in out + [cur]]


def run_fixture(fx, engine_factory=None):
    app = App(fixture_app(fx), engine_factory)
    for i, ev in enumerate(fx["events"]):
        app.send(fx["stream"], [[parse_literal(t) for t in ev]], [TS0 + i])
    return app


def cell_matches(want, got):
    """An expected cell of a fixture row (a literal token, 'null' or {'type': t}) against a value."""
    if isinstance(want, dict):
        ok = {"int": lambda v: isinstance(v, int) and not isinstance(v, bool),
              "long": lambda v: isinstance(v, int) and not isinstance(v, bool),
              "float": lambda v: isinstance(v, np.float32), "double": lambda v: isinstance(v, float),
              "bool": lambda v: isinstance(v, (bool, np.bool_)), "string": lambda v: isinstance(v, str)}
        return got is not None and ok[want["type"]](got)
    from harness import values_equal
    return values_equal(want, got)


def check_fixture_rows(fx, rows):
    assert len(rows) == fx["expected_count"], f"{len(rows)} rows, the reference test expects {fx['expected_count']}"
    for k, (want, got) in enumerate(zip(fx["expected_rows"], rows)):
        for c, w in want.items():
            assert cell_matches(w, got[int(c)]), f"row {k} column {c}: {got[int(c)]!r}, the reference asserts {w}"


# ---- quirk pins: (name, define, select expression, event row, the literal the reference computes) ----
_T = "define stream S (i int, j int, l long, m long, f float, g float, d double, e double, b bool, s string);"
I32MAX, I32MIN, I64MAX, I64MIN = 2 ** 31 - 1, -2 ** 31, 2 ** 63 - 1, -2 ** 63


def _row(**kw):
    names = ["i", "j", "l", "m", "f", "g", "d", "e", "b", "s"]
    return [kw.get(n) for n in names]


PINS = [
    # maximum folds from Double.MIN_VALUE, the smallest POSITIVE double: negatives never win
    ("max_negative_ints_is_0", "maximum(e1.i, e1.j)", _row(i=-3, j=-5), 0),
    ("max_negative_const_ints_is_0", "maximum(-3, -5)", _row(), 0),
    ("max_all_null_doubles_is_MIN_VALUE", "maximum(e1.d, e1.e)", _row(), 4.9e-324),
    ("max_all_null_ints_is_0", "maximum(e1.i, e1.j)", _row(), 0),
    ("max_all_null_floats_is_0f", "maximum(e1.f, e1.g)", _row(), np.float32(0.0)),
    ("max_single_null_passes_through", "maximum(e1.i)", _row(), None),
    ("max_single_negative_passes_through", "maximum(e1.i)", _row(i=-7), -7),
    ("min_single_null_passes_through", "minimum(e1.d)", _row(), None),
    ("max_nan_never_wins", "maximum(e1.d, e1.e)", _row(d=float("nan"), e=2.5), 2.5),
    ("max_null_never_wins", "maximum(e1.d, e1.e)", _row(e=-1.0), 4.9e-324),
    # minimum folds from Double.MAX_VALUE and casts back with (int) / (long) / (float)
    ("min_all_null_ints_is_INT_MAX", "minimum(e1.i, e1.j)", _row(), I32MAX),
    ("min_all_null_longs_is_LONG_MAX", "minimum(e1.l, e1.m)", _row(), I64MAX),
    ("min_all_null_floats_is_Infinity", "minimum(e1.f, e1.g)", _row(), np.float32("inf")),
    ("min_all_null_doubles_is_MAX_VALUE", "minimum(e1.d, e1.e)", _row(), 1.7976931348623157e308),
    ("min_nan_never_wins", "minimum(e1.d, e1.e)", _row(d=float("nan"), e=2.5), 2.5),
    # longs fold in double: above 2^53 they lose bits, and (long) of a double saturates
    ("max_long_above_2_53_loses_bits", "maximum(e1.l, e1.m)", _row(l=2 ** 53 + 1, m=1), 2 ** 53),
    ("max_long_MAX_saturates", "maximum(e1.l, e1.m)", _row(l=I64MAX, m=1), I64MAX),
    ("min_long_MIN_saturates", "minimum(e1.l, e1.m)", _row(l=I64MIN, m=1), I64MIN),
    ("max_long_near_MAX_rounds_up_and_saturates", "maximum(e1.l, e1.m)", _row(l=I64MAX - 1, m=0), I64MAX),
    # convert: Java's narrowing
    ("convert_1e20f_int_saturates", "convert(1e20f, 'int')", _row(), I32MAX),
    ("convert_minus_1e20f_int_saturates", "convert(e1.f, 'int')", _row(f=np.float32(-1e20)), I32MIN),
    ("convert_nan_long_is_0", "convert(e1.d, 'long')", _row(d=float("nan")), 0),
    ("convert_nan_float_int_is_0", "convert(e1.f, 'int')", _row(f=np.float32("nan")), 0),
    ("convert_inf_long_saturates", "convert(e1.d, 'long')", _row(d=float("inf")), I64MAX),
    ("convert_double_int_truncates", "convert(e1.d, 'int')", _row(d=-45.9), -45),
    ("convert_long_int_wraps", "convert(e1.l, 'int')", _row(l=2 ** 32 + 5), 5),
    ("convert_long_float_rounds_to_nearest", "convert(e1.l, 'float')", _row(l=2 ** 24 + 1), np.float32(16777216.0)),
    ("convert_long_float_rounds_once", "convert(e1.l, 'float')", _row(l=2 ** 54 + 2 ** 30 + 1),
     np.float32(1.8014400656965632e16)),
    ("convert_double_float_overflows_to_inf", "convert(e1.d, 'float')", _row(d=1e300), np.float32("inf")),
    ("convert_int_bool_is_eq_1", "convert(e1.i, 'bool')", _row(i=2), False),
    ("convert_double_one_bool", "convert(e1.d, 'bool')", _row(d=1.0), True),
    ("convert_bool_long", "convert(e1.b, 'long')", _row(b=True), 1),
    ("convert_bool_float", "convert(e1.b, 'FLOAT')", _row(b=False), np.float32(0.0)),
    ("convert_null_is_null", "convert(e1.i, 'double')", _row(), None),
    ("cast_int_long_widens", "cast(e1.i, 'long')", _row(i=-9), -9),
    # ifThenElse / coalesce / default / instanceOf
    ("ifThenElse_null_cond_takes_else", "ifThenElse(e1.b, 1, 2)", _row(), 2),
    ("ifThenElse_null_compare_takes_else", "ifThenElse(e1.i > 0, 'a', 'z')", _row(), "z"),
    ("ifThenElse_true_with_null_then", "ifThenElse(e1.b, e1.i, 5)", _row(b=True), None),
    ("coalesce_first_non_null", "coalesce(e1.i, e1.j, 4)", _row(j=8), 8),
    ("coalesce_all_null", "coalesce(e1.s, e1.s)", _row(), None),
    ("default_of_null", "default(e1.f, 2.5f)", _row(), np.float32(2.5)),
    ("instanceOfInteger_of_null", "instanceOfInteger(e1.i)", _row(), False),
    ("instanceOfInteger_of_int", "instanceOfInteger(e1.i)", _row(i=0), True),
    ("instanceOfLong_of_int", "instanceOfLong(e1.i)", _row(i=0), False),
    ("instanceOfString_of_string", "instanceOfString(e1.s)", _row(s="x"), True),
    ("function_is_null", "coalesce(e1.i, e1.j) is null", _row(), True),
]


def pin_app(expr):
    return f"{_T} @info(name = 'q') from every e1=S select {expr} as o insert into O;"


def same_value(a, b):
    """Bit-level equality of two Python values of one type (any NaN equals any NaN)."""
    if a is None or b is None:
        return a is None and b is None
    if type(a) is not type(b) and not (isinstance(a, (bool, np.bool_)) and isinstance(b, (bool, np.bool_))):
        return False
    if isinstance(a, (float, np.float32)) and a != a:
        return b != b
    if isinstance(a, (float, np.float32)):
        return a == b and np.signbit(a) == np.signbit(b)
    return a == b


# ---- refusals: (app text, what the message must name) ----
_R = "define stream S (i int, l long, f float, d double, b bool, s string); @info(name = 'q') from every e1=S"
REFUSALS = [
    (f"{_R}[eventTimestamp() > 5L] select e1.i as o insert into O;", "eventTimestamp"),
    (f"{_R} select currentTimeMillis() as o insert into O;", "currentTimeMillis"),
    (f"{_R} select UUID() as o insert into O;", "UUID"),
    (f"{_R} select createSet(e1.i) as o insert into O;", "createSet"),
    (f"{_R} select sizeOfSet(e1.i) as o insert into O;", "sizeOfSet"),
    (f"{_R} select myScript(e1.i) as o insert into O;", "myScript"),
    (f"{_R} select str:concat(e1.s, 'x') as o insert into O;", "str:concat"),
    (f"{_R} select convert(e1.i, 'string') as o insert into O;", "convert"),
    (f"{_R} select convert(e1.s, 'int') as o insert into O;", "convert"),
    (f"{_R} select convert(e1.i, 'decimal') as o insert into O;", "decimal"),
    (f"{_R} select convert(e1.i, e1.s) as o insert into O;", "convert"),
    (f"{_R} select cast(e1.d, 'int') as o insert into O;", "ClassCastException"),
    (f"{_R} select ifThenElse(e1.b, 1, 2L) as o insert into O;", "ifThenElse"),
    (f"{_R} select ifThenElse(e1.i, 1, 2) as o insert into O;", "ifThenElse"),
    (f"{_R} select ifThenElse(e1.b, 1) as o insert into O;", "ifThenElse"),
    (f"{_R} select coalesce() as o insert into O;", "coalesce"),
    (f"{_R} select coalesce(e1.i, e1.l) as o insert into O;", "coalesce"),
    (f"{_R} select default(e1.i, e1.i) as o insert into O;", "default"),
    (f"{_R} select default(e1.i, 2L) as o insert into O;", "default"),
    (f"{_R} select maximum(e1.i, e1.l) as o insert into O;", "maximum"),
    (f"{_R} select minimum(e1.s) as o insert into O;", "minimum"),
    (f"{_R} select instanceOfLong(e1.l, e1.i) as o insert into O;", "instanceOfLong"),
    (f"{_R} select eventTimestamp(e1.i) as o insert into O;", "eventTimestamp"),
]


def too_deep_app():
    """13 entries: a right-nested ifThenElse keeps every enclosing condition and then-branch pending."""
    e = "e1.i"
    for k in range(6):
        e = f"ifThenElse(e1.b, {k}, {e})"
    return f"{_R}[{e} > 0] select e1.i as o insert into O;"


# ---- seeded expressions over one stream: every function, every legal type combination ----
GEN_DEF = "define stream S (i int, j int, l long, m long, f float, g float, d double, e double, b bool, c bool, s string, t string);"
_COLS = {"int": "ij", "long": "lm", "float": "fg", "double": "de", "bool": "bc", "string": "st"}
_NUMT = ("int", "long", "float", "double")
_RANK = {"int": 0, "long": 1, "float": 2, "double": 3}
_LIT = {"int": ["0", "1", "-1", "7", "2147483647", "-5"], "long": ["0L", "1L", "-3L", "9007199254740993L"],
        "float": ["0.0f", "1.0f", "-2.25f", "1e20f"], "double": ["0.0", "1.0", "-3.75", "1e300", "4.9e-324"],
        "bool": ["true", "false"], "string": ["'a'", "'zz'"]}


_INSTANCE = {"Integer": "int", "Long": "long", "Float": "float", "Double": "double", "Boolean": "bool",
             "String": "string"}


def gen_leaf(rng, t, ref="e1", lit=0.3):
    if rng.random() < lit:
        return rng.choice(_LIT[t])
    return f"{ref}.{rng.choice(_COLS[t])}"


def gen_expr(rng, t, depth, ref="e1"):
    """A random expression of static type t, at most `depth` levels of functions / operators."""
    if depth <= 0:
        return gen_leaf(rng, t, ref)
    sub = lambda ty: gen_expr(rng, ty, depth - 1, ref)  # noqa: E731
    kinds = ["ifThenElse", "coalesce", "default", "leaf"]
    if t in _NUMT:
        kinds += ["maximum", "minimum", "convert", "convert", "arith", "max1"]
        if t == "long":
            kinds += ["cast"]
    if t == "bool":
        kinds += ["convert", "cmp", "cmp", "instanceOf", "isnull", "not", "logic"]
    k = rng.choice(kinds)
    if k == "leaf":
        return gen_leaf(rng, t, ref)
    if k == "ifThenElse":
        return f"ifThenElse({sub('bool')}, {sub(t)}, {sub(t)})"
    if k == "coalesce":
        return "coalesce(" + ", ".join(sub(t) for _ in range(rng.randint(1, 3))) + ")"
    if k == "default":
        return f"default({sub(t)}, {rng.choice(_LIT[t])})"
    if k in ("maximum", "minimum"):
        return f"{k}(" + ", ".join(sub(t) for _ in range(rng.randint(2, 3))) + ")"
    if k == "max1":
        return f"{rng.choice(['maximum', 'minimum'])}({sub(t)})"
    if k == "convert":
        src = rng.choice([x for x in _NUMT + ("bool",)])
        return f"convert({sub(src)}, '{t}')"
    if k == "cast":
        return f"cast({sub('int')}, 'long')"
    if k == "arith":
        other = rng.choice([x for x in _NUMT if _RANK[x] <= _RANK[t]])
        a, b = (sub(t), sub(other)) if rng.random() < 0.5 else (sub(other), sub(t))
        return f"({a} {rng.choice('+-*/%')} {b})"
    if k == "cmp":
        if rng.random() < 0.25:
            ty = rng.choice(["bool", "string"])
            return f"({sub(ty)} {rng.choice(['==', '!='])} {sub(ty)})"
        return f"({sub(rng.choice(_NUMT))} {rng.choice(['<', '<=', '>', '>=', '==', '!='])} {sub(rng.choice(_NUMT))})"
    if k == "instanceOf":
        ty = rng.choice(list(_COLS))
        fn = rng.choice(["Integer", "Long", "Float", "Double", "Boolean", "String"])
        return f"instanceOf{fn}({sub(ty)})"
    if k == "isnull":
        return f"(({sub(rng.choice(list(_COLS)))}) is null)"
    if k == "not":
        return f"(not {sub('bool')})"
    return f"({sub('bool')} {rng.choice(['and', 'or'])} {sub('bool')})"


_SPECIAL = {
    "int": [0, 1, -1, I32MAX, I32MIN, 7],
    "long": [0, 1, -1, I64MAX, I64MIN, 2 ** 53 + 1, 2 ** 53 - 1, -(2 ** 53) - 1, 2 ** 31, -(2 ** 31), I64MAX - 1],
    "float": [0.0, -0.0, 1.0, -1.0, float("nan"), float("inf"), float("-inf"), 2.0 ** 31, -(2.0 ** 31), 2.0 ** 63,
              -(2.0 ** 63), 3.4028235e38, 1e20, 1.4e-45],
    "double": [0.0, -0.0, 1.0, -1.0, float("nan"), float("inf"), float("-inf"), 2.0 ** 31, -(2.0 ** 31) - 1.0,
               2.0 ** 63, -(2.0 ** 63), 2.0 ** 53 + 2.0, 4.9e-324, 1.7976931348623157e308, 2147483647.5, 1e20],
}


def gen_value(rng, t):
    if rng.random() < 0.15:
        return None
    if t == "bool":
        return rng.random() < 0.5
    if t == "string":
        return rng.choice(["a", "zz", "q"])
    if rng.random() < 0.5:
        v = rng.choice(_SPECIAL[t])
    elif t == "int":
        v = rng.randint(-20, 20)
    elif t == "long":
        v = rng.randint(-2 ** 40, 2 ** 40)
    else:
        v = rng.uniform(-100.0, 100.0)
    return np.float32(v) if t == "float" else v


def gen_events(n, seed):
    rng = random.Random(seed)
    order = [("int", 2), ("long", 2), ("float", 2), ("double", 2), ("bool", 2), ("string", 2)]
    return [[gen_value(rng, t) for t, k in order for _ in range(k)] for _ in range(n)]


def gen_cases(seed=4711, per_type=6):
    """(name, output type, expression): per function and per legal type at least one expression with
    that function at the root, nested two deep, then mixed ones."""
    rng = random.Random(seed)
    out = []
    for t in ("int", "long", "float", "double", "bool", "string"):
        roots = ["ifThenElse", "coalesce", "default"] + (["maximum", "minimum", "max1", "convert"] if t in _NUMT else [])
        roots += ["convert", "instanceOf"] if t == "bool" else []
        roots += ["cast"] if t == "long" else []
        for r in roots:
            for _ in range(2000):
                e = gen_expr(rng, t, 3)
                head = {"max1": ("maximum(", "minimum(")}.get(r, (r,))
                if e.startswith(head) and (r not in ("maximum", "minimum") or "," in e) and _plans(e):
                    break
            else:
                raise AssertionError(f"no {r} expression of type {t}")
            out.append((f"{t}_{r}", t, e))
        if t == "bool":   # every instanceOf*, over its own type (null decides) and over another (always false)
            for fn, ty in _INSTANCE.items():
                other = rng.choice([x for x in _COLS if x != ty])
                out.append((f"bool_instanceOf{fn}", t, f"instanceOf{fn}({gen_expr(rng, ty, 2)})"))
                out.append((f"bool_instanceOf{fn}_of_{other}", t, f"instanceOf{fn}({gen_expr(rng, other, 1)})"))
        k = 0
        while k < per_type:
            e = gen_expr(rng, t, 3)
            if _plans(e):   # (a rare one needs more than the engine's evaluation stack: refused at create)
                out.append((f"{t}_mixed{k}", t, e))
                k += 1
    return out


def _plans(expr):
    from siddhi_amd import ql
    from siddhi_amd.planner import plan
    try:
        plan(ql.parse(gen_app([expr])))
        return True
    except ql.SiddhiAppCreationException:
        return False


def as_filter(t, expr):
    """A BOOL expression over `expr` of type t."""
    return {"bool": expr, "string": f"({expr} == 'a')"}.get(t, f"({expr} > 0)")


def gen_app(exprs, flt=None, name="q"):
    outs = ", ".join(f"{e} as o{k}" for k, e in enumerate(exprs))
    return f"{GEN_DEF} @info(name = '{name}') from every e1=S{'[' + flt + ']' if flt else ''} select {outs} insert into O;"


def encode_row(app, q, row):
    """(cells, null bits) of one projected row, the raw encoding poll_rows returns."""
    cells, bits = [], 0
    for c, (v, o) in enumerate(zip(row, q.outputs)):
        raw, isnull = encode_value(v, o.type, app.dictionary)
        bits |= (1 << c) if isnull else 0
        cells.append(0 if isnull else int(np.array([raw & ((1 << 64) - 1)], np.uint64).view(np.int64)[0]))
    return cells, bits


# ---- twins: a function query and a function-free query that are equal on every input ----
TWIN_STOCK = "define stream S (symbol string, price float, volume int); "
TWIN_TXN = "define stream S (k int, amount double, v int); "


def twin_queries(kind, n):
    """(function app, twin app) of n queries that differ in a constant."""
    fq, tq = [], []
    for p in range(n):
        if kind == "T1":
            head = f"@info(name = 'q{p}') from every e1=S[price > {60 + p % 35}.0f] -> e2=S["
            tail = "] within 1 sec select e1.price as a, e2.price as b insert into O;"
            fq.append(head + "ifThenElse(price > e1.price, true, false)" + tail)
            tq.append(head + "price > e1.price" + tail)
        elif kind == "T2":
            head = f"@info(name = 'q{p}') from every e1=S[price > {60 + p % 35}.0f] -> e2=S["
            tail = "] within 1 sec select e1.price as a, e2.price as b insert into O;"
            fq.append(head + "coalesce(price, e1.price) > e1.price" + tail)
            tq.append(head + "price > e1.price" + tail)
        elif kind == "T3":
            head = f"@info(name = 'q{p}') from every e1=S[amount > {100 + p % 40}.0], e2=S["
            tail = "] select e1.amount as a, e2.amount as b insert into O;"
            fq.append(head + "maximum(amount, e1.amount) == amount" + tail)
            tq.append(head + "amount >= e1.amount" + tail)
        elif kind == "T4":
            head = f"@info(name = 'q{p}') from every e1=S[v > {10 + p % 30}]<2:3> -> e2=S["
            tail = "] select e1[0].v as a, e2.v as b insert into O;"
            fq.append(head + "convert(v, 'double') > 50.0" + tail)
            tq.append(head + "v > 50.0" + tail)
        else:   # T5: T4's filters in C3's count form, the shape K_part's compact tables hold
            head = (f"@info(name = 'q{p}') from every e1=S[v > {60 + p % 30}] -> e2=S[v > 10]<2:3> -> e3=S[")
            tail = "] within 10 sec select e1.v as a, e2[0].v as b, e3.v as c insert into O;"
            fq.append(head + "convert(v, 'double') > 50.0" + tail)
            tq.append(head + "v > 50.0" + tail)
    if kind in ("T4", "T5"):
        wrap = lambda qs: TWIN_TXN + "partition with (k of S) begin " + " ".join(qs) + " end;"  # noqa: E731
        return wrap(fq), wrap(tq)
    d = TWIN_STOCK if kind in ("T1", "T2") else TWIN_TXN
    return d + " ".join(fq), d + " ".join(tq)


def twin_events(kind, n, seed=99):
    """rows and timestamps: 5% nulls and some NaN in the compared column."""
    rng = random.Random(seed)
    rows, ts = [], []
    for k in range(n):
        if kind in ("T1", "T2"):
            r = rng.random()
            price = None if r < 0.05 else np.float32("nan") if r < 0.08 else np.float32(rng.uniform(0.0, 100.0))
            rows.append([f"SYM{rng.randint(0, 5)}", price, rng.randint(1, 100)])
        else:
            r = rng.random()
            amount = None if r < 0.05 else float("nan") if r < 0.08 else rng.uniform(0.0, 200.0)
            v = None if rng.random() < 0.05 else rng.randint(0, 100)
            rows.append([rng.randint(0, 7), amount, v])
        ts.append(TS0 + 400 * k)
    return rows, ts
