"""Built-in functions in filters and select lists (ifThenElse, coalesce, default, maximum, minimum,
convert, cast, instanceOf*, eventTimestamp), on the CPU: the planner's lowering, the host builds of the
interpreter (tests/native/kgen_host.cpp) and of the selector's lane body (select_host.cpp), against
siddhi_amd/selector.py -- the Python restatement of core/executor/function/*.java -- and against the
rows the reference's own function suites assert (tests/golden/reference_function_kat.json,
transcribed by tests/golden/extract_function_tests.py). The oracle never sees a function."""
import json
import os
import re

import numpy as np
import pytest

import function_cases as fc
from harness import App
from kgen_host import KGenHostEngine
from select_host import HostSelector, assert_cells_equal, reference_cells
from siddhi_amd import ir, ql
from siddhi_amd.planner import plan
from siddhi_amd.ql import SiddhiAppCreationException, SiddhiParserException
from siddhi_amd.selector import evaluate, project

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_OPS = ("OP_SELECT", "OP_COALESCE", "OP_CONVERT", "OP_MAX2", "OP_MIN2", "OP_EVENT_TS")


# ---- 1. reference fixtures ----
@pytest.mark.parametrize("fx", fc.FIXTURES, ids=[f["id"] for f in fc.FIXTURES])
def test_reference_function_fixture(fx):
    if fx.get("expect_creation_error"):
        with pytest.raises(SiddhiAppCreationException):
            App(fc.fixture_app(fx), engine_factory=lambda blob: None)
        return
    app = fc.run_fixture(fx, KGenHostEngine)
    fc.check_fixture_rows(fx, app.rows_for_query("query1"))


def test_reference_function_fixture_coverage():
    """Every suite is transcribed; CastFunctionExecutorTestCase reads an object-typed attribute in
    each of its tests, so all of them sit in the skipped list (with that reason)."""
    got = {f["id"].split(".")[0] for f in fc.FIXTURES}
    listed = got | {s[0].split(".")[0] for s in fc.KAT["skipped"]}
    assert listed == set(fc.SUITES)
    assert got == set(fc.SUITES) - {"CastFunctionExecutorTestCase"}
    assert all("object" in why for tid, why in fc.KAT["skipped"] if tid.startswith("CastFunctionExecutorTestCase."))
    assert all(why for _, why in fc.KAT["skipped"])
    n_fx, n_skip = len(fc.FIXTURES), len(fc.KAT["skipped"])
    assert n_skip / (n_fx + n_skip) < 0.5, f"{n_skip} of {n_fx + n_skip} reference tests skipped"
    assert len(fc.RUNNABLE) >= 12


# ---- 2. interpreter and selector body against the Python restatement, seeded ----
CASES = fc.gen_cases()
EVENTS = fc.gen_events(300, seed=31)


def _send_events(app):
    app.send("S", EVENTS, [fc.TS0 + k for k in range(len(EVENTS))])


def test_seeded_cases_cover_every_function_and_type():
    text = " ".join(e for _, _, e in CASES)
    for fn in ("ifThenElse", "coalesce", "default", "maximum", "minimum", "convert", "cast", "instanceOfInteger",
               "instanceOfLong", "instanceOfFloat", "instanceOfDouble", "instanceOfBoolean", "instanceOfString"):
        assert fn + "(" in text, fn
    assert len(CASES) >= 60


@pytest.mark.parametrize("name,t,expr", CASES, ids=[c[0] for c in CASES])
def test_seeded_filter_on_host_interpreter(name, t, expr):
    """every e1=S[f]: the matched sequence numbers are the events selector.evaluate finds TRUE."""
    app = App(fc.gen_app(["e1.i"], fc.as_filter(t, expr)), KGenHostEngine)
    _send_events(app)
    code = app.ir.queries[0].states[0].filters[0]
    want = [k for k in range(len(EVENTS))
            if evaluate(code, [[k]], app.log, None, app.dictionary, app.ir.strings) is True]
    assert [m[3][0][0] for m in app.matches] == want


def test_seeded_outputs_on_host_selector():
    """select lists through the selector's lane body: cells and null bits equal selector.project."""
    for lo in range(0, len(CASES), 8):
        chunk = CASES[lo:lo + 8]
        app = App(fc.gen_app([e for _, _, e in chunk]), KGenHostEngine)
        _send_events(app)
        assert len(app.matches) == len(EVENTS)
        hs = HostSelector(app.blob)
        cells, nulls, err = hs.project(app.matches, app.log)
        assert err == 0
        assert_cells_equal(app, app.matches, cells, nulls, *reference_cells(app, app.matches, hs.width))


_CONV_VALUES = {"int": fc._SPECIAL["int"], "long": fc._SPECIAL["long"],
                "float": [np.float32(v) for v in fc._SPECIAL["float"]], "double": fc._SPECIAL["double"],
                "bool": [True, False]}


@pytest.mark.parametrize("src", list(_CONV_VALUES))
def test_convert_pairs(src):
    """convert(x, T) for every non-string pair over the corner values, host selector body against the
    restatement; the restatement's own saturation is pinned by the literals of test_quirk_pin."""
    col = fc._COLS[src][0]
    tos = ["int", "long", "float", "double", "bool"]
    app = App(fc.gen_app([f"convert(e1.{col}, '{to}')" for to in tos]), KGenHostEngine)
    names = "ijlmfgdebcst"
    rows = [[v if n == col else None for n in names] for v in _CONV_VALUES[src]] + [[None] * 12]
    app.send("S", rows, [fc.TS0 + k for k in range(len(rows))])
    hs = HostSelector(app.blob)
    cells, nulls, err = hs.project(app.matches, app.log)
    assert err == 0 and len(app.matches) == len(rows)
    assert_cells_equal(app, app.matches, cells, nulls, *reference_cells(app, app.matches, hs.width))
    assert int(nulls[-1]) & 0x1F == 0x1F  # a null converts to null


# ---- 3. quirk pins ----
@pytest.mark.parametrize("name,expr,row,want", fc.PINS, ids=[p[0] for p in fc.PINS])
def test_quirk_pin(name, expr, row, want):
    app = App(fc.pin_app(expr), KGenHostEngine)
    app.send("S", [row], [fc.TS0])
    (got,), = app.rows_for_query("q")
    assert fc.same_value(got, want), f"{expr} over {row}: {got!r}, the reference computes {want!r}"
    hs = HostSelector(app.blob)
    cells, nulls, err = hs.project(app.matches, app.log)
    assert_cells_equal(app, app.matches, cells, nulls, *reference_cells(app, app.matches, hs.width))


def test_event_timestamp_is_the_match_timestamp():
    """eventTimestamp() in a select list reads the StateEvent's timestamp (the match's ts column)."""
    src = ("define stream S (i int); @info(name = 'q') from every e1=S -> e2=S[i > e1.i] "
           "select eventTimestamp() as t, eventTimestamp() - 5L as u, e1.i as a insert into O;")
    app = App(src, KGenHostEngine)
    app.send("S", [[1], [0], [2]], [1000, 1010, 1025])
    q = app.ir.queries[0]
    rows = [project(q, m[3], app.log, None, app.dictionary, app.ir.strings, ts=m[2]) for m in app.matches]
    assert rows == [[1025, 1020, 1], [1025, 1020, 0]]
    assert [m[2] for m in app.matches] == [1025, 1025]
    with pytest.raises(ValueError, match="eventTimestamp"):
        app.rows_for_query("q")  # (without the match's timestamp there is nothing to read)


# ---- 4. refusals ----
@pytest.mark.parametrize("src,names", fc.REFUSALS, ids=[f"{k}_{r[1]}" for k, r in enumerate(fc.REFUSALS)])
def test_refused_form_is_named(src, names):
    with pytest.raises(SiddhiAppCreationException, match=re.escape(names)):
        plan(ql.parse(src))


def test_maximum_star_is_refused():
    with pytest.raises(SiddhiParserException, match=r"maximum\(\*\)"):
        ql.parse(fc._R + " select maximum(*) as o insert into O;")


def test_too_deep_program_is_refused_at_create():
    with pytest.raises(SiddhiAppCreationException, match="evaluation stack"):
        plan(ql.parse(fc.too_deep_app()))


def test_depth_of_a_ternary_program():
    """ifThenElse nested on its else side keeps two entries pending per level: 2 * levels + 1."""
    from siddhi_amd.planner import code_depth
    e = "e1.i"
    for k in range(3):
        e = f"ifThenElse(e1.b, {k}, {e})"
    irp = plan(ql.parse(fc.gen_app([e])))
    assert code_depth(irp.queries[0].outputs[0].code) == 7
    # and the host lowering agrees: 7 entries need the indexed stack (RSTACK = 6), which computes the same
    app = App(fc.gen_app([e]), KGenHostEngine)
    _send_events(app)
    hs = HostSelector(app.blob)
    cells, nulls, err = hs.project(app.matches, app.log)
    assert_cells_equal(app, app.matches, cells, nulls, *reference_cells(app, app.matches, hs.width))


# ---- 5. function-free programs keep their bytes ----
def test_function_free_programs_keep_their_bytes():
    """Every workload and every reference_kat.json app serializes to the bytes it had before functions
    existed (tests/golden/ir_digests.json, recorded from the commit before: make_ir_digests.py)."""
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_ir_digests
    want = json.load(open(os.path.join(HERE, "golden", "ir_digests.json")))["digests"]
    got = make_ir_digests.digests()
    assert len(want) >= 140
    assert set(got) == set(want)
    diff = [k for k in want if got[k] != want[k]]
    assert not diff, diff


def test_ir_header_names_the_new_opcodes():
    """include/siddhi_hip_ir.h, siddhi_amd/ir.py and kgen.h agree on the function opcodes, which are
    additions after SDH_OP_ARITH; IR_VERSION stays."""
    root = os.path.dirname(HERE)
    text = open(os.path.join(root, "include", "siddhi_hip_ir.h")).read()
    defs = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"#define SDH_(\w+) \(?(-?\d+)\)?", text))
    for k, name in enumerate(NEW_OPS):
        assert defs[name] == getattr(ir, name) == defs["OP_ARITH"] + 1 + k, name
        assert re.search(r"\*\s+SDH_" + name + r"\b", text), f"{name} has no grammar line"
    assert defs["IR_VERSION"] == ir.VERSION == 2
    kgen = open(os.path.join(root, "siddhi_amd", "csrc", "kgen.h")).read()
    m = re.search(r"enum \{ OP_CONST = 1,(.*?)\};", kgen, re.S)
    names = [x.strip() for x in re.sub(r"//[^\n]*", "", m.group(1)).split(",") if x.strip()]
    assert ["OP_CONST"] + names == [n for n, _ in sorted(((n, v) for n, v in defs.items() if n.startswith("OP_")),
                                                         key=lambda x: x[1])]


def test_apps_of_the_readme_parse_plan_and_run():
    src = ("define stream S (symbol string, price float, qty int); @info(name = 'q') "
           "from every e1=S[price > 20.0f] -> e2=S[coalesce(price, e1.price) > e1.price] "
           "select ifThenElse(e2.price > e1.price, 'up', 'down') as dir, convert(e1.qty, 'double') * e2.price as x "
           "insert into O;")
    app = App(src, KGenHostEngine)
    app.send("S", [["a", np.float32(25.0), 3], ["a", None, 1], ["a", np.float32(30.5), 2]], [1, 2, 3])
    assert app.rows_for_query("q") == [["up", 91.5]]
