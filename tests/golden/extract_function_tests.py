#!/usr/bin/env python3
"""Transcribe the reference's built-in function known-answer tests (IfThenElse, Convert, Cast,
InstanceOf, Maximum / MinimumFunctionExtension and FunctionTestCase suites) into JSON fixtures.

Reads the TestNG sources under ``/root/reference`` (at generation time only) and writes DATA: per
``@Test`` method the stream definition, the ``select`` list and filter of the query the callback
observes (SiddhiQL text), the events sent in order, and the expected outcome -- the rows the callback
asserts (``assertEquals(V, event.getData(c))`` under ``if (count == k)`` / ``case k:``, or for every
row when unconditional; ``instanceof`` type asserts and ``assertNull``-style checks too), the final
``assertEquals(N, count)``, or that app creation must fail
(``expectedExceptions = SiddhiAppCreationException``).

A plain query ``from S[f] select <list>`` emits one row per event that passes ``f`` -- the rows of the
one-state pattern ``from every e1=S[f] select <list>``, which is how tests/test_functions.py runs them.

Skipped (listed in the output with the reason): what the accelerated path refuses -- conversion to or
from string, ``maximum(*)``, object-typed attributes and values whose Java class is not the column's
type (but for an Integer sent to a wider numeric column, or a Double to a float column, of a maximum /
minimum test: the fold widens them alike), functions outside the built-in set -- and tests built through the Java query API.

Usage:  python tests/golden/extract_function_tests.py  (writes tests/golden/reference_function_kat.json)
"""
from __future__ import annotations

import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from extract_reference_tests import (_concat_value, _literal, _methods, _split_top,  # noqa: E402
                                     _statement, _strip_comments)

REF = "/root/reference/modules/siddhi-core/src/test/java/org/wso2/siddhi/core/query/function"
FILES = ["IfThenElseFunctionTestCase.java", "ConvertFunctionTestCase.java", "CastFunctionExecutorTestCase.java",
         "InstanceOfFunctionTestCase.java", "MaximumFunctionExtensionTestCase.java",
         "MinimumFunctionExtensionTestCase.java", "FunctionTestCase.java"]
_JAVA_CLASS = {"Integer": "int", "Long": "long", "Float": "float", "Double": "double", "Boolean": "bool",
               "String": "string"}
_KIND = {"i": "int", "l": "long", "f": "float", "d": "double", "b": "bool", "s": "string"}
_BUILTINS = {"ifThenElse", "coalesce", "default", "maximum", "minimum", "convert", "cast", "instanceOfInteger",
             "instanceOfLong", "instanceOfFloat", "instanceOfDouble", "instanceOfBoolean", "instanceOfString"}


def _refused(define_attrs, select, flt):
    """Why the accelerated path refuses this query by design (None: it does not)."""
    types = dict(define_attrs)
    if "object" in types.values():
        return "object-typed attribute"
    text = select + " " + (flt or "")
    if re.search(r"\w+\s*\(\s*\*\s*\)", text):
        return "function(*)"
    for fn in re.findall(r"([\w:]+)\s*\(", text):
        if fn not in _BUILTINS:
            return f"function {fn}() is outside the built-in set"
    for m in re.finditer(r"convert\s*\(\s*(\w+)\s*,\s*'(\w+)'\s*\)", text):
        src, to = types.get(m.group(1)), m.group(2).lower()
        if (src == "string") != (to == "string"):
            return "string conversion"
    return None


def _blocks(cb: str):
    """(row number or None, text) pieces of a callback body: `if (count == k) {..}` / `case k: .. break`."""
    out, rest = [], cb
    for m in re.finditer(r"if\s*\(\s*count(?:\.get\(\))?\s*==\s*(\d+)\s*\)\s*\{(.*?)\}", cb, re.S):
        out.append((int(m.group(1)), m.group(2)))
        rest = rest.replace(m.group(0), "")
    for m in re.finditer(r"case\s+(\d+)\s*:(.*?)break\s*;", cb, re.S):
        out.append((int(m.group(1)), m.group(2)))
        rest = rest.replace(m.group(0), "")
    out.append((None, rest))
    return out


def _asserts(text: str):
    """{column: expectation} of one block: a literal token, {'type': t} or 'null'."""
    cells = {}
    for m in re.finditer(r"assertEquals\(\s*(.+?)\s*,\s*\w+\.getData\(\s*(\d+)\s*\)\s*\)\s*;", text, re.S):
        cells[int(m.group(2))] = _literal(m.group(1))
    for m in re.finditer(r"assertEquals\(\s*\w+\.getData\(\s*(\d+)\s*\)\s*,\s*(.+?)\s*\)\s*;", text, re.S):
        cells[int(m.group(1))] = _literal(m.group(2))
    for m in re.finditer(r"assertTrue\(\s*\w+\.getData\(\s*(\d+)\s*\)\s*instanceof\s+(\w+)\s*\)", text):
        cells.setdefault(int(m.group(1)), {"type": _JAVA_CLASS[m.group(2)]})
    for m in re.finditer(r"assertTrue\(\s*\w+\.getData\(\s*(\d+)\s*\)\s*==\s*null\s*\)|assertNull\(\s*\w+\.getData\(\s*(\d+)\s*\)",
                         text):
        cells[int(m.group(1) or m.group(2))] = "null"
    return cells


def extract_method(body: str, expects_exception: bool):
    if "new Query()" in body or "Query.query()" in body:
        return None, "built through the Java query API"
    env = {}
    for m in re.finditer(r"String\s+(\w+)\s*=\s*", body):
        expr = _statement(body, m.end()).strip()
        if expr.startswith("(") and expr.endswith(")"):   # String query = ("..." + "...");
            expr = expr[1:-1]
        try:
            env[m.group(1)] = _concat_value(expr, env)
        except ValueError:
            pass
    m = re.search(r"createSiddhiAppRuntime\(", body)
    if not m:
        return None, "no createSiddhiAppRuntime"
    app = _concat_value(_statement(body, m.end())[:-1], env)
    defs = re.findall(r"define stream (\w+)\s*\(([^)]*)\)", app)
    qm = re.search(r"from\s+(\w+)\s*(?:\[(.*?)\])?\s*select\s+(.*?)\s*insert into", app, re.S)
    if not qm or len(defs) != 1 or qm.group(1) != defs[0][0]:
        return None, "not one plain query over one defined stream"
    stream, attrs_text = defs[0]
    attrs = [tuple(a.split()) for a in attrs_text.split(",")]
    flt, select = qm.group(2), re.sub(r"\s+", " ", qm.group(3))
    why = _refused(attrs, select, flt)
    if why:
        return None, why
    fx = {"define": f"define stream {stream} ({', '.join(' '.join(a) for a in attrs)});", "stream": stream,
          "select": select, "filter": flt.strip() if flt else None}
    if expects_exception:
        fx["expect_creation_error"] = True
        return fx, None
    only_fold = set(re.findall(r"([\w:]+)\s*\(", select + " " + (flt or ""))) <= {"maximum", "minimum"}
    cb_start = body.find("addCallback(")
    if cb_start < 0:
        return None, "no callback"
    send0 = body.find(".start()", cb_start)
    cb, rest = body[cb_start:send0], body[send0:]
    events = []
    for sm in re.finditer(r"\w+\.send\(new Object\[\]\s*\{(.*?)\}\s*\);|for\s*\(", rest, re.S):
        if sm.group(1) is None:
            return None, "loop in send sequence"
        ev = [_literal(t) for t in _split_top(sm.group(1))]
        while len(ev) < len(attrs):           # a short Object[]: the missing attributes read null
            ev.append("null")
        for k, (tok, (_, ty)) in enumerate(zip(ev, attrs)):
            if tok != "null" and _KIND[tok[0]] != ty:
                # maximum / minimum widen every argument to double by its Java class
                # (MaximumFunctionExecutor.execute:104-121), so an Integer sent into a long / float /
                # double column folds like that column's own value: recorded as the column's type
                # (a Double sent into a float column too: rounding to float is monotone, so
                # (float) max(d..) == max((float) d..))
                if only_fold and ((tok[0] == "i" and ty in ("long", "float", "double")) or
                                  (tok[0] == "d" and ty == "float")):
                    ev[k] = ty[0] + tok[1:]
                    fx["coerced_literals"] = True
                    continue
                return None, f"a sent {_KIND[tok[0]]} value in a {ty} column (its Java class decides the result)"
        events.append(ev)
    rows = {}
    every = {}
    for k, text in _blocks(cb):
        cells = _asserts(text)
        if k is None:
            every = cells
        else:
            rows.setdefault(k, {}).update(cells)
    exact = re.findall(r"assertEquals\(\s*(\d+)\s*,\s*count(?:\.get\(\))?\s*\)", rest)
    if not exact:
        return None, "no count expectation"
    n = int(exact[-1])
    fx["events"] = events
    fx["expected_count"] = n
    # per emitted row {column: expectation}; unconditional asserts hold for every row
    fx["expected_rows"] = [{str(c): v for c, v in {**every, **rows.get(k, {})}.items()} for k in range(1, n + 1)]
    return fx, None


def main():
    out, skipped = [], []
    for rel in FILES:
        raw = open(os.path.join(REF, rel)).read()
        src = _strip_comments(raw)
        for name, _, body in _methods(src):
            m = re.search(r"(@Test[^\n]*)\n\s*public void " + name + r"\s*\(", src)
            exc = bool(m and "SiddhiAppCreationException" in m.group(1))
            rm = re.search(r"public void " + name + r"\s*\(", raw)
            line = raw.count("\n", 0, rm.start()) + 1 if rm else 0
            tid = f"{rel[:-5]}.{name}"
            try:
                fx, why = extract_method(body, exc)
            except Exception as ex:  # noqa: BLE001
                fx, why = None, f"extract error: {ex}"
            if fx is None:
                skipped.append((tid, why))
                continue
            fx["id"] = tid
            fx["source"] = f"modules/siddhi-core/src/test/java/org/wso2/siddhi/core/query/function/{rel}:{line}"
            out.append(fx)
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_function_kat.json")
    with open(dst, "w") as f:
        json.dump({"generator": "tests/golden/extract_function_tests.py", "fixtures": out, "skipped": skipped},
                  f, indent=1)
    print(f"{len(out)} fixtures, {len(skipped)} skipped -> {dst}")


if __name__ == "__main__":
    main()
