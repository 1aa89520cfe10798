"""The device selector's lane body on the host (tests/native/select_host.cpp builds
siddhi_amd/csrc/select_body.h and the store's row layout with g++): the oracle's matches, projected
from a row-major event store, must equal siddhi_amd/selector.py's project() bit for bit (cells and
null masks; any NaN equals any NaN of its type), and the decoded rows must satisfy the reference's own
expected rows."""
import numpy as np
import pytest

from harness import App
from select_host import (HAND_APPS, HostSelector, assert_cells_equal, callback_rows, reference_cells, seeded_apps,
                         seeded_events)
from siddhi_amd.selector import decode_rows
from test_absent_kat import FIXTURES as ABSENT_FIXTURES
from test_absent_kat import check_absent_rows, out_of_scope, run_absent_fixture
from test_oracle_reference_kat import KAT, OUT_OF_SCOPE, check_rows, run_fixture


def host_rows(app, cap=0):
    """Project the app's matches with the host body, compare with project(), return the decoded rows."""
    hs = HostSelector(app.blob)
    cells, nulls, err = hs.project(app.matches, app.log, cap)
    assert err == 0
    want_cells, want_nulls = reference_cells(app, app.matches, hs.width)
    assert_cells_equal(app, app.matches, cells, nulls, want_cells, want_nulls)
    q = np.array([m[0] for m in app.matches], np.int32)
    z = np.zeros(len(q), np.int64)
    return decode_rows(app.ir, (q, z, z, cells, nulls), app.dictionary)


IN_SCOPE = [f for f in KAT["fixtures"] if f["id"] not in OUT_OF_SCOPE]


@pytest.mark.parametrize("fx", IN_SCOPE, ids=[f["id"] for f in IN_SCOPE])
def test_reference_kat_rows(fx):
    app, _ = run_fixture(fx)
    rows = host_rows(app)
    check_rows(fx, callback_rows(fx["callback_kind"] == "QueryCallback", fx["callback"], app, app.matches, rows))


def test_every_in_scope_kat_runs():
    assert len(IN_SCOPE) == len(KAT["fixtures"]) - 2 and len(IN_SCOPE) >= 130


@pytest.mark.parametrize("fx", ABSENT_FIXTURES, ids=[f["id"] for f in ABSENT_FIXTURES])
def test_absent_kat_rows(fx):
    if "select" not in fx["app"] or out_of_scope(fx):
        return  # (no select list, or an app the planner refuses: nothing to project)
    app, _, checks = run_absent_fixture(fx)
    rows = host_rows(app)
    check_absent_rows(fx, callback_rows(fx["callback_kind"] == "query", fx["callback"], app, app.matches, rows), checks)


def run_events(src, events, engine_factory=None):
    app = App(src, engine_factory)
    for stream, row, ts in events:
        app.send(stream, [row], [ts])
    return app


@pytest.mark.parametrize("name,src,events", HAND_APPS, ids=[a[0] for a in HAND_APPS])
def test_hand_written_apps(name, src, events):
    app = run_events(src, events)
    assert app.matches, "the app must produce matches"
    rows = host_rows(app)
    if name == "arith_pairs":  # /0 and %0 are null, INT_MIN / -1 wraps
        assert any(v is None for r in rows for v in r) and any(v == -(2 ** 31) for r in rows for v in r)
    if name == "count_chain":  # a chain shorter than the index reads null
        assert any(r[3] is None and r[2] is not None for r in rows) and any(r[2] is None for r in rows)
    if name == "logical_or":
        assert any(r[1] is None for r in rows) and any(r[2] is None for r in rows)


def test_shapes_share_and_direct_loads():
    """Queries that differ in a constant only share one shape; a single-attribute output is marked for
    the direct load."""
    from select_host import lib
    src = ("define stream S (p float, v int); " +
           " ".join(f"@info(name = 'q{k}') from every e1=S[p > {k}.5f] -> e2=S[p > e1.p] select e1.p as a, "
                    f"e2.v + {k} as b insert into O{k};" for k in range(5)) +
           " @info(name = 'other') from every e1=S -> e2=S select e2.p as a insert into P;")
    app = App(src)
    hs = HostSelector(app.blob)
    L = lib()
    assert L.slh_shapes(hs.h) == 2
    assert len({L.slh_shape_of(hs.h, q) for q in range(5)}) == 1
    assert L.slh_out_direct(hs.h, 0, 0) == 1 and L.slh_out_direct(hs.h, 0, 1) == 0
    assert [L.slh_n_out(hs.h, q) for q in range(6)] == [2] * 5 + [1] and hs.width == 2
    for k in range(6):
        app.send("S", [[np.float32(k + 0.75), 10 * k]], [100 + k])
    host_rows(app)


SEEDED = seeded_apps()


@pytest.mark.parametrize("name,src", SEEDED, ids=[a[0] for a in SEEDED])
def test_seeded_select_lists(name, src):
    app = run_events(src, seeded_events())
    assert len(app.matches) >= 10
    host_rows(app)


def test_ring_and_evicted_events():
    """A store smaller than the log: rows over recent events are right across wraps, and a match
    that reads an evicted event reports it."""
    src = ("define stream S (v int); @info(name = 'q') from every e1=S -> e2=S[v == e1.v + 1] "
           "select e1.v as a, e2.v as b insert into O;")
    app = run_events(src, [("S", [k], k) for k in range(40)])
    assert len(app.matches) == 39
    hs = HostSelector(app.blob)
    recent = [m for m in app.matches if min(s[0] for s in m[3]) >= 40 - 8]
    cells, nulls, err = hs.project(recent, app.log, cap=8)
    assert err == 0
    want = reference_cells(app, recent, hs.width)
    assert_cells_equal(app, recent, cells, nulls, *want)
    _, _, err = hs.project(app.matches, app.log, cap=8)
    assert err == 1


def test_placed_rows_form():
    """K_ratchet's compact rows {query, e2 - seq_ref, e2 - e1, 0} project like the same matches as tuples."""
    src = ("define stream S (p float, v int); @info(name = 'q') from every e1=S[v > 0] -> e2=S[p > e1.p] "
           "select e1.p as a, e2.p as b, e2.v - e1.v as d insert into O;")
    app = run_events(src, [("S", [np.float32((k * 7) % 5), k], k) for k in range(20)])
    assert app.matches
    hs = HostSelector(app.blob)
    seq_ref = 3
    ms = [m for m in app.matches if m[3][1][0] >= seq_ref]
    crow = np.array([[m[0], m[3][1][0] - seq_ref, m[3][1][0] - m[3][0][0], 0] for m in ms], np.int32)
    cells, nulls, err = hs.project_pairs(crow, seq_ref, app.log)
    assert err == 0
    assert_cells_equal(app, ms, cells, nulls, *reference_cells(app, ms, hs.width))
