"""Built-in functions on the device: filters on every plan that evaluates bytecode (K_gen, the K_seq
interpreter and its shape-compiled form, K_part) and select lists in sdh_engine_poll_rows.

No oracle sees a function. One-state queries are checked against siddhi_amd/selector.py (the Python
restatement of core/executor/function/*.java) and the rows the reference's own suites assert;
multi-state behaviour is checked through twins: a function query paired with a function-free query
that is equal on every input, the twin run on the oracle (test_twin_against_the_oracle)."""
import functools

import numpy as np
import pytest

import function_cases as fc
from harness import App, decode_matches
from select_host import assert_cells_equal
from siddhi_amd.events import encode_rows
from siddhi_amd.selector import decode_rows, evaluate, project

pytestmark = pytest.mark.gpu

SDH_FLAG_FORCE_GEN = 4
PLANS = ("K_ratchet", "K_gate", "K_chain", "K_part", "K_slab", "K_seq", "K_gen")


def plan_counts(engine):
    pq = engine.stats().plan_queries
    return {name: int(pq[k]) for k, name in enumerate(PLANS) if pq[k]}


def reference_cells_ts(app, matches, width):
    """select_host.reference_cells with the match's timestamp handed to project (eventTimestamp())."""
    n = len(matches)
    cells = np.zeros((width, n), np.int64)
    nulls = np.zeros(n, np.uint64)
    for i, m in enumerate(matches):
        q = app.ir.queries[m[0]]
        row = project(q, m[3], app.log, None, app.dictionary, app.ir.strings, ts=m[2])
        c, bits = fc.encode_row(app, q, row)
        cells[:len(c), i] = c
        nulls[i] = bits | (((1 << 64) - 1) & ~((1 << len(row)) - 1))
    return cells, nulls


def check_polled(app, tuples, rows):
    """rows (poll_rows of one engine) against tuples (poll(with_seq=True) of its twin engine), both
    against the restatement; returns the matches and the decoded rows."""
    q, k, ts, off, words, seq, tb = tuples
    rq, rts, rseq, cells, nulls = rows
    assert np.array_equal(rq, q) and np.array_equal(rts, ts) and np.array_equal(rseq, seq)
    matches = decode_matches(len(q), q, k, ts, off, words, lambda i: len(app.ir.queries[i].states))
    w = max([len(x.outputs) for x in app.ir.queries] + [0])
    assert cells.shape == (w, len(q))
    assert_cells_equal(app, matches, cells, nulls, *reference_cells_ts(app, matches, w))
    return matches, decode_rows(app.ir, rows, app.dictionary)


class Pair:
    """harness.App engine: two HipEngines fed alike, `a` polled with poll(), `b` (retaining events) with
    poll_rows(); every take compares them and the restatement."""

    def __init__(self, blob, retain=4096, **kw):
        from siddhi_amd.engine import HipEngine
        self.a = HipEngine(blob, **kw)
        self.b = HipEngine(blob, **kw)
        self.b.retain_events(retain)
        self.app = None
        self.rows = []

    def send(self, *args, **kw):
        self.a.send(*args, **kw)
        self.b.send(*args, **kw)

    def set_strings(self, ids, texts):
        self.a.set_strings(ids, texts)
        self.b.set_strings(ids, texts)

    def take_matches(self, n_slots_of):
        matches, rows = check_polled(self.app, self.a.poll(with_seq=True), self.b.poll_rows())
        self.rows += rows
        return matches


def pair_app(src, **kw):
    app = App(src, engine_factory=lambda blob: None)
    app.engine = Pair(app.blob, stream_types=[s.attr_types for s in app.ir.streams], **kw)
    app.engine.app = app
    return app


def passing(app, n, qi=0):
    """event numbers the restatement passes through query qi's one-state filter (all without one)"""
    fs = app.ir.queries[qi].states[0].filters
    return [k for k in range(n)
            if all(evaluate(f, [[k]], app.log, None, app.dictionary, app.ir.strings) is True for f in fs)]


# ---- 6. the reference's fixtures and the quirk pins ----
@pytest.mark.parametrize("flags", [0, SDH_FLAG_FORCE_GEN], ids=["planned", "force_gen"])
@pytest.mark.parametrize("fx", fc.RUNNABLE, ids=[f["id"] for f in fc.RUNNABLE])
def test_reference_function_fixture_on_gpu(fx, flags):
    app = pair_app(fc.fixture_app(fx), flags=flags)
    for i, ev in enumerate(fx["events"]):
        app.send(fx["stream"], [[fc.parse_literal(t) for t in ev]], [fc.TS0 + i])
    assert [m[3][0][0] for m in app.matches] == passing(app, len(fx["events"]))
    fc.check_fixture_rows(fx, app.engine.rows)


@pytest.mark.parametrize("flags", [0, SDH_FLAG_FORCE_GEN], ids=["planned", "force_gen"])
def test_quirk_pins_on_gpu(flags):
    """Every pin as one query of its own app (one push each): the literal the reference computes."""
    for name, expr, row, want in fc.PINS:
        app = pair_app(fc.pin_app(expr), flags=flags)
        app.send("S", [row], [fc.TS0])
        assert len(app.engine.rows) == 1, name
        got = app.engine.rows[0][0]
        assert fc.same_value(got, want), f"{name}: {expr} over {row}: {got!r}, the reference computes {want!r}"


# ---- 7. seeded, device against the restatement ----
N_EVENTS, N_PUSH, N_QUERIES = 2000, 4, 130


def shape_events():
    """the seeded events with i in 0 .. 140 and j in 0 .. 30, so that the queries' constants decide"""
    import random
    rng = random.Random(8)
    ev = fc.gen_events(N_EVENTS, seed=57)
    for row in ev:
        row[0] = None if rng.random() < 0.1 else rng.randint(0, 140)
        row[1] = None if rng.random() < 0.1 else rng.randint(0, 30)
    return ev


EVENTS = shape_events()


def shape_const(p):
    """13 constants over 130 queries: the restatement runs once per constant, every query is checked"""
    return 10 * (p % 13)


def shape_query(p, c):
    f = (f"ifThenElse(e1.b, maximum(e1.i, {c}) == e1.i and e1.i < {c} + 12, coalesce(e1.j, {c}) < 2)")
    return (f"@info(name = 'q{p}') from every e1=S[{f}] "
            f"select minimum(e1.i, {c}) as a, default(e1.f, {c}.25f) as b, convert(e1.d, 'long') as c insert into O;")


def shape_app():
    """130 one-state queries of one shape that differ in constants inside function arguments."""
    return fc.GEN_DEF + " " + " ".join(shape_query(p, shape_const(p)) for p in range(N_QUERIES))


@functools.lru_cache(maxsize=None)
def shape_reference():
    """per constant the passing events, by the restatement (computed once for both SDH_SPEC settings)"""
    app = App(fc.GEN_DEF + " " + " ".join(shape_query(k, 10 * k) for k in range(13)), engine_factory=lambda blob: None)
    vals, nulls = encode_rows(EVENTS, app.ir.streams[0].attr_types, app.dictionary)
    app.log.append(0, [fc.TS0 + k for k in range(N_EVENTS)], vals, nulls)
    return {10 * k: passing(app, N_EVENTS, k) for k in range(13)}


@pytest.mark.parametrize("spec", ["1", "0"], ids=["spec", "interpreted"])
def test_seeded_shape_of_130_queries(spec):
    ref = shape_reference()
    want = [ref[shape_const(p)] for p in range(N_QUERIES)]
    assert 5000 < sum(len(w) for w in want) < 30000 and len({tuple(w) for w in ref.values()}) == 13
    app = pair_app(shape_app(), debug=f"SDH_SPEC={spec}")
    step = N_EVENTS // N_PUSH
    for lo in range(0, N_EVENTS, step):
        app.send("S", EVENTS[lo:lo + step], [fc.TS0 + k for k in range(lo, lo + step)])
    got = [[] for _ in range(N_QUERIES)]
    for m in app.matches:
        got[m[0]].append(m[3][0][0])
    assert got == want
    print("plans", plan_counts(app.engine.a), "spec kernels", app.engine.a.stats().spec_kernels)


def _nested(levels):
    e = "e1.i"
    for k in range(levels):
        e = f"ifThenElse(e1.b, {k}, {e})"
    return e


def test_deep_output_reaches_the_indexed_stack():
    """ifThenElse nested on its else side needs 2 * levels + 1 entries: 9 is past RSTACK (6)."""
    from siddhi_amd.planner import code_depth
    app = pair_app(fc.gen_app([_nested(4), "maximum(e1.i, e1.j)"]))
    assert code_depth(app.ir.queries[0].outputs[0].code) == 9
    app.send("S", EVENTS[:300], [fc.TS0 + k for k in range(300)])
    assert len(app.matches) == 300


def test_mixed_function_shapes_in_one_wave():
    """Three select shapes over the same events: adjacent rows of a wave belong to different shapes."""
    outs = ["ifThenElse(e1.b, e1.i, e1.j) as a",
            "maximum(e1.l, e1.m) as a, convert(e1.f, 'int') as b",
            "coalesce(e1.s, e1.t, 'none') as a, instanceOfDouble(e1.d) as b, minimum(e1.d, e1.e, 0.5) as c"]
    src = fc.GEN_DEF + " ".join(f"@info(name = 'm{k}') from every e1=S select {o} insert into O{k};"
                                for k, o in enumerate(outs))
    app = pair_app(src)
    app.send("S", EVENTS[:100], [fc.TS0 + k for k in range(100)])
    assert len(app.matches) == 300
    assert len({m[0] for m in app.matches[:64]}) == 3


@pytest.mark.parametrize("second_producer", [False, True], ids=["placed", "sorted"])
def test_event_timestamp_in_placed_and_sorted_windows(second_producer):
    """eventTimestamp() reads the row's ts in both input forms of the selector: K_ratchet's placed
    compact rows (a C2-shaped query alone) and the sorted table (a K_chain query in the window)."""
    from test_gpu_rows import CHAIN_QUERY, push_stock, stock_app
    qs = " ".join(f"@info(name='p{p}') from every e1=StockStream[price > {30 + 10 * p}.0] -> "
                  f"e2=StockStream[price > e1.price] within 1 sec select eventTimestamp() as t, e1.price as p1, "
                  f"ifThenElse(e2.price > 90.0, eventTimestamp() - {p}L, 0L) as u insert into OutStream;" for p in range(3))
    src = "define stream StockStream (symbol string, price float, volume int); " + qs
    app, a, b = stock_app(src + (CHAIN_QUERY if second_producer else ""))
    b.retain_events(1024)
    placed0 = b.stats().placed_pushes
    total = 0
    for lo in (0, 200):
        push_stock(app, (a, b), lo, 200)
        matches, rows = check_polled(app, a.poll(with_seq=True), b.poll_rows())
        assert all(r[0] == m[2] for m, r in zip(matches, rows) if m[0] < 3)
        total += len(matches)
    assert total > 128
    assert b.stats().placed_pushes == placed0 + (0 if second_producer else 2)


# ---- 8. twins against the oracle ----
#
# T1  e2=S[ifThenElse(price > e1.price, true, false)]  ==  e2=S[price > e1.price]: the compare is TRUE,
#     FALSE (never null: a compare with a null or NaN operand is FALSE); ifThenElse maps TRUE -> true and
#     anything else -> false, and the filter passes exactly on true.
# T2  e2=S[coalesce(price, e1.price) > e1.price]  ==  the same twin: e1.price is non-null (it passed
#     `> 20`); a non-null price gives the twin's compare; a null price gives e1.price > e1.price = FALSE,
#     as the twin's compare with null.
# T3  e2=S[maximum(amount, e1.amount) == amount]  ==  e2=S[amount >= e1.amount], amount double:
#     e1.amount > 100 beats the seed (Double.MIN_VALUE), so the fold is e1.amount unless amount is
#     non-null, not NaN and > e1.amount, when it is amount. amount > e1.amount: amount == amount TRUE, twin
#     TRUE. amount == e1.amount: e1.amount == amount TRUE, twin TRUE. amount < e1.amount: e1.amount ==
#     amount FALSE, twin FALSE. amount null / NaN: the fold is e1.amount, and == null / NaN is FALSE; twin FALSE.
# T4  e2=S[convert(v, 'double') > 50.0]  ==  e2=S[v > 50.0], v int: the twin's compare runs in double
#     ((double)v > 50.0, GreaterThanCompareConditionExpressionExecutorIntDouble), exactly what convert
#     yields; a null v converts to null and the compare is FALSE in both.
# T5  T4's filters on the last state of `every e1=S[v > a] -> e2=S[v > 10]<2:3> -> e3=S[..] within 10 sec`,
#     the count form of workloads.c3_query: the issue's T4 text (`every e1=S[..]<2:3> -> e2=S[..]`, a count
#     at the start) is not a K_part shape -- its twin runs on K_gen too -- so T4 keeps that text and pins
#     "the twin's plan", and T5 carries the function onto K_part.
TWINS = [(k, n, None) for k in ("T1", "T2", "T3", "T4", "T5") for n in (65, 130)]
TWINS += [("T3", 130, "1"), ("T3", 130, "0"), ("T5", 130, "1"), ("T5", 130, "0")]  # hiprtc-compiled / interpreted
# where each function query must run, and where its twin runs (the twins are function-free: the planner
# and the lowerings treat function-free programs as the commit before functions did)
FUNCTION_PLAN = {"T3": "K_seq", "T4": "K_gen", "T5": "K_part"}
TWIN_PLAN = {"T1": "K_ratchet", "T2": "K_ratchet", "T3": "K_seq", "T4": "K_gen", "T5": "K_part"}


def run_twin(kind, n_queries, n_events, spec=None):
    from siddhi_amd.engine import HipEngine
    f_src, t_src = fc.twin_queries(kind, n_queries)
    rows, ts = fc.twin_events(kind, n_events)
    oracle = App(t_src)
    types = [s.attr_types for s in oracle.ir.streams]
    kw = {"debug": f"SDH_SPEC={spec}"} if spec else {}
    dev = App(f_src, engine_factory=lambda blob: HipEngine(blob, stream_types=types, **kw))
    twin_dev = App(t_src, engine_factory=lambda blob: HipEngine(blob, stream_types=types, **kw))
    step = n_events // 4
    for lo in range(0, n_events, step):
        for app in (oracle, dev, twin_dev):
            app.send("S", rows[lo:lo + step], ts[lo:lo + step])
    return oracle, dev, twin_dev


@pytest.mark.parametrize("kind,n_queries,spec", TWINS, ids=[f"{k}_{n}" + (f"_spec{s}" if s else "") for k, n, s in TWINS])
def test_twin_against_the_oracle(kind, n_queries, spec):
    oracle, dev, twin_dev = run_twin(kind, n_queries, 1200, spec)
    assert len(oracle.matches) > 200
    assert dev.matches == oracle.matches
    assert twin_dev.matches == oracle.matches
    got, twin = plan_counts(dev.engine), plan_counts(twin_dev.engine)
    print(kind, n_queries, spec, "function plan", got, "twin plan", twin, "spec kernels",
          dev.engine.stats().spec_kernels, twin_dev.engine.stats().spec_kernels)
    assert sum(got.values()) == n_queries and not set(got) & {"K_ratchet", "K_gate", "K_chain"}
    if kind in FUNCTION_PLAN:
        assert got == {FUNCTION_PLAN[kind]: n_queries}
    assert twin == {TWIN_PLAN[kind]: n_queries}
    if spec:  # a function keeps the query on the shape-compiled kernel (spec.hip emit_filter)
        assert (dev.engine.stats().spec_kernels > 0) == (spec == "1")


def seq_query(p, c):
    f1 = f"ifThenElse(e1.b, maximum(e1.i, {c}) == e1.i and e1.i < {c} + 40, coalesce(e1.j, {c}) < 3)"
    f2 = f"coalesce(e2.j, {c}) < 9 or minimum(e2.i, e1.i, {c}) == convert(e1.i, 'double')"
    return (f"@info(name = 'q{p}') from every e1=S[{f1}], e2=S[{f2}] "
            f"select maximum(e1.i, e2.i, {c}) as a, ifThenElse(e2.b, e1.f, e2.f) as b insert into O;")


@functools.lru_cache(maxsize=None)
def seq_reference():
    """per constant the (k, k + 1) windows of a two-state strict sequence: e1's filter over event k and
    e2's over (k, k + 1) -- every event opens a partial, the next event closes or drops it"""
    app = App(fc.GEN_DEF + " " + " ".join(seq_query(k, 10 * k) for k in range(13)), engine_factory=lambda blob: None)
    vals, nulls = encode_rows(EVENTS, app.ir.streams[0].attr_types, app.dictionary)
    app.log.append(0, [fc.TS0 + k for k in range(N_EVENTS)], vals, nulls)
    ev = lambda code, slots: evaluate(code, slots, app.log, None, app.dictionary, app.ir.strings) is True  # noqa: E731
    out = {}
    for k in range(13):
        f1, f2 = (st.filters[0] for st in app.ir.queries[k].states)
        out[10 * k] = [e for e in range(N_EVENTS - 1) if ev(f1, [[e]]) and ev(f2, [[e], [e + 1]])]
    return out


@pytest.mark.parametrize("spec", ["1", "0"], ids=["spec", "interpreted"])
def test_seeded_sequence_shape_of_130_queries(spec):
    """The shape of test_seeded_shape_of_130_queries as a two-state sequence: K_seq, hiprtc-compiled from
    the shape's bytecode (SDH_SPEC=1) or interpreted, constants from the lane-constant table."""
    ref = seq_reference()
    want = [ref[shape_const(p)] for p in range(N_QUERIES)]
    assert sum(len(w) for w in want) > 5000 and len({tuple(w) for w in ref.values()}) == 13
    app = pair_app(fc.GEN_DEF + " " + " ".join(seq_query(p, shape_const(p)) for p in range(N_QUERIES)),
                   debug=f"SDH_SPEC={spec}")
    step = N_EVENTS // N_PUSH
    for lo in range(0, N_EVENTS, step):
        app.send("S", EVENTS[lo:lo + step], [fc.TS0 + k for k in range(lo, lo + step)])
    got = [[] for _ in range(N_QUERIES)]
    for m in app.matches:
        assert m[3][1][0] == m[3][0][0] + 1
        got[m[0]].append(m[3][0][0])
    assert got == want
    st = app.engine.a.stats()
    assert plan_counts(app.engine.a) == {"K_seq": N_QUERIES} and (st.spec_kernels > 0) == (spec == "1")


# ---- 9. snapshot ----
@pytest.mark.parametrize("kind", ["T1", "T3"])
def test_snapshot_of_a_function_bearing_engine(kind):
    """The filters live in the program blob: a function-bearing engine snapshotted mid-stream and
    restored into a fresh engine continues to the matches of an uninterrupted run."""
    from siddhi_amd.engine import HipEngine
    f_src, _ = fc.twin_queries(kind, 65)
    rows, ts = fc.twin_events(kind, 1000)
    probe = App(f_src, engine_factory=lambda blob: None)
    types = [s.attr_types for s in probe.ir.streams]
    make = lambda blob: HipEngine(blob, stream_types=types)  # noqa: E731
    whole, first, second = App(f_src, make), App(f_src, make), App(f_src, make)
    for lo in range(0, 1000, 250):
        whole.send("S", rows[lo:lo + 250], ts[lo:lo + 250])
    for lo in (0, 250):
        first.send("S", rows[lo:lo + 250], ts[lo:lo + 250])
    second.engine.restore(first.engine.snapshot())
    second.dictionary, second._strings_sent = first.dictionary, first._strings_sent
    for lo in (500, 750):
        second.send("S", rows[lo:lo + 250], ts[lo:lo + 250])
    n = len(first.matches)
    assert 0 < n < len(whole.matches)
    assert first.matches + second.matches == whole.matches
