"""K_chain's general predicates on the device: filters with or / not / is null / arithmetic, compares
of computed values and several capture-reading conjuncts in one state run as residual programs
(siddhi_amd/csrc/chain_pred.h) inside nfa_chain.hip's two kernels, against the CPU oracle push by push.

Every case asserts that its queries run on K_chain (stats().plan_queries[2]) and that the oracle
itself produces the matches or reaches the live-partial count the case is about.
"""
import ctypes
import functools

import numpy as np
import pytest

import chain_host as ch
from harness import App, decode_matches, oracle_lib
from select_host import assert_cells_equal, reference_cells

pytestmark = pytest.mark.gpu

SDH_FLAG_DEVICE_MATCHES, SDH_FLAG_NO_RATCHET, SDH_FLAG_FORCE_GEN = 1, 2, 4


def hip_app(src, **kw):
    app = App(src, engine_factory=lambda blob: None)
    from siddhi_amd.engine import HipEngine
    app.engine = HipEngine(app.blob, stream_types=[s.attr_types for s in app.ir.streams], **kw)
    return app


def oracle_live(o):
    return int(oracle_lib().oracle_live_partials(o.engine.h))


def f32_words(x):
    return np.asarray(x, np.float32).view(np.uint32).astype(np.int64)


def take(app):
    return app.engine.take_matches(lambda q: len(app.ir.queries[q].states))


def push_both(o, g, stream, ts, vals, nulls=None):
    """One push of the same events into the oracle and the engine; returns the oracle's matches after
    asserting that the engine delivered the same ones in the same order."""
    si = o.ir.stream_index(stream)
    ts = np.asarray(ts, np.int64)
    vals = np.ascontiguousarray(vals, np.int64).reshape(len(ts), -1)
    o.engine.send(si, ts, vals, nulls)
    g.engine.send(si, ts, vals, nulls)
    om, gm = take(o), take(g)
    assert gm == om, f"{len(gm)} GPU matches, {len(om)} oracle matches"
    return om


# ---- 1. the seeded app: every residual opcode over the typed stream, through every table form ----

def typed_pred_source():
    qs = [ch.TYPED_STREAM]
    for k, f in enumerate(ch.pred_filters()):
        qs.append(f"@info(name='p{k}') from every e1=T -> e2=T[{f}] within 40 milliseconds "
                  f"select e1.i as x insert into O;")
    return " ".join(qs), len(ch.pred_filters())


def typed_pushes(mode):
    rows = ch.typed_events(200 if mode == "single" else 460)
    sizes = [1] if mode == "single" else [1, 63, 64, 65, 130]
    out, k, j = [], 0, 0
    while k < len(rows):
        n = min(sizes[j % len(sizes)], len(rows) - k)
        out.append((rows[k:k + n], [1000 + x for x in range(k, k + n)]))
        k += n
        j += 1
    return out


@functools.lru_cache(maxsize=None)
def typed_reference(mode):
    """The oracle's matches per push, computed once per push pattern."""
    src, _ = typed_pred_source()
    o = App(src)
    per_push = []
    for rows, ts in typed_pushes(mode):
        before = len(o.matches)
        o.send("T", rows, ts)
        per_push.append(o.matches[before:])
    return per_push


TABLES = {"64": dict(partials=64), "128": dict(partials=128), "256": dict(partials=256), "512": dict(partials=512),
          "growing": dict(), "paged": dict(debug={"SDH_CHAIN_PAGED": 1})}


@pytest.mark.parametrize("mode", ["single", "blocks"])
@pytest.mark.parametrize("table", list(TABLES))
def test_seeded_predicates_on_k_chain(table, mode):
    src, n = typed_pred_source()
    g = hip_app(src, **TABLES[table])
    assert n >= 40 and g.engine.stats().plan_queries[2] == n
    want = typed_reference(mode)
    assert sum(len(m) for m in want) > 1000
    for (rows, ts), om in zip(typed_pushes(mode), want):
        before = len(g.matches)
        g.send("T", rows, ts)
        assert g.matches[before:] == om


# ---- 2. several capture-reading conjuncts in one state ----

def test_several_capture_reading_conjuncts_in_one_state():
    """`s == e1.s and p > e1.p` (and a third, `v != e1.v`): every conjunct must hold. The events give each
    one-conjunct query a different match set on the oracle, so a dropped conjunct cannot pass.
    (Before the partial residual the kernels read a state's first capture-reading atom only: on these
    events the engine then delivered 112 matches more than the oracle.)"""
    conj = {"a": "s == e1.s", "b": "p > e1.p", "c": "v != e1.v", "ab": "s == e1.s and p > e1.p",
            "abc": "s == e1.s and p > e1.p and v != e1.v", "ba": "p > e1.p and s == e1.s"}
    src = "define stream S (s string, p float, v int); " + " ".join(
        f"@info(name='{k}') from every e1=S -> e2=S[{f}] within 30 milliseconds select e1.v as x insert into O;"
        for k, f in conj.items())
    o, g = App(src), hip_app(src)
    pq = g.engine.stats().plan_queries
    assert pq[0] + pq[1] + pq[2] == len(conj) and pq[2] >= 5  # (`p > e1.p` alone is K_ratchet's)
    rng = np.random.default_rng(2)
    n = 300
    rows = [[str(rng.choice(["x", "y", "z"])), float(np.float32(rng.uniform(0, 100))), int(rng.integers(0, 3))]
            for _ in range(n)]
    for k in range(0, n, 50):
        o.send("S", rows[k:k + 50], list(range(k, k + 50)))
        g.send("S", rows[k:k + 50], list(range(k, k + 50)))
    sets = {k: {m[3] for m in o.matches if m[0] == o.ir.query_index(k)} for k in conj}
    assert len({frozenset(s) for k, s in sets.items() if k != "ba"}) == 5 and sets["ab"] == sets["ba"]
    assert all(len(s) > 100 for s in sets.values())
    assert g.matches == o.matches


# ---- 3. three and four states over two streams ----

def test_three_and_four_states_over_two_streams():
    src = ("define stream A (v int, p float); define stream B (v int, p float); "
           "@info(name='q3') from every e1=A[p > 10] -> e2=B[p > e1.p * 1.01 or v == e1.v] -> e3=A[v + e1.v > e2.v] "
           "within 300 milliseconds select e1.v as a insert into O; "
           "@info(name='q4') from every e1=A -> e2=B[v > e1.v] -> e3=A[v + e1.v > e2.v] -> e4=B[v * 2 > e3.v] "
           "within 200 milliseconds select e1.v as a insert into O; "
           "@info(name='once') from e1=A[p > 50] -> e2=B[p * 2 < e1.p] select e1.v as a insert into O; "
           "@info(name='plain') from every e1=A[v > 50] -> e2=B[v < e1.v] within 100 milliseconds "
           "select e1.v as a insert into O; "
           "@info(name='ratchet') from every e1=A[v > 0] -> e2=A[p > e1.p] within 50 milliseconds "
           "select e1.v as a insert into O;")
    o, g = App(src), hip_app(src)
    pq = g.engine.stats().plan_queries
    assert pq[0] == 1 and pq[2] == 4
    rng = np.random.default_rng(11)
    t = 0
    by_q = {}
    for k in range(24):
        stream = "A" if k % 2 == 0 else "B"
        n = [90, 64, 130, 1][k % 4]
        v = rng.integers(0, 60, n).astype(np.int64)
        p = rng.uniform(0, 100, n) if stream == "A" else rng.uniform(0, 60, n)
        for m in push_both(o, g, stream, t + np.arange(n), np.stack([v, f32_words(p)], 1)):
            by_q[m[0]] = by_q.get(m[0], 0) + 1
        t += n
    count = {name: by_q.get(o.ir.query_index(name), 0) for name in ("q3", "q4", "once", "plain", "ratchet")}
    assert count["once"] == 1  # (no `every`: its one match consumed the seed)
    assert count["q3"] > 300 and count["q4"] > 300 and count["plain"] > 100 and count["ratchet"] > 100, count
    assert g.engine.stats().pool_regrows >= 1


# ---- 4. growth through every form with a residual ----

def cross_stream_pushes(seed=7):
    """(stream, ts, words) pushes: A opens partials far faster than B's low prices complete them, in
    pushes of 1, 63, 64, 65 and 500 events (the pattern of test_gpu_chain_grow.cross_stream_pushes)."""
    rng = np.random.default_rng(seed)
    sizes = [1, 63, 64, 65, 500]
    t = 0
    out = []
    for k in range(15):
        n = sizes[k % 5]
        out.append(("A", t + np.arange(n), f32_words(rng.uniform(0, 100, n))))
        t += n
        nb = min(sizes[(k + 2) % 5] if k % 3 == 0 else 1, 65)
        out.append(("B", t + np.arange(nb), f32_words(rng.uniform(0, 22, nb))))
        t += nb
    return out, t, rng


def test_growth_through_every_form_with_a_residual():
    src = ("define stream A (p float); define stream B (p float); "
           "@info(name='q') from every e1=A[p > 10] -> e2=B[p > e1.p * 1.0] within 4000 milliseconds "
           "select e1.p as a insert into O;")
    o, g = App(src), hip_app(src)
    assert g.engine.stats().plan_queries[2] == 1
    pushes, t, rng = cross_stream_pushes()
    marks = set()
    for stream, ts, words in pushes:
        push_both(o, g, stream, ts, words)
        marks |= {m for m in (64, 128, 256, 512, 1024) if oracle_live(o) > m}
    assert marks == {64, 128, 256, 512, 1024}
    assert abs(g.engine.stats().live_partials - oracle_live(o)) <= 1  # (the oracle may count the seed)
    assert g.engine.stats().pool_regrows >= 3
    # the burst: rising prices complete most of the table, leaving a partly filled last page
    nb = 300
    m = push_both(o, g, "B", t + np.arange(nb), f32_words(np.linspace(10, 93, nb)))
    assert len(m) > 1000
    left = g.engine.stats().live_partials
    assert 0 < left < 300 and left % 64 != 0 and abs(left - oracle_live(o)) <= 1
    t += nb
    push_both(o, g, "A", t + np.arange(70), f32_words(rng.uniform(0, 100, 70)))
    m = push_both(o, g, "B", t + 70 + np.arange(5), f32_words([100.0] * 5))
    assert len(m) > 50 and g.engine.stats().live_partials == 0 and oracle_live(o) <= 1


# ---- 5. past K_gen's pools ----

def test_more_open_partials_than_k_gen_holds():
    """4,500 open partials of one arithmetic query: K_gen's pools end at 4,096 StateEvents per instance."""
    src = ("define stream A (p float); define stream B (p float); "
           "@info(name='q') from every e1=A -> e2=B[p > e1.p * 1.05] select e1.p as a insert into O;")
    o, g = App(src), hip_app(src)
    assert g.engine.stats().plan_queries[2] == 1
    rng = np.random.default_rng(9)
    push_both(o, g, "A", np.arange(4500), f32_words(rng.uniform(10, 100, 4500)))
    push_both(o, g, "B", [4500], f32_words([0.0]))  # (completes nothing; the oracle's lists catch up)
    assert oracle_live(o) > 4096 and g.engine.stats().live_partials == 4500
    m = push_both(o, g, "B", 4501 + np.arange(64), f32_words(np.linspace(5, 120, 64)))
    assert len(m) == 4500 and g.engine.stats().live_partials == 0


# ---- 6. chunked equals unchunked ----

def gate_like_events(n, seed, t0=0):
    rng = np.random.default_rng(seed)
    closer = rng.random(n) < 0.02
    v = np.where(closer, -1, 1).astype(np.int64)
    w = np.where(closer, rng.integers(0, 300, n), rng.integers(0, 1000, n)).astype(np.int64)
    return t0 + np.arange(n, dtype=np.int64), np.stack([v, w], 1)


@pytest.mark.parametrize("unordered", [False, True])
def test_chunked_equals_unchunked_with_a_residual(unordered):
    src = ("define stream S (v int, w int); @info(name='q') from every e1=S[v > 0] -> "
           "e2=S[v < 0 and w > e1.w + 0] within 1500 milliseconds select e1.w as a insert into O;")
    o = App(src)
    gc = hip_app(src, chunk_events=512)
    gu = hip_app(src, chunk_events=0)
    assert gc.engine.stats().plan_queries[2] == 1 and gu.engine.stats().plan_queries[2] == 1
    ts, vals = gate_like_events(8000, 3)
    if unordered:
        ts = ts.copy()
        ts[7000:7100] -= 5000
    total = 0
    for a, b in ((0, 3000), (3000, 8000)):
        o.engine.send(0, ts[a:b], vals[a:b], None)
        om = take(o)
        for g in (gc, gu):
            g.engine.send(0, ts[a:b], vals[a:b], None)
            assert take(g) == om
        total += len(om)
    assert total > 2000
    assert gc.engine.stats().live_partials == gu.engine.stats().live_partials > 512


# ---- 7. a tile residual on the start state of a ratchet-shaped query ----

def test_tile_residual_on_the_start_state_runs_on_k_chain():
    src = ("define stream S (v int, w int); @info(name='q') from every e1=S[v * 2 > w or e1.w is null] -> "
           "e2=S[w > e1.w] within 50 milliseconds select e1.w as a insert into O;")
    o, g = App(src), hip_app(src)
    pq = g.engine.stats().plan_queries
    assert pq[0] == 0 and pq[1] == 0 and pq[2] == 1
    rng = np.random.default_rng(4)
    t = 0
    total = 0
    for n in (1, 63, 64, 65, 130, 200):
        vals = np.stack([rng.integers(0, 100, n), rng.integers(0, 150, n)], 1).astype(np.int64)
        nulls = np.zeros((n, 2), np.uint8)
        nulls[:, 1] = rng.random(n) < 0.1
        total += len(push_both(o, g, "S", t + np.arange(n), vals, nulls))
        t += n
    # (523 events; about two in three pass e1's filter, and a partial matches at most once)
    assert total > 200


# ---- 8. delivery ----

RESID_SRC = ("define stream S (v int, w int); "
             "@info(name='q') from every e1=S[v > 0] -> e2=S[w > e1.w * 2 or v + e1.v == 0] within 40 milliseconds "
             "select e1.w as a, e2.w - e1.w as d, e2.v as v insert into O;")


def resid_events(n=1500, seed=21):
    rng = np.random.default_rng(seed)
    return (np.arange(n, dtype=np.int64),
            np.stack([rng.integers(-3, 4, n), rng.integers(0, 1000, n)], 1).astype(np.int64))


def _host(ptr, n, dtype):
    out = np.zeros(n, dtype)
    if n:
        lib = ctypes.CDLL("libamdhip64.so")
        lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        assert lib.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
    return out


def test_device_records_of_a_residual_query():
    ts, vals = resid_events()
    normal = hip_app(RESID_SRC)
    assert normal.engine.stats().plan_queries[2] == 1
    o = App(RESID_SRC)
    want = push_both(o, normal, "S", ts, vals)
    want = sorted((q, t, slots[0][0], slots[1][0]) for q, _, t, slots in want)
    assert len(want) > 500
    dev = hip_app(RESID_SRC, flags=SDH_FLAG_DEVICE_MATCHES)
    assert dev.engine.stats().plan_queries[2] == 1
    dev.engine.send(0, ts, vals, None)
    rec = dev.engine.poll_records()
    assert rec.c_n == len(want) and rec.c_words == 4
    offs = _host(rec.c_off, rec.c_items, np.int64)
    cnts = _host(rec.c_count, rec.c_items, np.int64)
    assert int(cnts.sum()) == rec.c_n
    got = []
    for off, c in zip(offs.tolist(), cnts.tolist()):
        for r in _host(rec.c_base + off * rec.c_words * 8, c * rec.c_words, np.int64).reshape(-1, rec.c_words):
            got.append((int(r[0]), int(r[1]), int(r[2]), int(r[3])))
    assert sorted(got) == want


def test_rows_of_a_residual_query():
    """retain_events + poll_rows: the device selector's rows of a residual query's matches against
    selector.project over the twin's tuples."""
    ts, vals = resid_events()
    a, b = hip_app(RESID_SRC), hip_app(RESID_SRC)
    b.engine.retain_events(2048)
    for app in (a, b):
        app.log.append(0, ts, vals, None)
        app.engine.send(0, ts, vals, None)
    q, k, mts, off, words, seq, tb = a.engine.poll(with_seq=True)
    rq, rts, rseq, cells, nulls = b.engine.poll_rows()
    assert len(q) > 500 and np.array_equal(rq, q) and np.array_equal(rts, mts) and np.array_equal(rseq, seq)
    matches = decode_matches(len(q), q, k, mts, off, words, lambda i: 2)
    assert cells.shape == (3, len(q))
    assert_cells_equal(a, matches, cells, nulls, *reference_cells(a, matches, 3))


# ---- 9. snapshot ----

def test_snapshot_across_a_paged_residual_table():
    from siddhi_amd.engine import EngineError
    src = ("define stream A (p float); define stream B (p float); "
           "@info(name='q') from every e1=A[p > 10] -> e2=B[p > e1.p + 1 or e2.p is null] select e1.p as a insert into O;")
    o, a = App(src), hip_app(src)
    assert a.engine.stats().plan_queries[2] == 1
    rng = np.random.default_rng(5)
    push_both(o, a, "A", np.arange(800), f32_words(rng.uniform(0, 100, 800)))
    push_both(o, a, "B", [800], f32_words([0.0]))
    assert 650 <= oracle_live(o) <= 760
    snap = a.engine.snapshot()
    b = hip_app(src)  # a fresh default engine: its tables start at 128
    b.engine.restore(snap)
    assert b.engine.stats().live_partials == a.engine.stats().live_partials >= 650
    t = 801
    for stream, n, hi in (("B", 65, 40), ("A", 200, 100), ("B", 30, 100)):
        ts = t + np.arange(n)
        words = f32_words(rng.uniform(0, hi, n))
        om = push_both(o, a, stream, ts, words)
        b.engine.send(b.ir.stream_index(stream), ts, words.reshape(n, 1), None)
        assert take(b) == om
        t += n
    # the same program planned without residuals (the query on K_gen) is another program to a snapshot
    old = hip_app(src, debug={"SDH_CHAIN_PRED": 0})
    assert old.engine.stats().plan_queries[2] == 0
    old.engine.send(0, np.arange(10), f32_words(rng.uniform(20, 100, 10)).reshape(10, 1), None)
    c = hip_app(src)
    with pytest.raises(EngineError) as ei:
        c.engine.restore(old.engine.snapshot())
    assert "snapshot of a different program" in str(ei.value)
    o2 = App(src)  # ... and the refused engine is as it was: usable
    push_both(o2, c, "A", np.arange(10), f32_words(np.linspace(20, 60, 10)))
    assert len(push_both(o2, c, "B", [10], f32_words([50.0]))) > 3


# ---- 10. what still declines ----

def test_declines_stay_off_k_chain_and_exact():
    deep = "i + (i + (i + (i + (i + (i + (i + e1.i)))))) > 0"
    long_ = " or ".join(f"i + {k} > e1.i" for k in range(9))
    src = ch.TYPED_STREAM + " " + " ".join(
        f"@info(name='{n}') from every e1=T -> e2=T[{f}] within 40 milliseconds select e1.i as x insert into O;"
        for n, f in (("deep", deep), ("long", long_), ("streamnull", "e1 is null or i > e1.i")))
    o, g = App(src), hip_app(src)
    assert g.engine.stats().plan_queries[2] == 0
    rows = ch.typed_events(200)
    for k in range(0, 200, 40):
        o.send("T", rows[k:k + 40], [1000 + x for x in range(k, k + 40)])
        g.send("T", rows[k:k + 40], [1000 + x for x in range(k, k + 40)])
    assert len(o.matches) > 300  # (of at most 600: three queries, 200 partials each, one match per partial)
    assert g.matches == o.matches
