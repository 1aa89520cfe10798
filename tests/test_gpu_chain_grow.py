"""K_chain tables that grow (sdh_config.partials_per_inst == 0) and the paged form of the kernel past
512 partials per query (nfa_chain.hip), against the CPU oracle push by push.

Every case asserts that the oracle itself reaches the live-partial count the case is about, so a change
of a generator cannot quietly shrink it, and that the queries run on K_chain (stats().plan_queries[2]).
"""
import ctypes

import numpy as np
import pytest

from harness import App, oracle_lib

pytestmark = pytest.mark.gpu

OVERFLOW_SRC = ("define stream S (v int); @info(name='q') from every e1=S[v > 0] -> e2=S[v < 0] "
                "select e1.v as a insert into O;")


def hip_app(src, **kw):
    app = App(src, engine_factory=lambda blob: None)
    from siddhi_amd.engine import HipEngine
    app.engine = HipEngine(app.blob, stream_types=[s.attr_types for s in app.ir.streams], **kw)
    return app


def oracle_live(o):
    """Entries of the oracle's pending lists. A partial joins its state's list at the next event of that
    state's stream, so between pushes the count is a lower bound of the partials the engine holds."""
    return int(oracle_lib().oracle_live_partials(o.engine.h))


def f32_words(x):
    return np.asarray(x, np.float32).view(np.uint32).astype(np.int64)


def take(app):
    return app.engine.take_matches(lambda q: len(app.ir.queries[q].states))


def push_both(o, g, stream, ts, vals):
    """One push of the same events into the oracle and the engine; returns the oracle's matches after
    asserting that the engine delivered the same ones in the same order."""
    si = o.ir.stream_index(stream)
    ts = np.asarray(ts, np.int64)
    vals = np.ascontiguousarray(vals, np.int64).reshape(len(ts), -1)
    o.engine.send(si, ts, vals, None)
    g.engine.send(si, ts, vals, None)
    om, gm = take(o), take(g)
    assert gm == om, f"{len(gm)} GPU matches, {len(om)} oracle matches"
    return om


def test_default_engine_has_no_wall():
    """The stream of test_gpu_chain.test_lane_capacity_overflow_is_loud on a default engine: 200 open
    partials (the tables start at 128), then one event that completes them all."""
    o = App(OVERFLOW_SRC)
    g = hip_app(OVERFLOW_SRC)
    assert g.engine.stats().plan_queries[2] == 1
    push_both(o, g, "S", np.arange(200), np.ones(200, np.int64))
    assert oracle_live(o) >= 199
    assert g.engine.stats().live_partials == 200
    m = push_both(o, g, "S", [200], [-1])
    assert len(m) == 200
    st = g.engine.stats()
    assert st.pool_regrows >= 1 and st.live_partials == 0


def cross_stream_pushes(seed=7):
    """(stream, ts, words) pushes of the cross-stream case: A opens partials far faster than B's low
    prices complete them, in pushes of 1, 63, 64, 65 and 500 events; at the end a burst of B."""
    rng = np.random.default_rng(seed)
    sizes = [1, 63, 64, 65, 500]
    t = 0
    out = []
    for k in range(15):
        n = sizes[k % 5]
        ts = t + np.arange(n)
        t += n
        out.append(("A", ts, f32_words(rng.uniform(0, 100, n))))
        nb = sizes[(k + 2) % 5] if k % 3 == 0 else 1
        nb = min(nb, 65)
        ts = t + np.arange(nb)
        t += nb
        out.append(("B", ts, f32_words(rng.uniform(0, 22, nb))))
    return out, t, rng


def test_growth_through_every_form():
    src = ("define stream A (p float); define stream B (p float); "
           "@info(name='q') from every e1=A[p > 10] -> e2=B[p > e1.p] within 4000 milliseconds "
           "select e1.p as a insert into O;")
    o = App(src)
    g = hip_app(src)
    assert g.engine.stats().plan_queries[2] == 1
    pushes, t, rng = cross_stream_pushes()
    marks = set()
    for stream, ts, words in pushes:
        push_both(o, g, stream, ts, words)
        marks |= {m for m in (64, 128, 256, 512, 1024) if oracle_live(o) > m}
    assert marks == {64, 128, 256, 512, 1024} and 1300 <= oracle_live(o) <= 1700
    assert abs(g.engine.stats().live_partials - oracle_live(o)) <= 1  # (the oracle may count the seed)
    assert g.engine.stats().pool_regrows >= 3  # 256, 512, and at least one paged size
    # the burst: rising prices complete most of the table, leaving a partly filled last page
    nb = 300
    m = push_both(o, g, "B", t + np.arange(nb), f32_words(np.linspace(10, 93, nb)))
    assert len(m) > 1000
    left = g.engine.stats().live_partials
    assert 0 < left < 300 and left % 64 != 0 and abs(left - oracle_live(o)) <= 1
    # and the drained table goes on working
    t += nb
    push_both(o, g, "A", t + np.arange(70), f32_words(rng.uniform(0, 100, 70)))
    m = push_both(o, g, "B", t + 70 + np.arange(5), f32_words([100.0] * 5))
    assert len(m) > 50 and g.engine.stats().live_partials == 0 and oracle_live(o) <= 1


def test_middle_states_paged_beside_a_small_query():
    """Three states over two streams with captures: the partials wait at states 1 and 2. The second
    query never grows, but shares the grown tables."""
    src = ("define stream A (v int, p float); define stream B (v int, p float); "
           "@info(name='q1') from every e1=A[p > 10] -> e2=B[p > e1.p] -> e3=A[v == e1.v] within 5000 "
           "milliseconds select e1.v as a insert into O; "
           "@info(name='q2') from e1=A[p > 50] -> e2=B[p < e1.p] select e1.v as a insert into O;")
    o = App(src)
    g = hip_app(src)
    assert g.engine.stats().plan_queries[2] == 2
    rng = np.random.default_rng(11)
    q2 = o.ir.query_index("q2")
    t, total, q2_matches = 0, 0, 0
    for k in range(40):
        stream = "A" if k % 2 == 0 else "B"
        n = [90, 64, 130, 1][k % 4]
        v = rng.integers(0, 60, n).astype(np.int64)
        p = rng.uniform(0, 100, n) if stream == "A" else rng.uniform(0, 60, n)
        m = push_both(o, g, stream, t + np.arange(n), np.stack([v, f32_words(p)], 1))
        total += len(m)
        q2_matches += sum(1 for x in m if x[0] == q2)
        t += n
    live = oracle_live(o)
    assert live > 700 and total > 300  # (e3 completes matches: state 2 is populated)
    assert q2_matches == 1  # (no `every`: its one match consumed the seed)
    assert g.engine.stats().live_partials >= live - 2  # (the oracle counts seeds)
    assert g.engine.stats().pool_regrows >= 1


def gate_like_events(n, seed, t0=0):
    """One-stream events for `every e1=S[v > 0] -> e2=S[v < 0 and w > e1.w]`: one event in fifty
    completes the open partials below its (low) w."""
    rng = np.random.default_rng(seed)
    closer = rng.random(n) < 0.02
    v = np.where(closer, -1, 1).astype(np.int64)
    w = np.where(closer, rng.integers(0, 300, n), rng.integers(0, 1000, n)).astype(np.int64)
    return t0 + np.arange(n, dtype=np.int64), np.stack([v, w], 1)


CHUNK_SRC = ("define stream S (v int, w int); @info(name='q') from every e1=S[v > 0] -> "
             "e2=S[v < 0 and w > e1.w] within 1500 milliseconds select e1.w as a insert into O;")


@pytest.mark.parametrize("unordered", [False, True])
def test_chunked_equals_unchunked_at_paged_size(unordered):
    from siddhi_amd.engine import SDH_FLAG_NO_RATCHET
    o = App(CHUNK_SRC)
    gc = hip_app(CHUNK_SRC, chunk_events=512, flags=SDH_FLAG_NO_RATCHET)
    gu = hip_app(CHUNK_SRC, chunk_events=0, flags=SDH_FLAG_NO_RATCHET)
    assert gc.engine.stats().plan_queries[2] == 1 and gu.engine.stats().plan_queries[2] == 1
    ts, vals = gate_like_events(8000, 3)
    if unordered:  # as test_gpu_chain.test_unordered_timestamps_fall_back_exactly
        ts = ts.copy()
        ts[7000:7100] -= 5000
    total = 0
    for a, b in ((0, 3000), (3000, 8000)):
        o.engine.send(0, ts[a:b], vals[a:b], None)
        om = take(o)
        assert oracle_live(o) > 512
        for g in (gc, gu):
            g.engine.send(0, ts[a:b], vals[a:b], None)
            assert take(g) == om
        total += len(om)
    assert total > 2000
    assert gc.engine.stats().live_partials == gu.engine.stats().live_partials > 512


TYPED_STREAM = "define stream T (i int, l long, f float, d double, b bool, s string);"
NUMERIC = ["i", "l", "f", "d"]
OPS = ["==", "!=", ">", ">=", "<", "<="]


def typed_events(n=400, seed=3):
    """Adversarial values for Java's typed compares: int->float and long->float/double rounding
    boundaries, signed zeros, NaN, infinities, extremes; some nulls."""
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


def typed_app_source():
    qs = [TYPED_STREAM]
    n = 0
    for a in NUMERIC:
        for b in NUMERIC:
            for op in OPS:
                qs.append(f"@info(name='u{n}') from every e1=T[{a} {op} {b}] select e1.i as x insert into O;")
                qs.append(f"@info(name='x{n}') from every e1=T -> e2=T[{a} {op} e1.{b}] "
                          f"select e1.i as x insert into O;")
                n += 1
    for op in ("==", "!="):
        qs.append(f"@info(name='bb{op}') from every e1=T -> e2=T[b {op} e1.b] select e1.i as x insert into O;")
        qs.append(f"@info(name='ss{op}') from every e1=T -> e2=T[s {op} e1.s and s {op} 'b'] "
                  f"select e1.i as x insert into O;")
    qs.append("@info(name='flag') from every e1=T[b] select e1.i as x insert into O;")
    qs.append("@info(name='consts') from every e1=T[f > 16777216 and l < 3.0f and d >= 7L] "
              "select e1.i as x insert into O;")
    return " ".join(qs)


def test_forced_paged_typed_compare_semantics():
    """The app and events of test_gpu_chain.test_typed_compare_semantics with the paged form forced at
    every size: nulls, NaN and the promotion domains through the paged kernel's per-partial compares."""
    src = typed_app_source()
    o = App(src)
    g = hip_app(src, debug={"SDH_CHAIN_PAGED": 1})
    assert g.engine.stats().plan_queries[2] > 100
    for k, row in enumerate(typed_events()):
        o.send("T", [row], [1000 + k])
        g.send("T", [row], [1000 + k])
    assert len(o.matches) > 1000
    assert g.matches == o.matches


MIXED_SRC = ("define stream S (v int, w int); "
             "@info(name='chain') from every e1=S[v > 0] -> e2=S[v < 0] select e1.v as a insert into O; "
             "@info(name='gen') from every e1=S[w > 900] -> e2=S[w > 500] and e3=S[w < 200] within 60 "
             "milliseconds select e1.w as a insert into O; "
             "@info(name='ratchet') from every e1=S[v > 0] -> e2=S[w > e1.w] within 50 milliseconds "
             "select e1.w as a insert into O;")


def mixed_events():
    rng = np.random.default_rng(21)
    n = 300
    v = np.ones(n, np.int64)
    v[-1] = -1  # the last event completes the chain query's 299 partials
    return np.arange(n, dtype=np.int64), np.stack([v, rng.integers(0, 1000, n).astype(np.int64)], 1)


def test_growth_inside_a_mixed_push():
    """The chain query overflows its tables inside a push that K_gen and K_ratchet queries share: the
    re-run is K_chain's alone, so the other plans' matches appear once."""
    o = App(MIXED_SRC)
    g = hip_app(MIXED_SRC)
    pq = g.engine.stats().plan_queries
    assert pq[0] == 1 and pq[2] == 1 and pq[5] + pq[6] == 1
    ts, vals = mixed_events()
    m = push_both(o, g, "S", ts, vals)
    by_q = {name: sum(1 for x in m if x[0] == o.ir.query_index(name)) for name in ("chain", "gen", "ratchet")}
    assert by_q["chain"] == 299 and by_q["gen"] > 5 and by_q["ratchet"] > 100
    assert g.engine.stats().pool_regrows >= 1


def _host(ptr, n, dtype):
    out = np.zeros(n, dtype)
    if n:
        lib = ctypes.CDLL("libamdhip64.so")
        lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        assert lib.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
    return out


def test_device_records_after_growth():
    """The same overflowing push in device-record mode: the K_chain segments hold the matches of the
    run that succeeded, once each."""
    from siddhi_amd.engine import SDH_FLAG_DEVICE_MATCHES
    normal = hip_app(MIXED_SRC)
    ts, vals = mixed_events()
    normal.engine.send(0, ts, vals, None)
    chain_q = normal.ir.query_index("chain")
    want = sorted((q, t, slots[0][0], slots[1][0]) for q, _, t, slots in take(normal) if q == chain_q)
    assert len(want) == 299
    dev = hip_app(MIXED_SRC, flags=SDH_FLAG_DEVICE_MATCHES)
    assert dev.engine.stats().plan_queries[2] == 1
    dev.engine.send(0, ts, vals, None)
    rec = dev.engine.poll_records()
    assert rec.c_n == 299 and rec.c_words == 4
    offs = _host(rec.c_off, rec.c_items, np.int64)
    cnts = _host(rec.c_count, rec.c_items, np.int64)
    assert int(cnts.sum()) == rec.c_n
    got = []
    for off, c in zip(offs.tolist(), cnts.tolist()):
        for r in _host(rec.c_base + off * rec.c_words * 8, c * rec.c_words, np.int64).reshape(-1, rec.c_words):
            got.append((int(r[0]), int(r[1]), int(r[2]), int(r[3])))
    assert sorted(got) == want
    assert dev.engine.stats().pool_regrows >= 1


def test_snapshot_across_growth():
    from siddhi_amd.engine import EngineError
    src = ("define stream A (p float); define stream B (p float); "
           "@info(name='q') from every e1=A[p > 10] -> e2=B[p > e1.p] select e1.p as a insert into O;")
    o = App(src)
    a = hip_app(src)
    assert a.engine.stats().plan_queries[2] == 1
    rng = np.random.default_rng(5)
    push_both(o, a, "A", np.arange(800), f32_words(rng.uniform(0, 100, 800)))
    push_both(o, a, "B", [800], f32_words([0.0]))  # (completes nothing; the oracle's lists catch up)
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
    assert b.engine.stats().live_partials == a.engine.stats().live_partials
    fixed = hip_app(src, partials=64)
    with pytest.raises(EngineError) as ei:
        fixed.engine.restore(snap)
    assert ei.value.code == -1
