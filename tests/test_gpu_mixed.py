"""Interleaved pushes (sdh_engine_push_mixed; DESIGN.md §3.2 "Interleaved pushes") on the GPU.

Every call is compared three ways: against the CPU oracle fed the call's maximal same-part runs (what
the call is defined against), against a second engine that takes the same calls under SDH_MIX_SPLIT=1
(the engine's own run pushes), and on sdh_stats (live_partials, events, pattern_events, matches). Each
test asserts through debug_mixed_pushes() that its engines took the path it is about, and a floor on
the oracle's match count (read off the oracle when the seeds and constants were chosen), so an empty
comparison cannot pass.
"""
import ctypes

import numpy as np
import pytest

from harness import App, oracle_lib
from siddhi_amd.engine import SDH_FLAG_DEVICE_MATCHES, SDH_FLAG_NO_RATCHET, EngineError, mixed_runs

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -2


def f32_words(x):
    return np.asarray(x, np.float32).view(np.uint32).astype(np.int64)


def hip_app(src, **kw):
    app = App(src, engine_factory=lambda blob: None)
    from siddhi_amd.engine import HipEngine
    app.engine = HipEngine(app.blob, stream_types=[s.attr_types for s in app.ir.streams], **kw)
    return app


def take(app):
    return app.engine.take_matches(lambda q: len(app.ir.queries[q].states))


def oracle_runs(o, parts, order):
    """The call's runs into the oracle (and its event log, which the row checks read)."""
    for p, off, n in mixed_runs([len(x[1]) for x in parts], order):
        stream, ts, vals, nulls = parts[p]
        si = o.ir.stream_index(stream)
        nl = None if nulls is None else nulls[off:off + n]
        o.log.append(si, ts[off:off + n], vals[off:off + n], nl)
        o.engine.send(si, ts[off:off + n], vals[off:off + n], nl)


def by_index(app, parts):
    return [(app.ir.stream_index(s), ts, vals, nulls) for s, ts, vals, nulls in parts]


def call_of(order, t0, gens, rng, ts_of=None):
    """One call: part p = gens[p] = (stream, fn(rng, n) -> (words[n, attrs], nulls or None)); the events
    take their merged position as timestamp (t0 + k), or ts_of(p, positions)."""
    order = np.asarray(order, np.int32)
    parts = []
    for p, (stream, gen) in enumerate(gens):
        pos = np.flatnonzero(order == p)
        ts = (t0 + pos if ts_of is None else ts_of(p, t0 + pos)).astype(np.int64)
        vals, nulls = gen(rng, len(pos))
        vals = np.ascontiguousarray(vals, np.int64)
        if vals.ndim == 1:  # (one attribute)
            vals = vals.reshape(len(pos), 1)
        parts.append((stream, ts, vals, nulls))
    return parts, order


class Trio:
    """The oracle, an engine on the native path and one under SDH_MIX_SPLIT=1, fed alike."""

    def __init__(self, src, native=True, **kw):
        dbg = dict(kw.pop("debug", {}))
        self.o = App(src)
        self.n = hip_app(src, debug=dbg, **kw)
        self.s = hip_app(src, debug={**dbg, "SDH_MIX_SPLIT": 1}, **kw)
        self.native = native
        self.calls = 0
        self.total = 0

    def check_paths(self):
        assert self.n.engine.debug_mixed_pushes() == ((self.calls, 0) if self.native else (0, self.calls))
        assert self.s.engine.debug_mixed_pushes() == (0, self.calls)

    def check_stats(self):
        a, b = self.n.engine.stats(), self.s.engine.stats()
        assert a.live_partials == b.live_partials
        assert (a.events, a.pattern_events, a.matches) == (b.events, b.pattern_events, b.matches)

    def mixed(self, parts, order):
        oracle_runs(self.o, parts, order)
        self.n.engine.send_mixed(by_index(self.n, parts), order)
        self.s.engine.send_mixed(by_index(self.s, parts), order)
        self.calls += 1 if len(order) else 0
        om, nm, sm = take(self.o), take(self.n), take(self.s)
        assert nm == om, f"native: {len(nm)} matches, oracle {len(om)}"
        assert sm == om, f"split: {len(sm)} matches, oracle {len(om)}"
        self.check_stats()
        self.check_paths()
        self.total += len(om)
        return om

    def plain(self, stream, ts, vals, nulls=None):
        ts = np.asarray(ts, np.int64)
        vals = np.ascontiguousarray(vals, np.int64).reshape(len(ts), -1)
        for app in (self.o, self.n, self.s):
            app.engine.send(app.ir.stream_index(stream), ts, vals, nulls)
        om, nm, sm = take(self.o), take(self.n), take(self.s)
        assert nm == om and sm == om
        self.check_stats()
        self.total += len(om)
        return om


def price(lo, hi):
    return lambda rng, n: (f32_words(rng.uniform(lo, hi, n)), None)


def fixed(values):
    return lambda rng, n: (f32_words(values[:n]), None)


# ---- 1. tile edges -----------------------------------------------------------------------------------
EDGE_SRC = "define stream A (p float); define stream B (p float); " + " ".join(
    f"@info(name='q{i}') from every e1=A[p > {5 * i}] -> e2=B[p > e1.p] within 40 milliseconds "
    f"select e1.p as a, e2.p as b insert into O;" for i in range(20))
AB = [("A", price(0, 100)), ("B", price(0, 100))]


def edge_calls():
    rng = np.random.default_rng(5)
    calls, t = [], 0

    def add(order, gens=AB):
        nonlocal t
        calls.append(call_of(order, t, gens, rng))
        t += len(order)

    for n in (1, 63, 64, 65, 130):
        add(rng.integers(0, 2, n))
    add(np.arange(130) % 2)                      # ABAB...
    add([0] * 64 + [1] * 64)                     # one tile all A, then one all B
    # an A at lane 63 completed by a B at lane 0 of the next tile (the B events before it are too low)
    add([1] * 63 + [0] + [1] + [0] * 5,
        [("A", fixed([50.0] + [99.5] * 5)), ("B", fixed([1.0] * 63 + [99.0]))])
    # a partial opened at lane 10 and completed at lane 11
    add([1] * 10 + [0, 1] + [1] * 5, [("A", fixed([60.0])), ("B", fixed([2.0] * 10 + [98.0] + [3.0] * 5))])
    add([1] * 10, AB)                            # an empty part
    add([0] * 7, [("A", price(0, 100))])         # one part only
    add(rng.integers(0, 2, 65))
    return calls


def test_tile_edges():
    t = Trio(EDGE_SRC)
    assert t.n.engine.stats().plan_queries[2] == 20
    for k, (parts, order) in enumerate(edge_calls()):
        m = t.mixed(parts, order)
        if k == 7:
            assert any(x[3][0][0] + 1 == x[3][1][0] for x in m)  # lane 63 -> lane 0
        if k == 8:
            assert len(m) >= 10
    assert t.total >= 2500
    assert t.n.engine.debug_mixed_pushes() == (len(edge_calls()), 0)  # the MIX kernels ran every call


# ---- 2. three streams, up to four states -------------------------------------------------------------
THREE_SRC = (
    "define stream A (v int, p float); define stream B (v int, p float); define stream C (v int, p float); "
    "@info(name='abc') from every e1=A[p > 20] -> e2=B[p > e1.p] -> e3=C[v == e1.v] within 300 milliseconds "
    "select e1.v as a insert into O; "
    "@info(name='aba') from every e1=A[p > 30] -> e2=B[v == e1.v] -> e3=A[p > e2.p] within 300 milliseconds "
    "select e1.v as a insert into O; "
    "@info(name='abac') from every e1=A[p > 40] -> e2=B[p > e1.p] -> e3=A[p < e2.p] -> e4=C[v != e1.v] "
    "within 200 milliseconds select e1.v as a insert into O; "
    "@info(name='a') from every e1=A[p > 70] -> e2=A[v == e1.v] within 100 milliseconds select e1.v as a insert into O; "
    "@info(name='b') from e1=B[p > 50] -> e2=B[v != e1.v] select e1.v as a insert into O; "
    "@info(name='a1') from every e1=A[p > 97] select e1.v as a insert into O;")


def vp(null_rate):
    def gen(rng, n):
        vals = np.stack([rng.integers(0, 6, n).astype(np.int64), f32_words(rng.uniform(0, 100, n))], 1)
        nulls = (rng.random((n, 2)) < null_rate).astype(np.uint8)
        return vals, nulls
    return gen


def three_calls():
    rng = np.random.default_rng(9)
    gens = [("A", vp(0.05)), ("B", vp(0.05)), ("C", vp(0.0))]
    # B's clock lags A's by 150 ms and timestamps repeat across streams (two events per millisecond)
    lag = lambda p, x: x // 2 - (150 if p == 1 else 0)  # noqa: E731
    calls, t = [], 1000
    for n in (130, 64, 1, 200, 65, 63, 300):
        calls.append(call_of(rng.integers(0, 3, n), t, gens, rng, ts_of=lag))
        t += n
    return calls


def test_three_streams_four_states():
    t = Trio(THREE_SRC, flags=SDH_FLAG_NO_RATCHET)
    assert t.n.engine.stats().plan_queries[2] == 6
    for parts, order in three_calls():
        t.mixed(parts, order)
    per_query = {}
    # (the floor holds per chain, so each shape is compared on matches of its own)
    o2 = App(THREE_SRC)
    for parts, order in three_calls():
        oracle_runs(o2, parts, order)
    for m in take(o2):
        per_query[m[0]] = per_query.get(m[0], 0) + 1
    assert all(per_query.get(o2.ir.query_index(q), 0) >= f
               for q, f in (("abc", 100), ("aba", 30), ("abac", 30), ("a", 20), ("b", 1), ("a1", 5))), per_query


# ---- 3. residual programs ----------------------------------------------------------------------------
RESID_SRC = (
    "define stream A (v int, p float); define stream B (v int, p float); "
    "@info(name='r1') from every e1=A[p > 20] -> e2=B[p > e1.p * 1.05 or v == e1.v] within 60 milliseconds "
    "select e1.v as a insert into O; "
    "@info(name='r2') from every e1=A[v + 1 > 2] -> e2=B[p - e1.p > 10 and not (v == e1.v)] within 60 milliseconds "
    "select e1.v as a insert into O; "
    "@info(name='plain') from every e1=A[p > 50] -> e2=B[p > e1.p] within 60 milliseconds "
    "select e1.v as a insert into O;")


def test_residual_programs():
    t = Trio(RESID_SRC)
    assert t.n.engine.stats().plan_queries[2] == 3
    rng = np.random.default_rng(13)
    gens = [("A", vp(0.05)), ("B", vp(0.05))]
    tt = 0
    for n in (130, 65, 64, 1, 63, 200):
        t.mixed(*call_of(rng.integers(0, 2, n), tt, gens, rng))
        tt += n
    assert t.total >= 400


# ---- 4. growth ---------------------------------------------------------------------------------------
GROW_SRC = ("define stream A (p float); define stream B (p float); "
            "@info(name='q') from every e1=A[p > 10] -> e2=B[p > e1.p] select e1.p as a insert into O; "
            "@info(name='small') from every e1=A[p > 99] -> e2=B[p > e1.p] select e1.p as a insert into O;")


@pytest.mark.parametrize("opened", [200, 600])
def test_growth_inside_a_call(opened):
    """The A events of one call open more partials than the tables hold (they start at 128 per query)
    before the call's B events complete them: the launch re-runs at a larger table, part[cur] untouched."""
    t = Trio(GROW_SRC)
    rng = np.random.default_rng(opened)
    order = [0] * opened + [1] * 20 + [0] * 10 + [1] * 3
    m = t.mixed(*call_of(order, 0, [("A", price(11, 90)), ("B", price(0, 100))], rng))
    assert len(m) >= opened // 2
    assert t.n.engine.stats().pool_regrows >= 1 and t.s.engine.stats().pool_regrows >= 1
    # the grown table goes on working, through a plain push too
    t.plain("B", [2000, 2001], f32_words([95.0, 99.9]))
    t.mixed(*call_of(rng.integers(0, 2, 65), 3000, AB, rng))
    assert t.total >= opened


# ---- 5. delivery forms -------------------------------------------------------------------------------
def test_seqs_and_compact_rows():
    src = EDGE_SRC
    n, s = hip_app(src), hip_app(src, debug={"SDH_MIX_SPLIT": 1})
    n2, s2 = hip_app(src), hip_app(src, debug={"SDH_MIX_SPLIT": 1})
    total = 0
    for parts, order in edge_calls()[:6]:
        for g in (n, s, n2, s2):
            g.engine.send_mixed(by_index(g, parts), order)
        a, b = n.engine.poll(with_seq=True), s.engine.poll(with_seq=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        ca, cb = n2.engine.poll_compact(), s2.engine.poll_compact()
        assert ca[0] == cb[0] and np.array_equal(ca[1], cb[1]) and len(ca[1]) == len(a[0])
        total += len(a[0])
    assert total >= 1500
    assert n.engine.debug_mixed_pushes() == (6, 0) and s.engine.debug_mixed_pushes() == (0, 6)


RATCHET_SRC = EDGE_SRC + (" @info(name='r') from every e1=A[p > 50] -> e2=A[p > e1.p] within 40 milliseconds "
                          "select e1.p as a insert into O;")


def test_device_records():
    normal, dev = hip_app(EDGE_SRC), hip_app(EDGE_SRC, flags=SDH_FLAG_DEVICE_MATCHES)
    total = 0
    for parts, order in edge_calls()[:6]:
        normal.engine.send_mixed(by_index(normal, parts), order)
        dev.engine.send_mixed(by_index(dev, parts), order)
        want = len(normal.engine.poll()[0])
        r = dev.engine.poll_records()
        assert (r.n, r.c_n, r.n_events) == (want, want, len(order))
        total += want
    assert total >= 1500 and dev.engine.debug_mixed_pushes() == (6, 0)
    # a call that cannot run natively (a K_ratchet query reads A) is refused in this mode, nothing changed
    g = hip_app(RATCHET_SRC, flags=SDH_FLAG_DEVICE_MATCHES)
    assert g.engine.stats().plan_queries[0] == 1
    parts, order = edge_calls()[1]
    before = g.engine.stats()
    with pytest.raises(EngineError) as ex:
        g.engine.send_mixed(by_index(g, parts), order)
    assert ex.value.code == E_UNSUPPORTED
    after = g.engine.stats()
    assert (after.events, after.pattern_events, after.live_partials) == (before.events, before.pattern_events, 0)
    assert g.engine.debug_mixed_pushes() == (0, 0)


def test_poll_rows_over_mixed_pushes():
    from test_gpu_rows import check_polled
    o = App(EDGE_SRC)
    a, b = hip_app(EDGE_SRC), hip_app(EDGE_SRC)
    b.engine.retain_events(256)
    total = 0
    for parts, order in edge_calls():
        oracle_runs(o, parts, order)
        a.engine.send_mixed(by_index(a, parts), order)
        b.engine.send_mixed(by_index(b, parts), order)
        matches, _ = check_polled(o, a.engine.poll(with_seq=True), b.engine.poll_rows(), width=2)
        assert matches == take(o)
        total += len(matches)
    assert total >= 2500 and b.engine.debug_mixed_pushes()[1] == 0


def test_event_store_keeps_the_last_events_of_a_long_call():
    """A call longer than the ring: rows of its last ev_cap merged events only (`within` keeps every match
    inside them)."""
    from test_gpu_rows import check_polled
    o = App(EDGE_SRC)
    a, b = hip_app(EDGE_SRC), hip_app(EDGE_SRC)
    b.engine.retain_events(64)
    rng = np.random.default_rng(2)
    warm = call_of(rng.integers(0, 2, 10), 0, AB, rng)
    long_call = call_of([0] * 100 + [1] * 100 + [0] * 40, 1000, AB, rng)
    last = call_of([1, 0, 1, 1], 1240, [("A", price(0, 100)), ("B", fixed([99.9, 99.95, 99.99]))], rng)
    for k, (parts, order) in enumerate((warm, long_call, last)):
        oracle_runs(o, parts, order)
        a.engine.send_mixed(by_index(a, parts), order)
        b.engine.send_mixed(by_index(b, parts), order)
        if k == 1:  # (its matches reach back past the ring: drop them, the store itself is what is checked)
            a.engine.poll(), b.engine.poll(), take(o)
            continue
        matches, _ = check_polled(o, a.engine.poll(with_seq=True), b.engine.poll_rows(), width=2)
        assert matches == take(o)
        assert k == 0 or (len(matches) >= 200 and min(m[3][0][0] for m in matches) < 250)  # reach back into the ring


# ---- 6. eligibility ----------------------------------------------------------------------------------
def test_a_ratchet_query_takes_the_split_path():
    calls = edge_calls()[:7]
    t = Trio(RATCHET_SRC, native=False)
    assert t.n.engine.stats().plan_queries[0] == 1
    for parts, order in calls:
        t.mixed(parts, order)
    assert t.total >= 1800
    t2 = Trio(RATCHET_SRC, native=True, flags=SDH_FLAG_NO_RATCHET)
    assert t2.n.engine.stats().plan_queries[0] == 0
    for parts, order in calls:
        t2.mixed(parts, order)
    assert t2.total == t.total


# ---- 7. continuity -----------------------------------------------------------------------------------
def test_mixed_and_plain_pushes_alternate():
    t = Trio(EDGE_SRC)
    rng = np.random.default_rng(21)
    tt = 0
    for k in range(8):
        t.mixed(*call_of(rng.integers(0, 2, [65, 1, 130, 64][k % 4]), tt, AB, rng))
        tt += 130
        stream = "AB"[k % 2]
        t.plain(stream, tt + np.arange(70), f32_words(rng.uniform(0, 100, 70)))
        tt += 70
    assert t.total >= 2500


def test_snapshot_after_a_mixed_call():
    t = Trio(EDGE_SRC)
    rng = np.random.default_rng(22)
    t.mixed(*call_of(rng.integers(0, 2, 130), 0, AB, rng))
    blob = t.n.engine.snapshot()
    # a fresh engine restored from the native engine's snapshot continues on either path
    rn = hip_app(EDGE_SRC)
    rs = hip_app(EDGE_SRC, debug={"SDH_MIX_SPLIT": 1})
    rn.engine.restore(blob)
    rs.engine.restore(blob)
    total = 0
    for k, n in enumerate((65, 130)):
        parts, order = call_of(rng.integers(0, 2, n), 130 + 200 * k, AB, rng)
        want = t.mixed(parts, order)
        for g in (rn, rs):
            g.engine.send_mixed(by_index(g, parts), order)
            assert take(g) == want
        total += len(want)
    assert total >= 600
    assert rn.engine.debug_mixed_pushes() == (2, 0) and rs.engine.debug_mixed_pushes() == (0, 2)
    assert rn.engine.stats().live_partials == t.n.engine.stats().live_partials == rs.engine.stats().live_partials


def test_two_shards_together_equal_the_oracle():
    o = App(EDGE_SRC)
    shards = [hip_app(EDGE_SRC, shard_rank=r, shard_world=2) for r in range(2)]
    total = 0
    for parts, order in edge_calls()[:7]:
        oracle_runs(o, parts, order)
        got = []
        for g in shards:
            g.engine.send_mixed(by_index(g, parts), order)
            q, k, ts, off, words, seq, tb = g.engine.poll(with_seq=True)
            got += [(int(seq[i]), int(q[i]), tuple(words[off[i]:off[i + 1]].tolist())) for i in range(len(q))]
        meta = []
        om = o.engine.take_matches(lambda q: 2, meta)
        want = [(sq, m[0], (1, m[3][0][0], 1, m[3][1][0])) for m, (sq, _) in zip(om, meta)]
        assert sorted(got) == sorted(want)
        total += len(want)
    assert total >= 1800
    assert all(g.engine.debug_mixed_pushes() == (7, 0) and g.engine.stats().plan_queries[2] == 10 for g in shards)


# ---- 8. refusals -------------------------------------------------------------------------------------
def raw_parts(n_a, n_b, n_cols=(1, 1), chunk=(0, 0), streams=(0, 1), on_device=(0, 0)):
    """Host sdh_mixed_part records with one float column each, every field open to the caller."""
    from siddhi_amd.engine import SdhBatch, SdhMixedPart
    keep, arr = [], (SdhMixedPart * 2)()
    for i, n in enumerate((n_a, n_b)):
        ts = np.arange(n, dtype=np.int64) + 10_000
        col = np.full(max(n, 1), 50.0 + i, np.float32)
        cp = (ctypes.c_void_p * 2)(col.ctypes.data, col.ctypes.data)
        keep += [ts, col, cp]
        arr[i].stream = streams[i]
        arr[i].batch = SdhBatch(n=n, ts=ts.ctypes.data, cols=cp, nulls=None, n_cols=n_cols[i], on_device=on_device[i],
                                chunk=chunk[i])
    return arr, keep


@pytest.mark.parametrize("split", [0, 1], ids=["native", "split"])
def test_refusals_leave_the_state_untouched(split):
    import torch
    src = EDGE_SRC
    o = App(src)
    g = hip_app(src, debug={"SDH_MIX_SPLIT": split})
    h = g.engine
    rng = np.random.default_rng(31)
    parts, order = call_of(rng.integers(0, 2, 65), 0, AB, rng)
    oracle_runs(o, parts, order)
    h.send_mixed(by_index(g, parts), order)
    assert take(g) == take(o)
    before = h.stats()

    def refused(raw, order, n_order=None, on_device=0, n_parts=2):
        arr, keep = raw  # (keep: the arrays the records point into)
        order = np.asarray(order, np.int32)
        ptr = order.ctypes.data
        if on_device:
            dev = torch.from_numpy(order).to("cuda:0")
            torch.cuda.synchronize()
            ptr = dev.data_ptr()
        rc = h.lib.sdh_engine_push_mixed(h.h, n_parts, arr, ptr, len(order) if n_order is None else n_order, on_device)
        assert rc == E_INVALID, rc

    ok_order = [0, 1, 0, 1, 1]
    refused(raw_parts(2, 3, streams=(0, 0)), ok_order)            # a stream named twice
    refused(raw_parts(2, 3, chunk=(0, 1)), ok_order)               # a chunk part
    refused(raw_parts(2, 3, n_cols=(1, 2)), ok_order)              # a column count that is not the stream's
    refused(raw_parts(2, 3), ok_order + [1])                       # n_order != the sum of the parts' n
    refused(raw_parts(2, 3), ok_order, n_order=4)
    refused(raw_parts(2, 3), [0, 0, 0, 1, 1])                      # a part's count in order
    refused(raw_parts(2, 3), [0, 1, 0, 1, 2])                      # an order entry that names no part
    refused(raw_parts(2, 3), [0, 0, 0, 1, 1], on_device=1)         # a device order with a wrong count
    refused(raw_parts(2, 3), [0, 1, 0, 1, 7], on_device=1)
    refused(raw_parts(2, 3, on_device=(0, 1)), ok_order)           # host and device parts
    refused(raw_parts(2, 3, streams=(0, 5)), ok_order)             # no such stream
    after = h.stats()
    assert (after.events, after.pattern_events, after.matches, after.live_partials) == (
        before.events, before.pattern_events, before.matches, before.live_partials)
    assert h.pending_matches() == 0
    # n_order == 0 is a no-op, and the next call's result shows the state is where the first call left it
    arr, keep = raw_parts(0, 0)
    assert h.lib.sdh_engine_push_mixed(h.h, 2, arr, None, 0, 0) == 0
    parts, order = call_of(rng.integers(0, 2, 130), 65, AB, rng)
    oracle_runs(o, parts, order)
    h.send_mixed(by_index(g, parts), order)
    got, want = take(g), take(o)
    assert got == want and len(want) >= 500
    assert h.debug_mixed_pushes() == ((0, 2) if split else (2, 0))


def test_max_batch_and_device_parts():
    """A total above max_batch is refused; device-resident parts with a device order equal the host form."""
    import torch
    from siddhi_amd.engine import SdhConfig, debug_string, load_library
    o = App(EDGE_SRC)
    g = hip_app(EDGE_SRC)
    rng = np.random.default_rng(41)
    total = 0
    for n in (130, 64, 1):
        parts, order = call_of(rng.integers(0, 2, n), total, AB, rng)
        oracle_runs(o, parts, order)
        keep, dparts = [], []
        for stream, ts, vals, _ in parts:
            t_ts = torch.from_numpy(ts).to("cuda:0")
            t_col = torch.from_numpy(vals[:, 0].astype(np.uint32).view(np.int32).copy()).to("cuda:0")
            keep += [t_ts, t_col]
            dparts.append((g.ir.stream_index(stream), len(ts), t_ts.data_ptr(), [t_col.data_ptr()]))
        d_order = torch.from_numpy(order).to("cuda:0")
        torch.cuda.synchronize()
        g.engine.push_mixed_device(dparts, d_order.data_ptr(), len(order))
        assert take(g) == take(o)
        total += n
    assert g.engine.debug_mixed_pushes() == (3, 0) and g.engine.stats().matches >= 500
    # max_batch
    lib = load_library()
    cfg = SdhConfig(device=0, shard_rank=0, shard_world=1, max_batch=4, debug=debug_string(None))
    hd = ctypes.c_void_p()
    blob = ctypes.create_string_buffer(o.blob, len(o.blob))
    assert lib.sdh_engine_create(blob, len(o.blob), ctypes.byref(cfg), ctypes.byref(hd)) == 0
    try:
        order = np.array([0, 1, 0, 1, 1], np.int32)
        arr, keep = raw_parts(2, 3)
        assert lib.sdh_engine_push_mixed(hd, 2, arr, order.ctypes.data, 5, 0) == E_INVALID
        arr, keep = raw_parts(2, 2)
        assert lib.sdh_engine_push_mixed(hd, 2, arr, order[:4].ctypes.data, 4, 0) == 0
    finally:
        lib.sdh_engine_destroy(hd)
