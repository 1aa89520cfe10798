"""sdh_engine_poll_rows: the matches projected into output rows on the device, from the event store
in HBM (sdh_engine_retain_events).

Every comparison is against a twin engine fed the same pushes and polled with sdh_engine_poll: its
tuples, projected by siddhi_amd/selector.py project() over the host event log and encoded
(events.encode_value), must equal the device's cells and null masks bit for bit (any NaN equals any NaN
of its type), in the same order with the same query / ts / seq columns."""
import ctypes

import numpy as np
import pytest

from harness import App, decode_matches
from select_host import HAND_APPS, assert_cells_equal, callback_rows, reference_cells, seeded_apps, seeded_events
from siddhi_amd.selector import decode_rows
from test_oracle_reference_kat import KAT, OUT_OF_SCOPE, check_rows, run_fixture

pytestmark = pytest.mark.gpu

SDH_FLAG_DEVICE_MATCHES, SDH_FLAG_FORCE_GEN = 1, 4
E_INVALID, E_CAPACITY = -1, -4
FIXTURES = [f for f in KAT["fixtures"] if f["id"] not in OUT_OF_SCOPE]


def check_polled(app, tuples, rows, width=None):
    """rows (poll_rows of one engine) against tuples (poll(with_seq=True) of its twin); returns the
    twin's matches and the decoded rows."""
    q, k, ts, off, words, seq, tb = tuples
    rq, rts, rseq, cells, nulls = rows
    assert np.array_equal(rq, q) and rq.dtype == np.int32
    assert np.array_equal(rts, ts) and np.array_equal(rseq, seq)
    matches = decode_matches(len(q), q, k, ts, off, words, lambda i: len(app.ir.queries[i].states))
    w = max([len(x.outputs) for x in app.ir.queries] + [0])
    assert cells.shape == (w, len(q)) and (width is None or w == width)
    assert_cells_equal(app, matches, cells, nulls, *reference_cells(app, matches, w))
    return matches, decode_rows(app.ir, rows, app.dictionary)


class Twin:
    """harness.App engine: two HipEngines fed alike, `a` polled with poll(), `b` (retaining events)
    with poll_rows(); every take compares them."""

    def __init__(self, blob, retain=1024, **kw):
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

    def start(self, t):
        self.a.start(t)
        self.b.start(t)

    def advance_time(self, t):
        self.a.advance_time(t)
        self.b.advance_time(t)

    def take_matches(self, n_slots_of):
        matches, rows = check_polled(self.app, self.a.poll(with_seq=True), self.b.poll_rows())
        self.rows += rows
        return matches


def twin_app(src, **kw):
    app = App(src, engine_factory=lambda blob: None)
    app.engine = Twin(app.blob, stream_types=[s.attr_types for s in app.ir.streams], **kw)
    app.engine.app = app
    return app


def send_all(app, events, batch):
    """per event, or runs of up to `batch` consecutive same-stream events as one push"""
    i = 0
    while i < len(events):
        j = i + 1
        while j < len(events) and events[j][0] == events[i][0] and j - i < batch:
            j += 1
        app.send(events[i][0], [r for _, r, _ in events[i:j]], [t for _, _, t in events[i:j]])
        i = j


@pytest.mark.parametrize("flags", [0, SDH_FLAG_FORCE_GEN], ids=["planned", "force_gen"])
@pytest.mark.parametrize("fx", FIXTURES, ids=[f["id"] for f in FIXTURES])
def test_reference_kat_rows_on_gpu(fx, flags):
    from harness import parse_literal
    app = twin_app(fx["app"], flags=flags)
    for ev in fx["events"]:
        app.send(ev["stream"], [[parse_literal(t) for t in ev["data"]]], [ev["ts"]])
    check_rows(fx, callback_rows(fx["callback_kind"] == "QueryCallback", fx["callback"], app, app.matches,
                                 app.engine.rows))


@pytest.mark.parametrize("batch", [1, 40], ids=["per_event", "batched"])
@pytest.mark.parametrize("name,src,events", HAND_APPS, ids=[a[0] for a in HAND_APPS])
def test_hand_written_apps_on_gpu(name, src, events, batch):
    app = twin_app(src)
    send_all(app, events, batch)
    assert app.matches


SEEDED = seeded_apps()


@pytest.mark.parametrize("batch", [1, 40], ids=["per_event", "batched"])
@pytest.mark.parametrize("name,src", SEEDED, ids=[a[0] for a in SEEDED])
def test_seeded_select_lists_on_gpu(name, src, batch):
    app = twin_app(src)
    send_all(app, seeded_events(), batch)
    assert len(app.matches) >= 10


def stock_app(src, **kw):
    """(app with a host log, engine a, engine b) for pushes of the seeded StockStream"""
    from siddhi_amd.engine import HipEngine
    app = App(src, engine_factory=lambda blob: None)
    assert len(app.dictionary) == 0
    for k in range(100):  # (the generator's symbol ids are the dictionary ids of "SYM<k>")
        app.dictionary.intern(f"SYM{k}")
    types = [s.attr_types for s in app.ir.streams]
    return app, HipEngine(app.blob, stream_types=types, **kw), HipEngine(app.blob, stream_types=types, **kw)


def push_stock(app, engines, lo, n, symbols=100):
    from siddhi_amd.workloads import stock_events
    ts, sym, price, vol = stock_events(lo, n, symbols)
    vals = np.stack([sym.astype(np.int64), price.view(np.uint32).astype(np.int64), vol.astype(np.int64)], 1)
    app.log.append(0, ts, vals, None)
    for e in engines:
        e.push_columns(0, ts, [sym, price.view(np.uint32), vol])


CHAIN_QUERY = (" @info(name='x3') from every e1=StockStream[price > 90] -> e2=StockStream[price < 10] "
               "-> e3=StockStream[price > e1.price] within 1 sec select e1.price as a, e3.volume as v, e2.symbol as s "
               "insert into O;")


@pytest.mark.parametrize("second_producer", [False, True], ids=["placed", "sorted"])
def test_placed_and_sorted_windows(second_producer):
    """K_ratchet windows: placed compact rows (no other producer), or the sorted table (a K_chain query
    in the window); more than one wave of rows, the last one partial."""
    from siddhi_amd.workloads import c2_app
    app, a, b = stock_app(c2_app(3) + (CHAIN_QUERY if second_producer else ""))
    b.retain_events(1024)
    placed0 = b.stats().placed_pushes
    seen = []
    for lo in (0, 200):
        push_stock(app, (a, b), lo, 200)
        matches, _ = check_polled(app, a.poll(with_seq=True), b.poll_rows(), 3 if second_producer else 2)
        assert len(matches) > 64 and len(matches) % 64 != 0
        seen += matches
    if second_producer:
        assert b.stats().placed_pushes == placed0 and any(m[0] == 3 for m in seen)
    else:
        assert b.stats().placed_pushes == placed0 + 2


def test_mixed_shapes_in_one_wave():
    """Four queries over one stream with four select lists, all matching the same events: adjacent rows
    belong to different shapes; the null mask carries the bits past each query's outputs."""
    outs = ["e1.price as a",
            "e1.price as a, e2.volume as b",
            "e2.price - e1.price as a, e1.symbol as b, e2.volume > e1.volume as c",
            "e1.volume * 2 as a, e2.symbol as b, e1.price as c, e2.price as d, e1.volume + e2.volume as e"]
    src = ("define stream StockStream (symbol string, price float, volume int); " +
           " ".join(f"@info(name='m{k}') from every e1=StockStream[price > 50.0] -> e2=StockStream[price > e1.price] "
                    f"within 1 sec select {o} insert into O{k};" for k, o in enumerate(outs)))
    app, a, b = stock_app(src)
    b.retain_events(512)
    assert [len(b.query_outputs(k)) for k in range(4)] == [1, 2, 3, 5]
    push_stock(app, (a, b), 0, 300)
    rows = b.poll_rows()
    matches, _ = check_polled(app, a.poll(with_seq=True), rows, 5)
    q, nulls = rows[0], rows[4]
    assert len(q) > 256 and len(set(q[:64].tolist())) == 4
    for k, n_out in enumerate((1, 2, 3, 5)):
        sel = nulls[q == k]
        assert len(sel) and np.all(sel >> np.uint64(n_out) == np.uint64((1 << (64 - n_out)) - 1))
        assert np.all(sel & np.uint64((1 << n_out) - 1) == 0)


def test_ring_wraps_and_capacity():
    from siddhi_amd.engine import EngineError
    src = ("define stream S (v int, w long); "
           "@info(name='short') from every e1=S[v >= 0] -> e2=S[v > e1.v] within 40 milliseconds "
           "select e1.v as a, e2.w as b, e2.v - e1.v as d insert into O; "
           "@info(name='long') from every e1=S[v == -1] -> e2=S[v == -2] select e1.w as a, e2.w as b insert into P;")
    app = twin_app(src, retain=64)
    rng = np.random.default_rng(5)
    t = 1000

    def events(vs):
        nonlocal t
        out = [("S", [int(v), 7 * t], t + k) for k, v in enumerate(vs)]
        t += len(vs)
        return out
    # 300 events in pushes of 1 .. 25: every e1 is at most 40 events old, the ring wraps four times
    ev = events(rng.integers(0, 50, 300))
    i = 0
    while i < len(ev):
        n = int(rng.integers(1, 26))
        app.send("S", [r for _, r, _ in ev[i:i + n]], [x for _, _, x in ev[i:i + n]])
        i += n
    assert len(app.matches) > 200
    # an e1 100 events old has left the ring of 64
    a, b = app.engine.a, app.engine.b
    old = events([-1] + [0] * 100 + [-2])
    for e in (a, b):
        for _, r, x in old:
            e.send(0, [x], np.array([r], np.int64), None)
    for _, r, x in old:
        vals = np.array([r], np.int64)
        app.log.append(0, [x], vals, None)
    with pytest.raises(EngineError) as ex:
        b.poll_rows()
    assert ex.value.code == E_CAPACITY and "retain_events" in str(ex.value)
    ga, gb = a.poll(with_seq=True), b.poll(with_seq=True)  # the window stayed pending
    assert len(ga[0]) > 0 and 1 in ga[0]
    for x, y in zip(ga, gb):
        assert np.array_equal(x, y)
    b.retain_events(256)
    n0 = len(app.matches)
    send_all(app, events([-1] + [0] * 100 + [-2]), 40)
    assert any(m[0] == 1 for m in app.matches[n0:])


def test_two_streams_interleaved():
    """Streams of four and one attributes alternating in pushes of 1, 7 and 64 events: seq -> row."""
    src = ("define stream A (a int, b float, c long, d string); define stream B (x double); "
           "@info(name='q') from every e1=A[a > 2] -> e2=B[x > e1.b] within 1 sec "
           "select e1.a as a, e1.c as c, e1.d as d, e2.x as x, e2.x + e1.b as s insert into O;")
    app = twin_app(src, retain=256)
    rng = np.random.default_rng(11)
    t = 5000
    for k in range(24):
        n = (1, 7, 64)[k % 3]
        if (k // 3) % 2 == 0:
            rows = [[int(rng.integers(0, 9)), np.float32(rng.uniform(0, 10)), int(rng.integers(-2 ** 40, 2 ** 40)),
                     "s%d" % rng.integers(0, 5)] for _ in range(n)]
            app.send("A", rows, list(range(t, t + n)))
        else:
            app.send("B", [[float(rng.uniform(0, 12))] for _ in range(n)], list(range(t, t + n)))
        t += n
    assert len(app.matches) > 50


def test_append_under_exact_reruns():
    """K_gen pools that start tiny overflow and re-run their pushes exactly: the store's rows, written
    by seq, are the same."""
    from fuzz_apps import random_app, random_events
    seed = 7
    app = twin_app(random_app(seed, partition=seed % 3 == 0), flags=SDH_FLAG_FORCE_GEN, gen_pool_states=2,
                   gen_pool_nodes=4, gen_list_cap=2)
    send_all(app, random_events(seed), 40)
    assert app.engine.b.stats().pool_regrows > 0 and app.matches


def test_append_under_journal_split():
    """A push forced to split into halves (SDH_JOURNAL_BUDGET) appends each half's events."""
    from siddhi_amd.workloads import c3_app
    app, a, b = stock_app(c3_app(12), flags=SDH_FLAG_FORCE_GEN, gen_pool_states=2, gen_pool_nodes=4, gen_list_cap=2,
                          gen_max_keys=1024, debug={"SDH_JOURNAL_BUDGET": 1})
    b.retain_events(1024)
    total = 0
    for lo, n in ((0, 200), (200, 300)):
        push_stock(app, (a, b), lo, n, 40)
        total += len(check_polled(app, a.poll(with_seq=True), b.poll_rows())[0])
    assert total > 20


SNAP_SRC = ("define stream S (k int, v int, p float); "
            "@info(name='c') from every e1=S[v > 3] <2:4> -> e2=S[p > e1[last].p] "
            "select e1[0].v as a, e1[last].p as b, e2.p as c insert into O; "
            "@info(name='r') from every e1=S[p > 2.0] -> e2=S[p > e1.p] select e1.p as a, e2.v as b insert into P;")


def _snap_events(n, seed):
    rng = np.random.default_rng(seed)
    return [("S", [int(rng.integers(0, 4)), int(rng.integers(0, 10)), np.float32(rng.uniform(0, 10))], 100 + i)
            for i in range(n)]


def test_snapshot_restore_with_retention():
    """Partials opened before the snapshot complete after the restore: their rows read events the
    snapshot carried (version 9)."""
    ev = _snap_events(120, 3)
    app = twin_app(SNAP_SRC, retain=256)
    send_all(app, ev[:60], 7)
    snap = app.engine.b.snapshot()
    assert np.frombuffer(snap[:16], np.int64)[1] == 9
    assert np.frombuffer(app.engine.a.snapshot()[:16], np.int64)[1] == 8
    from siddhi_amd.engine import HipEngine
    fresh = HipEngine(app.blob, stream_types=[s.attr_types for s in app.ir.streams])
    fresh.retain_events(256)
    fresh.restore(snap)
    app.engine.b = fresh
    n0 = len(app.matches)
    send_all(app, ev[60:], 7)
    new = app.matches[n0:]
    assert any(min(s[0] for s in m[3] if s) < 60 for m in new), "a match must read pre-snapshot events"


def test_version8_snapshot_restores_empty_store():
    from siddhi_amd.engine import EngineError, HipEngine
    ev = _snap_events(80, 4)
    app = twin_app(SNAP_SRC, retain=256)
    send_all(app, ev[:40], 7)
    snap8 = app.engine.a.snapshot()  # an engine that keeps no events: version 8
    fresh = HipEngine(app.blob, stream_types=[s.attr_types for s in app.ir.streams])
    fresh.retain_events(256)
    fresh.restore(snap8)
    si = 0
    for stream, row, t in ev[40:]:
        from siddhi_amd.events import encode_rows
        vals, nulls = encode_rows([row], app.ir.streams[si].attr_types, app.dictionary)
        app.engine.a.send(si, [t], vals, nulls)
        fresh.send(si, [t], vals, nulls)
    with pytest.raises(EngineError) as ex:
        fresh.poll_rows()
    assert ex.value.code == E_CAPACITY
    ga, gb = app.engine.a.poll(with_seq=True), fresh.poll(with_seq=True)
    assert len(ga[0]) > 0
    for x, y in zip(ga, gb):
        assert np.array_equal(x, y)


def test_call_errors():
    from siddhi_amd.engine import EngineError
    from siddhi_amd.workloads import c2_app
    app, a, b = stock_app(c2_app(3))
    push_stock(app, (a,), 0, 100)
    with pytest.raises(EngineError) as ex:
        a.poll_rows()
    assert ex.value.code == E_INVALID and a.pending_matches() > 0
    with pytest.raises(EngineError) as ex:
        a.retain_events(0)
    assert ex.value.code == E_INVALID
    app, d, _ = stock_app(c2_app(3), flags=SDH_FLAG_DEVICE_MATCHES)
    d.retain_events(256)
    push_stock(app, (d,), 0, 100)
    assert d.pending_matches() > 0 and len(d.poll_rows()[0]) == 0


def test_device_arrays_equal_host_form():
    import torch
    from siddhi_amd.workloads import c2_app
    app, a, b = stock_app(c2_app(3) + CHAIN_QUERY)
    a.retain_events(512)
    b.retain_events(512)
    push_stock(app, (a, b), 0, 300)
    host = a.poll_rows()
    r = b.poll_rows(device=True)
    n, w = r.n, r.width
    assert n == len(host[0]) > 64 and w == 3

    def back(ptr, count, dtype):  # device to device into a torch tensor, then torch's copy to the host
        out = torch.empty(count, dtype=dtype, device="cuda:0")
        hip = ctypes.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        assert hip.hipMemcpy(out.data_ptr(), ctypes.cast(ptr, ctypes.c_void_p).value,
                             out.numel() * out.element_size(), 3) == 0
        return out.cpu().numpy()
    assert np.array_equal(back(r.query, n, torch.int32), host[0])
    assert np.array_equal(back(r.ts, n, torch.int64), host[1])
    assert np.array_equal(back(r.seq, n, torch.int64), host[2])
    assert np.array_equal(back(r.cells, n * w, torch.int64).reshape(w, n), host[3])
    assert np.array_equal(back(r.nulls, n, torch.int64).view(np.uint64), host[4])


def test_parent_behaviour_without_retention():
    """An engine that never calls retain_events: the oracle's matches on one KAT and one C2 push, and
    a version-8 snapshot."""
    from harness import parse_literal
    from siddhi_amd.engine import HipEngine
    from siddhi_amd.workloads import c2_app, stock_events
    fx = FIXTURES[0]
    o, _ = run_fixture(fx)
    probe = App(fx["app"], engine_factory=lambda blob: None)
    types = [s.attr_types for s in probe.ir.streams]
    g, grows = run_fixture(fx, engine_factory=lambda blob: HipEngine(blob, stream_types=types))
    assert g.matches == o.matches
    check_rows(fx, grows)
    ref = App(c2_app(16))
    gpu = HipEngine(ref.blob, stream_types=[s.attr_types for s in ref.ir.streams])
    ts, sym, price, vol = stock_events(0, 5000)
    vals = np.stack([sym.astype(np.int64), price.view(np.uint32).astype(np.int64), vol.astype(np.int64)], 1)
    ref.engine.send(0, ts, vals, None)
    gpu.push_columns(0, ts, [sym, price.view(np.uint32), vol])
    assert gpu.take_matches(lambda q: 2) == ref.engine.take_matches(lambda q: 2)
    assert np.frombuffer(gpu.snapshot()[:16], np.int64)[1] == 8
