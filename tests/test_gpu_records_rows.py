"""sdh_engine_records_rows: output rows projected from device records (SDH_FLAG_DEVICE_MATCHES).

The reference of every test is a normal-mode twin engine fed the same pushes with the same
retain_events: its poll_rows() and the device-record engine's records_rows() must be equal, bit for bit,
as sorted multisets of (query, seq, ts, nulls, cells...) -- records carry no delivery order -- and in
their row count. Tests 1 and 6 also check the twin itself through check_polled: against a third engine's
poll() and siddhi_amd/selector.py over the host event log, which the oracle pins elsewhere (test 6 with
tests/test_gpu_rows.py's; test 1, whose select lists call eventTimestamp() and ifThenElse, with the
form of it that hands the selector the match's timestamp, tests/test_gpu_functions.py's). Every test calls
records_rows before any push."""
import ctypes

import numpy as np
import pytest

from harness import App
from siddhi_amd.engine import (SDH_FLAG_DEVICE_MATCHES, SDH_FLAG_FORCE_GEN, SDH_REC_4, SDH_REC_8, EngineError, HipEngine,
                               mixed_runs)
from siddhi_amd.workloads import STOCK_STREAM, stock_events
from test_gpu_records import _host, walk_flat
from test_gpu_rows import check_polled

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED, E_CAPACITY = -1, -2, -4


def canon(rows):
    """(query, ts, seq, cells[w, n], nulls) -> the rows as a sorted int64 matrix [n, 4 + w]."""
    q, ts, seq, cells, nulls = rows[:5]
    m = np.column_stack([q.astype(np.int64), seq, ts, nulls.view(np.int64)] + [cells[c] for c in range(cells.shape[0])])
    return m[np.lexsort(m.T[::-1])] if len(m) else m


def same_rows(got, want):
    assert len(got[0]) == len(want[0]) and got[3].shape == want[3].shape
    assert got[0].dtype == np.int32 and np.array_equal(canon(got), canon(want))


def equal_exactly(x, y):
    assert all(np.array_equal(a, b) for a, b in zip(x[:5], y[:5]))


class Three:
    """harness.App engine: d in device-record mode read with records_rows(), its normal-mode twin b read
    with poll_rows(), and (check) a third engine a whose poll() pins the twin; every take compares them."""

    def __init__(self, app, retain, flags=0, check=None, dev_debug=None, twin_retain=None, **kw):
        types = [s.attr_types for s in app.ir.streams]
        self.app = app
        self.d = HipEngine(app.blob, stream_types=types, flags=flags | SDH_FLAG_DEVICE_MATCHES, debug=dev_debug, **kw)
        self.d.retain_events(retain)
        assert self.d.records_rows()[5] == 0  # (the new entry point, before anything else runs)
        self.b = HipEngine(app.blob, stream_types=types, flags=flags, **kw)
        self.b.retain_events(twin_retain or retain)
        self.check = check
        self.a = HipEngine(app.blob, stream_types=types, flags=flags, **kw) if check else None
        self.all = [e for e in (self.d, self.b, self.a) if e is not None]
        self.total = 0
        self.last = None

    def send(self, *args, **kw):
        for e in self.all:
            e.send(*args, **kw)

    def send_mixed(self, parts, order):
        for e in self.all:
            e.send_mixed(parts, order)

    def set_strings(self, ids, texts):
        for e in self.all:
            e.set_strings(ids, texts)

    def start(self, t):
        for e in self.all:
            e.start(t)

    def advance_time(self, t):
        for e in self.all:
            e.advance_time(t)

    def compare(self):
        got = self.d.records_rows()
        want = self.b.poll_rows()
        if self.a is not None:
            self.check(self.app, self.a.poll(with_seq=True), want)
        assert got[5] == len(want[0])
        same_rows(got, want)
        self.total += got[5]
        self.last = got
        return got

    def take_matches(self, n_slots_of):
        return [None] * self.compare()[5]


def three_app(src, retain, stock=False, **kw):
    app = App(src, engine_factory=lambda blob: None)
    if stock:  # (the generator's symbol ids are the dictionary ids of "SYM<k>")
        assert len(app.dictionary) == 0
        for k in range(100):
            app.dictionary.intern(f"SYM{k}")
    app.engine = Three(app, retain, **kw)
    return app


def push_stock(app, lo, n, symbols=100, nulls=None, gen=stock_events):
    ts, x, y, z = gen(lo, n, symbols)
    vals = np.stack([x.astype(np.int64), y.view(np.uint32).astype(np.int64), z.astype(np.int64)], 1)
    app.log.append(0, ts, vals, nulls)
    app.engine.send(0, ts, vals, nulls)
    return app.engine.compare()


SELECTS = ["e1.price as a, e2.price as b",
           "e2.volume - e1.volume as a, eventTimestamp() as b",
           "ifThenElse(e2.price > 100, e1.symbol, e2.symbol) as a",
           "e2.volume as a"]


def float_patterns(n):
    """n float-keyed C2-shape patterns, the four select lists round-robin (one wave holds all four shapes)."""
    return " ".join(
        f"@info(name='f{p}') from every e1=StockStream[price > 98.{p % 20:02d}] -> e2=StockStream[price > e1.price] "
        f"within {1000 if p % 5 == 0 else 200} milliseconds select {SELECTS[p % 4]} insert into F{p % 4};"
        for p in range(n))


def int_patterns(n):
    """int-keyed (8-B records in a rec4 push) and, every third, gated (K_gate) patterns on the same stream"""
    return " ".join(
        f"@info(name='i{p}') from every e1=StockStream[volume > {975 + p % 20}] -> e2=StockStream[volume > e1.volume"
        f"{' and price > 50.0' if p % 3 == 0 else ''}] within 200 milliseconds "
        f"select e1.volume as a, e2.price as b insert into I;" for p in range(n))


PUSHES = (4000, 17, 9000)


# ---- 1. rec4 blocks, the plain kernel -----------------------------------------------------------------
def test_rec4_plain_kernel():
    from test_gpu_functions import check_polled as check_polled_ts
    app = three_app(STOCK_STREAM + " " + float_patterns(130), 1 << 14, stock=True, check=check_polled_ts)
    assert app.engine.d.stats().plan_queries[0] == 130
    lo = 0
    for n in PUSHES:
        got = push_stock(app, lo, n)
        lo += n
        rec = app.engine.d.poll_records()
        assert rec.r_n == rec.n == got[5]
        if n > 1000:
            assert rec.r_format == SDH_REC_4 and got[5] > 3000
            assert len(set((got[0][:256] % 4).tolist())) == 4  # (adjacent rows of one block: every select shape)
    assert app.engine.d.debug_shared_pushes() == 0


# ---- 2. rec4 blocks, the shared-pops writer -----------------------------------------------------------
def test_rec4_shared_pops_writer():
    app = three_app(STOCK_STREAM + " " + float_patterns(130), 1 << 14, stock=True,
                    dev_debug={"SDH_RATCHET_SHARED_MIN": 1})
    lo = 0
    for n in PUSHES:
        push_stock(app, lo, n)
        lo += n
    # the last push completed partials of the pushes before it (pattern f0: e1.price > 98.00, one second,
    # one event per millisecond): the carried-phase side entries
    lo = PUSHES[0] + PUSHES[1]
    ts, _, price, _ = stock_events(0, lo + 1000)
    assert any(price[i] > 98.0 and np.any(price[lo:i + 1001] > price[i]) for i in range(lo - 1000, lo))
    d = app.engine.d
    assert d.debug_shared_pushes() == len(PUSHES) and app.engine.total > 8000
    assert d.poll_records().r_format == SDH_REC_4


# ---- 3. block roll, an event larger than a block, windows ---------------------------------------------
def test_block_roll_and_windows():
    src = STOCK_STREAM + " " + " ".join(
        f"@info(name='w{p}') from every e1=StockStream[price > 0] -> e2=StockStream[price > e1.price] "
        "select e1.price as a, e2.price as b insert into O;" for p in range(64))
    app = three_app(src, 4096, stock=True)
    n = 2101
    ts = 1_700_000_000_000 + np.arange(n, dtype=np.int64)
    price = np.concatenate([5000.0 - np.arange(n - 1), [9000.0]]).astype(np.float32)  # falling, then one above all
    vals = np.stack([np.arange(n) % 100, price.view(np.uint32).astype(np.int64), np.arange(n) + 1], 1).astype(np.int64)
    app.log.append(0, ts, vals, None)
    app.engine.send(0, ts, vals, None)
    full = app.engine.compare()
    d = app.engine.d
    rec = d.poll_records()
    assert full[5] == 2100 * 64 and rec.r_blocks > 8 and np.all(full[2] == n - 1)
    sizes, first, parts = (1, 63, 64, 65, 16000), 0, []
    while first < full[5]:
        w = d.records_rows(first, sizes[len(parts) % len(sizes)])
        assert w[5] == full[5] and 0 < len(w[0]) == min(sizes[len(parts) % len(sizes)], full[5] - first)
        parts.append(w)
        first += len(w[0])
    cat = [np.concatenate([p[k] for p in parts], axis=1 if k == 3 else 0) for k in range(5)]
    equal_exactly(cat, full)  # order included
    equal_exactly(d.records_rows(), full)


# ---- 4. 8-B blocks beside rec4 blocks in one push -----------------------------------------------------
def test_8b_blocks_beside_rec4_blocks():
    app = three_app(STOCK_STREAM + " " + float_patterns(130) + " " + int_patterns(70), 1 << 14, stock=True)
    st = app.engine.d.stats()
    assert st.plan_queries[0] + st.plan_queries[1] == 200 and st.plan_queries[1] > 0
    lo = 0
    for n in PUSHES:
        got = push_stock(app, lo, n)
        lo += n
    rec = app.engine.d.poll_records()
    side = _host(rec.r_side, rec.r_blocks, np.int32)
    cnt = _host(rec.r_count, rec.r_blocks, np.int32)
    assert rec.r_format == SDH_REC_4 and np.any(side[cnt > 0] < 0) and np.any(side[cnt > 0] >= 0)
    assert np.any(got[0] >= 130) and np.any(got[0] < 130) and app.engine.total > 8000


# ---- 5. a push of 8-B records --------------------------------------------------------------------------
def test_rec8_push():
    app = three_app(STOCK_STREAM + " " + float_patterns(130), 1 << 14, stock=True)
    lo = 0
    for n in PUSHES:
        nulls = np.zeros((n, 3), np.uint8)
        nulls[n // 2, 1] = 1  # one null in the key column: the SIM form is off
        got = push_stock(app, lo, n, nulls=nulls)
        lo += n
        rec = app.engine.d.poll_records()
        if got[5]:
            assert rec.r_format == SDH_REC_8
    assert app.engine.total > 8000


# ---- 6. flat records -----------------------------------------------------------------------------------
def _c3():
    from siddhi_amd.workloads import c3_app
    src = c3_app(128).replace("e2[0].volume as b", "e2[last].volume as b")
    assert "e2[last].volume" in src
    return src


KPART_CHAIN = (STOCK_STREAM + " partition with (symbol of StockStream) begin " + " ".join(
    f"@info(name='k{p}') from every e1=StockStream[price > {60 + p}] -> e2=StockStream[price < {40 - p}] -> "
    f"e3=StockStream[price > e1.price] within 10 sec select e1.price as a, e3.volume as v, e2.symbol as s "
    f"insert into O;" for p in range(8)) + " end;")


FLAT_PUSHES = (3000, 17, 9000)


def _stock_case(src, symbols, walk=False, **kw):
    app = three_app(src, 1 << 14, stock=True, **kw)
    lo, pads = 0, 0
    for n in FLAT_PUSHES:
        got = push_stock(app, lo, n, symbols)
        lo += n
        rec = app.engine.d.poll_records()
        assert rec.f_n == rec.n == got[5]
        if walk and 0 < rec.f_n < 20000:  # (a walk in Python, by the header's layout: the smaller pushes)
            recs, p = walk_flat(rec)
            assert len(recs) == rec.f_n
            pads += p
        equal_exactly(app.engine.d.records_rows(), got)  # (after poll_records: the same rows)
    return app, pads


def test_flat_kpart_narrow_records():
    app, pads = _stock_case(_c3(), 50, walk=True, gen_max_keys=4096)
    assert app.engine.d.stats().plan_queries[3] == 128 and app.engine.total > 1000
    assert pads > 0  # (pads were present: f_words is more than the records' words)


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_flat_kpart_chain_records(wide):
    app, _ = _stock_case(KPART_CHAIN, 20, gen_max_keys=4096, dev_debug={"SDH_KPART_WIDE": 1} if wide else None,
                         check=None if wide else check_polled)
    assert app.engine.d.stats().plan_queries[3] == 8 and app.engine.total > 500


def test_flat_kseq_records():
    from siddhi_amd.workloads import c4_app, txn_events
    app = three_app(c4_app(256), 1 << 14)
    lo = 0
    for n in FLAT_PUSHES:
        push_stock(app, lo, n, 2000, gen=txn_events)
        lo += n
    assert app.engine.d.stats().plan_queries[5] > 0 and app.engine.total > 100


def test_flat_full_records():
    app, _ = _stock_case(_c3(), 50, gen_max_keys=4096, flags=SDH_FLAG_FORCE_GEN)
    assert app.engine.d.stats().plan_queries[6] == 128 and app.engine.total > 1000


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_flat_kwave_records(wide):
    from wave_host import wave_events, wave_queries
    app = three_app(wave_queries(7, n=12), 4096, dev_debug={"SDH_KWAVE_WIDE": 1} if wide else None)
    ts, vals, nl = wave_events(7, 2000)
    for lo in range(0, 2000, 500):
        app.log.append(0, ts[lo:lo + 500], vals[lo:lo + 500], nl[lo:lo + 500])
        app.engine.send(0, ts[lo:lo + 500], vals[lo:lo + 500], nl[lo:lo + 500])
        app.engine.compare()
    assert app.engine.d.stats().plan_queries[7] == 12 and app.engine.total > 100


ABSENT_SRC = ("define stream A (v int, p float); define stream B (v int, p float); "
              "@info(name='t') from every e1=A[p > 20.0] -> not B[p > e1.p] for 30 milliseconds or e2=B[v == 0] "
              "select e1.v as a, e1.p as p, e2.p as q, e2.v is null as n insert into O; "
              "@info(name='n') from every e1=A[p > 60.0] -> e2=B[v > 1] and not A[p > 95.0] "
              "select e1.p as a, e2.v as b, eventTimestamp() as t insert into P;")


def test_flat_absent_and_timer_records():
    """Timer matches (stream 0xFFFF records: the side that did not arrive reads null) and a logical absent
    side, over pushes and time advances."""
    app = three_app(ABSENT_SRC, 4096)
    rng = np.random.default_rng(3)
    t = 10_000
    app.start(t)
    timers = 0
    for k in range(30):
        n = int(rng.integers(1, 40))
        rows = [[int(rng.integers(0, 4)), np.float32(rng.uniform(0, 100))] for _ in range(n)]
        app.send("AB"[k % 2], rows, [t + 2 * i for i in range(n)])
        t += 2 * n
        if k % 5 == 4:
            t += 100
            app.advance_time(t)
        last = app.engine.last
        timers += int(np.sum((last[0] == 0) & ((last[4] >> np.uint64(2)) & np.uint64(1) == 1)))
    assert app.engine.total > 100 and timers > 10


def test_flat_kslab_records():
    from fuzz_apps import random_slab_app, random_slab_events
    app = three_app(random_slab_app(0), 1024)
    ev = random_slab_events(0, n=500, keys=4)
    i = 0
    while i < len(ev):
        j = i + 1
        while j < len(ev) and ev[j][0] == ev[i][0] and j - i < 50:
            j += 1
        app.send(ev[i][0], [r for _, r, _ in ev[i:j]], [t for _, _, t in ev[i:j]])
        i = j
    assert app.engine.d.stats().plan_queries[4] > 0 and app.engine.total > 20


# ---- 7. K_chain segments -------------------------------------------------------------------------------
CHAIN3_SRC = "define stream A (p float); define stream B (p float); define stream C (p float); " + " ".join(
    f"@info(name='q{i}') from every e1=A[p > {60 + 2 * i}] -> e2=B[p > e1.p] -> e3=C[p < e2.p] within 60 milliseconds "
    f"select e1.p as a, e3.p as c, e2.p - e1.p as d insert into O;" for i in range(20))


def test_chain_segments_and_native_interleaved_push():
    from test_gpu_mixed import by_index, call_of, price
    app = three_app(CHAIN3_SRC, 1024)
    d = app.engine.d
    assert d.stats().plan_queries[2] == 20
    rng = np.random.default_rng(4)
    gens = [("A", price(0, 100)), ("B", price(0, 100)), ("C", price(0, 100))]
    t = 0
    # (a) run by run through sdh_engine_push
    for n in (130, 300):
        parts, order = call_of(rng.integers(0, 3, n), t, gens, rng)
        t += n
        for p, off, cnt in mixed_runs([len(x[1]) for x in parts], order):
            stream, ts, vals, nulls = parts[p]
            app.engine.send(app.ir.stream_index(stream), ts[off:off + cnt], vals[off:off + cnt], None)
            app.engine.compare()
    by_push = app.engine.total
    assert by_push > 50 and d.debug_mixed_pushes() == (0, 0)
    # (b) the same queries through native interleaved calls: the rows read the store at merged seqs
    for k, n in enumerate((65, 400, 64)):
        parts, order = call_of(rng.integers(0, 3, n), t, gens, rng)
        t += n
        app.engine.send_mixed(by_index(app, parts), order)
        got = app.engine.compare()
        rec = d.poll_records()
        assert rec.c_n == rec.n == got[5]
        assert d.debug_mixed_pushes() == (k + 1, 0) and app.engine.b.debug_mixed_pushes() == (k + 1, 0)
    assert app.engine.total - by_push > 100


# ---- 8. all three parts in one push --------------------------------------------------------------------
THREE_PARTS = (STOCK_STREAM + " " + float_patterns(70) +
               " @info(name='x3') from every e1=StockStream[price > 98] -> e2=StockStream[price < 3] "
               "-> e3=StockStream[price > e1.price] within 1 sec select e1.price as a, e3.volume as v, e2.symbol as s "
               "insert into X;"
               " @info(name='g') from every e1=StockStream[price > 99] -> e2=StockStream[volume > 990] or "
               "e3=StockStream[price < 0.5] within 200 milliseconds select e1.price as a, e2.volume as b, e3.price as c "
               "insert into G;")


def three_parts_app():
    app = three_app(THREE_PARTS, 1 << 14, stock=True)
    st = app.engine.d.stats()
    assert st.plan_queries[0] == 70 and st.plan_queries[2] == 1 and st.plan_queries[6] == 1
    return app


def test_all_three_parts_and_windows():
    app = three_parts_app()
    d = app.engine.d
    full = push_stock(app, 0, 6000)
    total = full[5]
    equal_exactly(d.records_rows(), full)  # two identical calls
    rec = d.poll_records()
    n1, n2, n3 = rec.r_n, rec.f_n, rec.c_n
    assert n1 > 1000 and n2 > 5 and n3 > 5 and n1 + n2 + n3 == total
    assert np.all(full[0][:n1] < 70) and np.all(full[0][n1:n1 + n2] == 71) and np.all(full[0][n1 + n2:] == 70)
    equal_exactly(d.records_rows(), full)  # and the same after poll_records

    def window(first, n):
        w = d.records_rows(first, n)
        assert w[5] == total
        equal_exactly(w, [full[k][:, first:first + n] if k == 3 else full[k][first:first + n] for k in range(5)])
        return len(w[0])

    for b in (n1, n1 + n2):  # windows that start and end at the part boundaries and one row to either side
        for first in (b - 1, b, b + 1):
            for end in (b - 1, b, b + 1, total):
                if end > first:
                    assert window(first, end - first) == end - first
        for first in (0, b - 70):
            for end in (b - 1, b, b + 1):
                assert window(first, end - first) == end - first
    assert window(0, n1) == n1 and window(n1, n2) == n2 and window(n1 + n2, n3) == n3
    assert window(total - 1, 5) == 1
    assert window(total, 5) == 0 and window(total + 9, 5) == 0 and window(0, 0) == 0
    # the next push's rows replace these
    nxt = push_stock(app, 6000, 3000)
    assert nxt[5] != total and not np.array_equal(nxt[2][:10], full[2][:10])


# ---- 9. the host form equals the device form -----------------------------------------------------------
def test_device_arrays_equal_host_form():
    import torch
    app = three_parts_app()
    d = app.engine.d
    host = push_stock(app, 0, 6000)
    r, total = d.records_rows(device=True)
    n, w = r.n, r.width
    assert n == total == host[5] and w == 3

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


# ---- 10. failures leave everything as it was -----------------------------------------------------------
def _state(e):
    st = e.stats()
    return (st.events, st.pattern_events, st.matches, st.live_partials, e.pending_matches())


def _fails(e, code, *args, **kw):
    before = _state(e)
    with pytest.raises(EngineError) as ex:
        e.records_rows(*args, **kw)
    assert ex.value.code == code, ex.value
    assert _state(e) == before
    return str(ex.value)


def test_failures_change_nothing():
    src = STOCK_STREAM + " " + float_patterns(8)
    app = App(src, engine_factory=lambda blob: None)
    types = [s.attr_types for s in app.ir.streams]
    ts, sym, price, vol = stock_events(0, 3000)
    cols = [sym, price.view(np.uint32), vol]
    d = HipEngine(app.blob, stream_types=types, flags=SDH_FLAG_DEVICE_MATCHES)
    _fails(d, E_INVALID)  # no retain_events (and, on a build without the entry point, no symbol)
    d.push_columns(0, ts, cols)
    assert d.pending_matches() > 0
    assert "retain_events" in _fails(d, E_INVALID)
    d.retain_events(4096)
    for args in ((-1, 5), (0, -1), (-3, -3)):
        _fails(d, E_INVALID, *args)
    normal = HipEngine(app.blob, stream_types=types)
    normal.retain_events(4096)
    normal.push_columns(0, ts, cols)
    assert "SDH_FLAG_DEVICE_MATCHES" in _fails(normal, E_INVALID)
    assert len(normal.poll_rows()[0]) == normal.stats().matches > 0  # the window stayed pending
    # a query with 65 outputs
    wide = App(STOCK_STREAM + " @info(name='w') from every e1=StockStream[price > 98] -> e2=StockStream[price > e1.price] "
               "within 200 milliseconds select " + ", ".join(f"e1.volume + {k} as o{k}" for k in range(65)) +
               " insert into W;", engine_factory=lambda blob: None)
    w = HipEngine(wide.blob, stream_types=types, flags=SDH_FLAG_DEVICE_MATCHES)
    w.retain_events(4096)
    w.push_columns(0, ts, cols)
    assert w.pending_matches() > 0
    _fails(w, E_UNSUPPORTED)
    assert w.poll_records().n > 0


def test_an_event_that_left_the_store():
    from siddhi_amd.events import encode_rows
    src = ("define stream S (v int, w long); "
           "@info(name='long') from every e1=S[v == -1] -> e2=S[v == -2] select e1.w as a, e2.w as b insert into P;")
    app = three_app(src, 64, twin_retain=1024)
    d = app.engine.d
    t = 1000

    def burst():
        nonlocal t
        vs = [-1] + [0] * 100 + [-2]
        rows, ts = [[v, 7 * (t + k)] for k, v in enumerate(vs)], [t + k for k in range(len(vs))]
        t += len(vs)
        return rows, ts
    rows, ts = burst()
    vals, nulls = encode_rows(rows, app.ir.streams[0].attr_types, app.dictionary)
    app.engine.send(0, ts, vals, nulls)  # e1 is 101 events old when e2 arrives; the store keeps 64
    assert d.pending_matches() == 1
    assert "retain_events" in _fails(d, E_CAPACITY)
    assert d.poll_records().n == 1  # the record stayed where it was
    assert len(app.engine.b.poll_rows()[0]) == 1
    d.retain_events(256)
    rows, ts = burst()
    app.send("S", rows, ts)  # a larger retention and the next push succeed
    assert app.engine.total == 1 and app.engine.last[3][0][0] == 7 * (t - 102)
