"""GPU parity of K_part's chain kind (part_body.h chain_tile): partitioned same-stream chains
`every e1=S[f1] -> e2=S[f2] [-> e3=S[f3] [-> e4=S[f4]]] [within T]` on compact partial tables, against
the oracle -- random filters over the earlier slots, `within` windows, nulls, out-of-order timestamps,
batched pushes, the order of one event's matches, forced table growth, more live partials than a
K_gen instance holds, compiled against interpreted kernels, K_part against K_gen, snapshot / restore,
device records (the chain record, and the wide path) and chunk pushes."""
import ctypes

import numpy as np
import pytest

from harness import App
from part_lower_host import STREAM, chain_events, chain_queries

pytestmark = pytest.mark.gpu

SDH_FLAG_DEVICE_MATCHES = 1
SDH_FLAG_FORCE_GEN = 4


def _hip_app(src, **kw):
    from siddhi_amd.engine import HipEngine
    app = App(src, engine_factory=lambda blob: None)
    app.engine = HipEngine(app.blob, stream_types=[s.attr_types for s in app.ir.streams], **kw)
    return app


def _nq(app):
    return lambda q: len(app.ir.queries[q].states)


def _run_pair(o_src, g_src, ts, vals, nl, batch, chunk=False, **kw):
    """The oracle on o_src and the engine on g_src (the same app, or its function-free twin for the
    oracle), push by push; the matches equal in order."""
    o = App(o_src)
    g = _hip_app(g_src, **kw)
    items = 0
    for lo in range(0, len(ts), batch):
        sl = slice(lo, lo + batch)
        o.engine.send(0, ts[sl], vals[sl], nl[sl], chunk)
        g.engine.send(0, ts[sl], vals[sl], nl[sl], chunk)
        om, gm = o.engine.take_matches(_nq(o)), g.engine.take_matches(_nq(o))
        assert gm == om, f"batch at {lo}: {len(gm)} vs {len(om)} matches"
        items = max(items, g.engine.stats().last_part_items)
    return o, g, items


# ---- 1. random apps ----

@pytest.mark.parametrize("seed", range(8))
def test_chain_random_apps(seed):
    src = chain_queries(seed)
    ts, vals, nl = chain_events(seed, 6000, keys=3 + seed % 5, unordered=seed % 4 == 3)
    _, g, items = _run_pair(chain_queries(seed, twin=True), src, ts, vals, nl, batch=[500, 1, 7, 6000][seed % 4])
    st = g.engine.stats()
    assert st.plan_queries[3] == 24 and items > 0  # every query on K_part
    assert st.matches > 100


# ---- 2. the order of one event's matches ----

def _ordered(src, rows):
    """rows: (p, v) of one key's events, 1 ms apart -> the engine's match tuples, equal to the oracle's."""
    n = len(rows)
    ts = np.arange(n, dtype=np.int64)
    p = np.array([r[0] for r in rows], np.float32)
    v = np.array([r[1] for r in rows], np.int64)
    vals = np.stack([np.zeros(n, np.int64), p.view(np.uint32).astype(np.int64), v, np.zeros(n, np.int64)], 1)
    nl = np.zeros((n, 4), np.uint8)
    o, g = App(src), _hip_app(src)
    o.engine.send(0, ts, vals, nl)
    g.engine.send(0, ts, vals, nl)
    om = o.engine.take_matches(_nq(o))
    gm = g.engine.take_matches(_nq(o))
    assert g.engine.stats().plan_queries[3] == 1
    assert gm == om
    return [m[3] for m in gm]


def test_chain_order_three_states():
    """e1 at seq 0 and 1; seq 1's partial passes f2 first (seq 2), seq 0's after it (seq 3); both
    complete at seq 4: the later-opened partial's row comes first."""
    src = (f"{STREAM} partition with (k of S) begin @info(name='q') from every e1=S[p > 10] -> e2=S[v > e1.v] -> "
           f"e3=S[p > 90] select e1.p as a insert into O; end;")
    slots = _ordered(src, [(20, 50), (20, 10), (5, 30), (5, 60), (95, 0)])
    assert slots == [((1,), (2,), (4,)), ((0,), (3,), (4,))]


def test_chain_order_four_states():
    """The most significant key is the last earlier slot's seq: seq 1's partial reaches e3's list first
    (seq 2 against seq 3) but e4's list second (seq 5 against seq 4)."""
    src = (f"{STREAM} partition with (k of S) begin @info(name='q') from every e1=S[p > 10] -> e2=S[v > e1.v] -> "
           f"e3=S[v < e2.v] -> e4=S[p > 90] select e1.p as a insert into O; end;")
    slots = _ordered(src, [(20, 50), (20, 10), (5, 30), (5, 60), (5, 40), (5, 20), (95, 0)])
    assert slots == [((0,), (3,), (4,), (6,)), ((1,), (2,), (5,), (6,))]


# ---- 3. growth ----

@pytest.mark.parametrize("cap", [1, 2])
def test_chain_table_growth_reruns_exactly(cap, monkeypatch):
    """Tiny initial tables (SDH_KPART_CAP): every overflow is undone and re-run with twice the room;
    device-record mode counts the same matches."""
    monkeypatch.setenv("SIDDHI_HIP_DEBUG", f"SDH_KPART_CAP={cap}")
    src, twin = chain_queries(77, n=12), chain_queries(77, n=12, twin=True)
    ts, vals, nl = chain_events(77, 5000, keys=2)
    _, g, _ = _run_pair(twin, src, ts, vals, nl, batch=1000)
    assert g.engine.stats().pool_regrows >= 1
    d = _hip_app(src, flags=SDH_FLAG_DEVICE_MATCHES)
    for lo in range(0, len(ts), 1000):
        d.engine.send(0, ts[lo:lo + 1000], vals[lo:lo + 1000], nl[lo:lo + 1000])
    assert d.engine.stats().matches == g.engine.stats().matches


# ---- 4. more live partials than a K_gen instance holds ----

def test_chain_past_the_kgen_pool(monkeypatch):
    """4,200 events of key 0 pass f1 with strictly falling prices -- no match, 4,200 live partials,
    past kgen.h's GMAXPOOL = 4,096 -- then one event above them all completes every one of them.
    The tables grow from the default 16 entries past 4,096. (The shape-compiled kernel runs it: one
    lane walks the whole table serially, DESIGN 3.3 "Chains".)"""
    monkeypatch.setenv("SIDDHI_HIP_DEBUG", "SDH_SPEC=require")
    src = (f"{STREAM} partition with (k of S) begin @info(name='q') from every e1=S[p > 1] -> e2=S[p > e1.p] "
           f"select e1.p as a, e2.p as b insert into O; end;")
    rng = np.random.default_rng(9)
    k, p = [], []
    fall = 0
    while fall < 4200:
        if rng.random() < 0.1:  # key 1: prices that never pass f1
            k.append(1)
            p.append(0.5)
        else:
            k.append(0)
            p.append(9000.0 - fall)
            fall += 1
    k.append(0)
    p.append(10000.0)
    n = len(k)
    ts = np.arange(n, dtype=np.int64)
    vals = np.stack([np.array(k, np.int64), np.array(p, np.float32).view(np.uint32).astype(np.int64),
                     np.zeros(n, np.int64), np.zeros(n, np.int64)], 1)
    nl = np.zeros((n, 4), np.uint8)
    o = App(src)
    g = _hip_app(src, gen_max_keys=64)
    got, want = [], []
    for lo in range(0, n, 500):
        sl = slice(lo, lo + 500)
        o.engine.send(0, ts[sl], vals[sl], nl[sl])
        g.engine.send(0, ts[sl], vals[sl], nl[sl])
        if lo + 500 < n:
            assert g.engine.stats().live_partials == int(np.sum(np.array(k[:lo + 500]) == 0))
        want += o.engine.take_matches(_nq(o))
        got += g.engine.take_matches(_nq(o))
    assert len(want) == 4200 and got == want
    st = g.engine.stats()
    assert st.pool_regrows >= 1 and st.plan_queries[3] == 1


# ---- 5. compiled equals interpreted ----

def _one_shape(n):
    qs = [f"@info(name='q{i}') from every e1=S[p > {10 + i % 80}.{i % 10}] -> e2=S[v > e1.v] -> e3=S[p > e2.p] "
          f"within {5 + i % 40} milliseconds select e1.p as a, e3.p as c insert into O;" for i in range(n)]
    return f"{STREAM} partition with (k of S) begin {' '.join(qs)} end;"


def test_chain_shape_compiled_equals_interpreted():
    src = _one_shape(130)
    ts, vals, nl = chain_events(3, 3000, keys=4)
    for flags in (0, SDH_FLAG_DEVICE_MATCHES):
        a = _hip_app(src, flags=flags, debug={"SDH_SPEC": "require"})
        b = _hip_app(src, flags=flags, debug={"SDH_SPEC": "0"})
        assert a.engine.stats().spec_kernels > 0 and b.engine.stats().spec_kernels == 0
        assert a.engine.stats().plan_queries[3] == 130
        for lo in (0, 1500):
            for x in (a, b):
                x.engine.send(0, ts[lo:lo + 1500], vals[lo:lo + 1500], nl[lo:lo + 1500])
                assert x.engine.stats().last_part_items > 0
            if flags:
                assert a.engine.stats().matches == b.engine.stats().matches
                continue
            for u, v in zip(a.engine.poll(), b.engine.poll()):
                assert np.array_equal(u, v)
        assert a.engine.stats().matches == b.engine.stats().matches > 1000


# ---- 6. K_part equals K_gen ----

def test_chain_kpart_equals_kgen():
    src = chain_queries(11)
    ts, vals, nl = chain_events(11, 3000, keys=4)
    a = _hip_app(src)
    b = _hip_app(src, flags=SDH_FLAG_FORCE_GEN, gen_pool_states=64, gen_pool_nodes=256, gen_list_cap=64)
    assert a.engine.stats().plan_queries[3] == 24 and b.engine.stats().plan_queries[3] == 0
    for lo, n in ((0, 1500), (1500, 1), (1501, 1499)):
        for x in (a, b):
            x.engine.send(0, ts[lo:lo + n], vals[lo:lo + n], nl[lo:lo + n])
        assert a.engine.stats().last_part_items > 0 and b.engine.stats().last_part_items == 0
        for u, v in zip(a.engine.poll(), b.engine.poll()):
            assert np.array_equal(u, v)
    assert a.engine.stats().matches > 500


# ---- 7. snapshot and restore ----

def test_chain_snapshot_restore():
    from siddhi_amd.engine import EngineError
    src, twin = chain_queries(5, n=18), chain_queries(5, n=18, twin=True)
    ts, vals, nl = chain_events(5, 4000, keys=4)
    o = App(twin)
    a = _hip_app(src)
    o.engine.send(0, ts[:2000], vals[:2000], nl[:2000])
    a.engine.send(0, ts[:2000], vals[:2000], nl[:2000])
    assert a.engine.take_matches(_nq(o)) == o.engine.take_matches(_nq(o))
    snap = a.engine.snapshot()
    b = _hip_app(src)
    b.engine.restore(snap)
    o.engine.send(0, ts[2000:], vals[2000:], nl[2000:])
    b.engine.send(0, ts[2000:], vals[2000:], nl[2000:])
    om = o.engine.take_matches(_nq(o))
    assert b.engine.take_matches(_nq(o)) == om and len(om) > 100
    # the same program planned without K_part keeps these chains in K_gen arenas: another layout
    c = _hip_app(src, debug={"SDH_NO_KPART": "1"})
    assert c.engine.stats().plan_queries[3] == 0
    with pytest.raises(EngineError):
        c.engine.restore(snap)


# ---- 8. device records ----

def _host(ptr, n, dtype):
    out = np.zeros(n, dtype)
    if n:
        lib = ctypes.CDLL("libamdhip64.so")
        lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        assert lib.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
    return out


def _walk_flat(rec):
    """Part 2 of the device records (include/siddhi_hip.h) -> [(query, key, trigger seq, slot words)]:
    a K_gen-format record starts with its positive length; a narrow one's low half of word 0 is
    -(words + kind << 16), kind 3 the chain record, kind 4 padding."""
    words = _host(rec.f_base, rec.f_words, np.int64)
    lo32 = lambda x: int(np.int32(np.uint32(int(x) & 0xFFFFFFFF)))  # noqa: E731
    hi32 = lambda x: int(np.int32(np.uint32((int(x) >> 32) & 0xFFFFFFFF)))  # noqa: E731
    key_tab, out, kinds, i = {}, [], set(), 0
    while i < len(words):
        l0 = lo32(words[i])
        if l0 >= 0:
            r = words[i:i + l0]
            assert (int(r[6]) >> 32) & 1  # a chain's wide record: tiebreaks from the slots
            out.append((int(r[1]), int(r[2]), int(r[4]), tuple(int(x) for x in r[7:l0])))
            kinds.add("wide")
            i += l0
            continue
        kind, nw = (-l0) >> 16, (-l0) & 0xFFFF
        assert nw > 0 and kind in (3, 4), (i, kind)
        if kind == 3:
            r = words[i:i + nw]
            q, sq, kid = hi32(r[0]), rec.seq_base + (int(r[1]) & 0xFFFFFFFF), (int(r[1]) >> 32) & 0xFFFFFFFF
            if q not in key_tab:  # f_query_keys[q]: the query's key table (device pointer)
                key_tab[q] = int(_host(rec.f_query_keys + 8 * q, 1, np.uint64)[0])
            key = int(_host(key_tab[q] + 8 * kid, 1, np.int64)[0])
            dist = [d for w in r[2:] for d in (lo32(w), hi32(w))]
            assert nw in (3, 4)
            slots = []
            for d in dist:
                if d != -(1 << 31):
                    slots += [1, sq - d]
            out.append((q, key, sq, tuple(slots + [1, sq])))
            kinds.add("narrow")
        i += nw
    assert i == len(words)
    return out, kinds


def test_chain_device_records():
    from siddhi_amd.engine import HipEngine
    src = chain_queries(21, n=18)
    ts, vals, nl = chain_events(21, 4000, keys=5)
    app = App(src, engine_factory=lambda blob: None)
    kw = dict(stream_types=[s.attr_types for s in app.ir.streams])
    normal = HipEngine(app.blob, **kw)
    wide = HipEngine(app.blob, debug={"SDH_KPART_WIDE": "1"}, **kw)
    devr = HipEngine(app.blob, flags=SDH_FLAG_DEVICE_MATCHES, **kw)
    devw = HipEngine(app.blob, flags=SDH_FLAG_DEVICE_MATCHES, debug={"SDH_KPART_WIDE": "1"}, **kw)
    total = 0
    for lo, n in ((0, 2500), (2500, 17), (2517, 1483)):
        for e in (normal, wide, devr, devw):
            e.send(0, ts[lo:lo + n], vals[lo:lo + n], nl[lo:lo + n])
        got = normal.poll(with_seq=True)
        for u, v in zip(got, wide.poll(with_seq=True)):  # the wide path: the same rows in the same order
            assert np.array_equal(u, v)
        q, k, t, off, words, seq, tb = got
        want = sorted((int(q[i]), int(k[i]), int(seq[i]), tuple(int(x) for x in words[off[i]:off[i + 1]]))
                      for i in range(len(q)))
        for e, kind in ((devr, "narrow"), (devw, "wide")):
            rec = e.poll_records()
            assert rec.n == rec.f_n == len(want)
            recs, kinds = _walk_flat(rec) if rec.f_n else ([], {kind})
            assert sorted(recs) == want and kinds == {kind}
        total += len(want)
    assert total > 300
    for e in (normal, wide, devr, devw):
        e.close()


# ---- 9. a chunk push, and compact rows ----

def test_chain_chunk_push():
    src, twin = chain_queries(13, n=12), chain_queries(13, n=12, twin=True)
    ts, vals, nl = chain_events(13, 3000, keys=4)
    _, g, items = _run_pair(twin, src, ts, vals, nl, batch=1000, chunk=True)
    assert items > 0 and g.engine.stats().matches > 100


def test_chain_compact_ex_equals_poll():
    from test_gpu_compact import _ex_equals_poll
    src = chain_queries(14, n=12)
    ts, vals, nl = chain_events(14, 3000, keys=4)
    a, b = _hip_app(src), _hip_app(src)
    total = 0
    for lo in range(0, 3000, 1000):
        for x in (a, b):
            x.engine.send(0, ts[lo:lo + 1000], vals[lo:lo + 1000], nl[lo:lo + 1000])
        total += _ex_equals_poll(a.engine, b.engine, True, False)
    assert total > 100


# ---- 10. a partition that keys two streams ----

def test_two_stream_partition():
    """Chains, a count chain and logical pairs over A and over B in one partition. A set's groups share
    one buffer selector per key, so every kind holds a set per stream, and a push over one stream runs
    that stream's sets only: the pushes come A, A, B, B, A, .. (the same stream twice in a row), and each
    push holds only some of the keys."""
    def qs(s, t):
        return [f"@info(name='{s}c2') from every e1={s}[p > 20] -> e2={s}[p > e1.p] within 30 milliseconds select e1.p as x insert into O;",
                f"@info(name='{s}c3') from every e1={s}[v > {t}] -> e2={s}[v < e1.v] -> e3={s}[p > e2.p] select e1.p as x insert into O;",
                f"@info(name='{s}n') from every e1={s}[p > {t // 10}] -> e2={s}[v > 300] <1:3> -> e3={s}[p > e2[last].p] within 40 milliseconds select e1.p as x insert into O;",
                f"@info(name='{s}a') from every e1={s}[p > 30] -> e2={s}[v > {t}] and e3={s}[d > 50.0] within 50 milliseconds select e1.p as x insert into O;",
                f"@info(name='{s}o') from every e1={s}[p > 60] -> e2={s}[v > 900] or e3={s}[d < 5.0] select e1.p as x insert into O;"]
    src = ("define stream A (k int, p float, v int, d double); define stream B (k int, p float, v int, d double); "
           f"partition with (k of A, k of B) begin {' '.join(qs('A', 300) + qs('B', 500))} end;")
    o, g = App(src), _hip_app(src)
    assert g.engine.stats().plan_queries[3] == 10
    total = 0
    for i in range(14):
        ts, vals, nl = chain_events(40 + i, 300, keys=5)
        keep = vals[:, 0] != i % 5  # (one key is missing from each push, another from the next)
        if i % 3 == 0:
            keep &= vals[:, 0] != (i + 2) % 5
        ts, vals, nl = ts[keep] + 700 * i, vals[keep], nl[keep]
        for x in (o, g):
            x.engine.send((i // 2) % 2, ts, vals, nl)
        om = o.engine.take_matches(_nq(o))
        assert g.engine.take_matches(_nq(o)) == om, f"push {i}"
        total += len(om)
    assert total > 500
