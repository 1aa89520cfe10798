"""GPU parity of K_wave (nfa_wave.hip): unpartitioned count patterns `every e1=S[f1] -> e2=S[f2]<min:max>
-> e3=S[f3] [within T]`, one wave per query and one lane per partial, against the oracle -- planning
and the switches that keep the family on K_gen, page and tile boundaries with forced table growth,
more live partials than a K_gen instance holds, many queries beside other plans, every delivery form,
the wide record, snapshot / restore and sharding."""
import numpy as np
import pytest

from harness import App, oracle_lib
from part_lower_host import STREAM
from wave_host import DEEP_APP, deep_events, pv_events, wave_events, wave_queries, wave_query

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


def oracle_live(o):
    return int(oracle_lib().oracle_live_partials(o.engine.h))


def _run_pair(src, ts, vals, nl, batch, chunk=False, **kw):
    """The oracle and the engine on one app, push by push; the matches equal in order."""
    o, g = App(src), _hip_app(src, **kw)
    total = 0
    for lo in range(0, len(ts), batch):
        sl = slice(lo, lo + batch)
        o.engine.send(0, ts[sl], vals[sl], nl[sl], chunk)
        g.engine.send(0, ts[sl], vals[sl], nl[sl], chunk)
        om, gm = o.engine.take_matches(_nq(o)), g.engine.take_matches(_nq(o))
        assert gm == om, f"batch at {lo}: {len(gm)} vs {len(om)} matches"
        total += len(om)
    return o, g, total


# ---- 1. planning ----

def test_family_plans_on_kwave_and_the_switches_keep_it_on_kgen():
    src = wave_queries(1, n=20, withins=(3, 12, 50))  # (`within` everywhere: the K_gen legs stay inside their pools)
    ts, vals, nl = wave_events(1, 2000, unordered=True)
    _, g, total = _run_pair(src, ts, vals, nl, 700)
    st = g.engine.stats()
    assert st.plan_queries[7] == 20 and st.plan_queries[6] == 0 and total > 100
    want = st.matches
    for kw in (dict(debug={"SDH_NO_KWAVE": "1"}), dict(flags=SDH_FLAG_FORCE_GEN)):
        _, k, _ = _run_pair(src, ts, vals, nl, 700, **kw)
        st = k.engine.stats()
        assert st.plan_queries[7] == 0 and st.plan_queries[6] == 20 and st.matches == want


def test_live_partials_equal_kgens_and_the_oracles():
    """live_partials push by push, on random streams whose pushes end on events that pass f1 for some
    queries and not for others: K_wave reports what K_gen reports for the same queries (pending-list
    entries of the non-start states), and the oracle's count less the start states' pending seeds,
    which the host driver (tests/wave_host.py) keeps."""
    from wave_host import WaveHostEngine
    src = wave_queries(2, n=20, withins=(3, 12, 50))
    ts, vals, nl = wave_events(2, 2100, unordered=True)
    o, w, k = App(src), _hip_app(src), _hip_app(src, debug={"SDH_NO_KWAVE": "1"})
    h = WaveHostEngine(o.blob)
    assert w.engine.stats().plan_queries[7] == 20 and k.engine.stats().plan_queries[6] == 20
    seeds = set()
    for lo in range(0, len(ts), 300):
        sl = slice(lo, lo + 300)
        for x in (o.engine, w.engine, k.engine, h):
            x.send(0, ts[sl], vals[sl], nl[sl])
        om = o.engine.take_matches(_nq(o))
        assert w.engine.take_matches(_nq(o)) == om and k.engine.take_matches(_nq(o)) == om
        h.take_matches(_nq(o))
        live = w.engine.stats().live_partials
        assert live == k.engine.stats().live_partials, f"push at {lo}"
        assert live == h.live() == oracle_live(o) - h.seeds(), f"push at {lo}"
        seeds.add(h.seeds())
    assert live > 0 and max(seeds) > 0  # (the seed term was there)


def test_declined_shapes_plan_on_kgen():
    from test_wave_host import DECLINES
    for name in ("max = 9", "min = 0", "<2:>", "f2 reads e1", "f3 reads e2[1]", "a second stream", "an and state"):
        st = _hip_app(DECLINES[name][0]).engine.stats()
        assert st.plan_queries[7] == 0 and st.plan_queries[6] == 1, name
    st = _hip_app(DECLINES["partitioned"][0]).engine.stats()
    assert st.plan_queries[7] == 0 and st.plan_queries[3] == 1
    st = _hip_app(DECLINES["a sequence"][0]).engine.stats()
    assert st.plan_queries[7] == 0 and st.plan_queries[5] + st.plan_queries[6] == 1


# ---- 2. boundaries ----

def test_page_tile_and_push_boundaries():
    """One query, tables that start at one page. Every event passes f1 and none f2 until the end, so
    the live partials are the events so far: pushes of 1, 63, 64, 65 and 130 events take them through
    63 -> 64 -> 65 and 128 -> 129; every tile has 64 events passing f1, a partial opened by its last
    event, and each push one opened by its last event. Then two events fill every chain to `min`, and
    the first event of the next push completes every partial."""
    p = np.concatenate([np.tile(np.arange(2, 9, dtype=np.float32), 47)[:323], [6000, 6001], [7000, 3, 4]])
    ts, vals, nl = pv_events(p)
    o, g = App(DEEP_APP), _hip_app(DEEP_APP, debug={"SDH_KWAVE_CAP": "64"})
    assert g.engine.stats().plan_queries[7] == 1
    lo, lives = 0, []
    for n in (1, 63, 64, 65, 130, 2, 3):
        sl = slice(lo, lo + n)
        o.engine.send(0, ts[sl], vals[sl], nl[sl])
        g.engine.send(0, ts[sl], vals[sl], nl[sl])
        om = o.engine.take_matches(_nq(o))
        assert g.engine.take_matches(_nq(o)) == om, f"push of {n} at {lo}"
        lives.append(g.engine.stats().live_partials)
        # (every push's last event passes f1: the oracle's count holds no start-state seed)
        assert lives[-1] == oracle_live(o), f"push of {n} at {lo}"
        if n == 3:
            assert len(om) == 323  # the 323 partials with two chain events complete on 7000, the push's first event
        lo += n
    assert lives[:5] == [0, 63, 127, 192, 322]  # (the partial a push's last event opens is not pending yet)
    assert g.engine.stats().pool_regrows >= 1


# ---- 3. past K_gen's pools ----

def test_past_the_kgen_pools():
    """4,200 events open a partial each and none passes f2: 4,200 partials short of `min`, which no
    `within` check reaches -- past kgen.h's GMAXPOOL = 4,096 StateEvents, where the general interpreter
    ends with SDH_E_CAPACITY. Then 6000, 6001, 6002 fill the chains and 7000 completes them. The oracle
    holds 4,199 pending partials after the first 4,200 events, returns 4,201 matches, and keeps 2."""
    ts, vals, nl = deep_events()
    o, g = App(DEEP_APP), _hip_app(DEEP_APP)
    assert g.engine.stats().plan_queries[7] == 1
    got, want = [], []
    for lo in range(0, len(ts), 500):
        sl = slice(lo, lo + 500)
        o.engine.send(0, ts[sl], vals[sl], nl[sl])
        g.engine.send(0, ts[sl], vals[sl], nl[sl])
        want += o.engine.take_matches(_nq(o))
        got += g.engine.take_matches(_nq(o))
        assert g.engine.stats().live_partials == oracle_live(o), f"push at {lo}"
        if lo == 3500:  # (4,000 events so far, each a partial; the last one joins its list at the next event)
            assert oracle_live(o) == 3999
    assert len(want) == 4201 and got == want
    st = g.engine.stats()
    assert st.live_partials == 2 and st.pool_regrows >= 1 and st.plan_queries[7] == 1


# ---- 4. many queries, mixed plans ----

def test_many_queries_beside_other_plans():
    """130 K_wave queries of one shape with different constants, 3 of a second shape (<1:8>, f3 reading
    nothing captured), a K_ratchet query and a declined count query on K_gen, on one stream: the merged
    poll order is the oracle's."""
    qs = [wave_query(i, 40 + (i * 7) % 55, 500 + (i * 13) % 400, (2, 5), "p > e1.p and v >= e2[0].v", [-1, 30][i % 2])
          for i in range(130)]
    qs += [wave_query(130 + i, 70 + 5 * i, 800, (1, 8), "v > 850", -1) for i in range(3)]
    qs.append("@info(name='r') from every e1=S[p > 50] -> e2=S[p > e1.p] within 20 milliseconds "
              "select e1.p as a insert into O;")
    qs.append("@info(name='g') from every e1=S[p > 90] -> e2=S[v > 700]<1:9> -> e3=S[p > e1.p] within 50 milliseconds "
              "select e1.p as a insert into O;")
    ts, vals, nl = wave_events(4, 3000, nulls=0.05)
    _, g, total = _run_pair(f"{STREAM} {' '.join(qs)}", ts, vals, nl, 700)
    st = g.engine.stats()
    assert st.plan_queries[7] == 133 and st.plan_queries[0] == 1 and st.plan_queries[6] == 1
    assert total > 2000


# ---- 5. delivery forms ----

def test_device_records_count_equals_normal_mode():
    src = wave_queries(5, n=20)
    ts, vals, nl = wave_events(5, 3000)
    _, g, total = _run_pair(src, ts, vals, nl, 1000)
    d = _hip_app(src, flags=SDH_FLAG_DEVICE_MATCHES)
    n = 0
    for lo in range(0, 3000, 1000):
        d.engine.send(0, ts[lo:lo + 1000], vals[lo:lo + 1000], nl[lo:lo + 1000])
        rec = d.engine.poll_records()
        assert rec.n == rec.f_n
        n += rec.n
    assert n == total == d.engine.stats().matches and total > 100


def test_compact_ex_equals_poll():
    from test_gpu_compact import _ex_equals_poll
    src = wave_queries(6, n=12)
    ts, vals, nl = wave_events(6, 3000)
    a, b = _hip_app(src), _hip_app(src)
    total = 0
    for lo in range(0, 3000, 1000):
        for x in (a, b):
            x.engine.send(0, ts[lo:lo + 1000], vals[lo:lo + 1000], nl[lo:lo + 1000])
        total += _ex_equals_poll(a.engine, b.engine, False, False)
    assert total > 100


def test_poll_rows_equals_the_selector():
    """select e1.p as a, e2[0].p as b, e2[last].p as c, e3.p as d through the device selector."""
    from test_gpu_rows import check_polled
    src = wave_queries(7, n=12)
    ts, vals, nl = wave_events(7, 2000)
    a, b = _hip_app(src), _hip_app(src)
    b.engine.retain_events(4096)
    total = 0
    for lo in range(0, 2000, 500):
        for x in (a, b):
            x.engine.send(0, ts[lo:lo + 500], vals[lo:lo + 500], nl[lo:lo + 500])
            x.log.append(0, ts[lo:lo + 500], vals[lo:lo + 500], nl[lo:lo + 500])
        matches, _ = check_polled(a, a.engine.poll(with_seq=True), b.engine.poll_rows(), 4)
        total += len(matches)
    assert total > 100


def test_chunk_push():
    src = wave_queries(8, n=12)
    ts, vals, nl = wave_events(8, 3000)
    _, g, total = _run_pair(src, ts, vals, nl, 1000, chunk=True)
    assert total > 100 and g.engine.stats().plan_queries[7] == 12


# ---- 6. records ----

def test_wide_record_equals_narrow():
    """SDH_KWAVE_WIDE forces the K_gen-format record a match takes when a distance passes int32."""
    src = wave_queries(9, n=20)
    ts, vals, nl = wave_events(9, 3000, unordered=True)
    a, b = _hip_app(src), _hip_app(src, debug={"SDH_KWAVE_WIDE": "1"})
    total = 0
    for lo in range(0, 3000, 750):
        for x in (a, b):
            x.engine.send(0, ts[lo:lo + 750], vals[lo:lo + 750], nl[lo:lo + 750])
        u, v = a.engine.poll(with_seq=True), b.engine.poll(with_seq=True)
        for x, y in zip(u, v):
            assert np.array_equal(x, y)
        total += len(u[0])
    assert total > 100


# ---- 7. snapshot ----

def test_snapshot_restore():
    src = wave_queries(10, n=16)
    ts, vals, nl = wave_events(10, 3000)
    o, a = App(src), _hip_app(src, debug={"SDH_KWAVE_CAP": "64"})
    snap, b = None, None
    for i, lo in enumerate(range(0, 3000, 500)):
        sl = slice(lo, lo + 500)
        o.engine.send(0, ts[sl], vals[sl], nl[sl])
        a.engine.send(0, ts[sl], vals[sl], nl[sl])
        om = o.engine.take_matches(_nq(o))
        assert a.engine.take_matches(_nq(o)) == om
        if b is not None:
            b.engine.send(0, ts[sl], vals[sl], nl[sl])
            assert b.engine.take_matches(_nq(o)) == om
            assert b.engine.stats().live_partials == a.engine.stats().live_partials
        if i == 2:  # after push 3 of 6, into a fresh engine
            snap = a.engine.snapshot()
            b = _hip_app(src)
            b.engine.restore(snap)
            assert b.engine.snapshot() == snap  # byte for byte
    assert np.frombuffer(snap[:16], np.int64)[1] == 10
    # an engine without K_wave queries still writes version 8, and each refuses the other's blob
    from siddhi_amd.engine import EngineError
    c = _hip_app(src, debug={"SDH_NO_KWAVE": "1"})
    c.engine.send(0, ts[:500], vals[:500], nl[:500])
    csnap = c.engine.snapshot()
    assert np.frombuffer(csnap[:16], np.int64)[1] == 8
    with pytest.raises(EngineError):
        c.engine.restore(snap)
    with pytest.raises(EngineError):
        b.engine.restore(csnap)


# ---- 8. sharding ----

def test_two_shards():
    src = wave_queries(12, n=6)
    ts, vals, nl = wave_events(12, 2000)
    o = App(src)
    ranks = [_hip_app(src, shard_rank=r, shard_world=2) for r in (0, 1)]
    assert [r.engine.stats().plan_queries[7] for r in ranks] == [3, 3]
    total = 0
    for lo in range(0, 2000, 500):
        sl = slice(lo, lo + 500)
        o.engine.send(0, ts[sl], vals[sl], nl[sl])
        om = o.engine.take_matches(_nq(o))
        got = []
        for r in ranks:
            r.engine.send(0, ts[sl], vals[sl], nl[sl])
            got += r.engine.take_matches(_nq(o))
        assert sorted(got) == sorted(om) and len(got) == len(om)
        total += len(om)
    assert total > 50
