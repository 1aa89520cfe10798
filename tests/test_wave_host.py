"""K_wave's shape selection (siddhi_amd/csrc/wave_lower.h) on planned blobs, and its per-partial step
(wave_step.h) run on the host by a driver that walks pages and tiles as the kernel does, against the
CPU oracle. CPU only; the GPU kernel is checked in test_gpu_wave.py."""
import pytest

from harness import App, oracle_lib
from part_lower_host import STREAM
from wave_host import (COUNTS, DEEP_APP, F3, F3_KEPT, PK_COUNT, WaveHostEngine, deep_events, wave_events,
                       wave_queries, wave_query)


def _host(src, tile=64):
    return App(src, engine_factory=lambda blob: WaveHostEngine(blob, tile=tile))


def _one(body, streams=STREAM):
    return f"{streams} @info(name='q') from {body} select e1.p as a insert into O;"


# ---- shape selection ----

def test_accepts_the_shape():
    for (lo, hi) in COUNTS:
        for kind, texts in F3.items():
            for f3 in texts:
                for within in (-1, 20):
                    app = _host(f"{STREAM} {wave_query(0, 60, 700, (lo, hi), f3, within)}")
                    s = app.engine.shape(0)
                    assert s[0] == PK_COUNT and s[3] == hi, (f3, app.engine.why(0))
                    assert tuple(bool(x) for x in s[4:7]) == F3_KEPT[kind], f3
                    assert app.engine.why(0) == ""
                    assert app.engine.shape(0, kpart=True)[0] == -1  # (unpartitioned: never K_part's)


T_STREAM = STREAM + " define stream T (k int, p float, v int, d double);"
DECLINES = {
    "max = 9": (_one("every e1=S[p > 1] -> e2=S[v > 5]<1:9> -> e3=S[p > e1.p]"), "count max beyond PK_CMAX"),
    "min = 0": (_one("every e1=S[p > 1] -> e2=S[v > 5]<0:3> -> e3=S[p > e1.p]"), "count min below 1"),
    "<2:>": (_one("every e1=S[p > 1] -> e2=S[v > 5]<2:> -> e3=S[p > e1.p]"), "an unbounded count"),
    "f2 reads e1": (_one("every e1=S[p > 1] -> e2=S[v > e1.v]<2:5> -> e3=S[p > e1.p]"),
                    "f2 reads more than the current event"),
    "f3 reads e2[1]": (_one("every e1=S[p > 1] -> e2=S[v > 5]<2:5> -> e3=S[p > e2[1].p]"),
                       "f3 reads a chain event other than e2[0] / e2[last]"),
    "a second stream": (_one("every e1=S[p > 1] -> e2=S[v > 5]<2:5> -> e3=T[p > e1.p]", T_STREAM),
                        "a second stream, or a state-level within / callback"),
    "partitioned": (f"{STREAM} partition with (k of S) begin @info(name='q') from every e1=S[p > 1] -> "
                    "e2=S[v > 5]<2:5> -> e3=S[p > e1.p] select e1.p as a insert into O; end;",
                    "a partitioned query (K_part)"),
    "a sequence": (_one("every e1=S[p > 1], e2=S[v > 5]<2:5>, e3=S[p > e1.p]"), "a sequence"),
    "an and state": (_one("every e1=S[p > 1] -> e2=S[v > 5] and e3=S[p > 50]"), "a logical state"),
    "count first": (_one("every e1=S[p > 1]<2:5> -> e2=S[v > 5] -> e3=S[p > 50]"), None),
    "count last": (_one("every e1=S[p > 1] -> e2=S[v > 5] -> e3=S[p > 50]<2:5>"), None),
    "a plain chain": (_one("every e1=S[p > 1] -> e2=S[v > 5] -> e3=S[p > e1.p]"), "no count state in the middle"),
}


@pytest.mark.parametrize("name", sorted(DECLINES))
def test_declines_with_its_reason(name):
    src, why = DECLINES[name]
    app = _host(src)
    assert app.engine.shape(0)[0] == -1
    assert app.engine.why(0) != ""
    if why is not None:
        assert app.engine.why(0) == why


def test_partitioned_twin_is_kparts_count():
    """The same pattern inside a partition is K_part's PK_COUNT with the same captured words."""
    for kind, texts in F3.items():
        body = f"every e1=S[p > 60] -> e2=S[v > 700]<2:5> -> e3=S[{texts[0]}] select e1.p as a insert into O;"
        w = _host(f"{STREAM} @info(name='q') from {body}").engine
        p = _host(f"{STREAM} partition with (k of S) begin @info(name='q') from {body} end;").engine
        assert w.shape(0) == p.shape(0, kpart=True) and w.shape(0)[0] == PK_COUNT
        assert p.shape(0)[0] == -1 and p.why(0) == "a partitioned query (K_part)"


def test_kpart_shape_answers_on_these_apps():
    """kpart_shape shares its helpers with wave_shape now; tests/test_part_lower_host.py pins its answers
    on the K_part tests' apps. On this file's apps it answers (kind, sA, sB, cmax, n_e1, n_first,
    n_last) as the commit before the shared helpers did: none of them is a K_part shape but the
    partitioned one, a PK_COUNT whose f3 reads e1 (two captured words)."""
    for name, (src, _) in DECLINES.items():
        want = (PK_COUNT, 1, 2, 5, 2, 0, 0) if name == "partitioned" else (-1, 1, 2, 0, 0, 0, 0)
        assert _host(src).engine.shape(0, kpart=True) == want, name


# ---- the step against the oracle ----

def oracle_live(o):
    return int(oracle_lib().oracle_live_partials(o.engine.h))


def _against_oracle(src, ts, vals, nl, tile, batch):
    o, h = App(src), _host(src, tile)
    nq = lambda q: len(o.ir.queries[q].states)  # noqa: E731
    assert all(h.engine.shape(qi)[0] == PK_COUNT for qi in range(len(o.ir.queries)))
    total = 0
    for lo in range(0, len(ts), batch):
        sl = slice(lo, lo + batch)
        o.engine.send(0, ts[sl], vals[sl], nl[sl])
        h.engine.send(0, ts[sl], vals[sl], nl[sl])
        om = o.engine.take_matches(nq)
        assert h.engine.take_matches(nq) == om, f"push at {lo}"
        # the oracle counts every pending list, the start states' seeds included
        assert h.engine.live() + h.engine.seeds() == oracle_live(o), f"push at {lo}"
        total += len(om)
    return total


@pytest.mark.parametrize("tile", [1, 3, 64])
@pytest.mark.parametrize("seed", range(8))
def test_wave_step_equals_oracle(seed, tile):
    """20 queries: every <min:max> of COUNTS with f3 reading e1, e2[0], e2[last], nothing captured and
    all three; `within` absent and 3-50 ms; 30 % null captured attributes; odd seeds with out-of-order
    timestamps; pushes of several sizes."""
    src = wave_queries(seed, n=20)
    ts, vals, nl = wave_events(seed, 1500, nulls=0.3, unordered=seed % 2 == 1)
    total = _against_oracle(src, ts, vals, nl, tile, [1500, 1, 333, 64, 65, 130, 63, 500][seed])
    assert total > 100


@pytest.mark.parametrize("reads", sorted(F3))
@pytest.mark.parametrize("cnt", COUNTS, ids=[f"{a}_{b}" for a, b in COUNTS])
def test_each_count_with_each_f3(cnt, reads):
    """Every (<min:max>, what f3 reads) pair on its own, with and without `within`, no nulls dropped:
    each case must produce matches."""
    qs = [wave_query(i, 60 + 5 * i, 600 + 40 * i, cnt, F3[reads][i % len(F3[reads])], w)
          for i, w in enumerate((-1, 3, 50, 12))]
    ts, vals, nl = wave_events(11, 1200, nulls=0.3, unordered=True)
    total = _against_oracle(f"{STREAM} {' '.join(qs)}", ts, vals, nl, 64, 300)
    assert total > 0


def test_deep_table_equals_oracle():
    """The stream that outgrows a K_gen instance's pools: 4,200 partials short of `min`, then the
    events that complete them. The oracle holds 4,199 pending partials after the first 4,200 events
    (the last one joins its list at the next event), returns 4,201 matches and keeps 2."""
    ts, vals, nl = deep_events()
    o, h = App(DEEP_APP), _host(DEEP_APP)
    nq = lambda q: 3  # noqa: E731
    got, want = [], []
    for lo in range(0, len(ts), 500):
        sl = slice(lo, lo + 500)
        o.engine.send(0, ts[sl], vals[sl], nl[sl])
        h.engine.send(0, ts[sl], vals[sl], nl[sl])
        want += o.engine.take_matches(nq)
        got += h.engine.take_matches(nq)
        assert h.engine.live() + h.engine.seeds() == oracle_live(o)
        if lo + 500 == 4000:
            assert oracle_live(o) == 3999
    assert len(want) == 4201 and got == want
    assert oracle_live(o) == 2 and h.engine.live() == 2
