"""K_part's shape selection (siddhi_amd/csrc/part_lower.h) on planned blobs, the chain kind's per-
partial step (part_chain.h) run on the host against the CPU oracle, and the compile check of the
chain kind's generated kernels. CPU only; the GPU kernel is checked in test_gpu_part_chain.py."""
import ctypes

import pytest

from harness import App
from part_lower_host import (PK_AND, PK_CHAIN, PK_COUNT, PK_OR, STREAM, PartHostEngine, chain_events,
                             chain_queries)


def _shapes(src):
    app = App(src, engine_factory=PartHostEngine)
    return [app.engine.shape(qi) for qi in range(len(app.ir.queries))]


def _part(body, streams=STREAM, keys="k of S"):
    return f"{streams} partition with ({keys}) begin @info(name='q') from {body} insert into O; end;"


def test_existing_kinds_decide_as_before():
    """The C3 family and test_gpu_part's generator: count chains PK_COUNT, logical pairs PK_AND /
    PK_OR, each with the captured words its e3 reads."""
    from siddhi_amd.workloads import c3_app
    from test_gpu_part import _queries
    sh = _shapes(c3_app(30))
    assert [s.kind for s in sh] == [PK_COUNT, PK_AND, PK_OR] * 10
    for s in sh[0::3]:  # e3 = price > e2[last].price
        assert (s.cmax, s.kept) == (5, (False, False, True))
    for seed in (0, 5, 77):
        sh = _shapes(_queries(seed))
        assert [s.kind for s in sh] == [PK_COUNT, PK_AND, PK_OR] * 8
        assert all(s.sA in (1, 2) and s.sB == 3 - s.sA for s in sh)
        assert all(1 <= s.cmax <= 8 for s in sh[0::3])


@pytest.mark.parametrize("within", ["", " within 10 milliseconds"])
def test_chains_are_pk_chain(within):
    cases = [
        ("every e1=S[p > 20] -> e2=S[p > e1.p]", 0, (True, False, False)),
        ("every e1=S[p > 20] -> e2=S[v > 5]", 0, (False, False, False)),
        ("every e1=S[p > 20] -> e2=S[p > e1.p] -> e3=S[p > e2.p]", 1, (True, True, False)),
        ("every e1=S[p > 20] -> e2=S[v > 5] -> e3=S[maximum(p, e1.p) == p]", 1, (True, False, False)),
        ("every e1=S[p > 20] -> e2=S[v > 5] -> e3=S[p > e2.p] -> e4=S[d > e3.d or e1.d is null]", 2,
         (True, True, True)),
        ("every e1=S[p > 20] -> e2=S[v > 5] -> e3=S[v > 6] -> e4=S[d > e3.d]", 2, (False, False, True)),
    ]
    for body, cmax, kept in cases:
        (s,) = _shapes(_part(f"{body}{within} select e1.p as a"))
        assert (s.kind, s.cmax, s.kept) == (PK_CHAIN, cmax, kept), body


DECLINES = {
    "five states": _part("every e1=S[p > 1] -> e2=S[p > 2] -> e3=S[p > 3] -> e4=S[p > 4] -> e5=S[p > 5] select e1.p as a"),
    "e1[1]": _part("every e1=S[p > 1] -> e2=S[p > e1[1].p] select e1.p as a"),
    "every inside": _part("every e1=S[p > 1] -> every e2=S[p > e1.p] -> e3=S[p > 3] select e1.p as a"),
    "no every": _part("e1=S[p > 1] -> e2=S[p > e1.p] select e1.p as a"),
    "count state": _part("every e1=S[p > 1] -> e2=S[v > 1] <1:2> -> e3=S[p > e1.p] -> e4=S[v > 1] select e1.p as a"),
    "absent state": _part("every e1=S[p > 1] -> not S[p > 50] for 10 milliseconds select e1.p as a"),
    "two streams": _part("every e1=S[p > 1] -> e2=T[p > e1.p] select e1.p as a",
                         streams=STREAM + " define stream T (k int, p float);", keys="k of S, k of T"),
    "fan-out stream": _part("every e1=T[p > 1] -> e2=T[p > e1.p] select e1.p as a",
                            streams=STREAM + " define stream T (k int, p float);"),
}


@pytest.mark.parametrize("name", sorted(DECLINES))
def test_declines(name):
    (s,) = _shapes(DECLINES[name])
    assert s.kind != PK_CHAIN
    assert s.kind == -1


def test_later_slot_reference_declines():
    """The planner refuses a reference to a later slot, so the blob is made by hand: e2's `e1.p`
    re-pointed at slot 2 in the planned IR."""
    from siddhi_amd.ir import OP_ATTR
    app = App(_part("every e1=S[p > 1] -> e2=S[p > e1.p] -> e3=S[p > 3] select e1.p as a"), engine_factory=PartHostEngine)
    assert app.engine.shape(0).kind == PK_CHAIN
    (ref,) = [i for i in app.ir.queries[0].states[1].filters[0] if i.op == OP_ATTR and i.a == 0]
    ref.a = 2
    assert PartHostEngine(app.ir.serialize(app.string_ids)).shape(0).kind == -1


def test_unpartitioned_chain_is_not_kpart():
    (s,) = _shapes(f"{STREAM} @info(name='q') from every e1=S[p > 20] -> e2=S[p > e1.p] select e1.p as a insert into O;")
    assert s.kind == -1


@pytest.mark.parametrize("seed", range(20))
def test_chain_step_equals_oracle(seed):
    """The shared step function under the entry-major tile walk: 12 chains of 2-4 states, 3 keys,
    2,000 events with nulls, some seeds with out-of-order timestamps, tiles of 64 events and
    narrower ones (a partial crosses more tile boundaries), pushes of several sizes."""
    src = chain_queries(seed, n=12)
    ts, vals, nl = chain_events(seed, 2000, keys=3, unordered=seed % 4 == 3)
    o = App(chain_queries(seed, n=12, twin=True))  # (no oracle sees a function: part_lower_host.MAXF)
    h = App(src, engine_factory=lambda blob: PartHostEngine(blob, tile=[64, 5, 17, 1][seed % 4]))
    assert all(h.engine.shape(qi).kind == PK_CHAIN for qi in range(12))
    nq = lambda q: len(o.ir.queries[q].states)  # noqa: E731
    batch = [2000, 1, 333, 64][(seed // 4) % 4]
    total = 0
    for lo in range(0, len(ts), batch):
        sl = slice(lo, lo + batch)
        o.engine.send(0, ts[sl], vals[sl], nl[sl])
        h.engine.send(0, ts[sl], vals[sl], nl[sl])
        om = o.engine.take_matches(nq)
        assert h.engine.take_matches(nq) == om, f"push at {lo}"
        total += len(om)
    assert total > 100


def test_spec_selftest_chain():
    """Every generated source of the chain kind (2, 3 and 4 states, with and without `within`)
    compiles for gfx950 without a device."""
    from siddhi_amd.engine import load_library
    lib = load_library()
    lib.sdh_spec_selftest_chain.restype = ctypes.c_int
    lib.sdh_spec_selftest_chain.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    log = ctypes.create_string_buffer(8192)
    n = lib.sdh_spec_selftest_chain(log, len(log))
    assert n == 6, log.value.decode(errors="replace")
