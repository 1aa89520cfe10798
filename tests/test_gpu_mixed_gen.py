"""Interleaved pushes on K_gen (sdh_engine_push_mixed; DESIGN.md §3.2 "Interleaved pushes"): unpartitioned
cross-stream patterns that plan on the K_gen kernel -- logical states, counts over a second stream, an
`every` inside a chain -- walk the merged sequence in one launch.

As tests/test_gpu_mixed.py: every call is compared against the CPU oracle fed the call's maximal same-part
runs, against a twin engine under SDH_MIX_SPLIT=1 and on sdh_stats; every test asserts the path
(debug_mixed_pushes), the plan (plan_queries[6], K_gen) and a floor on the oracle's match count (read off
the oracle when the seeds and constants were chosen)."""
import numpy as np
import pytest

from harness import App, oracle_lib
from siddhi_amd.engine import SDH_FLAG_DEVICE_MATCHES, SDH_FLAG_FORCE_GEN, EngineError
from test_gpu_mixed import EDGE_SRC, Trio, by_index, call_of, hip_app, oracle_runs, price, take

pytestmark = pytest.mark.gpu

E_UNSUPPORTED = -2
STREAMS = "define stream A (p float); define stream B (p float); define stream C (p float); define stream D (p float); "
ABC = [("A", price(0, 100)), ("B", price(0, 100)), ("C", price(0, 100))]
ABCD = ABC + [("D", price(0, 100))]


def logical(i, op="and", c=10, w=40):
    return (f"@info(name='l{op}{i}') from every e1=A[p > {c}] -> e2=B[p > e1.p] {op} e3=C[p > {c + 30}] "
            f"within {w} milliseconds select e1.p as a, e3.p as c insert into O;")


def counted(i, c=10, w=40):
    return (f"@info(name='n{i}') from every e1=A[p > {c}] -> e2=B[p > {c + 20}]<2:4> -> e3=C[p > e1.p] "
            f"within {w} milliseconds select e1.p as a, e3.p as c insert into O;")


def inner_every(i, c=10):
    """(Its `within` is longer than any test's clock runs: the reference throws a
    ConcurrentModificationException when a partial of this shape expires, and the engine then fails the
    push with SDH_E_REFERENCE as it must.)"""
    return (f"@info(name='v{i}') from e1=A[p > {c}] -> every e2=B[p > {c + 40}] -> e3=A[p > e2.p] "
            f"within 100 sec select e1.p as a, e3.p as c insert into O;")


def shapes_src(n=5, w=40):
    qs = []
    for i in range(n):
        qs += [logical(i, "and", 10 + 9 * i, w), logical(i, "or", 12 + 9 * i, w), counted(i, 8 + 9 * i, w),
               inner_every(i, 5 + 9 * i)]
    return STREAMS + " ".join(qs)


SHAPES_SRC = shapes_src()


def shape_calls():
    """edge_calls()-style orders over three streams, and a fourth that no query reads."""
    rng = np.random.default_rng(7)
    calls, t = [], 0

    def add(order, gens=ABC):
        nonlocal t
        calls.append(call_of(order, t, gens, rng))
        t += len(order)

    for n in (1, 63, 64, 65, 130):
        add(rng.integers(0, 3, n))
    add(np.arange(130) % 2)                         # ABAB..., C empty
    add([0] * 64 + [1] * 64 + [2] * 10)             # a tile of one part, then a tile of another
    add(rng.integers(0, 2, 40))                     # an empty part
    add([0] * 7, [("A", price(0, 100))])            # one part only
    add(rng.integers(0, 4, 100), ABCD)              # a part whose stream no query reads
    add(rng.integers(0, 3, 65))
    return calls


# ---- 1. logical and count shapes over three streams ------------------------------------------------
def test_logical_and_count_shapes():
    t = Trio(SHAPES_SRC)
    assert t.n.engine.stats().plan_queries[6] == 20
    for parts, order in shape_calls():
        t.mixed(parts, order)
    assert t.total >= 2400
    assert t.n.engine.debug_mixed_pushes() == (len(shape_calls()), 0)


# ---- 2. group boundary and partial readers ----------------------------------------------------------
def boundary_src():
    qs = [logical(i, "and", 5 + i, 60) for i in range(65)]
    qs += [f"@info(name='bc{i}') from every e1=B[p > {20 + 10 * i}] -> e2=C[p > e1.p] and e3=C[p < 70] "
           f"within 60 milliseconds select e1.p as a insert into O;" for i in range(3)]
    return STREAMS + " ".join(qs)


def test_group_boundary_and_partial_readers():
    t = Trio(boundary_src())
    assert t.n.engine.stats().plan_queries[6] == 68
    rng = np.random.default_rng(17)
    tt = 0
    # parts A and B only: the {B, C} group skips A's events, the last-lane group of the 65 reads both
    for gens, k, n in ((ABC[:2], 2, 65), (ABC[:2], 2, 130), (ABC, 3, 130), (ABC[1:], 2, 64), (ABC, 3, 65)):
        t.mixed(*call_of(rng.integers(0, k, n), tt, gens, rng))
        tt += n
    assert t.total >= 2500
    assert t.n.engine.stats().last_gen_items == 3  # two groups of the 65, one of the three
    assert t.n.engine.debug_mixed_pushes() == (5, 0)


# ---- 3. out-of-order timestamps across parts --------------------------------------------------------
def test_out_of_order_timestamps_across_parts():
    """B's clock lags A's by 6 ms and C's leads it by 3: `within 8 milliseconds` is decided on the merged
    timestamps, which go back and forth from event to event."""
    t = Trio(shapes_src(4, 8))
    assert t.n.engine.stats().plan_queries[6] == 16
    rng = np.random.default_rng(19)
    lag = lambda p, x: x // 2 + (0, -6, 3)[p]  # noqa: E731
    tt = 100
    for n in (130, 64, 1, 200, 65, 63):
        t.mixed(*call_of(rng.integers(0, 3, n), tt, ABC, rng, ts_of=lag))
        tt += n
    assert t.total >= 1000
    assert t.n.engine.debug_mixed_pushes() == (6, 0)


# ---- 4. pool growth inside a native call ------------------------------------------------------------
GROW_SRC = STREAMS + ("@info(name='g') from every e1=A[p > 10] -> e2=B[p > e1.p] and e3=C[p > 90] "
                      "select e1.p as a insert into O; "
                      "@info(name='h') from every e1=A[p > 50] -> e2=B[p > 60]<2:4> -> e3=C[p > e1.p] "
                      "select e1.p as a insert into O;")


def oracle_live(o):
    return int(oracle_lib().oracle_live_partials(o.engine.h))


def test_pool_growth_inside_a_native_call():
    """A opens partials that B does not complete: the tiny pools overflow inside the mixed call, the K_gen
    pass of the call is undone from its journal, re-laid and re-run. The oracle counts every pending list,
    the start states' seeds included (one per query here); sdh_stats counts the non-start states' lists."""
    t = Trio(GROW_SRC, gen_pool_states=2, gen_pool_nodes=4, gen_list_cap=2)
    assert t.n.engine.stats().plan_queries[6] == 2
    rng = np.random.default_rng(23)
    gens = [("A", price(11, 60)), ("B", price(0, 100)), ("C", price(0, 100))]
    before = t.n.engine.stats().pool_regrows
    m = t.mixed(*call_of([0] * 40 + [1] * 10 + [0] * 10 + [2] * 3 + [1] * 5, 0, gens, rng))
    assert len(m) >= 5
    assert t.n.engine.stats().pool_regrows > before and t.s.engine.stats().pool_regrows > 0
    live = t.n.engine.stats().live_partials
    assert live >= 20 and oracle_live(t.o) - 2 <= live <= oracle_live(t.o)
    # the grown pools go on working, through a plain push too
    t.plain("C", [2000, 2001], np.asarray([95.0, 99.9], np.float32).view(np.uint32).astype(np.int64))
    t.mixed(*call_of(rng.integers(0, 3, 65), 3000, gens, rng))
    assert t.total >= 60
    assert t.n.engine.debug_mixed_pushes() == (2, 0)


# ---- 5. K_chain and K_gen in one engine, one call ---------------------------------------------------
BOTH_SRC = EDGE_SRC + " define stream C (p float); define stream D (p float); " + " ".join(
    [logical(i, "and", 10 + 15 * i) for i in range(4)] + [logical(i, "or", 15 + 15 * i) for i in range(4)])


def test_chain_and_gen_in_one_call():
    t = Trio(BOTH_SRC)
    st = t.n.engine.stats()
    assert st.plan_queries[2] == 20 and st.plan_queries[6] == 8
    for parts, order in shape_calls():
        t.mixed(parts, order)  # (the merged poll order is the oracle's: take() compares lists)
    assert t.total >= 3500
    assert t.n.engine.debug_mixed_pushes() == (len(shape_calls()), 0)


# ---- 6. device records ------------------------------------------------------------------------------
def test_device_records():
    normal, dev = hip_app(BOTH_SRC), hip_app(BOTH_SRC, flags=SDH_FLAG_DEVICE_MATCHES)
    assert dev.engine.stats().plan_queries[6] == 8
    total = gen_total = 0
    for parts, order in shape_calls()[:7]:
        normal.engine.send_mixed(by_index(normal, parts), order)
        dev.engine.send_mixed(by_index(dev, parts), order)
        want = len(normal.engine.poll()[0])
        r = dev.engine.poll_records()
        assert (r.n, r.n_events) == (want, len(order)) and r.f_n + r.c_n == r.n
        total += want
        gen_total += r.f_n
    assert total >= 2500 and gen_total >= 300
    assert dev.engine.debug_mixed_pushes() == (7, 0) and normal.engine.debug_mixed_pushes() == (7, 0)


# ---- 7. journal budget ------------------------------------------------------------------------------
def test_journal_budget_splits_or_refuses():
    calls = shape_calls()[:7]
    t = Trio(SHAPES_SRC, native=False, debug={"SDH_JOURNAL_BUDGET": 1})
    assert t.n.engine.stats().plan_queries[6] == 20
    for parts, order in calls:
        t.mixed(parts, order)
    assert t.total >= 1500
    assert t.n.engine.debug_mixed_pushes() == (0, len(calls))
    g = hip_app(SHAPES_SRC, flags=SDH_FLAG_DEVICE_MATCHES, debug={"SDH_JOURNAL_BUDGET": 1})
    before = g.engine.stats()
    for parts, order in calls:
        with pytest.raises(EngineError) as ex:
            g.engine.send_mixed(by_index(g, parts), order)
        assert ex.value.code == E_UNSUPPORTED
    after = g.engine.stats()
    assert (after.events, after.pattern_events, after.matches, after.live_partials) == (
        before.events, before.pattern_events, before.matches, before.live_partials) == (0, 0, 0, 0)
    assert g.engine.debug_mixed_pushes() == (0, 0)


# ---- 8. poll_rows over native K_gen calls -----------------------------------------------------------
def test_poll_rows_over_native_gen_calls():
    from test_gpu_rows import check_polled
    o = App(SHAPES_SRC)
    a, b = hip_app(SHAPES_SRC), hip_app(SHAPES_SRC)
    b.engine.retain_events(1024)  # (every event of the test: inner_every's partials never expire)
    assert b.engine.stats().plan_queries[6] == 20
    total = 0
    for parts, order in shape_calls():
        oracle_runs(o, parts, order)
        a.engine.send_mixed(by_index(a, parts), order)
        b.engine.send_mixed(by_index(b, parts), order)
        matches, _ = check_polled(o, a.engine.poll(with_seq=True), b.engine.poll_rows(), width=2)
        assert matches == take(o)
        total += len(matches)
    assert total >= 2400
    assert b.engine.debug_mixed_pushes() == (len(shape_calls()), 0)


# ---- 9. continuity ----------------------------------------------------------------------------------
def test_mixed_and_plain_pushes_alternate():
    t = Trio(SHAPES_SRC)
    assert t.n.engine.stats().plan_queries[6] == 20
    rng = np.random.default_rng(29)
    tt = 0
    for k in range(6):
        t.mixed(*call_of(rng.integers(0, 3, [65, 1, 130, 64][k % 4]), tt, ABC, rng))
        tt += 130
        t.plain("ABC"[k % 3], tt + np.arange(30), price(0, 100)(rng, 30)[0])
        tt += 30
    assert t.total >= 1200
    assert t.n.engine.debug_mixed_pushes() == (6, 0)


def test_snapshot_after_a_native_call():
    """(No blob equality between the paths: pool layouts may differ after growth.)"""
    t = Trio(SHAPES_SRC)
    assert t.n.engine.stats().plan_queries[6] == 20
    rng = np.random.default_rng(31)
    t.mixed(*call_of(rng.integers(0, 3, 130), 0, ABC, rng))
    blob = t.n.engine.snapshot()
    rn, rs = hip_app(SHAPES_SRC), hip_app(SHAPES_SRC, debug={"SDH_MIX_SPLIT": 1})
    rn.engine.restore(blob)
    rs.engine.restore(blob)
    total = 0
    for k, n in enumerate((65, 130)):
        parts, order = call_of(rng.integers(0, 3, n), 130 + 200 * k, ABC, rng)
        want = t.mixed(parts, order)
        for g in (rn, rs):
            g.engine.send_mixed(by_index(g, parts), order)
            assert take(g) == want
        total += len(want)
    assert total >= 600
    assert rn.engine.debug_mixed_pushes() == (2, 0) and rs.engine.debug_mixed_pushes() == (0, 2)
    assert rn.engine.stats().live_partials == t.n.engine.stats().live_partials == rs.engine.stats().live_partials


def test_two_shards_together_equal_the_oracle():
    o = App(SHAPES_SRC)
    shards = [hip_app(SHAPES_SRC, shard_rank=r, shard_world=2) for r in range(2)]
    assert [g.engine.stats().plan_queries[6] for g in shards] == [10, 10]
    nq = lambda q: len(o.ir.queries[q].states)  # noqa: E731
    total = 0
    for parts, order in shape_calls()[:7]:
        oracle_runs(o, parts, order)
        got = []
        for g in shards:
            g.engine.send_mixed(by_index(g, parts), order)
            got += take(g)
        want = o.engine.take_matches(nq)
        assert sorted(got, key=repr) == sorted(want, key=repr)
        total += len(want)
    assert total >= 1500
    assert all(g.engine.debug_mixed_pushes() == (7, 0) for g in shards)


# ---- 10. still split, unchanged ---------------------------------------------------------------------
STILL_SPLIT = {
    "absent": (STREAMS + logical(0) + " @info(name='ab') from every e1=A[p > 50] -> not B[p > e1.p] for 5 milliseconds "
               "select e1.p as a insert into O;", (0, 0, 0, 0, 0, 0, 2, 0), 0),
    # (SDH_FLAG_FORCE_GEN keeps the partition's query on the K_gen kernel, off K_part / K_slab)
    "partitioned": (STREAMS + logical(0) + " partition with (p of A, p of B, p of C) begin " + logical(1) + " end;",
                    (0, 0, 0, 0, 0, 0, 2, 0), SDH_FLAG_FORCE_GEN),
    "wave": (STREAMS + logical(0) + " @info(name='w') from every e1=A[p > 50] -> e2=A[p > 60]<2:4> -> e3=A[p > e1.p] "
             "within 40 milliseconds select e1.p as a insert into O;", (0, 0, 0, 0, 0, 0, 1, 1), 0),
}


@pytest.mark.parametrize("name", list(STILL_SPLIT))
def test_still_split(name):
    src, plans, flags = STILL_SPLIT[name]
    t = Trio(src, native=False, flags=flags)
    assert tuple(t.n.engine.stats().plan_queries) == plans
    rng = np.random.default_rng(37)
    tt = 0
    for n in (65, 130, 64):
        t.mixed(*call_of(rng.integers(0, 3, n), tt, ABC, rng))
        tt += n
    assert t.total >= 30
    assert t.n.engine.debug_mixed_pushes() == (0, 3)
