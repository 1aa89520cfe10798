"""The emission kernel of K_ratchet's shared-pops form (nfa_ratchet_shared.hip): tiles
of 64 pairs with one lane per pair, take masks over the group's patterns, side entries from ballots,
entries staged through an LDS window.

The same three-way comparison as test_gpu_ratchet_shared.py (form forced, form off, the CPU oracle; by
digest and by decoded rows, with decode_records' checks of the side entries), on the smallest shapes at
which the tile code can go wrong. Every shape_*() returns the app and its pushes; the counts asserted
below are the oracle's."""
import numpy as np
import pytest

from test_gpu_ratchet_shared import Trio

pytestmark = pytest.mark.gpu


def _q(k, f0, op="v > e1.v", within="", col="v"):
    return (f"@info(name='q{k}') from every e1=S[{f0}] -> e2=S[{op}]{within} "
            f"select e1.{col} as x insert into O;")


def _u32(v):
    return np.asarray(v, np.float32).view(np.uint32)


def _run(src, pushes, counts, **kw):
    """Feeds the pushes [(ts, cols), ...] to a Trio; the oracle's match count of each push must be
    counts[k]. Returns the Trio, still open."""
    t = Trio(src, **kw)
    for k, (ts, cols) in enumerate(pushes):
        want = t.push(ts, cols)
        assert len(want) == counts[k], f"push {k}: the oracle has {len(want)} matches, the shape claims {counts[k]}"
    assert t.a.debug_shared_pushes() == len(pushes) and t.b.debug_shared_pushes() == 0
    return t


def shape_pair_counts():
    """Strictly rising prices pushed as 64, 65, 66 and 129 events: event i is popped by i + 1, so the
    pushes hold 63, 64, 65 and 128 pairs (a tile short by one, a full one, one over, two full ones), and
    from the second push on one carried match (the previous push's last event). Three patterns without
    `within`: v > 0.5 (every event but the first), v > 40.5 (from event 41 on), v > 1e6 (none)."""
    src = "define stream S (v float); " + " ".join([_q(0, "v > 0.5"), _q(1, "v > 40.5"), _q(2, "v > 1000000.0")])
    v = np.arange(324, dtype=np.float32)
    ts = np.arange(324, dtype=np.int64)
    pushes, lo = [], 0
    for n in (64, 65, 66, 129):
        pushes.append((ts[lo:lo + n], [_u32(v[lo:lo + n])]))
        lo += n
    return src, pushes, [62 + 22, 65 + 65, 66 + 66, 129 + 129]


def test_pair_count_boundaries():
    src, pushes, counts = shape_pair_counts()
    _run(src, pushes, counts).close()


def shape_lane_halves():
    """Two float columns. Column a: 64 `==` patterns in one group -- lanes 31 and 32 start at a == 5,
    lane 0 at a == 1, lane 63 at a == 2, the others at values that never occur -- so a pair is taken by
    the last lane of the mask's low half and the first of its high half, by lane 0 alone, by lane 63
    alone, or by nobody; and one `<` pattern, a group of exactly one lane. Column b: 65 `>` patterns
    with rising thresholds, a full group and a 1-lane group. 300 random events in two pushes."""
    qs = ["define stream S (a float, b float);"]
    for p in range(64):
        c = 5 if p in (31, 32) else 1 if p == 0 else 2 if p == 63 else 100 + p
        qs.append(_q(p, f"a == {c}.0", "a > e1.a", col="a"))
    qs.append(_q(64, "a < 3.0", "a < e1.a", col="a"))
    for p in range(65):
        qs.append(_q(65 + p, f"b > {p + 10}.5", "b > e1.b", col="b"))
    rng = np.random.default_rng(5)
    a = rng.integers(0, 10, 300).astype(np.float32)
    b = rng.integers(0, 100, 300).astype(np.float32)
    ts = np.arange(300, dtype=np.int64)
    pushes = [(ts[lo:hi], [_u32(a[lo:hi]), _u32(b[lo:hi])]) for lo, hi in ((0, 130), (130, 300))]
    return " ".join(qs), pushes, LANE_HALVES


LANE_HALVES = [4209, 6247]


def test_lane_mask_halves():
    """(The rows are the oracle's, and Trio.push has compared both engines' decoded rows with them.)"""
    src, pushes, counts = shape_lane_halves()
    t = Trio(src)
    pairs = {q: set() for q in range(130)}
    for k, (ts, cols) in enumerate(pushes):
        want = t.push(ts, cols)
        assert len(want) == counts[k]
        for q, e2, d in want:
            pairs[q].add((k, e2, d))
    # lanes 31 and 32 take the same pairs, lane 0 and lane 63 pairs nobody else of the group takes, the
    # other 60 lanes none; the 1-lane groups (q64; q129, the 65th pattern of column b) have matches
    assert pairs[31] and pairs[31] == pairs[32]
    assert pairs[0] and pairs[63] and not (pairs[0] & pairs[63]) and not ((pairs[0] | pairs[63]) & pairs[31])
    assert not any(pairs[q] for q in range(1, 63) if q not in (31, 32))
    assert pairs[64] and pairs[65] and pairs[128] and pairs[129]
    assert t.a.debug_shared_pushes() == len(pushes) and t.b.debug_shared_pushes() == 0
    t.close()


def shape_run_with_gaps():
    """A falling staircase of 100 steps (1000 - i) closed by one spike: 100 pairs share e2 = 100 and
    cross the tile boundary at pair 64. 52 `==` patterns in one group start at the odd steps only (steps
    63 and 65 twice), so the even pairs -- the run's first pair and the second tile's first pair among
    them -- have no taker: 52 matches, one side entry, `first` == 0."""
    qs = ["define stream S (v float);"]
    steps = list(range(1, 100, 2)) + [63, 65]
    for k, i in enumerate(steps):
        qs.append(_q(k, f"v == {1000 - i}.0"))
    v = np.concatenate([1000 - np.arange(100), [5000]]).astype(np.float32)
    return " ".join(qs), [(np.arange(101, dtype=np.int64), [_u32(v)])], [52]


def test_run_of_one_event_across_a_tile_with_gaps():
    src, pushes, counts = shape_run_with_gaps()
    _run(src, pushes, counts).close()


def shape_side_entry_heavy():
    """One pattern over 20,000 strictly rising events: every pair is its own event with one match, 4 B
    of entry and 8 B of side entry, so a 64-KiB block ends after some 5,460 pairs, inside a tile, and
    the side entries decide the room test. 19,999 matches."""
    src = "define stream S (v float); " + _q(0, "v > -1.0")
    v = np.arange(20000, dtype=np.float32)
    return src, [(np.arange(20000, dtype=np.int64), [_u32(v)])], [19999]


@pytest.mark.parametrize("capacity", [0, 1])
def test_side_entry_heavy_blocks(capacity):
    """(match_capacity=1: the first attempt has one block and re-runs on err[2].)"""
    src, pushes, counts = shape_side_entry_heavy()
    kw = {"match_capacity": 1} if capacity else {}
    _run(src, pushes, counts, oracle_key="emit_side_heavy", **kw).close()


def shape_tile_larger_than_window():
    """64 patterns that all take every pair of a 64-step staircase popped by one spike: one tile of
    4,096 entries, several staging windows. Then 10 and 20: the pair (65, 66) is a tile of its own with
    one entry (only the last pattern starts below 100). 4,097 matches."""
    qs = ["define stream S (v float);"]
    for p in range(64):
        qs.append(_q(p, "v > 100.0" if p < 63 else "v > 5.0"))
    v = np.concatenate([1000 - np.arange(64), [5000, 10, 20]]).astype(np.float32)
    return " ".join(qs), [(np.arange(67, dtype=np.int64), [_u32(v)])], [4097]


def test_tile_larger_than_the_staging_window():
    src, pushes, counts = shape_tile_larger_than_window()
    _run(src, pushes, counts).close()


def shape_carried_and_in_batch():
    """Push 1 leaves a staircase of ten steps (50 .. 41, 10 ms apart) pending. Push 2 starts 200 ms
    later with 30 and 45.5: event 1 pops event 0 in the batch and the carried steps 45 .. 41, so both
    phases write entries of e2 = 1 into one block; then 100 pops the rest. Four patterns, `within` 150 ms,
    180 ms, 1 sec and none: the age filter differs per lane."""
    qs = ["define stream S (v float);"]
    for k, w in enumerate((" within 150 milliseconds", " within 180 milliseconds", " within 1 sec", "")):
        qs.append(_q(k, "v > 0.0", within=w))
    v1 = (50 - np.arange(10)).astype(np.float32)
    ts1 = np.arange(10, dtype=np.int64) * 10
    v2 = np.array([30, 45.5, 100], np.float32)
    ts2 = np.array([290, 300, 310], dtype=np.int64)
    return " ".join(qs), [(ts1, [_u32(v1)]), (ts2, [_u32(v2)])], CARRIED


CARRIED = [0, 28]


def test_carried_and_in_batch_matches_at_one_event():
    src, pushes, counts = shape_carried_and_in_batch()
    _run(src, pushes, counts).close()


def shape_candidates_without_taker():
    """v > 10 within 5 ms and v > 50 within 1 hour; 70 times (20, 25), 100 ms apart, then 60 and 61 one
    ms apart. The pairs (20 -> 25) and (25 -> 60), 140 of them, lie inside the group's widest bounds
    (key >= 10, age <= 1 hour) but have no taker -- the lane whose threshold they pass has expired,
    the other's threshold is above them --, so two whole tiles write nothing. The last pair (60 -> 61)
    is taken by both: 2 matches, 16 B of records."""
    src = ("define stream S (v float); " + _q(0, "v > 10.0", within=" within 5 milliseconds") + " " +
           _q(1, "v > 50.0", within=" within 1 hour"))
    v = np.concatenate([np.tile([20, 25], 70), [60, 61]]).astype(np.float32)
    ts = np.concatenate([np.arange(140, dtype=np.int64) * 100, [14000, 14001]])
    return src, [(ts, [_u32(v)])], [2]


def test_candidates_of_the_widest_bounds_without_a_taker():
    src, pushes, counts = shape_candidates_without_taker()
    t = Trio(src)
    recs = []
    poll = t.a.poll_records
    t.a.poll_records = lambda: recs.append(poll()) or recs[-1]
    want = t.push(*pushes[0])
    assert len(want) == counts[0]
    assert recs[0].r_n == 2 and recs[0].r_bytes == 2 * 4 + 8  # (two entries, one side entry, nothing else)
    assert t.a.debug_shared_pushes() == 1 and t.b.debug_shared_pushes() == 0
    t.close()
