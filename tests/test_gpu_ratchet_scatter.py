"""The two scatter forms of K_ratchet's shared-pops emission (nfa_ratchet_shared.hip) and
its tile-uniform skip of the age and upper-bound compares.

A block part's entries reach the LDS window either with lane = pattern (one wave-wide write per pair
that has a taker; a pair every active pattern takes needs no rank) or with lane = pair (each lane walks
its own take mask); `SDH_RATCHET_SCATTER` forces one, unset chooses per block part. Every shape below
runs three ways -- `pair`, `lane`, unset -- and each run is the three-way comparison of
test_gpu_ratchet_shared.py (form on, form off, the CPU oracle; digest and decoded rows). The counts
asserted are the oracle's. No test looks at which form ran except through the forced runs."""
import numpy as np
import pytest

from test_gpu_ratchet_shared import Trio

pytestmark = pytest.mark.gpu

FORMS = {"pair": {"SDH_RATCHET_SHARED_MIN": 1, "SDH_RATCHET_SCATTER": "pair"},
         "lane": {"SDH_RATCHET_SHARED_MIN": 1, "SDH_RATCHET_SCATTER": "lane"},
         "rule": {"SDH_RATCHET_SHARED_MIN": 1}}
forms = pytest.mark.parametrize("form", list(FORMS))


def _q(k, f0, within=""):
    return f"@info(name='q{k}') from every e1=S[{f0}] -> e2=S[v > e1.v]{within} select e1.v as x insert into O;"


def _u32(v):
    return np.asarray(v, np.float32).view(np.uint32)


def _run(form, key, src, pushes, counts, **kw):
    """Feeds the pushes [(ts, v), ...] to a Trio whose first engine runs `form`; the oracle's match count
    of each push must be counts[k] (the oracle runs once per shape). Returns the oracle's rows per push."""
    t = Trio(src, a=FORMS[form], oracle_key=key, **kw)
    rows = []
    for k, (ts, v) in enumerate(pushes):
        want = t.push(np.asarray(ts, np.int64), [_u32(v)])
        assert len(want) == counts[k], f"push {k}: the oracle has {len(want)} matches, the shape claims {counts[k]}"
        rows.append(want)
    assert t.a.debug_shared_pushes() == len(pushes) and t.b.debug_shared_pushes() == 0
    t.close()
    return rows


# ---- a group of 40 patterns, one tile of full, partial and empty pairs ----
def shape_forty_lanes():
    """40 `v > c` patterns in one group; a pair is taken by {p : c_p < key and age <= within_p}. Lane 0:
    c = 100, no `within`; lanes 31 and 32: c = 50, 200 ms; lane 39: c = 10, 50 ms; the others: c = 100,
    200 ms. A falling staircase closed by a spike at ts 1010 (event 7) gives, by (key, age): 500 / 499 /
    498 at 1010 .. 1008 ms: lane 0 alone; 70 at 310 ms: inside the widest bounds, nobody; 69 at 110 ms:
    lanes 31 and 32; 20 at 10 ms: lane 39 alone; 5: below every threshold. Ten more steps (400 .. 391, a
    ms apart) and a second spike (event 18): pairs of at most 11 ms, taken by all 40 -- as is the first
    spike's own pair. 18 pairs, one tile; n_lanes = 40, so a full mask is short of 64 bits."""
    qs = ["define stream S (v float);"]
    for p in range(40):
        c, w = (100, "") if p == 0 else (50, " within 200 milliseconds") if p in (31, 32) else \
            (10, " within 50 milliseconds") if p == 39 else (100, " within 200 milliseconds")
        qs.append(_q(p, f"v > {c}.0", w))
    v = [500, 499, 498, 70, 69, 20, 5, 2000] + [400 - i for i in range(10)] + [2001]
    ts = [0, 1, 2, 700, 900, 1000, 1005, 1010] + [1011 + i for i in range(10)] + [1021]
    return " ".join(qs), [(ts, v)], FORTY


FORTY = [3 + 2 + 1 + 11 * 40]


@forms
def test_forty_lanes_full_partial_and_empty_pairs(form):
    src, pushes, counts = shape_forty_lanes()
    want = _run(form, "scatter_forty", src, pushes, counts)[0]
    takers = {}
    for q, e2, d in want:
        takers.setdefault(e2 - d, set()).add(q)  # by e1
    assert takers[0] == takers[1] == takers[2] == {0}
    assert 3 not in takers and 6 not in takers
    assert takers[4] == {31, 32} and takers[5] == {39}
    assert all(takers[i] == set(range(40)) for i in range(7, 18))


# ---- a pair across the pass boundary ----
def shape_pass_boundary(partial):
    """64 patterns over a 64-step staircase closed by one spike: one tile, one event. A pass of the
    window holds 2,044 entries. Full: every pattern takes every pair, 64 x 64 entries, entry 2,044 lies
    inside pair 31 (entries 1,984 .. 2,047), a pair all lanes take. Partial: patterns 10 and 40 start
    above 969.5 only, so pairs 31 .. 63 (keys 969 .. 937) have 62 takers: pair 31 holds entries 1,984 ..
    2,045, across the boundary again, and needs its ranks."""
    qs = ["define stream S (v float);"]
    for p in range(64):
        qs.append(_q(p, "v > 969.5" if partial and p in (10, 40) else "v > 100.0"))
    v = np.concatenate([1000 - np.arange(64), [5000]])
    return " ".join(qs), [(np.arange(65), v)], [31 * 64 + 33 * 62 if partial else 64 * 64]


@forms
@pytest.mark.parametrize("partial", [False, True])
def test_pair_across_the_pass_boundary(form, partial):
    src, pushes, counts = shape_pass_boundary(partial)
    _run(form, f"scatter_pass_{int(partial)}", src, pushes, counts)


# ---- a block roll inside a tile of full pairs ----
def shape_block_roll():
    """64 patterns that take every pair of a 300-step falling staircase closed by one spike: 19,200
    entries of one event, more than a 64-KiB block's 16K, so a block part ends inside a tile and the
    event's run continues behind a fresh side entry."""
    qs = ["define stream S (v float);"] + [_q(p, "v > 100.0") for p in range(64)]
    v = np.concatenate([1000 - np.arange(300), [5000]])
    return " ".join(qs), [(np.arange(301), v)], [19200]


@forms
@pytest.mark.parametrize("capacity", [0, 1])
def test_block_roll_inside_a_tile_of_full_pairs(form, capacity):
    """(match_capacity=1: the first attempt has one block and re-runs on err[2].)"""
    src, pushes, counts = shape_block_roll()
    _run(form, "scatter_roll", src, pushes, counts, **({"match_capacity": 1} if capacity else {}))


# ---- a dense and a sparse tile in one push ----
def shape_form_switch():
    """Two groups of 64 patterns, `v > 100` and `v == 1 .. 64`. A 64-step staircase (1000 - i) and a spike:
    a tile whose every pair all 64 `>` patterns take (64 pairs, 4,096 entries: 64^2 <= 4,096, the pair
    form by the rule). Then the staircase 64 .. 1 and a higher spike: pairs with exactly one taker each,
    a `==` pattern (63 pairs with 63 entries in that group's tile: the lane form), and the first spike's
    pair, which the `>` group takes whole."""
    qs = ["define stream S (v float);"] + [_q(p, "v > 100.0") for p in range(64)]
    qs += [_q(64 + p, f"v == {p + 1}.0") for p in range(64)]
    v = np.concatenate([1000 - np.arange(64), [5000], 64 - np.arange(64), [6000]])
    return " ".join(qs), [(np.arange(130), v)], [64 * 64 + 64 + 64]


@forms
def test_dense_then_sparse_tile(form):
    src, pushes, counts = shape_form_switch()
    _run(form, "scatter_switch", src, pushes, counts)


# ---- the tile-uniform skips ----
def shape_age_skip():
    """`within` 100 ms and 1 sec over rising prices (event i is popped by i + 1, the pair's age is the
    gap). Push 1: every gap 50 ms, the age compare is skipped. Push 2: one gap of exactly 100 ms, still
    skipped, and both patterns take the pair. Push 3: one gap of 101 ms, the compare stays and only the
    1-sec pattern takes that pair. (Each push's last event is popped in the next push, as a carried
    partial.)"""
    src = "define stream S (v float); " + _q(0, "v > 0.0", " within 100 milliseconds") + " " + \
        _q(1, "v > 0.0", " within 1 sec")
    pushes, t0, v0 = [], 0, 1
    for gap in (50, 100, 101):
        gaps = np.full(30, 50)
        gaps[17] = gap
        ts = t0 + np.cumsum(gaps)
        pushes.append((ts, v0 + np.arange(30)))
        t0, v0 = ts[-1], v0 + 30
    return src, pushes, AGE_SKIP


AGE_SKIP = [58, 60, 59]


@forms
def test_age_compare_skip_boundary(form):
    src, pushes, counts = shape_age_skip()
    rows = _run(form, "scatter_age", src, pushes, counts)
    # event 17 of a push closes the gap that differs: its pair is (e2 17, distance 1)
    assert [sorted(q for q, e2, d in r if (e2, d) == (17, 1)) for r in rows] == [[0, 1], [0, 1], [1]]


def shape_hi_skip():
    """The same for a finite upper bound: start filters `v < 50` and `v < 80` (one start atom over the key
    column is what the shared form takes; the smaller bound is the greatest float below 50). Push 1: keys
    below it. Push 2: a key at the bound, the compare is skipped and both patterns take the pair; the
    push ends with 70, which stays pending. Push 3: a pair with key 50.0, just above: the compare stays
    and only the second pattern takes it."""
    src = "define stream S (v float); " + _q(0, "v < 50.0") + " " + _q(1, "v < 80.0")
    at = np.nextafter(np.float32(50), np.float32(0))
    v1 = np.arange(1, 31, dtype=np.float32)
    v2 = np.concatenate([np.arange(31, 46, dtype=np.float32), [at, 70]]).astype(np.float32)
    v3 = np.array([20, 30, 50, 75], np.float32)
    pushes, t0 = [], 0
    for v in (v1, v2, v3):
        pushes.append((t0 + np.arange(len(v)), v))
        t0 += len(v)
    return src, pushes, HI_SKIP


HI_SKIP = [58, 34, 6]


@forms
def test_upper_bound_compare_skip_boundary(form):
    src, pushes, counts = shape_hi_skip()
    rows = _run(form, "scatter_hi", src, pushes, counts)
    assert sorted(q for q, e2, d in rows[1] if (e2, d) == (16, 1)) == [0, 1]  # the key at the bound
    assert sorted(q for q, e2, d in rows[2] if (e2, d) == (3, 1)) == [1]  # 50.0 -> 75
