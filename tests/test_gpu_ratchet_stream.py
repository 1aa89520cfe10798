"""The record store stream of K_ratchet's shared-pops emission (nfa_ratchet_shared.hip; DESIGN.md §3.1
round 10): block rolls, side entries, window passes that start off a quad and tiles that write nothing,
at the smallest shapes that reach them, and the write-stream probe (sdh_calibrate_store).

Every shape runs with the scatter forced `pair`, forced `lane` and by the rule, each run the three-way
comparison of test_gpu_ratchet_shared.py (form on, form off, the CPU oracle; digest and decoded rows).
The counts asserted are the oracle's."""
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


def _run(form, key, src, pushes, counts):
    t = Trio(src, a=FORMS[form], oracle_key=key)
    rows = []
    for k, (ts, v) in enumerate(pushes):
        want = t.push(np.asarray(ts, np.int64), [_u32(v)])
        assert len(want) == counts[k], f"push {k}: the oracle has {len(want)} matches, the shape claims {counts[k]}"
        rows.append(want)
    assert t.a.debug_shared_pushes() == len(pushes) and t.b.debug_shared_pushes() == 0
    t.close()
    return rows


# ---- a block roll inside a tile, then a spill into the fresh block ----
@forms
def test_block_roll_then_spill(form):
    """64 `v > 100` patterns over a 300-step falling staircase closed by a spike: 19,200 entries of one
    event, a 64-KiB block holds at most 16,382, so the block rolls inside a tile and the event's side
    entry is written again at the head of the fresh block. A second spike one step later closes the
    first one's pair: 64 more entries and a second side entry in that block."""
    src = " ".join(["define stream S (v float);"] + [_q(p, "v > 100.0") for p in range(64)])
    v = np.concatenate([1000 - np.arange(300), [5000, 6000]])
    rows = _run(form, "stream_roll_spill", src, [(np.arange(302), v)], [19200 + 64])[0]
    assert sum(1 for q, e2, d in rows if e2 == 301) == 64


# ---- more side entries in one block than 256 ----
def _saw(n):
    return np.where(np.arange(n) % 2 == 0, 200.0, 300.0)


def _saw_src():
    # patterns 0 and 1 start below 250, the others never: an even event (200) opens a partial of each,
    # the odd event behind it (300) closes the pair and opens nothing
    return " ".join(["define stream S (v float);"] + [_q(p, "v < 250.0" if p < 2 else "v < 50.0") for p in range(64)])


@forms
def test_side_entries_past_256_in_one_block(form):
    """A saw-tooth of 640 events: every second event closes exactly one pair, taken by patterns 0 and 1
    only. 320 side entries and 640 entries in one block."""
    rows = _run(form, "stream_saw", _saw_src(), [(np.arange(640), _saw(640))], [640])[0]
    assert {q for q, e2, d in rows} == {0, 1} and {d for q, e2, d in rows} == {1}
    assert len({e2 for q, e2, d in rows}) == 320


@forms
def test_side_entries_of_both_phases(form):
    """The same behind a push that leaves 60 partials per pattern (249 .. 190, nothing closes them). The
    second push's event 0 (200) closes the ten below 200, its event 1 (300) the other fifty and the
    pair (0, 1): the carried phase opens side entries too, and event 1 owns one of each phase."""
    p1 = (np.arange(60), 249.0 - np.arange(60))
    p2 = (60 + np.arange(640), _saw(640))
    rows = _run(form, "stream_saw_carried", _saw_src(), [p1, p2], [0, 60 * 2 + 640])[1]
    at1 = sorted(d for q, e2, d in rows if e2 == 1 and q == 0)
    assert at1 == [1] + list(range(12, 62))  # the pair, then the carried partials 200 .. 249 (events 49 .. 0 of push 1)
    assert sorted(d for q, e2, d in rows if e2 == 0 and q == 1) == list(range(1, 11))


# ---- several passes in one block part, starting off a quad ----
@forms
@pytest.mark.parametrize("lanes", [64, 40])
def test_passes_from_fill_three(form, lanes):
    """Patterns 0 .. 2 start above 100, the others above 500. Event 0 (200) is theirs alone and event 1
    (1000) closes it: 3 entries. Event 1 and a 99-step staircase below it are everybody's; a spike closes
    the 100 full pairs, whose 100 x lanes entries start at fill = 3: with 64 lanes, three and a bit
    passes of the window, ragged at both ends of each; with 40 lanes a full mask is short of 64 bits."""
    src = " ".join(["define stream S (v float);"] +
                   [_q(p, "v > 100.0" if p < 3 else "v > 500.0") for p in range(lanes)])
    v = np.concatenate([[200], 1000 - np.arange(100), [5000]])
    rows = _run(form, f"stream_fill3_{lanes}", src, [(np.arange(102), v)], [3 + 100 * lanes])[0]
    assert sorted(q for q, e2, d in rows if e2 == 1) == [0, 1, 2]
    assert sum(1 for q, e2, d in rows if e2 == 101) == 100 * lanes


# ---- a tile that writes nothing between two that write ----
@forms
def test_tile_without_taker_between_two_with(form):
    """Pattern A: above 100 within 10 ms; pattern B: above 500 within 1 sec. Tile 0: a 64-step staircase
    from 1000 at 1 ms steps, closed by 5000 (B takes all 64 pairs, A the 10 youngest). Tile 1: a staircase
    from 400 closed 37 ms after its last step by 450: 64 pairs inside the group's widest bounds, too old
    for A and too low for B. Then 1000 one ms later (A alone takes the pair of the 450) and the first
    staircase again under 4000: the window and block state go through the tile that returns early."""
    src = "define stream S (v float); " + _q(0, "v > 100.0", " within 10 milliseconds") + " " + \
        _q(1, "v > 500.0", " within 1 sec")
    v = np.concatenate([1000 - np.arange(64), [5000], 400 - np.arange(64), [450], 1000 - np.arange(64), [4000]])
    ts = np.concatenate([np.arange(64), [64], 100 + np.arange(64), [200], 201 + np.arange(64), [265]])
    rows = _run(form, "stream_empty_tile", src, [(ts, v)], [74 + 0 + 1 + 74])[0]
    assert not [r for r in rows if r[1] == 129]
    assert [(q, d) for q, e2, d in rows if e2 == 130] == [(0, 1)]


# ---- the probe ----
def test_store_probe_every_mode():
    """Every mode of sdh_calibrate_store returns a positive rate (256 MiB, one iteration)."""
    from siddhi_amd.engine import STORE_SIDE_WHOLE, calibrate_store
    n = 256 << 20
    for nt in (0, 1):
        assert calibrate_store(0, n, 1, "linear", nt=nt) > 0
    points = [{}, {"side": 170}, {"side": STORE_SIDE_WHOLE}, {"side": 170, "claim": 1}, {"nt": 1}, {"ragged": 1},
              {"block_kib": 16, "burst_kib": 4}, {"block_kib": 256, "burst_kib": 16, "side": 170, "ragged": 1}]
    for kw in points:
        assert calibrate_store(0, n, 1, "block", **kw) > 0, kw
