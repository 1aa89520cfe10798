"""The snapshot blob, section by section (siddhi_amd/csrc/engine_snap.hip): one tiny app per plan, pinned
in tests/golden/snapshots (snapshot_golden.py).

The fixtures were written by the build before the sections moved into their units, so equal bytes here
are the proof that the move left versions 8 and 9 alone; from then on they fail any change of the blob
that does not bump SNAP_VERSION (snapshot_golden.py says how they were recorded)."""
import numpy as np
import pytest

import snapshot_golden as sg

pytestmark = pytest.mark.gpu

E_INVALID, E_CAPACITY = -1, -4
_CACHE = {}


def fixture(plan):
    """(fixture, Replay, this build's blob after the fixture's first part), once per module"""
    if plan not in _CACHE:
        fx = sg.load(plan)
        r = sg.Replay(fx)
        eng = r.engine()
        try:
            assert len(r.run(eng, fx["before"])) == fx["n_matches_before"]
            _CACHE[plan] = (fx, r, eng.snapshot())
        finally:
            eng.close()
    return _CACHE[plan]


@pytest.mark.parametrize("plan", sg.PLANS)
def test_snapshot_restore_snapshot_is_idempotent(plan):
    """(every plan, K_slab's repacked ring included, gave equal bytes before the move as well)"""
    _, r, blob = fixture(plan)
    eng = r.engine()
    try:
        eng.restore(blob)
        assert eng.snapshot() == blob
    finally:
        eng.close()


@pytest.mark.parametrize("plan", sg.PLANS)
def test_pinned_format(plan):
    fx, r, blob = fixture(plan)
    assert np.frombuffer(fx["blob"][:16], np.int64)[1] == (9 if fx["retain"] else 8)
    assert len(blob) == len(fx["blob"])
    assert blob == fx["blob"], "this build writes another blob for the same state: bump SNAP_VERSION"
    eng = r.engine()
    try:
        eng.restore(fx["blob"])
        assert eng.snapshot() == fx["blob"], "this build does not load and save the recorded blob alike"
        assert r.run(eng, fx["after"]) == fx["matches_after"]
    finally:
        eng.close()


def test_failed_restore_marks_the_engine_broken():
    """Truncated K_chain blobs (no payload word is altered): past the prologue the restore has begun to
    load, so the engine refuses pushes until a good restore, which the same engine then takes."""
    from siddhi_amd.engine import EngineError
    fx, r, _ = fixture("chain")
    good = fx["blob"]
    prologue = 8 * (13 + len(r.types))
    eng = r.engine()
    try:
        for cut in (prologue + 8, prologue + 8 * (2 + 64), len(good) - 8):  # a header word, mid-table, the last word
            with pytest.raises(EngineError) as ei:
                eng.restore(good[:cut])
            assert ei.value.code == E_INVALID and "truncated" in str(ei.value)
            with pytest.raises(EngineError) as ei:
                r.run(eng, fx["after"][:1])
            assert ei.value.code == E_CAPACITY and "failed restore" in str(ei.value)
        eng.restore(good)
        assert r.run(eng, fx["after"]) == fx["matches_after"]
    finally:
        eng.close()


def test_refused_restore_leaves_the_engine_usable():
    """A blob refused by the prologue's checks (wrong magic, another query count, a cut inside the
    prologue) changes nothing: the engine goes on from the state it had."""
    from siddhi_amd.engine import EngineError
    fx, r, _ = fixture("chain")
    words = np.frombuffer(fx["blob"], np.int64)
    magic, nq = words.copy(), words.copy()
    magic[0] ^= 1
    nq[2] += 1
    eng = r.engine()
    try:
        r.run(eng, fx["before"])
        for bad in (magic.tobytes(), nq.tobytes(), fx["blob"][:8 * 5]):
            with pytest.raises(EngineError) as ei:
                eng.restore(bad)
            assert ei.value.code == E_INVALID
        assert r.run(eng, fx["after"]) == fx["matches_after"]
    finally:
        eng.close()
