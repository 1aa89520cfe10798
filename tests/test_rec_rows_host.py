"""siddhi_amd/csrc/rec_rows.h on the host: what sdh_engine_records_rows runs on the device to turn a
row of a push's device records into a match source -- the rec4 side-run expansion against a numpy
restatement of the header's rule (include/siddhi_hip.h: "entry i belongs to the trigger e2 of the last
side entry whose first <= i"), the flat record decode against the restatement of the table append's
(_slots, tests/test_gpu_records.py), and the row location. No GPU."""
import numpy as np
import pytest

import rec_rows_host as H
from test_gpu_records import _slots

I32MIN = -(1 << 31)
SB = (1 << 33) + 12345  # a seq_base past 32 bits


# ---- rec4 blocks built in numpy -----------------------------------------------------------------------
def rec4_block(blk_bytes, entries, sides):
    """entries: uint32 {d | lane << 26}; sides: [(first, e2)] -> the block's bytes (the free middle is
    filled with a pattern no decode may read as data)."""
    b = np.full(blk_bytes // 4, 0xDEADBEEF, np.uint32)
    b[:len(entries)] = entries
    for j, (f, e2) in enumerate(sides):
        at = blk_bytes // 4 - 2 * (j + 1)
        assert at >= len(entries), "entries and side entries overlap"
        b[at], b[at + 1] = f, e2
    return b.view(np.uint8)


def rule(entries, sides, i0, i1, sb):
    """The header's rule, restated: (e1, e2, lane) of entries [i0, i1)."""
    firsts = np.array([f for f, _ in sides], np.int64)
    e2s = np.array([e for _, e in sides], np.int64)
    i = np.arange(i0, i1)
    j = np.searchsorted(firsts, i, side="right") - 1
    ent = entries[i0:i1].astype(np.int64)
    e2 = sb + e2s[j]
    return np.stack([e2 - (ent & ((1 << 26) - 1)), e2, ent >> 26], 1), j


def make_entries(rng, n):
    return (rng.integers(0, 1 << 26, n, dtype=np.uint32) | (rng.integers(0, 64, n, dtype=np.uint32) << 26)).astype(np.uint32)


def check_runs(entries, sides, blk_bytes, run_lens, starts=None):
    blk = rec4_block(blk_bytes, entries, sides)
    n = len(entries)
    for L in run_lens:
        for i0 in (starts if starts is not None else sorted({0, 1, max(0, n - L), n // 3, n // 2})):
            i1 = min(n, i0 + L)
            if i1 <= i0:
                continue
            want, j = rule(entries, sides, i0, i1, SB)
            got, read = H.pairs(blk, 3, len(sides), i0, i1, SB)
            assert np.array_equal(got, want), (L, i0)
            # the run read exactly the side entries its entries belong to, once
            assert read == j[-1] - j[0] + 1
            assert H.side_of(blk, len(sides), i0) == j[0] and H.side_of(blk, len(sides), i1 - 1) == j[-1]


RUNS = (1, 63, 64, 65, 256)


def test_rec4_one_side_entry():
    rng = np.random.default_rng(1)
    check_runs(make_entries(rng, 700), [(0, 41)], 4096, RUNS)


def test_rec4_one_side_entry_per_entry():
    rng = np.random.default_rng(2)
    n = 300
    check_runs(make_entries(rng, n), [(i, 7 + 3 * i) for i in range(n)], 4096, RUNS)


def test_rec4_first_side_entry_continues_the_previous_blocks_event():
    """Side entry 0 (first == 0) names an event whose earlier entries filled the block before: its run
    ends where the block's own first event begins."""
    rng = np.random.default_rng(3)
    n = 500
    sides = [(0, 99), (37, 100), (38, 101), (290, 102)]
    check_runs(make_entries(rng, n), sides, 4096, RUNS, starts=(0, 1, 36, 37, 38, 39, 200, 289, 290, 291, n - 1))


def test_rec4_block_full_at_both_ends():
    """Entries and side entries meet: the last entry's dword is followed by the last side entry."""
    rng = np.random.default_rng(4)
    ns = 64
    blk_bytes = 2048
    n = (blk_bytes - 8 * ns) // 4
    firsts = np.sort(rng.choice(np.arange(1, n), ns - 1, replace=False))
    sides = [(0, 5)] + [(int(f), 6 + k) for k, f in enumerate(firsts)]
    assert 4 * n + 8 * ns == blk_bytes
    check_runs(make_entries(rng, n), sides, blk_bytes, RUNS + (n,))


def test_rec4_runs_that_start_mid_event():
    rng = np.random.default_rng(5)
    n = 1000
    sides = [(0, 1), (100, 2), (101, 3), (400, 4), (990, 5)]
    check_runs(make_entries(rng, n), sides, 8192, RUNS, starts=(50, 99, 100, 101, 102, 250, 399, 400, 401, 744, 989, 990, 999))


def test_rec4_side_entries_with_equal_first():
    """Two side entries with one first index (an event that wrote no entry): the rule's "last" wins."""
    rng = np.random.default_rng(6)
    n = 300
    sides = [(0, 1), (10, 2), (10, 3), (200, 4), (200, 5), (200, 6)]
    check_runs(make_entries(rng, n), sides, 4096, RUNS, starts=(0, 9, 10, 11, 199, 200, 201))


def test_8_and_16_byte_records():
    rng = np.random.default_rng(7)
    n = 200
    off = rng.integers(0, 1 << 26, n).astype(np.int64)
    ln = rng.integers(0, 64, n).astype(np.int64)
    d = rng.integers(0, 1 << 31, n).astype(np.int64)  # e2 - e1, past 26 bits
    e2 = SB + off
    e1 = e2 - d
    want = np.stack([e1, e2, ln], 1)
    r8 = np.zeros((n, 2), np.uint32)
    r8[:, 0] = (off | (ln << 26)).astype(np.uint32)
    r8[:, 1] = (e1 & 0xFFFFFFFF).astype(np.uint32)
    got, _ = H.pairs(r8.view(np.uint8).ravel(), 1, -1, 0, n, SB)
    assert np.array_equal(got, want)
    r16 = np.zeros((n, 4), np.uint32)
    r16[:, 0], r16[:, 1], r16[:, 2] = off, ln, (e1 & 0xFFFFFFFF)
    got, _ = H.pairs(r16.view(np.uint8).ravel(), 2, -1, 3, n - 2, SB)
    assert np.array_equal(got, want[3:n - 2])


# ---- flat records -------------------------------------------------------------------------------------
def pack(lo, hi):
    v = (int(lo) & 0xFFFFFFFF) | ((int(hi) & 0xFFFFFFFF) << 32)
    return v - (1 << 64) if v >= 1 << 63 else v


def full(q, key, ts, seq, idx, S, stream, slots, wide=False):
    w6 = S | (stream << 16) | ((1 << 32) if wide else 0)
    return [7 + len(slots), q, key, ts, seq, idx, w6] + list(slots)


def orand(q, off, kid, d1, da, db):
    return [pack(-4, q), pack(off, kid), pack(d1, da), pack(db, 0x5A5A5A5A)]


def count(q, off, kid, d1, dists):
    c = len(dists)
    words = 3 + (c + 1) // 2
    padded = list(dists) + [0x1234567] * (c & 1)
    return [pack(-(words + 0x10000), q), pack(off, kid), pack(d1, c)] + \
        [pack(padded[2 * k], padded[2 * k + 1]) for k in range((c + 1) // 2)]


def window(q, off, dists, kind=2, kid=0):
    """K_seq window (kind 2: S in w1's upper half) or K_part chain (kind 3: key id there, an unused upper
    half INT32_MIN) of S = len(dists) + 1 states."""
    S = len(dists) + 1
    words = 2 + S // 2
    padded = list(dists) + [I32MIN if kind == 3 else 0x7654321] * (2 * (words - 2) - len(dists))
    return [pack(-(words + (kind << 16)), q), pack(off, S if kind == 2 else kid)] + \
        [pack(padded[2 * k], padded[2 * k + 1]) for k in range(words - 2)]


def pad(words, rng):
    """A pad record: only its first word is written; what follows is whatever the buffer held."""
    junk = [int(x) for x in rng.integers(-(1 << 62), 1 << 62, words - 1)]
    return [(-(0x40000 + words)) & 0xFFFFFFFF] + junk


def chain_slots(r, sq):
    """A kind 3 record's slot words, restated from the header (S: 3 words -> 2 if w[2]'s upper half is
    INT32_MIN else 3; 4 words -> 4)."""
    lo = lambda x: int(np.int32(np.uint32(int(x) & 0xFFFFFFFF)))  # noqa: E731
    hi = lambda x: int(np.int32(np.uint32((int(x) >> 32) & 0xFFFFFFFF)))  # noqa: E731
    words = (-lo(r[0])) & 0xFFFF
    S = 4 if words >= 4 else 2 if hi(r[2]) == I32MIN else 3
    out = []
    for j in range(S - 1):
        out += [1, sq - (hi(r[2 + j // 2]) if j & 1 else lo(r[2 + j // 2]))]
    return out + [1, sq]


def expected(rec):
    """(query, trigger seq, own_ts, ts, slot words) of one record built above."""
    r = np.array(rec, np.int64)
    lo = int(np.int32(np.uint32(int(r[0]) & 0xFFFFFFFF)))
    if lo >= 0:
        return int(r[1]), int(r[4]), True, int(r[3]), tuple(int(x) for x in r[7:lo])
    kind = (-lo) >> 16
    sq = SB + (int(r[1]) & 0xFFFFFFFF)
    slots = chain_slots(r, sq) if kind == 3 else _slots(r, sq, kind)
    return int(r[0]) >> 32, sq, False, 0, tuple(slots)


def test_flat_records_decode_as_the_table_append_does():
    rng = np.random.default_rng(8)
    recs = [
        full(3, -1, 1111, SB + 9, 2, 3, 0, [1, SB + 1, 3, SB + 2, SB + 4, SB + 5, 1, SB + 9]),  # a count chain
        full(4, -1, 2222, SB + 10, 0, 2, 0xFFFF, [1, SB + 3, 0]),                              # a timer match
        full(9, 77, 3333, SB + 11, 0, 2, 0, [1, -1, 1, SB + 11]),            # the empty event of an absent side
        orand(5, 20, 6, 7, I32MIN, 0),
        orand(5, 21, 6, 8, 0, I32MIN),
        orand(6, 22, 1, 9, 3, 0),
        count(7, 30, 2, 11, [9, 8, 5]),
        count(7, 31, 2, 12, [9, 8, 5, 2]),
        count(7, 32, 2, 13, [4]),
        window(8, 40, [6, 2], kind=2),
        window(8, 41, [9, 6, 2], kind=2),
        window(8, 42, [12, 9, 6, 2], kind=2),
        window(10, 50, [5], kind=3, kid=4),
        window(10, 51, [7, 5], kind=3, kid=4),
        window(10, 52, [8, 7, 5], kind=3, kid=4),
        full(11, 5, 4444, SB + 60, 0, 3, 0, [1, SB - 5_000_000_000, 1, SB + 1, 1, SB + 60], wide=True),  # bit 32
    ]
    # pads between and after records (and one of a single word)
    buf, heads = [], []
    for k, r in enumerate(recs):
        heads.append(len(buf))
        buf += r
        if k % 3 == 1:
            buf += pad(1 + 5 * (k % 4), rng)
    buf += pad(1, rng) + pad(200, rng)
    got, pads = H.walk(buf, SB)
    assert pads == sum(1 for k in range(len(recs)) if k % 3 == 1) + 2
    assert [g[0] for g in got] == heads
    for g, r in zip(got, recs):
        assert g[1:] == expected(r), r
    assert len(got) == len(recs)
    # kind 3's S from the INT32_MIN upper half
    assert [len(g[5]) // 2 for g in got[12:15]] == [2, 3, 4]
    assert recs[12][2] >> 32 == I32MIN and (recs[14][3] >> 32) == I32MIN


def test_flat_and_chain_records_resolve_slot_indices():
    """StateEvent.getStreamEvent through the selector's event_of on the in-place match sources: first /
    last / counted-from-the-end events of a count chain, an empty logical side, a slot past the query's."""
    c = count(7, 30, 2, 11, [9, 8, 5])
    sq = SB + 30
    assert H.flat_event(c, SB, 0, 0) == sq - 11
    assert [H.flat_event(c, SB, 1, k) for k in (0, 1, 2, 3, -1, -2, -3, -4)] == \
        [sq - 9, sq - 8, sq - 5, None, sq - 5, sq - 8, sq - 9, None]
    assert H.flat_event(c, SB, 2, 0) == sq and H.flat_event(c, SB, 2, -1) == sq and H.flat_event(c, SB, 3, 0) is None
    o = orand(5, 20, 6, 7, I32MIN, 0)
    assert [H.flat_event(o, SB, s, 0) for s in range(4)] == [SB + 13, None, SB + 20, None]
    w = window(10, 51, [7, 5], kind=3, kid=4)
    assert [H.flat_event(w, SB, s, -1) for s in range(4)] == [SB + 44, SB + 46, SB + 51, None]
    f = full(3, -1, 1111, SB + 9, 2, 3, 0, [1, SB + 1, 3, SB + 2, SB + 4, SB + 5, 1, SB + 9])
    assert [H.flat_event(f, SB, 1, k) for k in (0, 2, 3, -1, -3, -4)] == [SB + 2, SB + 5, None, SB + 5, SB + 2, None]
    assert H.flat_event(f, SB, 2, 0) == SB + 9 and H.flat_event(f, SB, 3, 0) is None
    t = full(4, -1, 2222, SB + 10, 0, 2, 0xFFFF, [1, SB + 3, 0])
    assert H.flat_event(t, SB, 0, 0) == SB + 3 and H.flat_event(t, SB, 1, 0) is None
    k = [12, 999, 5, 6, 7]  # {query, ts, seq_0, seq_1, seq_2}
    assert [H.chain_event(k, 3, s, 0) for s in range(4)] == [5, 6, 7, None]
    assert H.chain_event(k, 3, 1, -1) == 6 and H.chain_event(k, 3, 1, 1) is None


# ---- row location -------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", [[3, 0, 0, 5, 1, 0], [0, 0, 4], [7], [0, 2, 0]])
def test_locate_skips_empty_items(counts):
    off = np.concatenate([[0], np.cumsum(counts)])
    want = np.repeat(np.arange(len(counts)), counts)
    for row in range(int(off[-1])):
        assert H.locate(off, row) == want[row]


@pytest.mark.parametrize("parts", [(5, 3, 4), (0, 3, 4), (5, 0, 4), (5, 3, 0), (0, 0, 4), (0, 2, 0), (6, 0, 0)])
def test_parts_first_and_last_rows(parts):
    total = sum(parts)
    want = [(p, k) for p in range(3) for k in range(parts[p])]
    assert [H.part_of(parts, r) for r in range(total)] == want
    # every window cuts into the parts' pieces that tile it in order
    for first in range(total + 2):
        for n in range(total + 2):
            rows = []
            for p in range(3):
                local, c = H.part_window(parts, p, first, n)
                rows += [(p, local + k) for k in range(c)]
            assert rows == want[first:first + n], (first, n)
