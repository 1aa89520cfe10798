"""The shared-pops form of K_ratchet (nfa_ratchet_shared.hip): the pops of the family
`every e1=S[f0] -> e2=S[cur.a OP e1.a] within T` computed once per push and filtered per group.

Every test feeds the same pushes, in device-record mode, to three engines -- the form forced
(SDH_RATCHET_SHARED_MIN=1), the form off (SDH_RATCHET_NO_SHARED=1) and the CPU oracle -- and compares
them push by push: by the record digest (count, order-independent hash; sdh_engine_debug_digest, the
oracle's computed here from its matches) and, at these small sizes, by the decoded (query, e2, e2 - e1)
rows. Each test also asserts through sdh_engine_debug_shared_pushes that the form really ran (and,
where a push must route to the existing kernel, that it did not)."""
import ctypes

import numpy as np
import pytest

from harness import App
from siddhi_amd.workloads import c2_app, stock_events

pytestmark = pytest.mark.gpu

ON = {"SDH_RATCHET_SHARED_MIN": 1}
OFF = {"SDH_RATCHET_NO_SHARED": 1}


def _mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def rows_digest(rows, seq_base):
    """matches.hip digest_ratchet_kernel over (query, e2 - seq_base, e2 - e1) rows."""
    if not len(rows):
        return (0, 0)
    r = np.asarray(rows, dtype=np.int64)
    with np.errstate(over="ignore"):
        s = (r[:, 1] + seq_base).astype(np.uint64)
        s1 = (r[:, 1] + seq_base - r[:, 2]).astype(np.uint64)
        h = _mix64(_mix64(s * np.uint64(0x9E3779B97F4A7C15) ^ r[:, 0].astype(np.uint64)) ^ s1)
        return (len(r), int(h.sum(dtype=np.uint64)))


def decode_records(rec):
    """K_ratchet device records -> sorted (query, e2 - seq_base, e2 - e1) rows, from the layouts in
    include/siddhi_hip.h (as tests/test_gpu_records.py decode_ratchet_torch, on the host)."""
    from siddhi_amd.engine import SDH_REC_4, SDH_REC_8
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]

    def host(ptr, n, dtype):
        out = np.zeros(n, dtype)
        if n:
            assert hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
        return out

    nb, bb = rec.r_blocks, rec.r_blk_bytes
    if nb == 0:
        return []
    blk = host(rec.r_base, nb * bb // 4, np.uint32).reshape(nb, bb // 4)
    cnt = host(rec.r_count, nb, np.int32)
    grp = host(rec.r_group, nb, np.int32)
    lq = host(rec.r_lane_query, (int(grp.max()) + 1) * 64, np.int32)
    out = []
    if rec.r_format == SDH_REC_4:
        side = host(rec.r_side, nb, np.int32)
        assert (side >= 0).all()
        for b in range(nb):
            n, ns = int(cnt[b]), int(side[b])
            if n == 0:
                continue
            pairs = blk[b].reshape(-1, 2)[::-1][:ns].astype(np.int64)  # side entry j = (first, e2)
            assert ns > 0 and pairs[0, 0] == 0 and (np.diff(pairs[:, 0]) > 0).all() and pairs[-1, 0] < n
            e2 = pairs[np.searchsorted(pairs[:, 0], np.arange(n), side="right") - 1, 1]
            ent = blk[b, :n].astype(np.int64)
            q = lq[grp[b] * 64 + (ent >> 26)]
            out.append(np.stack([q, e2, ent & ((1 << 26) - 1)], 1))
    else:
        assert rec.r_format == SDH_REC_8
        for b in range(nb):
            n = int(cnt[b])
            v = blk[b].reshape(-1, 2)[:n].astype(np.int64)
            e2 = v[:, 0] & ((1 << 26) - 1)
            d = (((rec.seq_base + e2) & 0xFFFFFFFF) - v[:, 1]) & 0xFFFFFFFF
            out.append(np.stack([lq[grp[b] * 64 + (v[:, 0] >> 26)], e2, d], 1))
    if not out:
        return []
    return sorted(map(tuple, np.concatenate(out).tolist()))


_ORACLE = {}  # oracle_key -> the oracle's rows per push (a run shared by several tests is computed once)


class Trio:
    """The oracle and two device-record engines (debug knobs `a` and `b`) fed the same pushes."""

    def __init__(self, src, a=ON, b=OFF, oracle_key=None, **kw):
        from siddhi_amd.engine import SDH_FLAG_DEVICE_MATCHES, HipEngine
        self.known = _ORACLE.get(oracle_key)
        self.rows = [] if oracle_key is not None and self.known is None else None
        self.oracle_key = oracle_key
        self.n_push = 0
        self.oracle = App(src) if self.known is None else None
        app = App(src, engine_factory=lambda blob: None)
        types = [s.attr_types for s in app.ir.streams]
        mk = lambda dbg: HipEngine(app.blob, stream_types=types, flags=SDH_FLAG_DEVICE_MATCHES, debug=dbg, **kw)  # noqa: E731
        self.a, self.b = mk(a), mk(b)
        self.seq = 0
        self.total = 0

    def push(self, ts, cols, rows=True):
        """One push to all three; returns the oracle's sorted rows."""
        ts = np.ascontiguousarray(ts, dtype=np.int64)
        if self.known is not None:
            want = self.known[self.n_push]
        else:
            self.oracle.engine.send(0, ts, np.stack([c.astype(np.int64) for c in cols], 1), None)
            om = self.oracle.engine.take_matches(lambda q: 2)
            want = sorted((m[0], m[3][1][0] - self.seq, m[3][1][0] - m[3][0][0]) for m in om)
            if self.rows is not None:
                self.rows.append(want)
        self.n_push += 1
        dw = rows_digest(want, self.seq)
        for name, e in (("a", self.a), ("b", self.b)):
            e.push_columns(0, ts, cols)
            dg = e.debug_digest()
            rec = e.poll_records()
            assert dg == dw, f"engine {name}, push at seq {self.seq} ({len(ts)} events): {dg} != oracle {dw}"
            assert rec.r_n == dw[0]
            if rows:
                assert decode_records(rec) == want, f"engine {name}, push at seq {self.seq}: rows differ"
        self.seq += len(ts)
        self.total += len(want)
        return want

    def close(self):
        if self.rows is not None:
            _ORACLE[self.oracle_key] = self.rows
        self.a.close()
        self.b.close()


def c2_cols(start, n):
    ts, sym, price, vol = stock_events(start, n)
    return ts, [sym, price.view(np.uint32), vol]


SIZES = (1, 63, 64, 65, 1000, 3807)


def test_tile_and_push_boundaries():
    """130 C2 patterns (two full groups and a 2-lane one), 5,000 events pushed as 1, 63, 64, 65, 1,000
    and 3,807 events: state carried across every boundary."""
    t = Trio(c2_app(130), oracle_key="c2_130_sizes")
    start = 0
    for n in SIZES:
        t.push(*c2_cols(start, n))
        start += n
    assert start == 5000 and t.total > 100000
    assert t.a.debug_shared_pushes() == len(SIZES) and t.b.debug_shared_pushes() == 0
    t.close()


def test_form_alternating_per_push():
    """The same run with the form on and off in alternate pushes: engine a takes it in the even pushes,
    engine b in the odd ones, so every push compares the two forms on states the other form left."""
    t = Trio(c2_app(130), a={"SDH_RATCHET_SHARED_MIN": 1, "SDH_RATCHET_SHARED_ALT": 0},
             b={"SDH_RATCHET_SHARED_MIN": 1, "SDH_RATCHET_SHARED_ALT": 1}, oracle_key="c2_130_sizes")
    start = 0
    for n in SIZES:
        t.push(*c2_cols(start, n))
        start += n
    assert t.a.debug_shared_pushes() == 3 and t.b.debug_shared_pushes() == 3
    t.close()


def test_orientations_and_ties():
    """All four of <, <=, >, >= over prices quantised to 8 values with NaNs mixed in: ties decide
    between the strict and non-strict next-greater / next-smaller element."""
    qs = ["define stream S (v float);"]
    k = 0
    for op in ("<", "<=", ">", ">="):
        for c in (1.5, 3.0, 4.5):
            f0 = f"v > {c}" if ">" in op else f"v < {c + 2}"
            w = "" if c == 3.0 else f" within {20 + 15 * k} milliseconds"
            qs.append(f"@info(name='q{k}') from every e1=S[{f0}] -> e2=S[v {op} e1.v]{w} select e1.v as a insert into O;")
            k += 1
    t = Trio(" ".join(qs))
    rng = np.random.default_rng(11)
    v = rng.integers(0, 8, 2000).astype(np.float32)
    v[rng.random(2000) < 0.07] = np.nan
    ts = np.cumsum(rng.integers(0, 4, 2000)).astype(np.int64)
    for lo, hi in ((0, 700), (700, 2000)):
        t.push(ts[lo:hi], [v[lo:hi].view(np.uint32)])
    assert t.total > 5000
    assert t.a.debug_shared_pushes() == 2 and t.b.debug_shared_pushes() == 0
    t.close()


@pytest.mark.parametrize("shape", ["falling", "rising", "constant"])
def test_key_shapes(shape):
    """Strictly falling, strictly rising and constant prices, 100K events, nothing expires.

    Falling: nothing pops, every event's search for its popper runs to the end of the batch (the tree
    bounds it: the test finishes in seconds), and the lanes end up holding 299, 699 and 1,199 partials
    -- past rML + rSC = 264 and the persisted 512, so the pushes come back through the err[0] re-runs;
    a closing spike then pops them all, which checks the state entry for entry. The start filters pass
    only the last 299 .. 1,199 events, which keeps the oracle's walk over the pending lists short; the
    second push starts with 600 of them carried.
    Constant: `>` patterns whose start filter passes would hold all 100K events pending (the oracle
    walks them per event), so the constant case runs `>=` and `<=` (each event pops its predecessor)
    and `>` / `<` with start filters that fail."""
    n = 100_000
    i = np.arange(n, dtype=np.float32)
    if shape == "falling":
        v = np.float32(n) - i
        cond = [(f"v < {c}.0", ">") for c in (300, 700, 1200)]
    elif shape == "rising":
        v = i
        cond = [("v > 10.0", ">"), ("v > 50000.0", ">="), ("v > 99000.0", "<")]
    else:
        v = np.full(n, 7.0, np.float32)
        cond = [("v > 5.0", ">="), ("v < 9.0", "<="), ("v > 8.0", ">"), ("v < 6.0", "<")]
    qs = ["define stream S (v float);"]
    for k, (f0, op) in enumerate(cond):
        qs.append(f"@info(name='q{k}') from every e1=S[{f0}] -> e2=S[v {op} e1.v] within 1000 sec "
                  "select e1.v as a insert into O;")
    t = Trio(" ".join(qs))
    ts = np.arange(n + 4, dtype=np.int64)
    v = np.concatenate([v, np.array([3e5, -5.0, 3e5, 7.0], np.float32)])  # (a closing spike and dip)
    cut = n - 600 if shape == "falling" else 60_000
    for lo, hi in ((0, cut), (cut, n), (n, n + 4)):
        t.push(ts[lo:hi], [v[lo:hi].view(np.uint32)], rows=hi - lo <= 4 or shape == "falling")
    assert t.total >= (2200 if shape == "falling" else 100_000)
    assert t.a.debug_shared_pushes() == 3 and t.b.debug_shared_pushes() == 0
    t.close()


def _window_src(withins):
    qs = ["define stream S (v float);"]
    for k, w in enumerate(withins):
        qs.append(f"@info(name='q{k}') from every e1=S[v > {10 + 7 * k}.0] -> e2=S[v > e1.v] {w} "
                  "select e1.v as a insert into O;")
    return " ".join(qs)


def test_window_one_millisecond():
    """`within 1 milliseconds` over timestamps stepping by 1: nearly everything expires."""
    t = Trio(_window_src(["within 1 milliseconds"] * 3 + ["within 2 milliseconds"]))
    v = (np.random.default_rng(3).integers(0, 1000, 3000) / 10).astype(np.float32)
    ts = np.arange(3000, dtype=np.int64)
    for lo, hi in ((0, 1000), (1000, 3000)):
        t.push(ts[lo:hi], [v[lo:hi].view(np.uint32)])
    assert 100 < t.total < 6000 and t.a.debug_shared_pushes() == 2
    t.close()


def test_window_equal_timestamp_runs():
    """Long runs of equal timestamps (50 events each, 7 ms apart) against windows of 1, 7, 10 and 30 ms."""
    t = Trio(_window_src(["within 1 milliseconds", "within 7 milliseconds", "within 10 milliseconds",
                          "within 30 milliseconds"]))
    v = (np.random.default_rng(4).integers(0, 1000, 3000) / 10).astype(np.float32)
    ts = (np.arange(3000, dtype=np.int64) // 50) * 7
    for lo, hi in ((0, 1025), (1025, 3000)):
        t.push(ts[lo:hi], [v[lo:hi].view(np.uint32)])
    assert t.total > 3000 and t.a.debug_shared_pushes() == 2
    t.close()


def test_window_carried_entry_older_than_2_31_ms():
    """Partials carried over a gap of more than 2^31 ms: one pattern never expires, one has a window of
    597 hours (2^31 ms + 1,716,352), which some of the carried partials outlive and some do not."""
    t = Trio(_window_src(["", "within 597 hours", "within 1 sec"]))
    v1 = (60 - np.arange(40) * 0.5).astype(np.float32)  # a falling staircase: all stay pending
    ts1 = np.arange(40, dtype=np.int64) * 100_000
    t.push(ts1, [v1.view(np.uint32)])
    gap = (1 << 31) + 1_716_352 + 2_000_000  # the 597-hour window ends inside the staircase (at step 20)
    ts2 = gap + np.arange(64, dtype=np.int64) * 10
    v2 = (35 + np.arange(64) * 0.5).astype(np.float32)  # rising: pops the staircase step by step
    want = t.push(ts2, [v2.view(np.uint32)])
    per_q = [sum(1 for r in want if r[0] == q) for q in range(3)]
    assert per_q[0] > per_q[1] > per_q[2] >= 0 and per_q[1] - per_q[2] > 5
    assert t.a.debug_shared_pushes() == 2
    t.close()


def test_window_batch_spanning_2_31_ms_routes_to_the_existing_kernel():
    """A batch spanning 2^31 - 2 ms or more is outside the pairs' 32-bit ages: it takes the existing
    kernel's full-expiry form (and still matches); the pushes around it take the shared form."""
    t = Trio(_window_src(["", "within 597 hours", "within 1 sec", "within 20 sec"]))
    rng = np.random.default_rng(6)
    v = (rng.integers(0, 1000, 900) / 10).astype(np.float32)
    ts = np.arange(900, dtype=np.int64) * 50
    ts[300:600] = ts[300] + np.arange(300, dtype=np.int64) * ((1 << 31) // 299 + 1)
    ts[600:] = ts[599] + 50 + np.arange(300, dtype=np.int64) * 50
    assert ts[599] - ts[300] >= (1 << 31) - 2
    for k, (lo, hi) in enumerate(((0, 300), (300, 600), (600, 900))):
        t.push(ts[lo:hi], [v[lo:hi].view(np.uint32)])
        assert t.a.debug_shared_pushes() == (1, 1, 2)[k]
    assert t.total > 1000
    t.close()


def test_window_out_of_order_batch():
    """A batch with a timestamp out of order sets err[1] in the pre-pass and re-runs exactly in the
    existing kernel's full-expiry form."""
    t = Trio(_window_src(["", "within 1 sec", "within 20 milliseconds", "within 5 sec"]))
    rng = np.random.default_rng(7)
    v = (rng.integers(0, 1000, 1200) / 10).astype(np.float32)
    ts = np.arange(1200, dtype=np.int64) * 5
    ts[700] = ts[690]
    t.push(ts[:500], [v[:500].view(np.uint32)])
    assert t.a.debug_shared_pushes() == 1
    t.push(ts[500:], [v[500:].view(np.uint32)])
    assert t.a.debug_shared_pushes() == 1  # (the re-run took the existing kernel)
    assert t.total > 1000
    t.close()


def test_blocks_one_event_crosses_a_block_and_first_attempt_runs_out():
    """match_capacity of one block: the first attempt runs out of blocks (err[2] re-run). 130 patterns
    hold a 400-step falling staircase; one spike pops 25,600 partials per full group, more than a
    block's 16K entries, so the event's run continues behind a second side entry in the next block."""
    qs = ["define stream S (v float);"]
    for k in range(130):
        qs.append(f"@info(name='q{k}') from every e1=S[v > {k % 5}.0] -> e2=S[v > e1.v] select e1.v as a insert into O;")
    t = Trio(" ".join(qs), match_capacity=1)
    v = np.concatenate([1000 - np.arange(400), [5000, 6000]]).astype(np.float32)
    ts = np.arange(402, dtype=np.int64)
    want = t.push(ts, [v.view(np.uint32)])
    assert len(want) == 130 * 401
    t.push(ts[:50] + 1000, [v[:50].view(np.uint32)])
    assert t.a.debug_shared_pushes() == 2
    t.close()


def test_state_is_byte_equal_and_restores_across_forms():
    """After the same pushes the two forms' snapshots are byte-equal; each engine then restores the
    other's snapshot and continues equal to the oracle."""
    t = Trio(c2_app(70))  # (a full group and a 6-lane one)
    t.push(*c2_cols(0, 1500), rows=False)
    t.push(*c2_cols(1500, 700), rows=False)
    sa, sb = t.a.snapshot(), t.b.snapshot()
    assert sa == sb
    t.a.restore(sb)
    t.b.restore(sa)
    t.push(*c2_cols(2200, 800))
    assert t.a.debug_shared_pushes() == 3 and t.b.debug_shared_pushes() == 0
    t.close()


def test_two_key_columns_on_one_stream():
    """Two float attributes of one stream, each the key of patterns with the same OP: both sets are
    SIM launches of one push, and each needs the pops of its own column (one pre-pass per stream, key
    column and OP)."""
    qs = ["define stream S (a float, b float);"]
    k = 0
    for col in ("a", "b"):
        for thr in (20, 45, 70):
            qs.append(f"@info(name='q{k}') from every e1=S[{col} > {thr}.0] -> e2=S[{col} > e1.{col}] "
                      f"within {30 + 40 * k} milliseconds select e1.{col} as x insert into O;")
            k += 1
    t = Trio(" ".join(qs))
    rng = np.random.default_rng(21)
    n = 3000
    a = (rng.integers(0, 1000, n) / 10).astype(np.float32)
    b = (100 - np.abs(np.arange(n) % 200 - 100) + rng.integers(0, 3, n)).astype(np.float32)  # (a saw-tooth: unlike a)
    ts = np.arange(n, dtype=np.int64)
    per_col = [0, 0]
    for lo, hi in ((0, 1100), (1100, n)):
        want = t.push(ts[lo:hi], [a[lo:hi].view(np.uint32), b[lo:hi].view(np.uint32)])
        for r in want:
            per_col[r[0] // 3] += 1
    assert min(per_col) > 1000 and per_col[0] != per_col[1]
    assert t.a.debug_shared_pushes() == 2 and t.b.debug_shared_pushes() == 0
    t.close()


def test_falling_search_is_bounded():
    """2M strictly falling prices: no event has a popper, and every tile's search for one must end by
    the tree (a few loads of 64 summaries per tile, some 1e5 loads in all), not by walking the rest of
    the column (n^2 / 64 / 2 = 3e10 loads of 64 events, tens of seconds at the ~1e9 dependent wave
    loads per second the chip sustains). The bound of 2 s on the forced form's push -- upload, pre-pass,
    launch and the read-back of the counts -- is a hundred times what the bounded search needs and a
    tenth of what the walk would take. A closing spike pops the 98 partials the last events opened."""
    import time
    src = ("define stream S (v float); @info(name='q') from every e1=S[v < 100.0] -> e2=S[v > e1.v] "
           "within 10 sec select e1.v as a insert into O;")
    t = Trio(src)
    n = 2_000_000
    v = np.float32(n) - np.arange(n, dtype=np.float32)
    v[-1] = 5e6
    ts = np.arange(n, dtype=np.int64)
    cols = [v.view(np.uint32)]
    t.push(ts[:4096], [cols[0][:4096]], rows=False)  # (the engines' first push allocates)
    t0 = time.perf_counter()
    t.a.push_columns(0, ts[4096:], [cols[0][4096:]])
    dt = time.perf_counter() - t0
    da = t.a.debug_digest()
    t.a.poll_records()
    print(f"forced form, {n - 4096} falling events: {dt:.3f} s")
    t.b.push_columns(0, ts[4096:], [cols[0][4096:]])
    db = t.b.debug_digest()
    t.b.poll_records()
    t.oracle.engine.send(0, ts[4096:], np.stack([cols[0][4096:].astype(np.int64)], 1), None)
    om = t.oracle.engine.take_matches(lambda q: 2)
    want = sorted((m[0], m[3][1][0] - 4096, m[3][1][0] - m[3][0][0]) for m in om)
    assert len(want) == 98
    assert da == db == rows_digest(want, 4096)
    assert t.a.debug_shared_pushes() == 2 and t.b.debug_shared_pushes() == 0
    assert dt < 2.0, f"the forced form's push of {n - 4096} falling events took {dt:.2f} s"
    t.close()
