"""bench.py --dump-outputs: the K_ratchet record decoder on hand-built blocks (CPU: no GPU is touched).

The blocks are laid out as include/siddhi_hip.h documents them (rec4 entries with side entries from the
block's end, 8-B records in a block whose r_side is negative) and decoded twice: by bench.ratchet_outputs
(torch, whole blocks at a time) and by a record-at-a-time walk of the same layout here."""
import ctypes

import numpy as np

import bench
from siddhi_amd.engine import SDH_REC_4, SdhRecords

W = 64  # int32 words per block
M26 = (1 << 26) - 1


def _blocks(rng, n_ev, seq_base):
    """-> (block words [nb, W] uint32, count, side, group, lane_query, the matches as (query, e2, d))."""
    lane_q = np.full(2 * 64, -1, np.int32)
    lane_q[0:5] = [4, 0, 7, 2, 9]       # group 0: lanes 0..4
    lane_q[64:67] = [1, 3, 8]           # group 1: lanes 0..2
    blk, cnt, side, grp, rows = [], [], [], [], []
    for b, (g, fmt) in enumerate([(0, 4), (1, 8), (0, 4), (1, 4), (0, 8)]):
        w = np.zeros(W, np.uint32)
        lanes = 5 if g == 0 else 3
        if b == 2:  # an empty rec4 block
            n, ns = 0, 0
        elif fmt == 4:
            runs = [int(x) for x in rng.integers(0, 6, 7)]  # (a run of 0: a side entry with no entry)
            runs[0] = max(runs[0], 1)
            n, ns, i = sum(runs), len(runs), 0
            for j, r in enumerate(runs):
                e2 = int(rng.integers(0, n_ev))
                w[W - 2 * (j + 1)], w[W - 2 * (j + 1) + 1] = i, e2
                for _ in range(r):
                    ln, d = int(rng.integers(0, lanes)), int(rng.integers(1, 1 << 20))
                    w[i] = d | (ln << 26)
                    rows.append((int(lane_q[g * 64 + ln]), e2, d))
                    i += 1
        else:
            n, ns = int(rng.integers(1, W // 2)), -1
            for i in range(n):
                e2, ln, d = int(rng.integers(0, n_ev)), int(rng.integers(0, lanes)), int(rng.integers(1, 1 << 20))
                w[2 * i], w[2 * i + 1] = e2 | (ln << 26), (seq_base + e2 - d) & 0xFFFFFFFF
                rows.append((int(lane_q[g * 64 + ln]), e2, d))
        blk.append(w)
        cnt.append(n)
        side.append(ns)
        grp.append(g)
    return np.stack(blk), np.array(cnt, np.int32), np.array(side, np.int32), np.array(grp, np.int32), lane_q, rows


def test_ratchet_outputs_decode_the_documented_layout(monkeypatch):
    import torch

    def host_copy(ptr, nbytes, dev):
        t = torch.empty(nbytes, dtype=torch.uint8)
        ctypes.memmove(t.data_ptr(), ptr, nbytes)
        return t

    monkeypatch.setattr(bench, "_dev_copy", host_copy)
    monkeypatch.setattr(bench, "DUMP_CHUNK_BLOCKS", 2)  # three passes, the last of one block
    n_ev, seq_base = 40, (1 << 32) - 7  # (e1's low 32 bits wrap)
    blk, cnt, side, grp, lane_q, rows = _blocks(np.random.default_rng(3), n_ev, seq_base)
    rec = SdhRecords()
    rec.n = rec.r_n = len(rows)
    rec.seq_base, rec.n_events = seq_base, n_ev
    rec.r_blocks, rec.r_blk_bytes, rec.r_format = len(blk), W * 4, SDH_REC_4
    rec.r_base, rec.r_count, rec.r_side = blk.ctypes.data, cnt.ctypes.data, side.ctypes.data
    rec.r_group, rec.r_lane_query = grp.ctypes.data, lane_q.ctypes.data
    out = bench.ratchet_outputs(rec, torch.device("cpu"))
    want = np.array(sorted(rows, key=lambda r: (r[1], r[0], r[2])), dtype=np.float64)
    assert len(rows) > 30
    per_q, dsum, per_e = np.zeros(10), np.zeros(10), np.zeros(n_ev)
    for q, e2, d in rows:
        per_q[q] += 1
        dsum[q] += d
        per_e[e2] += 1
    assert out["matches_per_query"].dtype == np.float64 and np.array_equal(out["matches_per_query"], per_q)
    assert np.array_equal(out["e1_distance_sum_per_query"], dsum)
    assert out["matches_per_event"].dtype == np.float32 and np.array_equal(out["matches_per_event"], per_e)
    # every event is among the DUMP_SAMPLE_EVENTS sampled ones only when there are no more than that
    # many: the sample of this push holds exactly the matches of the events it names
    picked = set(out["sampled_matches"][:, 1].astype(int).tolist())
    assert len(picked) <= bench.DUMP_SAMPLE_EVENTS
    assert np.array_equal(out["sampled_matches"], want[[int(r[1]) in picked for r in want]])
    rng = np.random.default_rng(0)
    named = set(np.sort(rng.choice(n_ev, min(bench.DUMP_SAMPLE_EVENTS, n_ev), replace=False)).tolist())
    assert picked == {int(r[1]) for r in want if int(r[1]) in named}


def test_dump_outputs_writes_the_pushes_counts(tmp_path):
    """A step of four pushes with flat records only (the C5 shape): one summary row per push, float64,
    under the byte cap; nothing is decoded and no engine is asked for a digest."""
    recs = {}
    for si in range(4):
        r = SdhRecords()
        r.n = r.f_n = 100 + si
        r.n_events, r.seq_base = 512, 4096 + 512 * si
        recs[si] = r
    bench.dump_outputs(str(tmp_path / "d"), None, recs, None, 0, 1)
    files = sorted(p.name for p in (tmp_path / "d").iterdir())
    assert files == ["records_summary.npy"]
    a = np.load(tmp_path / "d" / "records_summary.npy")
    assert a.dtype == np.float64 and a.nbytes <= bench.DUMP_CAP
    assert a.tolist() == [[100 + si, 0, 100 + si, 0, 512, 4096 + 512 * si] for si in range(4)]


def test_plain_run_leaves_the_other_legs_out(monkeypatch):
    """Without --full every leg but the timed steps is off; --full leaves the --no-* options in charge."""
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.steps == 3 and a.dump_outputs is None
    assert a.no_expansion and a.no_ingest and a.no_latency and a.no_cpu_baseline and a.no_calibrate and a.no_weak_leg
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--no-latency", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.dump_outputs == "d" and a.no_latency
    assert not (a.no_expansion or a.no_ingest or a.no_cpu_baseline or a.no_calibrate or a.no_weak_leg)
