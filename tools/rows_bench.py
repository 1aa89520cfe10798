#!/usr/bin/env python3
"""Measure the device selector (sdh_engine_poll_rows) on the README's "C2 delivered" leg: C2 at
10K patterns with the workload's own select list, 64K-event device pushes.

Legs (each on a fresh engine over the same pushes, one JSON line on stdout):
  compact   push + poll_compact(device=1), the existing path
  rows      retain_events + push + poll_rows(device=1); the push alone with and without retention
            (their difference is the store's append), the poll alone, the rows' byte count and its
            fraction of sdh_calibrate_hbm's copy rate
  records   (--records, or --legs records) SDH_FLAG_DEVICE_MATCHES + retain_events + push +
            records_rows(0, total, device=1): the rows projected from the push's device records; the bytes
            the projection moves (entries and side entries in, the row arrays out) over its time as a
            fraction of the copy rate; records_search: the same with SDH_RR_SEARCH=1 (the per-entry side
            search instead of the side-run expansion)
--lib PATH runs against another build of the library (the parent commit's, `--legs compact`).
For the kernels' own times run it under `rocprofv3 --kernel-trace --stats -- python tools/rows_bench.py`
(store_append_kernel, select_placed_kernel, ratchet_compact_kernel, select_ratchet_records_kernel)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=1 << 16)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--retain", type=int, default=1 << 17, help="events kept (C2's longest within is 60,000 events)")
    ap.add_argument("--legs", default="compact,rows")
    ap.add_argument("--records", action="store_true", help="the device-record legs (records,records_search) only")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--no-calibrate", action="store_true")
    ap.add_argument("--quick", action="store_true", help="rows leg: the timings only (no byte count, no twin engines)")
    args = ap.parse_args()
    if args.lib:
        os.environ["SIDDHI_HIP_LIB"] = args.lib
    import numpy as np
    import torch
    from siddhi_amd import ql
    from siddhi_amd.engine import HipEngine, calibrate_hbm
    from siddhi_amd.planner import plan
    from siddhi_amd.workloads import c2_app, stock_events_torch

    assert torch.cuda.is_available(), "rows_bench needs an MI355X"
    dev = torch.device("cuda:0")
    blob = plan(ql.parse(c2_app(args.patterns))).serialize()
    E, n = args.batch, args.steps + args.warmup
    bs = []
    for s in range(n):
        ts, sym, price, vol = stock_events_torch(s * E, E, 100, dev)
        bs.append([ts, sym, price.view(torch.int32), vol])
    torch.cuda.synchronize()
    legs = ["records", "records_search"] if args.records else args.legs.split(",")
    out = {"patterns": args.patterns, "events_per_push": E, "steps": args.steps}

    def run(retain, poll):
        """per-step (push ms, poll ms, rows) over the timed steps"""
        eng = HipEngine(blob)
        if retain:
            eng.retain_events(retain)
        push, pol, rows, last = [], [], [], None
        for i, cols in enumerate(bs):
            t0 = time.perf_counter()
            eng.push_device(0, E, cols[0].data_ptr(), [c.data_ptr() for c in cols[1:]])
            eng.lib.sdh_engine_flush(eng.h)
            t1 = time.perf_counter()
            last = poll(eng)
            eng.lib.sdh_engine_flush(eng.h)
            t2 = time.perf_counter()
            if i >= args.warmup:
                push.append((t1 - t0) * 1e3)
                pol.append((t2 - t1) * 1e3)
                rows.append(last.n)
        return eng, push, pol, rows, last

    med = statistics.median
    if "compact" in legs:
        eng, push, pol, rows, _ = run(0, lambda e: e.poll_compact(device=True))
        out["compact"] = {"push_ms": med(push), "poll_ms": med(pol), "ms_per_push": med([a + b for a, b in zip(push, pol)]),
                          "rows_per_push": med(rows), "placed_pushes": eng.stats().placed_pushes}
        eng.close()
    if "rows" in legs:
        eng, push, pol, rows, last = run(args.retain, lambda e: e.poll_rows(device=True))
        width = last.width
        both = [a + b for a, b in zip(push, pol)]
        if args.quick:
            out["rows"] = {"push_ms": med(push), "poll_ms": med(pol), "ms_per_push": med(both), "ms_per_push_min": min(both),
                           "ms_per_push_max": max(both), "rows_per_push": med(rows), "width": width}
            eng.close()
            legs = [x for x in legs if x != "rows"]
    if "rows" in legs:
        # the bytes the last poll could not avoid: the same window as compact rows on a twin engine
        twin = HipEngine(blob)
        for cols in bs:
            twin.push_device(0, E, cols[0].data_ptr(), [c.data_ptr() for c in cols[1:]])
            if cols is not bs[-1]:
                twin.poll_compact(device=True)
        base, crow = twin.poll_compact()
        e2 = base + crow[:, 1].astype(np.int64)
        events = len(np.unique(np.concatenate([e2, e2 - crow[:, 2]])))
        nrow = len(crow)
        assert nrow == rows[-1], (nrow, rows[-1])
        row_words = 2 + 3
        rd = 16 * nrow + 8 * len(np.unique(e2)) + 8 * row_words * events
        wr = (8 * width + 8 + 8 + 8 + 4) * nrow
        r = {"push_ms": med(push), "poll_ms": med(pol), "ms_per_push": med(both),
             "ms_per_push_min": min(both), "ms_per_push_max": max(both),
             "rows_per_push": med(rows), "width": width, "placed_pushes": eng.stats().placed_pushes,
             "rows_per_s_poll": med(rows) / (med(pol) * 1e-3),
             "last_poll": {"rows": nrow, "distinct_events": events, "bytes_read": rd, "bytes_written": wr,
                           "poll_ms": pol[-1], "gbps": (rd + wr) / (pol[-1] * 1e-3) / 1e9}}
        eng.close()
        twin.close()
        # the push alone without retention (same engine flow, compact poll): the append is the difference
        eng, push0, _, _, _ = run(0, lambda e: e.poll_compact(device=True))
        eng.close()
        r["push_ms_no_retention"] = med(push0)
        r["append_ms_by_difference"] = med(push) - med(push0)
        if not args.no_calibrate:
            copy_gbps, read_gbps = calibrate_hbm(0, 1 << 30, 5)
            r["hbm_copy_gbps"] = copy_gbps
            r["last_poll"]["fraction_of_copy_rate"] = r["last_poll"]["gbps"] / copy_gbps
        out["rows"] = r
    for leg in ("records", "records_search"):
        if leg not in legs:
            continue
        from siddhi_amd.engine import SDH_FLAG_DEVICE_MATCHES
        eng = HipEngine(blob, flags=SDH_FLAG_DEVICE_MATCHES, debug={"SDH_RR_SEARCH": 1} if leg == "records_search" else None)
        eng.retain_events(args.retain)
        push, pol, rows, nbytes, width = [], [], [], [], 0
        for i, cols in enumerate(bs):
            t0 = time.perf_counter()
            eng.push_device(0, E, cols[0].data_ptr(), [c.data_ptr() for c in cols[1:]])
            eng.lib.sdh_engine_flush(eng.h)
            t1 = time.perf_counter()
            r, total = eng.records_rows(0, 1 << 62, device=True)  # (one call: every row of the push)
            eng.lib.sdh_engine_flush(eng.h)
            t2 = time.perf_counter()
            assert r.n == total
            width = r.width
            if i >= args.warmup:
                push.append((t1 - t0) * 1e3)
                pol.append((t2 - t1) * 1e3)
                rows.append(total)
                # entries and side entries in, query + ts + seq + nulls + `width` cells per row out
                nbytes.append(eng.poll_records().r_bytes + (4 + 8 + 8 + 8 + 8 * width) * total)
        both = [a + b for a, b in zip(push, pol)]
        gbps = med([b / (t * 1e-3) / 1e9 for b, t in zip(nbytes, pol)])
        r = {"push_ms": med(push), "rows_ms": med(pol), "rows_ms_min": min(pol), "rows_ms_max": max(pol),
             "ms_per_push": med(both), "ms_per_push_min": min(both), "ms_per_push_max": max(both),
             "rows_per_push": med(rows), "width": width, "bytes_per_call": med(nbytes), "gbps": gbps,
             "rows_per_s": med(rows) / (med(pol) * 1e-3)}
        eng.close()
        if not args.no_calibrate and leg == "records":
            copy_gbps, _ = calibrate_hbm(0, 1 << 30, 5)
            r["hbm_copy_gbps"] = copy_gbps
            r["fraction_of_copy_rate"] = gbps / copy_gbps
        out[leg] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
