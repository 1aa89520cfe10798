"""Cost of an interleaved push (sdh_engine_push_mixed; DESIGN.md §3.2 "Interleaved pushes"): the
cross-stream family of tools/chain_density.py

    every e1=A[price > T_p] -> e2=B[price > e1.price] within W_p sec      (T_p as C2's, W_p = 1 + p % 10)

at --patterns patterns over workloads.stock_events (1 event / ms), where a seeded coin per event says
whether it belongs to A or B. Each call carries --events merged events, parts and order resident in HBM.

    python tools/mixed_bench.py                      every leg below, each a fresh process under --limit seconds
    python tools/mixed_bench.py --leg native --events 65536
                                                     one native call per --events events (device records)
    python tools/mixed_bench.py --leg native --events 65536 --records table
                                                     the same with the matches appended to the match table
    python tools/mixed_bench.py --leg split --events 2048
                                                     SDH_MIX_SPLIT=1: one push per same-stream run (what run
                                                     pushes through sdh_engine_push cost; match table mode,
                                                     device records do not survive a run push)

    python tools/mixed_bench.py --plan gen           the same legs over the cross-stream logical family

        every e1=A[price > T_p] -> e2=B[price > e1.price] and e3=A[price > T_p + 2] within W_p milliseconds

                                                     (W_p = 8 + p % 9, so a query holds a handful of partials, far
                                                     inside K_gen's pools: pool_regrows stays 0), which plans on
                                                     K_gen; native there is one K_gen launch over the merged sequence
    python tools/mixed_bench.py --plan gen --with-seq --leg native --events 65536 --records table
                                                     the known cost: one single-stream every-start sequence (kept on
                                                     K_gen by SDH_FLAG_FORCE_GEN) beside them, whose run pushes walk
                                                     in event chunks and whose native call does not

One JSON line per leg: ms_per_call is the median wall time of --calls calls after --warmup untimed ones,
the engine's stream drained inside the timed region; the match table is polled (on the device) outside it.
"""
import argparse
import json
import statistics
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=["all", "native", "split"], default="all")
ap.add_argument("--plan", choices=["chain", "gen"], default="chain")
ap.add_argument("--with-seq", action="store_true", help="--plan gen: add the single-stream sequence (SDH_FLAG_FORCE_GEN)")
ap.add_argument("--tile", type=int, default=0, help="--plan gen: SDH_MIX_GEN_TILE (events staged at a time; 1: unstaged)")
ap.add_argument("--patterns", type=int, default=1000)
ap.add_argument("--events", type=int, default=65536)
ap.add_argument("--calls", type=int, default=12)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--records", choices=["device", "table"], default="device")
ap.add_argument("--limit", type=int, default=240, help="seconds per leg (driver mode)")
ap.add_argument("--split-events", type=int, default=2048, help="driver mode: the split leg's call size")
ap.add_argument("--root", default=".")
a = ap.parse_args()

if a.leg == "all":
    base = [sys.executable, __file__, "--patterns", str(a.patterns), "--calls", str(a.calls), "--warmup", str(a.warmup),
            "--root", a.root, "--plan", a.plan]
    legs = [["--leg", "native", "--events", "2048"], ["--leg", "native", "--events", "65536"],
            ["--leg", "native", "--events", "2048", "--records", "table"],
            ["--leg", "native", "--events", "65536", "--records", "table"],
            ["--leg", "split", "--events", str(a.split_events)]]
    for leg in legs:
        try:
            r = subprocess.run(base + leg, timeout=a.limit, capture_output=True, text=True)
            line = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else json.dumps({"leg": leg, "failed": r.stderr[-300:]})
            print(line, flush=True)
            if r.returncode != 0:  # (a leg that died ends the run: nothing more starts on the card)
                sys.exit(r.returncode)
        except subprocess.TimeoutExpired:
            print(json.dumps({"leg": leg, "failed": f"no result within {a.limit} s"}), flush=True)
            sys.exit(124)
    sys.exit(0)

sys.path.insert(0, a.root)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from siddhi_amd import ql  # noqa: E402
from siddhi_amd.engine import SDH_FLAG_DEVICE_MATCHES, SDH_FLAG_FORCE_GEN, EngineError, HipEngine  # noqa: E402
from siddhi_amd.events import StringDictionary  # noqa: E402
from siddhi_amd.planner import plan  # noqa: E402
from siddhi_amd.workloads import c2_threshold_text, stock_events  # noqa: E402

COLS = "(symbol string, price float, volume int)"
src = [f"define stream A {COLS}; define stream B {COLS};"]
for p in range(a.patterns if a.plan == "gen" else 0):
    t10 = 200 + (p % 750)
    src.append(f"@info(name='p{p}') from every e1=A[price > {c2_threshold_text(p)}] -> e2=B[price > e1.price] and "
               f"e3=A[price > {(t10 + 20) // 10}.{t10 % 10}] within {8 + p % 9} milliseconds "
               f"select e1.price as p1, e3.price as p3 insert into OutStream;")
if a.with_seq:
    src.append("@info(name='seq') from every e1=A[price > 50], e2=A[price > e1.price], e3=A[price > e2.price] "
               "select e1.price as p1, e3.price as p3 insert into OutStream;")
for p in range(a.patterns if a.plan == "chain" else 0):
    src.append(f"@info(name='p{p}') from every e1=A[price > {c2_threshold_text(p)}] -> e2=B[price > e1.price] "
               f"within {1 + p % 10} sec select e1.price as p1, e2.price as p2 insert into OutStream;")
ir = plan(ql.parse(" ".join(src)))
d = StringDictionary()
blob = ir.serialize([d.intern(s) for s in ir.strings])
split = a.leg == "split"
records = "table" if split else a.records
out = {"leg": a.leg, "plan": a.plan, "patterns": a.patterns, "events": a.events, "records": records, "root": a.root}
debug = {"SDH_MIX_SPLIT": 1} if split else {}
if a.tile:
    debug["SDH_MIX_GEN_TILE"] = a.tile
    out["tile"] = a.tile
try:
    eng = HipEngine(blob, stream_types=[s.attr_types for s in ir.streams],
                    flags=(SDH_FLAG_DEVICE_MATCHES if records == "device" else 0) | (SDH_FLAG_FORCE_GEN if a.with_seq else 0),
                    debug=debug or None)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(17)
    ms, matches, runs = [], 0, 0
    for call in range(a.warmup + a.calls):
        ts, sym, price, vol = stock_events(call * a.events, a.events)
        order = rng.integers(0, 2, a.events).astype(np.int32)
        runs = 1 + int(np.count_nonzero(np.diff(order)))
        keep, parts = [], []
        for p in range(2):
            m = order == p
            cols = [torch.from_numpy(np.ascontiguousarray(c[m])).to(dev) for c in (ts, sym, price.view(np.int32), vol)]
            keep += cols
            parts.append((p, int(m.sum()), cols[0].data_ptr(), [c.data_ptr() for c in cols[1:]]))
        d_order = torch.from_numpy(order).to(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.push_mixed_device(parts, d_order.data_ptr(), a.events)
        eng.lib.sdh_engine_flush(eng.h)
        dt = (time.perf_counter() - t0) * 1e3
        if records == "device":
            matches += eng.poll_records().n
        else:
            matches += eng.poll_device().n
        if call >= a.warmup:
            ms.append(dt)
    st = eng.stats()
    out.update(ms_per_call=round(statistics.median(ms), 3), ms_min_max=[round(min(ms), 3), round(max(ms), 3)],
               runs_last_call=runs, matches=matches, live_per_query=round(st.live_partials / a.patterns, 1),
               pool_regrows=st.pool_regrows, mixed_pushes=list(eng.debug_mixed_pushes()),
               plan_queries=list(st.plan_queries))
    eng.close()
except EngineError as ex:
    out.update(failed=f"{ex.code}: {ex}")
print(json.dumps(out))
