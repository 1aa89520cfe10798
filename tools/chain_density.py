"""Cost of K_chain's tables at density: the cross-stream family

    every e1=A[price > T_p] -> e2=B[price > e1.price] within W_p sec      (T_p as C2's, W_p = 1 + p % 10)

at --patterns patterns over workloads.stock_events (1 event / ms), pushed device-resident in blocks
of --push events that alternate between A and B, in device-record mode (no host copy of the matches).
Nothing completes or expires a partial while A is pushed, so an A block leaves about push * (1 - T_p /
100) partials per query for the next B block. One run per process, one JSON line:

    python tools/chain_density.py --mode chain            the growing K_chain (paged past 512 partials)
    python tools/chain_density.py --mode gen              the same queries with SDH_FLAG_FORCE_GEN
    python tools/chain_density.py --mode chain --push 256 --partials 512
                                                          a case that stays in the register form
    python tools/chain_density.py --pred arith            e2=B[price > e1.price * 1.01]: a partial residual
    python tools/chain_density.py --pred or               e2=B[price > e1.price or volume > e1.volume]
                                                          (K_chain's general predicates; with
                                                          --mode gen the same queries on K_gen)

--root DIR imports the package (and its library) from another checkout, to compare two commits.
ms_per_push is the median wall time of a push (it returns when its kernels have finished); live_per_query
is sdh_stats.live_partials / patterns after the A block and after the B block of the last pair.
"""
import argparse
import json
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=["chain", "gen"], default="chain")
ap.add_argument("--patterns", type=int, default=1000)
ap.add_argument("--push", type=int, default=65536)
ap.add_argument("--pairs", type=int, default=6, help="timed (A block, B block) pairs")
ap.add_argument("--warmup", type=int, default=2, help="untimed pairs first (the tables grow in them)")
ap.add_argument("--partials", type=int, default=0)
ap.add_argument("--pred", choices=["plain", "arith", "or"], default="plain", help="e2's filter")
ap.add_argument("--root", default=".")
a = ap.parse_args()
sys.path.insert(0, a.root)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from siddhi_amd import ql  # noqa: E402
from siddhi_amd.engine import SDH_FLAG_DEVICE_MATCHES, SDH_FLAG_FORCE_GEN, EngineError, HipEngine  # noqa: E402
from siddhi_amd.events import StringDictionary  # noqa: E402
from siddhi_amd.planner import plan  # noqa: E402
from siddhi_amd.workloads import c2_threshold_text, stock_events  # noqa: E402

COLS = "(symbol string, price float, volume int)"
PRED = {"plain": "price > e1.price", "arith": "price > e1.price * 1.01",
        "or": "price > e1.price or volume > e1.volume"}[a.pred]
src = [f"define stream A {COLS}; define stream B {COLS};"]
for p in range(a.patterns):
    src.append(f"@info(name='p{p}') from every e1=A[price > {c2_threshold_text(p)}] -> e2=B[{PRED}] "
               f"within {1 + p % 10} sec select e1.price as p1, e2.price as p2 insert into OutStream;")
ir = plan(ql.parse(" ".join(src)))
d = StringDictionary()
blob = ir.serialize([d.intern(s) for s in ir.strings])
flags = SDH_FLAG_DEVICE_MATCHES | (SDH_FLAG_FORCE_GEN if a.mode == "gen" else 0)
out = {"mode": a.mode, "patterns": a.patterns, "push": a.push, "partials": a.partials, "pred": a.pred,
       "root": a.root}
try:
    eng = HipEngine(blob, stream_types=[s.attr_types for s in ir.streams], flags=flags, partials=a.partials)
    dev = torch.device("cuda:0")
    ms, live, matches = {"A": [], "B": []}, {}, 0
    for pair in range(a.warmup + a.pairs):
        for k, stream in enumerate("AB"):
            ts, sym, price, vol = stock_events((2 * pair + k) * a.push, a.push)
            t_ts = torch.from_numpy(ts).to(dev)
            cols = [torch.from_numpy(c).to(dev) for c in (sym, price.view(np.int32), vol)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.push_device(k, a.push, t_ts.data_ptr(), [c.data_ptr() for c in cols])
            dt = (time.perf_counter() - t0) * 1e3
            matches += eng.pending_matches()
            if pair >= a.warmup:
                ms[stream].append(dt)
            if pair == a.warmup + a.pairs - 1:
                live[stream] = eng.stats().live_partials / a.patterns
    st = eng.stats()
    out.update(ms_per_push_A=round(statistics.median(ms["A"]), 3), ms_per_push_B=round(statistics.median(ms["B"]), 3),
               ms_per_push=round(statistics.median(ms["A"] + ms["B"]), 3),
               ms_min_max=[round(min(ms["A"] + ms["B"]), 3), round(max(ms["A"] + ms["B"]), 3)],
               live_per_query_after_A=round(live["A"], 1), live_per_query_after_B=round(live["B"], 1),
               matches=matches, pool_regrows=st.pool_regrows, plan_queries=list(st.plan_queries))
    eng.close()
except EngineError as ex:
    out.update(failed=f"{ex.code}: {ex}")
print(json.dumps(out))
