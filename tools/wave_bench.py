"""K_wave against the general interpreter on the C3 family's count shape without its partition
(workloads.c3w_app): `python tools/wave_bench.py [--patterns 1000] [--events 65536] [--pushes 15]
[--warmup 3] [--legs kwave,nokwave,parent] [--root DIR] [--deep]`.

Legs: kwave (this build), nokwave (this build with SDH_NO_KWAVE=1: the same queries on K_gen) and parent
(--root DIR: the library and package of another checkout, the parent commit's, which plans them on
K_gen). Every leg is a fresh process: device-resident batches, device-record mode (the kernels' own
cost, no table sort), a synchronise inside the timed region, warm-up pushes, the median over the timed
pushes. The legs' match counts must be equal. The thresholds and `within 10 sec` are C3's: on the CPU
oracle 40 of these patterns hold 63 to 160 pending-list entries (1.6 to 4 per query) after each of six
5,000-event pushes, so the K_gen legs stay far inside their pools.

--deep: one query held at about 4,200 live partials (4,200 events that each open a partial and never
pass f2), then pushes of 500 events that open none: the table is walked and nothing changes. The shape
DESIGN §3.3 "One lane, deep table" timed for the partitioned chain. A K_gen leg cannot hold it (4,096
StateEvents per instance): it reports the error it ends with.
Prints one JSON line per leg and one summary line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEEP = ("@info(name='deep') from every e1=StockStream[price > 40.0] -> e2=StockStream[volume > 5000] <2:5> -> "
        "e3=StockStream[price > e1.price and price > e2[last].price] within 1 hour "
        "select e1.price as a, e3.price as c insert into OutStream;")


def run_leg(args):
    sys.path.insert(0, args.root if (args.root and args.leg == "parent") else HERE)
    import torch
    from siddhi_amd import ql
    from siddhi_amd.engine import SDH_FLAG_DEVICE_MATCHES, EngineError, HipEngine
    from siddhi_amd.planner import plan
    from siddhi_amd.workloads import STOCK_STREAM, c2_threshold_text, splitmix64, stock_events_torch, PATTERN_SEED
    try:
        from siddhi_amd.workloads import c3w_app
        src = c3w_app(args.patterns)
    except ImportError:  # (a checkout from before K_wave: the same text)
        qs = []
        for p in range(args.patterns):
            v = 100 + (splitmix64(PATTERN_SEED ^ (p + 1000)) % 800)
            qs.append(f"@info(name='w{p}') from every e1=StockStream[price > {c2_threshold_text(p)}] -> "
                      f"e2=StockStream[volume > {v // 4}] <2:5> -> e3=StockStream[price > e2[last].price] within 10 sec "
                      f"select e1.price as a, e2[0].volume as b, e3.price as c insert into OutStream;")
        src = STOCK_STREAM + " " + " ".join(qs)
    if args.deep:
        src = STOCK_STREAM + " " + DEEP
    ir = plan(ql.parse(src))
    debug = {"SDH_NO_KWAVE": "1"} if args.leg == "nokwave" else None
    eng = HipEngine(ir.serialize(), stream_types=[s.attr_types for s in ir.streams], flags=SDH_FLAG_DEVICE_MATCHES,
                    debug=debug, gen_pool_states=32, gen_pool_nodes=128, gen_list_cap=32)  # (K_gen: small pools, they grow)
    dev = torch.device("cuda:0")
    E = 500 if args.deep else args.events
    if args.deep:  # 4,200 openers (price 50), then pushes that open nothing (price 10)
        def flat(n, price, t0):
            return (torch.arange(t0, t0 + n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                    torch.full((n,), price, dtype=torch.float32, device=dev), torch.ones(n, dtype=torch.int32, device=dev))
        batches = [flat(4200, 50.0, 0)] + [flat(E, 10.0, 4200 + i * E) for i in range(args.pushes)]
    else:
        batches = [stock_events_torch(i * E, E, 1000, dev) for i in range(args.pushes)]
    torch.cuda.synchronize()
    ms, err = [], ""
    try:
        for i, (ts, sym, price, vol) in enumerate(batches):
            t0 = time.perf_counter()
            eng.push_device(0, len(ts), ts.data_ptr(), [sym.data_ptr(), price.data_ptr(), vol.data_ptr()])
            torch.cuda.synchronize()
            if i >= args.warmup + (1 if args.deep else 0):
                ms.append((time.perf_counter() - t0) * 1e3)
    except EngineError as ex:
        err = f"{ex.code}: {ex}"
    st = eng.stats() if not err else None
    out = dict(leg=args.leg, deep=bool(args.deep), patterns=1 if args.deep else args.patterns, events=E, pushes=len(ms), error=err,
               median_ms=statistics.median(ms) if ms else None, min_ms=min(ms) if ms else None,
               max_ms=max(ms) if ms else None, matches=int(st.matches) if st else None,
               live_partials=int(st.live_partials) if st else None, plan_queries=list(st.plan_queries) if st else None,
               pool_regrows=int(st.pool_regrows) if st else None)
    print("LEG " + json.dumps(out), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", type=int, default=1000)
    ap.add_argument("--events", type=int, default=1 << 16)
    ap.add_argument("--pushes", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="kwave,nokwave,parent")
    ap.add_argument("--deep", action="store_true")
    ap.add_argument("--root", default=None, help="the parent commit's checkout (built): the parent leg runs on its package and library")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--leg-timeout", type=int, default=240)
    args = ap.parse_args()
    if args.pushes - args.warmup < 12:
        ap.error("the median is over at least 12 timed pushes")
    if args.leg:
        return run_leg(args)
    legs = []
    for leg in args.legs.split(","):
        if leg == "parent" and not args.root:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--patterns", str(args.patterns), "--events",
               str(args.events), "--pushes", str(args.pushes), "--warmup", str(args.warmup)]
        cmd += ["--deep"] if args.deep else []
        cmd += ["--root", args.root] if args.root else []
        # (a fresh process per leg; a leg that fails or runs out of time ends the run)
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.leg_timeout)
        except subprocess.TimeoutExpired:
            print(f"leg {leg} ran out of time ({args.leg_timeout} s)", flush=True)
            return 1
        sys.stderr.write(p.stderr[-2000:])
        if p.returncode != 0:
            print(f"leg {leg} failed with status {p.returncode}", flush=True)
            return 1
        line = [x for x in p.stdout.splitlines() if x.startswith("LEG ")][-1]
        print(line, flush=True)
        legs.append(json.loads(line[4:]))
    ok = [x for x in legs if not x["error"]]
    assert len({x["matches"] for x in ok}) <= 1, "the legs disagree on the match count"
    print(json.dumps(dict(summary={x["leg"]: (round(x["median_ms"], 3) if not x["error"] else x["error"]) for x in legs},
                          matches=ok[0]["matches"] if ok else None)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
