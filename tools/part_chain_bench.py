"""K_part's chain kind against the general interpreter on the C2 family per symbol (workloads.c2p_app):
`python tools/part_chain_bench.py [--patterns 1000] [--symbols 1000] [--events 65536] [--pushes 15]
[--warmup 3] [--legs compiled,interp,kgen] [--root DIR]`.

Legs: compiled (shape-compiled K_part, SDH_SPEC=require), interp (SDH_SPEC=0) and kgen
(SDH_FLAG_FORCE_GEN: what a build without the chain kind runs for these queries; --root DIR runs a leg on
the library and package of another checkout, e.g. the parent commit's). Every leg is a fresh process:
device-resident batches, device-record mode (the kernels' own cost, no table sort), a synchronise
inside the timed region, warm-up pushes, the median over the timed pushes. The legs' match counts
must be equal. Prints one JSON line per leg and one summary line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_leg(args):
    sys.path.insert(0, args.root or HERE)
    import numpy as np  # noqa: F401
    import torch
    from siddhi_amd import ql
    from siddhi_amd.engine import SDH_FLAG_DEVICE_MATCHES, SDH_FLAG_FORCE_GEN, HipEngine
    from siddhi_amd.planner import plan
    from siddhi_amd.workloads import STOCK_STREAM, c2_threshold_text, c2_within_sec, stock_events_torch
    try:
        from siddhi_amd.workloads import c2p_app
        src = c2p_app(args.patterns)
    except ImportError:  # (a checkout from before the chain kind: the same text)
        qs = [f"@info(name='p{p}') from every e1=StockStream[price > {c2_threshold_text(p)}] -> "
              f"e2=StockStream[price > e1.price] within {c2_within_sec(p)} sec "
              f"select e1.price as p1, e2.price as p2 insert into OutStream;" for p in range(args.patterns)]
        src = f"{STOCK_STREAM} partition with (symbol of StockStream) begin {' '.join(qs)} end;"
    ir = plan(ql.parse(src))
    blob = ir.serialize()
    flags = SDH_FLAG_DEVICE_MATCHES | (SDH_FLAG_FORCE_GEN if args.leg == "kgen" else 0)
    debug = {"compiled": {"SDH_SPEC": "require"}, "interp": {"SDH_SPEC": "0"}, "kgen": None}[args.leg]
    eng = HipEngine(blob, stream_types=[s.attr_types for s in ir.streams], flags=flags, debug=debug,
                    gen_pool_states=32, gen_pool_nodes=128, gen_list_cap=32,  # (K_gen: small pools, they grow)
                    gen_max_keys=max(64, 2 * args.symbols))
    eng.reserve_keys(args.symbols)
    dev = torch.device("cuda:0")
    E = args.events
    batches = [stock_events_torch(i * E, E, args.symbols, dev) for i in range(args.pushes)]
    torch.cuda.synchronize()
    ms = []
    for i, (ts, sym, price, vol) in enumerate(batches):
        t0 = time.perf_counter()
        eng.push_device(0, E, ts.data_ptr(), [sym.data_ptr(), price.data_ptr(), vol.data_ptr()])
        torch.cuda.synchronize()
        if i >= args.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    st = eng.stats()
    out = dict(leg=args.leg, root=args.root or "", patterns=args.patterns, symbols=args.symbols, events=E,
               pushes=len(ms), median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms),
               events_per_s=E / (statistics.median(ms) * 1e-3), matches=int(st.matches),
               live_partials=int(st.live_partials), plan_queries=list(st.plan_queries),
               spec_kernels=int(st.spec_kernels), last_part_items=int(st.last_part_items))
    print("LEG " + json.dumps(out), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", type=int, default=1000)
    ap.add_argument("--symbols", type=int, default=1000)
    ap.add_argument("--events", type=int, default=1 << 16)
    ap.add_argument("--pushes", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="compiled,interp,kgen")
    ap.add_argument("--root", default=None, help="another checkout (e.g. the parent commit's): the kgen leg, and only it, runs on that "
                    "checkout's package and library; the other legs always run on this one")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--leg-timeout", type=int, default=240)
    args = ap.parse_args()
    if args.pushes - args.warmup < 12:
        ap.error("the median is over at least 12 timed pushes")
    if args.leg:
        return run_leg(args)
    legs = []
    for leg in args.legs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--patterns", str(args.patterns), "--symbols",
               str(args.symbols), "--events", str(args.events), "--pushes", str(args.pushes), "--warmup", str(args.warmup)]
        if args.root and leg == "kgen":
            cmd += ["--root", args.root]
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
    assert len({x["matches"] for x in legs}) == 1, "the legs disagree on the match count"
    base = legs[-1]["median_ms"]
    print(json.dumps(dict(summary={x["leg"]: round(x["median_ms"], 3) for x in legs}, matches=legs[0]["matches"],
                          speedup_over_last_leg={x["leg"]: round(base / x["median_ms"], 2) for x in legs})))
    return 0


if __name__ == "__main__":
    sys.exit(main())
