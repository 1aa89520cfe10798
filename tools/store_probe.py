#!/usr/bin/env python3
"""Sweep of the write-stream probe (sdh_calibrate_store): one JSON line per point.

  tools/store_probe.py [--gib 16] [--iters 5] [--device 0] [--quick]
  tools/store_probe.py --point linear            one launch set of the linear fill (for a counter run)
  tools/store_probe.py --point block             the block pattern at the emission kernel's settings

The block pattern's base point is the emission kernel's: 64-KiB blocks, 8-KiB bursts, 170 side entries
as 8-byte stores, the claim behind the last burst, default store policy, whole quads. Each switch is
swept alone from that point, then the best settings together. A counter run (WRITE_SIZE) is a
`rocprofv3 --pmc WRITE_SIZE -- python tools/store_probe.py --point ...` of its own, no tracing beside it.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BASE = {"side": 170, "claim": 0, "nt": 0, "block_kib": 64, "burst_kib": 8, "ragged": 0}


def points(quick):
    from siddhi_amd.engine import STORE_SIDE_WHOLE
    yield "linear", {"nt": 0}
    yield "linear", {"nt": 1}
    yield "block", dict(BASE)
    sweeps = [("side", (0, STORE_SIDE_WHOLE)), ("claim", (1,)), ("nt", (1,)), ("block_kib", (16, 256)),
              ("burst_kib", (4, 16)), ("ragged", (1,))]
    for name, values in sweeps:
        for v in values:
            yield "block", dict(BASE, **{name: v})
    if not quick:
        yield "block", dict(BASE, side=0, ragged=0, claim=1)
        yield "block", dict(BASE, side=STORE_SIDE_WHOLE, claim=1)
        yield "block", dict(BASE, side=STORE_SIDE_WHOLE, claim=1, nt=1)
        yield "block", dict(BASE, side=STORE_SIDE_WHOLE, claim=1, block_kib=256, burst_kib=16)
        yield "block", dict(BASE, burst_kib=4, ragged=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=16.0, help="buffer size (far beyond the 256-MiB Infinity Cache)")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--quick", action="store_true", help="the single-switch sweeps only")
    ap.add_argument("--point", choices=("linear", "block"), default=None)
    a = ap.parse_args()
    if not 0.25 <= a.gib <= 64 or not 1 <= a.iters <= 50 or a.device < 0:
        ap.error("--gib in [0.25, 64], --iters in [1, 50], --device >= 0")
    from siddhi_amd.engine import calibrate_store
    nbytes = int(a.gib * (1 << 30)) & ~((1 << 20) - 1)
    todo = list(points(a.quick))
    if a.point:
        todo = [("linear", {"nt": 0})] if a.point == "linear" else [("block", dict(BASE))]
    for mode, kw in todo:
        gbps = calibrate_store(a.device, nbytes, a.iters, mode, **kw)
        print(json.dumps({"probe": "store", "mode": mode, **kw, "gib": a.gib, "iters": a.iters,
                          "gbps": round(gbps, 1)}), flush=True)


if __name__ == "__main__":
    main()
