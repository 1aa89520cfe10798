"""The pinned snapshot fixtures (tests/golden/snapshots/<plan>.json.gz) and how to replay them.

One gzipped JSON file per plan: the app text, the HipEngine config, the engine calls made before the
snapshot, the blob sdh_engine_snapshot returned then (base64), the calls made after it, the oracle's
matches of that second part and, of the first part, only how many it found (K_ratchet's 78,000 would not
fit the file). Gzip is what keeps the files small: a partitioned table has at least 64 keys, so the
blobs of gen, fanout and part are 6.8, 28 and 36 MB of mostly zeroed tables, and those tests decode that.

How they were recorded, and would be again with a bump of SNAP_VERSION: the oracle ran the whole stream
with every call on it written down as a step; an engine of the build before the sections moved into
their units replayed the first part and was snapshotted; a fresh engine restored the blob and replayed
the rest equal to the oracle. Before the snapshot the partitioned apps push one event at a time: keys that
first appear within one push take their ids in the order an atomic hands them out, so only then is the
blob a function of the events. One blob is not that build's output byte for byte: it saved key_of_id
past n_keys as the device memory happened to be, and the 58 such words of gen.json.gz (words 439106 to
439163, all 282) were set to zero, which is what a build that clears the table at creation writes.

Test infrastructure only."""
import base64
import gzip
import json
import os

import numpy as np

from harness import App

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "snapshots")
PLANS = ("chain", "ratchet", "gate", "gen", "fanout", "part", "seq", "slab", "absent", "retain")


def _tuples(matches):
    return [(q, k, ts, tuple(tuple(s) for s in slots)) for q, k, ts, slots in matches]


def load(plan):
    with gzip.open(os.path.join(GOLDEN, plan + ".json.gz"), "rt") as f:
        fx = json.load(f)
    fx["blob"] = base64.b64decode(fx.pop("blob_b64"))
    fx["matches_after"] = _tuples(fx["matches_after"])
    return fx


class Replay:
    """The fixture's app compiled by this build, and fresh engines of the fixture's config."""

    def __init__(self, fx):
        self.fx = fx
        self.app = App(fx["app"], engine_factory=lambda blob: None)
        self.types = [s.attr_types for s in self.app.ir.streams]

    def engine(self):
        from siddhi_amd.engine import HipEngine
        e = HipEngine(self.app.blob, stream_types=self.types, **self.fx["config"])
        if self.fx["retain"]:
            e.retain_events(self.fx["retain"])
        return e

    def run(self, eng, steps):
        """Makes the recorded calls on `eng`; returns its matches."""
        n_slots = lambda q: len(self.app.ir.queries[q].states)  # noqa: E731
        out = []
        for s in steps:
            op = s["op"]
            if op == "send":
                n = len(s["ts"])
                vals = np.array(s["vals"], dtype=np.int64).reshape(n, len(self.types[s["stream"]]))
                nulls = None if s["nulls"] is None else np.array(s["nulls"], dtype=np.uint8).reshape(vals.shape)
                eng.send(s["stream"], np.array(s["ts"], dtype=np.int64), vals, nulls, s["chunk"])
            elif op == "strings":
                eng.set_strings(s["ids"], s["texts"])
            elif op == "start":
                eng.start(s["t"])
            elif op == "advance":
                eng.advance_time(s["t"])
            else:
                raise ValueError(op)
            if op in ("send", "advance"):
                out.extend(eng.take_matches(n_slots))
        return out
