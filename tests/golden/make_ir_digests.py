"""Record the serialized program of every function-free app the suite plans, as SHA-256 digests, into
tests/golden/ir_digests.json. tests/test_functions.py::test_function_free_programs_keep_their_bytes
compares the planner against this list, so the list is generated from the commit BEFORE a change to
the planner or the IR (run this script with that commit's package on the path), never from the
change itself.

    python tests/golden/make_ir_digests.py            # rewrites ir_digests.json
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def apps():
    """(id, app text) of every workload of siddhi_amd/workloads.py (at small pattern counts: a
    query's bytes do not depend on how many follow it) and of every reference_kat.json fixture."""
    from siddhi_amd import workloads as w
    yield "workloads.c1", w.c1_app()
    yield "workloads.c2", w.c2_app(130)
    yield "workloads.c2x", w.c2x_app(130)
    yield "workloads.c3", w.c3_app(130)
    yield "workloads.c4", w.c4_app(130)
    yield "workloads.c5", w.c5_app(130)
    kat = json.load(open(os.path.join(HERE, "reference_kat.json")))
    for fx in kat["fixtures"]:
        yield "reference_kat." + fx["id"], fx["app"]


def digests():
    from siddhi_amd import ql
    from siddhi_amd.planner import plan
    out = {}
    for name, src in apps():
        try:
            blob = plan(ql.parse(src)).serialize()
        except (ql.SiddhiParserException, ql.SiddhiAppCreationException):
            continue  # (apps the front end refuses have no bytes to pin)
        out[name] = hashlib.sha256(blob).hexdigest()
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    d = digests()
    with open(os.path.join(HERE, "ir_digests.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_ir_digests.py", "digests": d}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(d), "digests")
