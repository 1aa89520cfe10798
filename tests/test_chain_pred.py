"""K_chain's general predicates on the host: what siddhi_amd/csrc/chain_lower.h decides for a query
(atoms, tile residual, partial residual, refusals) and what the kernels' lane body (chain_pred.h)
evaluates, against siddhi_amd.selector.evaluate. tests/native/chain_host.cpp compiles both for the CPU."""
import os
import subprocess

import numpy as np
import pytest

import chain_host as ch
from harness import App
from siddhi_amd.events import EventLog, encode_rows
from siddhi_amd.ir import OP_ATTR
from siddhi_amd.selector import evaluate

T = ch.TYPED_STREAM + " "


def lowering(src, allow=True, name="q"):
    app = App(src, engine_factory=lambda blob: None)
    return ch.HostChain(app.blob).lower(app.ir.query_index(name), allow)


def q(pattern):
    return T + f"@info(name='q') from {pattern} select e1.i as x insert into O;"


def test_atoms_only_is_as_before():
    L = lowering(q("every e1=T[i > 3] -> e2=T[f > e1.f and i < 7]"))
    assert L.ok and L.n_code == 0
    assert (L.n_col, L.n_cap, L.n_xa, L.n_atoms) == (2, 1, 1, 3)
    assert L.xa_count[:2] == [0, 1] and L.tile_atoms[:2] == [1, 1]
    assert L.tile_code == [0] * 4 and L.partial_code == [0] * 4
    assert L.ratchet  # (K_gate's shape: nothing here changes what K_ratchet / K_gate take)


def test_tile_residual_keeps_a_ratchet_shape_on_k_chain():
    L = lowering(q("every e1=T[i * 2 > l or e1.d is null] -> e2=T[f > e1.f] within 10 milliseconds"))
    assert L.ok and L.tile_code[0] > 0 and L.partial_code == [0] * 4 and L.tile_code[1] == 0
    assert L.xa_count[1] == 1
    assert not L.ratchet  # K_ratchet and K_gate know atoms only


def test_partial_residual():
    L = lowering(q("every e1=T -> e2=T[f > e1.f * 1.05 and i > 0]"))
    assert L.ok and L.partial_code[1] == 5 and L.tile_code == [0] * 4
    assert L.tile_atoms[1] == 1 and L.xa_count[1] == 0 and L.n_cap == 1
    assert not L.ratchet
    # the residual's raw column of the float is not the atom's key column of the int
    assert L.n_col == 2


def test_second_capture_reading_atom_goes_to_the_partial_residual():
    L = lowering(q("every e1=T -> e2=T[s == e1.s and f > e1.f]"))
    assert L.ok and L.xa_count[1] == 1 and L.partial_code[1] == 3 and L.n_cap == 2
    L = lowering(q("every e1=T -> e2=T[s == e1.s and f > e1.f and i != e1.i]"))
    assert L.ok and L.xa_count[1] == 1 and L.partial_code[1] == 7 and L.n_cap == 3  # (two compares and an AND)
    assert not L.ratchet


def test_a_long_or_double_residual_operand_shares_the_key_column():
    L = lowering(q("every e1=T[d > 1.0 and l > 1 and (d + l > 5 or e1.d is null)] -> e2=T"))
    assert L.ok and L.n_col == 2 and L.tile_code[0] > 0


def test_three_states_read_two_earlier_slots():
    L = lowering(T + "define stream U (i int, f float); @info(name='q') from every e1=T -> e2=U[f > e1.f + 1 or i > e1.i] "
                 "-> e3=T[i > e1.i + e2.i] select e1.i as x insert into O;")
    assert L.ok and L.partial_code[1] > 0 and L.partial_code[2] == 5 and L.n_cap == 3


REFUSALS = [
    ("function", "every e1=T -> e2=T[ifThenElse(b, i, 3) > e1.i]", "function"),
    ("function in an or", "every e1=T[i > 3 or coalesce(l, 1l) > 2] -> e2=T", "function"),
    ("too long", "every e1=T -> e2=T[" + " or ".join(f"i + {k} > e1.i" for k in range(9)) + "]", "longer than 48"),
    ("too deep", "every e1=T -> e2=T[i + (i + (i + (i + (i + (i + (i + e1.i)))))) > 0]", "stack entries"),
    ("columns", "every e1=T[i > 1 and i > 1.0f and i > 1.0 and l > 1 and l > 1.0f and f > 1.0f and d > 1.0 and "
     "(i + 1 > 0 or f + 1 > 0 or b or e1.s is null)] -> e2=T", "too many columns"),
    ("captures", "every e1=T -> e2=T[i + e1.i > 0 or l > e1.l + 1 or f > e1.f + 1 or d > e1.d + 1 or not e1.b]",
     "too many columns / captures"),
]


@pytest.mark.parametrize("pattern,reason", [(p, r) for _, p, r in REFUSALS], ids=[n for n, _, _ in REFUSALS])
def test_refusals_name_their_reason(pattern, reason):
    L = lowering(q(pattern))
    assert not L.ok and reason in L.why, L.why


def test_a_later_slot_is_refused():
    """The planner resolves no later alias, so the reference is patched into the IR: e1's filter reads e2.l."""
    app = App(q("every e1=T[i + 1 > e1.l] -> e2=T"), engine_factory=lambda blob: None)
    reads_l = [ins for ins in app.ir.queries[0].states[0].filters[0] if ins.op == OP_ATTR and ins.imm == 1]
    assert len(reads_l) == 1
    reads_l[0].a = 1
    L = ch.HostChain(app.ir.serialize(app.string_ids)).lower(0)
    assert not L.ok and "later slot" in L.why, L.why


def test_at_the_limits_it_is_taken():
    """One step inside each limit: 48 instructions, 6 stack entries."""
    L = lowering(q("every e1=T -> e2=T[" + " or ".join(f"i + {k} > e1.i" for k in range(8)) + "]"))
    assert L.ok and L.partial_code[1] == 47, L.why
    L = lowering(q("every e1=T -> e2=T[i + (i + (i + (i + (i + e1.i)))) > 0]"))
    assert L.ok, L.why


def test_the_knob_declines_every_residual():
    for pattern in ("every e1=T -> e2=T[f > e1.f * 1.05]", "every e1=T[i > 3 or l > 3] -> e2=T",
                    "every e1=T -> e2=T[s == e1.s and f > e1.f]"):
        L = lowering(q(pattern), allow=False)
        assert not L.ok and "SDH_CHAIN_PRED" in L.why
        assert lowering(q(pattern)).ok
    L = lowering(q("every e1=T[i > 3] -> e2=T[f > e1.f and i < 7]"), allow=False)
    assert L.ok and L.ratchet


# ---- evaluation: the kernels' lane body over (event, captured events) against selector.evaluate ----

def _cases(app, n_slots, n=300, seed=11):
    """(vals, nulls)[case][slot][attribute] drawn from the adversarial events, and the log they index."""
    rows = ch.typed_events()
    vals, nulls = encode_rows(rows, app.stream_types("T"), app.dictionary)
    log = EventLog()
    log.append(0, list(range(len(rows))), vals, nulls)
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(rows), (n, n_slots))
    return log, pick, vals[pick], nulls[pick]


def _check(src, names, state, n_slots):
    app = App(src, engine_factory=lambda blob: None)
    log, pick, vals, nulls = _cases(app, n_slots)
    host = ch.HostChain(app.blob)
    n_true = 0
    for name in names:
        qi = app.ir.query_index(name)
        L = host.lower(qi)
        assert L.ok and L.n_code > 0, (name, L.why)
        got = host.state_pass(qi, state, vals, nulls)
        filters = app.ir.queries[qi].states[state].filters
        want = np.array([all(evaluate(f, [[int(x)] for x in row], log, None, app.dictionary, app.ir.strings) is True
                             for f in filters) for row in pick])
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, f"{name}: case {bad[0]} events {pick[bad[0]]} got {got[bad[0]]}"
        n_true += int(want.sum())
    return n_true


def _typed_app(filters, pattern):
    qs = [T]
    for k, f in enumerate(filters):
        qs.append(f"@info(name='p{k}') from {pattern.format(f=f)} select e1.i as x insert into O;")
    return " ".join(qs), [f"p{k}" for k in range(len(filters))]


def test_partial_residuals_evaluate_as_the_selector():
    src, names = _typed_app(ch.pred_filters(), "every e1=T -> e2=T[{f}]")
    assert _check(src, names, 1, 2) > 1000  # (the filters are not all false)


def test_tile_residuals_evaluate_as_the_selector():
    fs = [f"{a} {op} {b} > 1" for a, b, op in zip("ilfdil", "lfdiid", "+-*/%/")]
    fs += ["(i / l) is null", "(f % d) is null", "not (f > d)", "i > l or e1.d is null", "e1.s is null", "not b",
           "b or i > 7", "i + l > f * d", "i * 2 > l or e1.f is null", "s == 'a' or s == 'c'", "not (s == 'b')"]
    src, names = _typed_app(fs, "every e1=T[{f}] -> e2=T")
    assert _check(src, names, 0, 2) > 300


def test_a_middle_state_reads_two_earlier_slots():
    fs = ["i > e1.i + e2.i", "f > e1.f or d > e2.d", "(l / e2.l) is null and not (i == e1.i)",
          "s == e1.s and s == e2.s and i >= e2.i", "e1[1].i is null and i > e2.i - 1"]
    src, names = _typed_app(fs, "every e1=T -> e2=T -> e3=T[{f}]")
    assert _check(src, names, 2, 3) > 100


def test_standalone_program_under_the_sanitizers(tmp_path):
    """chain_host.cpp's own main, built with the address and undefined-behaviour sanitizers: the lane body
    over a table of hand-written programs. A stand-alone CPU program; nothing of it is loaded here."""
    exe = str(tmp_path / "chain_host_main")
    subprocess.check_call([os.environ.get("CXX", "g++")] + ch.CXXFLAGS +
                          ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DCHAIN_HOST_MAIN",
                           "-o", exe, ch.SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr
