"""Which path an interleaved push takes (siddhi_amd/csrc/mix_plan.h), on the host: a call is native when
every consumer of a named stream is a K_chain query or a query the K_gen kernel runs in the unpartitioned
set, and nothing engine-wide stands in the way; every other case names its reason."""
import pytest

from mix_plan_host import lib, why_split

NATIVE = [
    ["chain", "chain"],            # K_chain only
    ["gen", "gen", "gen"],         # K_gen unpartitioned only
    ["chain gen", "gen", "chain"],  # both, one stream read by both
    ["", "chain"],                 # a stream no query reads
    ["gen"],                       # one part
    [],                            # (no parts: nothing to decline)
    ["chain gen"] * 8,             # the most parts
]


@pytest.mark.parametrize("parts", NATIVE, ids=lambda p: "|".join(p) or "none")
def test_native_calls(parts):
    assert why_split(parts) is None


DECLINING = [("ratchet", "K_ratchet"), ("gate", "K_gate"), ("seq", "K_seq"), ("wave", "K_wave"), ("part", "K_part"),
             ("slab", "K_slab"), ("gen_part", "partitioned K_gen"), ("range", "stream range")]


@pytest.mark.parametrize("kind,word", DECLINING, ids=[k for k, _ in DECLINING])
def test_each_declining_consumer_names_its_reason(kind, word):
    # alone, beside eligible consumers of the same stream, and on a later part
    for parts in ([kind], ["chain gen " + kind], ["chain", "gen", kind]):
        why = why_split(parts)
        assert why is not None and word in why, (parts, why)
    # another stream's consumers do not matter: only named streams are asked about
    assert why_split(["chain", "gen"]) is None


def test_engine_wide_facts():
    ok = ["chain gen", "gen"]
    assert why_split(ok) is None
    assert "absent" in why_split(ok, timed=True)
    assert "communicator" in why_split(ok, comm=True)
    assert why_split(ok, knob=True) == "SDH_MIX_SPLIT"
    assert lib().mph_max_parts() == 8
    assert "8 parts" in why_split(["chain"] * 9)
    assert why_split(ok, total=2**31 - 2) is None
    assert "2^31" in why_split(ok, total=2**31 - 1)


def test_the_order_of_reasons():
    """The knob, the communicator and the part count come before anything about the plans (as the engine
    checked them before this function existed), and the first declining part gives the reason."""
    assert why_split(["ratchet"] * 9, knob=True, comm=True, timed=True) == "SDH_MIX_SPLIT"
    assert "communicator" in why_split(["ratchet"] * 9, comm=True, timed=True)
    assert "8 parts" in why_split(["ratchet"] * 9, timed=True)
    assert "absent" in why_split(["ratchet"], timed=True)
    assert "K_wave" in why_split(["chain", "wave", "ratchet"])
    assert "K_ratchet" in why_split(["wave ratchet"])
