"""The launch sequence of a decoder layer, on a host without a device: every caller of the layer body (BatchedDecoder.step, BatchedDecoder.prefill /
PagedBatchedDecoder.prefill_many through _prefill_rows, DecoderBlock.prefill, and the generators' admissions on top of them) issues, call for call and argument role
for argument role, what tests/golden/layer_trace_parent.json holds -- the trace scripts/layer_trace_record.py took of the tree BEFORE the three hand-written copies of
the layer became one body.  tests/layer_trace_cases.py is the harness (stub block, stub attention, patched launch wrappers, LoraPool(device="cpu")) and says how
tensors get their role names."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layer_trace_cases as lt  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layer_trace_parent.json")
with open(GOLDEN) as f:
    PARENT = json.load(f)
CASES = lt.cases()


def _json(events):
    return json.loads(json.dumps(events))  # (tuples -> lists, as the file holds them)


def _launches(events):
    """the device launches among the events: everything but the markers, the bookkeeping and a pair launch that was refused before it launched"""
    return [e for e in events if e["call"] not in ("--", "buffers", "raised", "allocator.reserve_many", "embed_rows") and e.get("rc", 0) == 0]


def test_the_recorded_cases_are_the_harness_cases():
    assert sorted(PARENT) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_layer_issues_the_parents_calls(name):
    got = _json(lt.run(CASES[name]))
    want = PARENT[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: event {i} differs"
    assert len(got) == len(want), f"{name}: {len(got)} events, the parent issued {len(want)}"


def test_launch_counts_are_the_documented_ones():
    from tinychatengine_amd.batch_decode import BatchedDecoder
    from tinychatengine_amd.decoder_block import DecoderBlock
    assert BatchedDecoder.LAUNCHES == 7 and DecoderBlock.LAUNCHES == 5 and DecoderBlock.PREFILL_LAUNCHES == 8
    for name, per_step in {"step/none": 7, "step/default": 13, "step/gate_up": 15}.items():
        events = _json(lt.run(CASES[name]))
        assert len(_launches(events)) == 2 * per_step and events[-1]["LAUNCHES"] == per_step
    # DecoderBlock.prefill counts the rotation + append and the attention as two launches; the stub attention is one event
    blk = _json(lt.run(CASES["block_prefill/m3,m130,m3"]))
    cuts = [i for i, e in enumerate(blk) if e["call"] == "--"] + [len(blk)]
    assert [len(_launches(blk[a:b])) + 1 for a, b in zip(cuts, cuts[1:])] == [10, 8, 10]


def test_refused_pairs_fall_back_for_good_and_a_hip_error_raises():
    events = _json(lt.run(CASES["step/none/pairs_refused"]))
    cuts = [i for i, e in enumerate(events) if e["call"] == "--"] + [len(events) - 1]
    first, second = (events[a + 1:b] for a, b in zip(cuts, cuts[1:]))
    assert len(_launches(first)) == 9 and len(_launches(second)) == 9
    assert sum(1 for e in first if "SILU_MUL_PAIRS" in e.get("flags", ())) == 1, "the first step asks for the pairs once"
    assert not any("SILU_MUL_PAIRS" in e.get("flags", ()) for e in second), "the second step must not ask for the pairs again"
    three = lambda evs: [(e["call"], e.get("linear"), e.get("out") or e.get("u")) for e in evs if e.get("linear") in ("gate", "up") or e["call"] == "tce_silu_mul_half"]
    assert three(first) == three(second) == [("w4a16_forward", "gate", "act"), ("w4a16_forward", "up", "up"), ("tce_silu_mul_half", None, "up")]
    assert events[-1]["_up"] == "up", "_up is the tensor the three launches used, in both steps"
    hip = _json(lt.run(CASES["step/none/pairs_hip_error"]))
    assert hip[-2] == {"call": "raised", "type": "TceError", "code": -4} and hip[-1]["_up"] is None
    assert hip[-3]["flags"] == ["SILU_MUL_PAIRS"], "nothing may be launched behind the failed pair launch"


def test_row_words_are_each_slots_word_per_row():
    for name, want in {"prefill_many/paged/default": [12, 12, 10, 10, 10], "prefill_many/paged/default/rows_per_seq3": [16, 16, 10, 10, 10]}.items():
        words = [e["row_adapter"] for e in _json(lt.run(CASES[name])) if "row_adapter" in e]
        assert len(words) == 6 and all(w == {"row_words": want} for w in words), name


def test_contiguous_prefill_many_is_one_prefill_per_admission():
    got = _json(lt.run(lambda tr, mp: lt._two_admissions(tr, via_many=True)))
    assert got == PARENT["two_admissions/contiguous"]
