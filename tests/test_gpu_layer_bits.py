"""The residual rows of every caller of the decoder layer's launch sequence, bit for bit what the tree computed BEFORE the three hand-written copies of the layer became
one body: a SHA-256 per case against tests/golden/layer_bits_parent.json (scripts/layer_bits_record.py wrote it on the device, from that earlier commit; every case ran
twice there and all reproduced).  tests/layer_bits_cases.py holds the model and the cases:

* one step at position 0 and a second at position 1, contiguous and paged decoders, without a pool / with a default pool (words [0, -1, 1, 2]) / with a gate_up=True pool;
* SpeculativeDecoder.step with T = 3 rows per slot and a gate_up=True pool built for rows;
* prefill at m = 5 and m = 130, contiguous and paged, with and without a pool; prefill_many with segments of 5 and 7 rows and a pool;
* DecoderBlock.prefill at m = 5 and m = 130.
"""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layer_bits_cases as lb  # noqa: E402

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layer_bits_parent.json")) as f:
    PARENT = json.load(f)


@pytest.fixture(scope="module")
def model():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return lb.Model(torch.device("cuda:0"))


def test_every_case_was_recorded():
    assert PARENT["unstable"] == {}
    assert sorted({k.rsplit("/", 1)[0] for k in PARENT["digests"]}) == sorted(lb.cases())


@pytest.mark.parametrize("name", sorted(lb.cases()))
def test_residual_rows_are_the_parents_bits(model, name):
    got = lb.run(model, name)
    want = {k: v for k, v in PARENT["digests"].items() if k.rsplit("/", 1)[0] == name}
    assert want, f"{name}: not in the recorded file"
    assert got == want, f"{name}: the residual rows differ from the parent commit's"
