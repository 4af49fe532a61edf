"""Tail-free and typical sampling through the generators (generate.BatchedGenerator(stages=True), speculative.SpeculativeGenerator(stages=True)) on the tiny model of
tests/test_gpu_generate.py: the captured graph emits the eager loop's ids with slots on different settings, the speculative generator at rows_per_seq = 4 emits the
batched generator's tokens id for id, and a generator built without stages=True refuses a non-default SamplingParams at admission with nothing launched."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_generate as G  # noqa: E402  (the tiny model and its shapes)
import test_gpu_speculative as S  # noqa: E402  (the speculative decoders over the same model)

dev = G.dev
MAX_NEW = 12


def _admissions():
    from tinychatengine_amd.generate import SamplingParams
    rng = np.random.default_rng(61)
    ps = [SamplingParams(temp=0.9, top_k=40, top_p=0.95, repeat_penalty=1.1, tfs_z=0.95, typical_p=0.9), SamplingParams(temp=0.8, top_k=20, top_p=0.9, typical_p=0.5),
          SamplingParams(temp=1.0, top_k=40, top_p=1.0, tfs_z=0.5), SamplingParams(temp=0.7, top_k=10, top_p=0.9)]
    return [(s, rng.integers(0, G.VOCAB, n).tolist(), ps[s], 70 + s, MAX_NEW) for s, n in ((0, 7), (1, 3), (2, 5), (3, 2))]


def _batched(m, graph):
    from tinychatengine_amd.generate import BatchedGenerator
    return BatchedGenerator(m.decoders(), m.final_gamma, m.lm_head, m.table, max_new=MAX_NEW, graph=graph, stages=True)


def test_graph_run_equals_the_eager_loop_with_slots_on_different_settings(dev):
    m = G._model(dev, G.SMALL)
    adm = _admissions()
    out = []
    for graph in (True, False):
        gen = _batched(m, graph)
        assert gen.launches_per_token == 7 * len(m.blocks) + 5 and gen.sampler.stages
        gen.admit(adm[:2])
        gen.run(3)
        gen.admit(adm[2:])
        gen.run(MAX_NEW)
        assert gen.book.live() == []
        out.append([gen.tokens(s) for s in range(G.BATCH)])
        assert gen.sampler.srows.cpu().numpy().tolist() == [[np.float32(p.tfs_z), np.float32(p.typical_p)] for _, _, p, _, _ in adm]
    assert all(len(t) == MAX_NEW for t in out[0]) and out[0] == out[1]
    # the settings matter: slot 2 at tfs_z 0.5 does not emit what the same admission emits with the stages off
    from tinychatengine_amd.generate import SamplingParams
    s2 = adm[2]
    gen = _batched(m, True)
    gen.admit([(2, s2[1], SamplingParams(**{**s2[2].__dict__, "tfs_z": 1.0}), s2[3], s2[4])])
    gen.run(MAX_NEW)
    assert gen.tokens(2) != out[0][2]


T = 4


def _batched_at_the_speculative_m(m):
    """BatchedGenerator(stages=True) over the same layers with BATCH * T slots, so that its linears run at the speculative generator's M.  Why: "id for id" needs
    both generators to compute a row with the same arithmetic, and the dispatcher picks the linears' kernel by M -- measured on an MI355X with this model, lm_head, o
    and down rows differ in their last fp16 bit between M = 4 and M = 16 (largest differences 9.8e-4, 3.1e-5, 4.9e-4), and with a 4-slot BatchedGenerator the
    tokens parted after 4 to 10 tokens in every slot.  tests/test_gpu_window_rows.py gives its plain generator B T slots for the same reason."""
    from tinychatengine_amd.generate import BatchedGenerator
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchedDecoder
    alloc = PageAllocator(G.NUM_PAGES, G.PAGE_KEYS, G.BATCH * T, G.MAX_KEYS // G.PAGE_KEYS, m.dev)
    return BatchedGenerator([PagedBatchedDecoder(b, alloc) for b in m.blocks], m.final_gamma, m.lm_head, m.table, max_new=MAX_NEW, stages=True)


def test_speculative_rows_emit_the_batched_generators_tokens(dev):
    """SpeculativeGenerator(stages=True, rows_per_seq=4) emits BatchedGenerator(stages=True)'s tokens id for id, with every slot on its own (tfs_z, typical_p) and
    scripted drafts: all right (4, 4, 3 tokens per step), wrong at two tokens, wrong at every token.  The batched generator holds the sequences in slots 0, T, 2 T of
    BATCH * T slots (see _batched_at_the_speculative_m); a row's logits must not depend on its index in that launch: asserted, not assumed."""
    from tinychatengine_amd.speculative import SpeculativeGenerator
    m = G._model(dev, G.SMALL)
    assert S._rows_do_not_depend_on_their_index(m), "a row's logits depend on its index in the M = 16 launch: plain decoding is no reference for rows t > 0"
    adm = _admissions()[:3]
    plain = _batched_at_the_speculative_m(m)
    assert plain.batch == G.BATCH * T and plain.sampler.stages
    plain.admit([(s * T, ids, p, sd, mn) for s, ids, p, sd, mn in adm])
    plain.run(MAX_NEW)
    assert plain.book.live() == []
    want = {s: plain.tokens(s * T) for s, *_ in adm}
    assert all(len(t) == MAX_NEW for t in want.values())
    spec = SpeculativeGenerator(S._spec_decoders(m, T, "fp16"), m.final_gamma, m.lm_head, m.table, max_new=MAX_NEW, script=True, stages=True)
    assert spec.launches_per_token == 7 * len(m.blocks) + 4 + 3 and spec.sampler.stages and spec.rows_per_seq == T
    corrupted = {0: set(), 1: {2, 5}, 2: set(range(1, MAX_NEW))}
    for s, prompt, *_ in adm:
        spec.set_script(s, [-1] * len(prompt) + [(t + 1) % G.VOCAB if i in corrupted[s] else t for i, t in enumerate(want[s])])
    spec.admit(adm)
    for _ in range(MAX_NEW):
        if spec.book.live():
            spec.run(1)
    assert spec.book.live() == []
    for s, *_ in adm:
        assert spec.tokens(s) == want[s], f"slot {s}: the speculative generator's tokens differ from the batched generator's"
    em = spec.emitted_per_step()
    for s, *_ in adm:
        assert [int(e) for e in em[:, s] if e] == S._expected_emitted(MAX_NEW, corrupted[s], T), f"slot {s}: emitted per step"
    assert [int(e) for e in em[:, 0] if e] == [4, 4, 3]  # the drafts were accepted: rows t > 0 were sampled under the stages and emitted
    assert spec.embed_violations() == 0


def test_a_generator_without_stages_refuses_at_admission_with_nothing_launched(dev):
    from tinychatengine_amd.generate import BatchedGenerator, SamplingParams
    m = G._model(dev, G.SMALL)
    gen = BatchedGenerator(m.decoders(), m.final_gamma, m.lm_head, m.table, max_new=MAX_NEW)
    before = (gen.sampler.rows.clone(), gen.pos.clone(), [list(p) for p in gen.allocator.pages], list(gen.allocator.free))
    for p in (SamplingParams(tfs_z=0.95), SamplingParams(typical_p=0.9)):
        with pytest.raises(ValueError, match="not built"):
            gen.admit(0, [1, 2, 3], p, 5, 4)
    assert torch.equal(gen.sampler.rows, before[0]) and torch.equal(gen.pos, before[1]) and gen.book.live() == []
    assert ([list(p) for p in gen.allocator.pages], list(gen.allocator.free)) == before[2:]
    with pytest.raises(ValueError):
        _batched(m, False).admit(0, [1, 2, 3], SamplingParams(mirostat=1), 5, 4)
