"""Mirostat through the batched generator (generate.BatchedGenerator(mirostat_rows=True)) on the tiny model of tests/test_gpu_generate.py: the closed loop emits, id for
id and mu for mu, what Sampler.step gives when it is fed the same logits token by token; the captured graph equals the eager loop; a slot's tokens and mu do not depend
on its index or its neighbours; a slot changes hands to another mode with no recapture and starts at 2 * tau; the speculative generator at rows_per_seq = 4 emits the
batched generator's tokens id for id and ends on its mu bit for bit; and generators built without the flag refuse mirostat at admission."""
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
    rng = np.random.default_rng(67)
    ps = [SamplingParams(temp=0.9, top_k=40, repeat_penalty=1.1, mirostat=2, mirostat_tau=3.0, mirostat_eta=0.2), SamplingParams(temp=0.8, top_k=20, mirostat=1, mirostat_tau=4.0),
          SamplingParams(temp=1.0, top_k=40, top_p=0.9, tfs_z=0.9), SamplingParams(temp=0.7, top_k=30, mirostat=2)]
    return [(s, rng.integers(0, G.VOCAB, n).tolist(), ps[s], 90 + s, MAX_NEW) for s, n in ((0, 7), (1, 3), (2, 5), (3, 2))]


def _batched(m, graph, debug=False):
    from tinychatengine_amd.generate import BatchedGenerator
    return BatchedGenerator(m.decoders(), m.final_gamma, m.lm_head, m.table, max_new=MAX_NEW, graph=graph, debug=debug, mirostat_rows=True)


def _mus(gen) -> list:
    """the slots' mu words, as bits (of a generator, or of a Sampler)"""
    return getattr(gen, "sampler", gen).mrows.cpu().numpy()[:, 4].copy().view(np.uint32).tolist()


def test_the_loop_emits_what_the_sampler_gives_on_the_same_logits(dev):
    """The eager generator, stepped one token at a time with its logits copied out, against a stand-alone Sampler(mirostat_rows=True) fed those logits: tokens and
    the mu after every token, bit for bit."""
    from tinychatengine_amd.generate import Sampler
    m = G._model(dev, G.SMALL)
    adm = _admissions()
    gen = _batched(m, False)
    assert gen.sampler.mirostat_rows and gen.sampler.stages and gen.launches_per_token == 7 * len(m.blocks) + 5
    gen.admit(adm)
    fed, mus = [gen.logits.clone()], [_mus(gen)]
    for _ in range(MAX_NEW - 1):
        gen.run(1)
        fed.append(gen.logits.clone())
        mus.append(_mus(gen))
    assert gen.book.live() == []
    alone = Sampler(G.BATCH, G.VOCAB, MAX_NEW, dev, top_k_bound=gen.sampler.top_k_bound, mirostat_rows=True)
    for s, prompt, p, seed, mn in adm:
        alone.set_row(s, p, seed, mn, prompt)
    assert [alone.mirostat_row(s).mu for s, _, p, *_ in adm] == [float(np.float32(2.0) * np.float32(p.mirostat_tau)) for _, _, p, *_ in adm]
    pos = torch.tensor([len(prompt) - 1 for _, prompt, *_ in adm], dtype=torch.int32, device=dev)
    for t in range(MAX_NEW):
        alone.step(fed[t], pos, gen.pos_bound)
        torch.cuda.synchronize()
        assert _mus(alone) == mus[t], f"token {t}: mu"
    for s, *_ in adm:
        assert gen.tokens(s) == alone.out_log[s].cpu().numpy().tolist() and len(gen.tokens(s)) == MAX_NEW
    assert mus[0][2] == mus[-1][2] and mus[0][0] != mus[-1][0]  # the mode-0 slot's mu word never moves; a mirostat slot's does


def test_graph_equals_eager_and_a_slot_does_not_depend_on_its_index_or_neighbours(dev):
    m = G._model(dev, G.SMALL)
    adm = _admissions()
    out = []
    for graph in (True, False):
        gen = _batched(m, graph)
        for a in adm:  # each by a call of its own (a prompt's prefill launches are then the same whoever else is admitted), staggered
            gen.admit([a])
            gen.run(1)
        gen.run(MAX_NEW)
        assert gen.book.live() == []
        out.append(([gen.tokens(s) for s in range(G.BATCH)], _mus(gen)))
    assert all(len(t) == MAX_NEW for t in out[0][0]) and out[0] == out[1]
    # slot 0's request in slot 3 beside another neighbour on another mode: the same tokens and the same mu
    s0, s1 = adm[0], adm[1]
    gen = _batched(m, True)
    gen.admit([(1, s1[1][::-1], s0[2], 7, s1[4])])
    gen.run(2)
    gen.admit([(3, s0[1], s0[2], s0[3], s0[4])])
    gen.run(MAX_NEW)
    assert gen.tokens(3) == out[0][0][0] and _mus(gen)[3] == out[0][1][0], "a sequence's tokens or its mu depend on its slot or its neighbours"
    # the mode matters: the same request with mirostat off emits other tokens
    from tinychatengine_amd.generate import SamplingParams
    gen = _batched(m, True)
    gen.admit([(0, s0[1], SamplingParams(**{**s0[2].__dict__, "mirostat": 0}), s0[3], s0[4])])
    gen.run(MAX_NEW)
    assert gen.tokens(0) != out[0][0][0]


def test_a_slot_changes_hands_to_another_mode_without_recapture(dev):
    from tinychatengine_amd.generate import SamplingParams
    m = G._model(dev, G.SMALL)
    adm = _admissions()
    gen = _batched(m, True, debug=True)
    graph = gen._graph
    gen.admit([adm[0]])
    gen.run(MAX_NEW)
    assert gen.book.live() == [] and gen.sampler.mirostat_row(0).mode == 2
    gen.release(0)
    p1 = SamplingParams(temp=0.8, top_k=20, mirostat=1, mirostat_tau=4.0)
    gen.admit([(0, adm[1][1], p1, 91, MAX_NEW)])
    d = gen.sampler.mirostat_debug_row(0)
    assert (d.mode, d.mu_in) == (1, 8.0)  # the first token of the new request was drawn at mu = 2 * tau, not at what the last request left
    gen.run(MAX_NEW)
    assert gen._graph is graph and gen.sampler.mirostat_row(0).mode == 1
    # the same request in a fresh generator: the same tokens, the same mu
    fresh = _batched(m, True)
    fresh.admit([(0, adm[1][1], p1, 91, MAX_NEW)])
    fresh.run(MAX_NEW)
    assert gen.tokens(0) == fresh.tokens(0) and _mus(gen)[0] == _mus(fresh)[0]


T = 4


def test_speculative_rows_emit_the_batched_generators_tokens_and_mu(dev):
    """SpeculativeGenerator(mirostat_rows=True, rows_per_seq=4) with scripted drafts -- all right, wrong at two tokens, wrong at every token -- emits
    BatchedGenerator(mirostat_rows=True)'s tokens id for id and ends with its mu bit for bit.  The batched generator holds the sequences in slots 0, T, 2 T of BATCH * T
    slots, so that its linears run at the speculative generator's M (tests/test_gpu_sampler_stages_generate.py says why)."""
    from tinychatengine_amd.generate import BatchedGenerator
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchedDecoder
    from tinychatengine_amd.speculative import SpeculativeGenerator
    m = G._model(dev, G.SMALL)
    assert S._rows_do_not_depend_on_their_index(m), "a row's logits depend on its index in the M = 16 launch: plain decoding is no reference for rows t > 0"
    adm = [_admissions()[i] for i in (0, 1, 3)]  # modes 2, 1, 2
    adm = [(i, ids, p, sd, mn) for i, (_, ids, p, sd, mn) in enumerate(adm)]
    alloc = PageAllocator(G.NUM_PAGES, G.PAGE_KEYS, G.BATCH * T, G.MAX_KEYS // G.PAGE_KEYS, m.dev)
    plain = BatchedGenerator([PagedBatchedDecoder(b, alloc) for b in m.blocks], m.final_gamma, m.lm_head, m.table, max_new=MAX_NEW, mirostat_rows=True)
    plain.admit([(s * T, ids, p, sd, mn) for s, ids, p, sd, mn in adm])
    plain.run(MAX_NEW)
    assert plain.book.live() == []
    want = {s: plain.tokens(s * T) for s, *_ in adm}
    want_mu = {s: _mus(plain)[s * T] for s, *_ in adm}
    assert all(len(t) == MAX_NEW for t in want.values())
    spec = SpeculativeGenerator(S._spec_decoders(m, T, "fp16"), m.final_gamma, m.lm_head, m.table, max_new=MAX_NEW, script=True, mirostat_rows=True)
    assert spec.launches_per_token == 7 * len(m.blocks) + 4 + 4 and spec.sampler.mirostat_rows and spec.rows_per_seq == T
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
        assert _mus(spec)[s] == want_mu[s], f"slot {s}: mu"
    em = spec.emitted_per_step()
    for s, *_ in adm:
        assert [int(e) for e in em[:, s] if e] == S._expected_emitted(MAX_NEW, corrupted[s], T), f"slot {s}: emitted per step"
    assert [int(e) for e in em[:, 0] if e] == [4, 4, 3]  # the drafts were accepted: rows t > 0 were walked with mu carried and emitted
    assert spec.embed_violations() == 0


def test_generators_without_the_flag_refuse_mirostat_at_admission(dev):
    from tinychatengine_amd.generate import BatchedGenerator, SamplingParams
    from tinychatengine_amd.speculative import SpeculativeGenerator
    m = G._model(dev, G.SMALL)
    for kw in (dict(), dict(stages=True)):
        gen = BatchedGenerator(m.decoders(), m.final_gamma, m.lm_head, m.table, max_new=MAX_NEW, **kw)
        before = (gen.sampler.rows.clone(), gen.pos.clone())
        for mode in (1, 2):
            with pytest.raises(ValueError, match="not built"):
                gen.admit(0, [1, 2, 3], SamplingParams(mirostat=mode), 5, 4)
        assert torch.equal(gen.sampler.rows, before[0]) and torch.equal(gen.pos, before[1]) and gen.book.live() == []
    spec = SpeculativeGenerator(S._spec_decoders(m, 4, "fp16"), m.final_gamma, m.lm_head, m.table, max_new=MAX_NEW, stages=True)
    with pytest.raises(ValueError, match="not built"):
        spec.admit([(0, [1, 2, 3], SamplingParams(mirostat=2), 5, 4)])
    with pytest.raises(ValueError):
        _batched(m, False).admit(0, [1, 2, 3], SamplingParams(mirostat=3), 5, 4)
