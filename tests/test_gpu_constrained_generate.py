"""Constrained decoding through the generators (generate.BatchedGenerator / speculative.SpeculativeGenerator with constraints=True): the automaton advances inside
the captured token step, a slot changes automaton without recapture, log-probabilities stay those of the raw logits, and the speculative verifier is lossless --
drafts accepted, a forbidden draft, a draft whose transition is DONE.  The small model shape of tests/test_gpu_generate.py (512 hidden, 4 heads, 1 KV head, 2 layers,
vocabulary 4096), synthetic weights."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HD, VOCAB = 128, 4096
HIDDEN, HEADS, KV_HEADS, FFN, LAYERS = 512, 4, 1, 1408, 2
MAX_KEYS, PAGE_KEYS, BATCH, NUM_PAGES = 64, 16, 4, 12


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


class _Model:
    def __init__(self, dev, seed=552):
        from tinychatengine_amd.decoder_block import DecoderBlock
        from tinychatengine_amd.linear import Linear_half_int4
        rng = np.random.default_rng(seed)
        ang = rng.uniform(0, 2 * np.pi, (MAX_KEYS, HD // 2))
        cos = torch.from_numpy(np.concatenate([np.cos(ang), np.cos(ang)], axis=1).astype(np.float16)).to(dev)
        sin = torch.from_numpy(np.concatenate([np.sin(ang), np.sin(ang)], axis=1).astype(np.float16)).to(dev)
        self.dev = dev
        self.blocks = [DecoderBlock(HIDDEN, HEADS, FFN, MAX_KEYS, dev, cos, sin, seed=seed + i, kv_heads=KV_HEADS) for i in range(LAYERS)]
        g = torch.Generator(device=dev).manual_seed(seed + 100)
        self.final_gamma = (1.0 + 0.1 * torch.empty(HIDDEN, device=dev).normal_(0, 1, generator=g)).float()
        self.lm_head = Linear_half_int4.from_float(torch.empty(VOCAB, HIDDEN, device=dev).normal_(0.0, HIDDEN ** -0.5, generator=g)).prepack()
        self.table = torch.empty(VOCAB, HIDDEN, device=dev).normal_(0.0, 1.0, generator=g).half()

    def allocator(self):
        from tinychatengine_amd.paged_kv import PageAllocator
        return PageAllocator(NUM_PAGES, PAGE_KEYS, BATCH, MAX_KEYS // PAGE_KEYS, self.dev)

    def generator(self, graph=True, max_new=12, **kw):
        from tinychatengine_amd.generate import BatchedGenerator
        from tinychatengine_amd.paged_kv import PagedBatchedDecoder
        alloc = self.allocator()
        return BatchedGenerator([PagedBatchedDecoder(b, alloc) for b in self.blocks], self.final_gamma, self.lm_head, self.table, max_new=max_new, graph=graph,
                                constraints=True, **kw)

    def spec_generator(self, T, max_new=24, **kw):
        from tinychatengine_amd.speculative import SpeculativeDecoder, SpeculativeGenerator
        alloc = self.allocator()
        return SpeculativeGenerator([SpeculativeDecoder(b, alloc, T) for b in self.blocks], self.final_gamma, self.lm_head, self.table, max_new=max_new, script=True,
                                    constraints=True, **kw)


@pytest.fixture(scope="module")
def model(dev):
    return _Model(dev)


SEQS = [[50, 51, 52], [50, 51, 53, 54], [50, 60], [70, 71, 72, 73, 74]]


def _choice_run(model, graph, slot_of):
    """8 seeds, sampled, each constrained to one of SEQS; seed i sits in slot slot_of[i % 4] of round i // 4.  Returns the outputs by seed."""
    from tinychatengine_amd.constrain import TokenAutomaton
    from tinychatengine_amd.generate import SamplingParams
    gen = model.generator(graph=graph)
    a = gen.sampler.table.register(TokenAutomaton.from_sequences(VOCAB, SEQS))
    sampled = SamplingParams(temp=1.0, top_k=40, top_p=0.95, repeat_penalty=1.1)
    rng = np.random.default_rng(4)
    prompts = [rng.integers(0, VOCAB, 3 + i % 4).tolist() for i in range(8)]
    out = {}
    for rnd in range(2):
        seeds = list(range(4 * rnd, 4 * rnd + 4))
        adm = [(slot_of[i % 4], prompts[i], sampled, 1000 + i, 12) for i in seeds]
        gen.admit(adm, constraints={s: (a, None) for s, *_ in adm})
        retired = gen.run(5)
        assert gen.book.live() == [] and sorted(retired) == [0, 1, 2, 3], "every slot retires behind its sequence (none is longer than 5 tokens)"
        for i in seeds:
            out[i] = gen.tokens(slot_of[i % 4])
            gen.release(slot_of[i % 4])
    assert gen.violations() == 0 and gen.embed_violations() == 0
    return out


def test_choice_among_sequences_graph_eager_and_permuted_slots(model):
    graph = _choice_run(model, True, [0, 1, 2, 3])
    for i, toks in graph.items():
        assert toks in SEQS, f"seed {i}: {toks} is none of the sequences"
    assert len({tuple(t) for t in graph.values()}) >= 2, "eight sampled seeds all took one sequence: the test shows nothing about the draw"
    assert _choice_run(model, False, [0, 1, 2, 3]) == graph, "the graph run and the eager run differ"
    assert _choice_run(model, True, [2, 0, 3, 1]) == graph, "the run with the slots permuted differs"


def test_a_slot_changes_automaton_without_recapture(model):
    from tinychatengine_amd.constrain import TokenAutomaton
    from tinychatengine_amd.generate import SamplingParams
    gen = model.generator(max_new=8)
    g0 = gen._graph
    first = gen.sampler.table.register(TokenAutomaton.from_sequences(VOCAB, [[5, 6, 7]]))
    assert gen.admit(1, [9, 8, 7, 6], SamplingParams(), 3, 8, automaton=first) == []
    gen.run(3)
    assert gen.tokens(1) == [5, 6, 7] and gen.book.live() == []
    gen.release(1)
    only = [4000, 17, 2222]
    second = gen.sampler.table.register(TokenAutomaton.any_of(VOCAB, only))
    gen.admit(1, [1, 2, 3], SamplingParams(temp=1.5, top_k=40, top_p=1.0, repeat_penalty=1.0), 4, 8, automaton=second, logit_bias={17: 1.0})
    with pytest.raises(ValueError):
        gen.sampler.table.unregister(second)
    gen.sampler.table.unregister(first)  # (no row names it any more)
    gen.run(7)
    toks = gen.tokens(1)
    assert len(toks) == 8 and set(toks) <= set(only) and gen._graph is g0 and gen.violations() == 0
    gen.release(1)
    gen.admit(1, [1, 2, 3], SamplingParams(temp=0.0), 4, 8)  # and back to no constraint: the plain generator's tokens
    gen.run(7)
    from tinychatengine_amd.generate import BatchedGenerator
    from tinychatengine_amd.paged_kv import PagedBatchedDecoder
    alloc = model.allocator()
    plain = BatchedGenerator([PagedBatchedDecoder(b, alloc) for b in model.blocks], model.final_gamma, model.lm_head, model.table, max_new=8)
    plain.admit(1, [1, 2, 3], SamplingParams(temp=0.0), 4, 8)
    plain.run(7)
    assert gen.tokens(1) == plain.tokens(1) and gen.violations() == 0


def test_logprobs_are_those_of_the_raw_logits(model):
    """Eager steps, the logits kept after each: logprobs(slot) equals logprob_reference on them -- the mask and the bias do not enter.  Tolerance: the header's bound for
    the device's LSE, 2^-16 for rows with every |x| <= 64 (asserted), plus half an ulp of the fp32 result (|logprob| < 32: 2^-20)."""
    from tinychatengine_amd.constrain import TokenAutomaton
    from tinychatengine_amd.generate import SamplingParams, logprob_reference
    gen = model.generator(graph=False, max_new=6, logprobs=True)
    a = gen.sampler.table.register(TokenAutomaton.any_of(VOCAB, [11, 12, 13, 3000]))
    gen.admit(2, [5, 4, 3], SamplingParams(temp=1.0, top_k=4, top_p=1.0), 9, 6, automaton=a, logit_bias={12: 2.0})
    kept = [gen._adm_logits[2, :VOCAB].cpu().numpy().copy()]
    for _ in range(5):
        gen.run(1)
        kept.append(gen.logits[2, :VOCAB].cpu().numpy().copy())
    toks, lps = gen.tokens(2), gen.logprobs(2)
    assert len(toks) == 6 and set(toks) <= {11, 12, 13, 3000} and lps.shape == (6,)
    for i, (t, lp) in enumerate(zip(toks, lps)):
        assert np.abs(kept[i].astype(np.float32)).max() <= 64
        want = logprob_reference(kept[i], t)
        print(f"token {i} = {t}: logprob {lp!r}, float64 reference {want!r}")
        assert abs(float(lp) - want) <= 2.0 ** -16 + 2.0 ** -20 and want < -2.0, "(an allowed token of a random model is an unlikely one: the value is not renormalised)"
    assert gen.violations() == 0


A = [100, 101, 102, 103, 104, 105, 106, 107]
X_SEQS = [A, [100, 101, 102, 900], [100, 200, 201], [300, 301]]
LINE = [7, 8, 9, 10, 11, 12]


@pytest.mark.parametrize("logprobs", [False, True])
def test_speculative_verifier_is_lossless_under_constraints(model, logprobs):
    """T = 4, scripted drafts.  Slots 0 .. 2 run automaton X (a trie over X_SEQS) and are steered down sequence A by a logit bias of +30 on A's tokens, greedy; slot 3
    runs a single-path automaton, sampled.  Scripts: slot 0 the true tokens (every draft accepted; A's last token, DONE, is drawn by row 2 and the row behind it is
    unreachable); slot 1 a FORBIDDEN token as the draft of token 2 (row 2 of the first step); slot 2 token 900 as the draft of token 3 -- allowed there, its transition
    DONE, but not what is drawn.  The emitted tokens and the state words equal the constrained BatchedGenerator's, one token per replay.  logprobs=True runs the
    same through the verifier's log-probability forms: the values are the raw logits' (far below the 0 a renormalised single candidate would get) and equal the plain
    run's within 2^-5 = four fp16 steps of a logit below 8 -- the M = 16 and M = 4 lm_head launches need not round alike, which is why this is no bit comparison."""
    from tinychatengine_amd.constrain import TokenAutomaton
    from tinychatengine_amd.generate import SamplingParams
    T = 4
    greedy, sampled = SamplingParams(temp=0.0, repeat_penalty=1.0), SamplingParams(temp=0.9, top_k=20, top_p=0.9, repeat_penalty=1.2)
    rng = np.random.default_rng(31)
    prompts = [rng.integers(0, VOCAB, n).tolist() for n in (5, 3, 6, 4)]
    steer = {t: 30.0 for t in A}

    def admit(gen):
        x = gen.sampler.table.register(TokenAutomaton.from_sequences(VOCAB, X_SEQS))
        line = gen.sampler.table.register(TokenAutomaton.from_sequences(VOCAB, [LINE]))
        adm = [(s, prompts[s], greedy if s < 3 else sampled, 40 + s, 24) for s in range(BATCH)]
        assert gen.admit(adm, constraints={0: (x, steer), 1: (x, steer), 2: (x, steer), 3: (line, None)}) == []

    plain = model.generator(max_new=24, logprobs=logprobs)
    admit(plain)
    plain.run(8)
    want = {s: plain.tokens(s) for s in range(BATCH)}
    assert [want[s] for s in range(BATCH)] == [A, A, A, LINE] and plain.book.live() == [] and plain.violations() == 0
    states = [plain.sampler.constraint_row(s).state for s in range(BATCH)]

    spec = model.spec_generator(T, logprobs=logprobs)
    script = {s: [-1] * len(prompts[s]) + want[s] + [100, 100, 100, 100] for s in range(BATCH)}  # (behind a sequence's end: drafts no reachable row is fed)
    script[1][len(prompts[1]) + 2] = 4000
    script[2][len(prompts[2]) + 3] = 900
    for s in range(BATCH):
        spec.set_script(s, script[s])
    admit(spec)
    retired = []
    for _ in range(3):
        retired += spec.run(1)
    em = spec.emitted_per_step()
    got = {s: [int(e) for e in em[:, s] if e] for s in range(BATCH)}
    print("emitted per step:", got)
    for s in range(BATCH):
        assert spec.tokens(s) == want[s], f"slot {s}: {spec.tokens(s)}, the constrained BatchedGenerator emits {want[s]}"
        assert spec.sampler.constraint_row(s).state == states[s], f"slot {s}: state word"
        if logprobs:
            a, b = spec.logprobs(s), plain.logprobs(s)
            print(f"slot {s}: logprobs {a.tolist()} | plain {b.tolist()}")
            assert a.shape == b.shape == (len(want[s]),) and np.isfinite(a).all() and (a < -1.0).all() and np.abs(a - b).max() <= 2.0 ** -5
    assert got == {0: [4, 3], 1: [2, 4, 1], 2: [3, 4], 3: [4, 1]}
    assert sorted(retired) == [0, 1, 2, 3] and spec.book.live() == [] and spec.violations() == 0 and spec.embed_violations() == 0


def test_speculative_verifier_retires_an_invalid_row(model):
    """Rule 6 through the verifier: a state word written from outside is out of range -- the step emits nothing for the slot, retires it and counts one violation; the
    slot beside it is not disturbed."""
    from tinychatengine_amd.constrain import TokenAutomaton
    from tinychatengine_amd.generate import SamplingParams
    spec = model.spec_generator(4)
    line = spec.sampler.table.register(TokenAutomaton.from_sequences(VOCAB, [LINE]))
    greedy = SamplingParams(temp=0.0, repeat_penalty=1.0)
    assert spec.admit([(0, [9, 9, 9], greedy, 1, 24), (2, [4, 5], greedy, 2, 24)], constraints={0: (line, None), 2: (line, None)}) == []
    assert spec.tokens(0) == LINE[:1] and spec.tokens(2) == LINE[:1]
    spec.sampler.crows[0, 1] = 999
    assert spec.run(1) == [0]
    assert spec.tokens(0) == LINE[:1] and spec.emitted_per_step()[-1].tolist() == [0, 0, 1, 0] and spec.tokens(2) == LINE[:2]
    assert spec.violations() == 1 and spec.sampler.constraint_row(0).state == 999
    assert spec.run(4) == [2] and spec.tokens(2) == LINE and spec.violations() == 1  # (no script was set: no drafts, one token per step)
