"""The closed decode loop (tinychatengine_amd/generate.py: BatchedGenerator): embed -> layers -> final norm -> lm_head -> tce_sample_f16 captured in ONE graph,
one replay = one token for all slots, no host round trip.

Greedy: every slot's token ids are IDENTICAL to a host-driven loop over the same kind of decoders (HostDrivenLoop: eager steps, logits copied to the host, the
lowest-id argmax in numpy, the row looked up on the host and copied back) -- the logits come from the same kernels, so there is no tolerance.  Sampled: the graph run
equals the same generator run eagerly, and equals itself with the slots permuted and other prompts beside it.  Synthetic weights, as everywhere in this tree."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HD = 128
VOCAB = 4096
MAX_KEYS, PAGE_KEYS, BATCH, NUM_PAGES = 64, 16, 4, 12  # fewer pages than 4 slots x 4: the runs only fit because pages follow the tokens and come back


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


class _Model:
    def __init__(self, dev, hidden, heads, kv_heads, ffn, layers, seed):
        from tinychatengine_amd.decoder_block import DecoderBlock
        from tinychatengine_amd.linear import Linear_half_int4
        rng = np.random.default_rng(seed)
        ang = rng.uniform(0, 2 * np.pi, (MAX_KEYS, HD // 2))
        cos = torch.from_numpy(np.concatenate([np.cos(ang), np.cos(ang)], axis=1).astype(np.float16)).to(dev)
        sin = torch.from_numpy(np.concatenate([np.sin(ang), np.sin(ang)], axis=1).astype(np.float16)).to(dev)
        self.dev, self.hidden = dev, hidden
        self.blocks = [DecoderBlock(hidden, heads, ffn, MAX_KEYS, dev, cos, sin, seed=seed + i, kv_heads=kv_heads) for i in range(layers)]
        g = torch.Generator(device=dev).manual_seed(seed + 100)
        self.final_gamma = (1.0 + 0.1 * torch.empty(hidden, device=dev).normal_(0, 1, generator=g)).float()
        self.lm_head = Linear_half_int4.from_float(torch.empty(VOCAB, hidden, device=dev).normal_(0.0, hidden ** -0.5, generator=g)).prepack()
        self.table = torch.empty(VOCAB, hidden, device=dev).normal_(0.0, 1.0, generator=g).half()

    def decoders(self, paged=True, free_order=None):
        from tinychatengine_amd.batch_decode import BatchedDecoder
        from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchedDecoder
        if not paged:
            return [BatchedDecoder(b, BATCH) for b in self.blocks]
        alloc = PageAllocator(NUM_PAGES, PAGE_KEYS, BATCH, MAX_KEYS // PAGE_KEYS, self.dev, free_order=free_order)
        return [PagedBatchedDecoder(b, alloc) for b in self.blocks]

    def generator(self, paged=True, graph=True, stop_ids=(), free_order=None, max_new=40):
        from tinychatengine_amd.generate import BatchedGenerator
        return BatchedGenerator(self.decoders(paged, free_order), self.final_gamma, self.lm_head, self.table, max_new=max_new, stop_ids=stop_ids, graph=graph)

    def host_loop(self, paged=True, stop_ids=(), free_order=None):
        from tinychatengine_amd.generate import HostDrivenLoop
        return HostDrivenLoop(self.decoders(paged, free_order), self.final_gamma, self.lm_head, self.table, stop_ids=stop_ids)


_models = {}


def _model(dev, shape):
    if shape not in _models:
        _models.clear()  # one model in memory at a time
        _models[shape] = _Model(dev, *shape, seed=40 + shape[0])
    return _models[shape]


SMALL, LLAMA3_8B_LAYER = (512, 4, 1, 1408, 2), (4096, 32, 8, 14336, 1)


def _keys(dec, slot, n):
    k, v = dec.attention.read_back(slot, n)
    return k.contiguous().view(torch.int16), v.contiguous().view(torch.int16)


@pytest.mark.parametrize("shape", [SMALL, LLAMA3_8B_LAYER])
def test_greedy_graph_run_equals_the_host_driven_loop(dev, shape):
    """Four slots on 16-key pages (12 pages), staggered admissions, run() in chunks under the captured graph, slot 0 retiring on a stop id and a new prompt admitted
    into it that reuses released pages, slot 3 retiring on its budget."""
    from tinychatengine_amd.generate import SamplingParams
    m = _model(dev, shape)
    rng = np.random.default_rng(shape[0])
    greedy = SamplingParams(temp=0.0, repeat_penalty=1.0)  # (the host-driven loop takes a plain argmax: no penalties)
    # discovery: the schedule below without a stop id, on the host-driven loop (a row's tokens do not depend on its neighbours).  The stop id is a token slot 0's
    # sequence produces for the first time at index 6 .. 19 -- slot 0 holds five tokens (indices 0 .. 4) when the last slot is admitted, so it retires in the chunked
    # runs after that -- and that no other sequence of the schedule produces at all.  Prompts are drawn until such a token exists.
    stop = None
    for _ in range(8):
        prompts = {s: rng.integers(0, VOCAB, n).tolist() for s, n in {0: 20, 1: 3, 2: 4, 3: 2, "new": 6}.items()}
        probe = m.host_loop()
        probe.admit([(0, prompts[0], 40), (3, prompts[3], 12)])  # (admitted as below: the prompts' rows then go through the same launches)
        probe.step(), probe.step()
        probe.admit(1, prompts[1], 40)
        probe.step(), probe.step()
        probe.admit(2, prompts[2], 40)
        for _ in range(24):
            probe.step()
        seq0, others = list(probe.out[0]), set(probe.out[1]) | set(probe.out[2]) | set(probe.out[3])
        probe.release(0)
        probe.admit(0, prompts["new"], 40)
        for _ in range(12):
            probe.step()
        others |= set(probe.out[0])
        del probe
        found = [i for i in range(6, 20) if seq0[i] not in seq0[:i] and seq0[i] not in others]
        if found:
            stop_at, stop = found[0], seq0[found[0]]
            break
    assert stop is not None, "no prompt set gave slot 0 a token of its own at index 6 .. 19"

    order = np.random.default_rng(13).permutation(NUM_PAGES).tolist()
    gen = m.generator(stop_ids=[stop], free_order=order)
    host = m.host_loop(stop_ids=[stop], free_order=order)
    assert gen.launches_per_token == 7 * len(m.blocks) + 5
    alloc = gen.allocator

    def both_run(n):
        retired = gen.run(n)
        for _ in range(n):
            host.step()
        alloc.check_invariants()
        for s in range(BATCH):
            assert gen.tokens(s) == host.out[s], f"slot {s}: the graph run and the host-driven loop disagree"
        return retired

    assert gen.admit([(0, prompts[0], greedy, 0, 40), (3, prompts[3], greedy, 0, 12)]) == []  # two admissions, one prefill_many
    host.admit([(0, prompts[0], 40), (3, prompts[3], 12)])
    assert both_run(2) == []
    gen.admit(1, prompts[1], greedy, 0, 40)
    host.admit(1, prompts[1], 40)
    assert both_run(2) == []
    gen.admit(2, prompts[2], greedy, 0, 40)
    host.admit(2, prompts[2], 40)
    retired = []
    while 0 not in retired:
        retired += both_run(3)
        assert len(gen.tokens(1)) < 30, "slot 0 never met its stop id"
    assert gen.tokens(0)[-1] == stop and len(gen.tokens(0)) == stop_at + 1 and gen.tokens(0) == seq0[:stop_at + 1]
    released = gen.release(0)
    host.release(0)
    assert 2 <= len(released) <= 3  # 20 prompt keys + the tokens before the stop id (+ what the last run(3) reserved ahead)
    gen.admit(0, prompts["new"], greedy, 0, 40)
    host.admit(0, prompts["new"], 40)
    assert set(alloc.pages[0]) & set(released), "the new sequence reuses none of the released pages"
    for _ in range(4):
        retired += both_run(3)
    assert 3 in retired and len(gen.tokens(3)) == 12  # its budget
    assert gen.embed_violations() == 0
    alloc.check_invariants()
    host.allocator.check_invariants()
    # every live slot's keys, gathered from the pages, equal the host-driven twin's
    assert gen.book.live() == [s for s in range(BATCH) if host.pos_host[s] >= 0] and len(gen.book.live()) >= 3
    for s in gen.book.live():
        n = gen.book.pos[s]
        assert n == host.pos_host[s]
        for dg, dh in zip(gen.decoders, host.decoders):
            kg, vg = _keys(dg, s, n)
            kh, vh = _keys(dh, s, n)
            assert torch.equal(kg, kh) and torch.equal(vg, vh), f"slot {s}: cached keys differ"


def test_greedy_on_contiguous_caches(dev):
    """The same front over BatchedDecoder (no pages): graph run = host-driven loop."""
    from tinychatengine_amd.generate import SamplingParams
    m = _model(dev, SMALL)
    rng = np.random.default_rng(5)
    gen, host = m.generator(paged=False), m.host_loop(paged=False)
    for s, n in [(2, 5), (0, 9)]:
        ids = rng.integers(0, VOCAB, n).tolist()
        gen.admit(s, ids, SamplingParams(temp=0.0, repeat_penalty=1.0), 0, 20)
        host.admit(s, ids, 20)
    retired = gen.run(25)
    for _ in range(25):
        host.step()
    assert sorted(retired) == [0, 2]
    for s in (0, 2):
        assert gen.tokens(s) == host.out[s] and len(gen.tokens(s)) == 20


def test_sampled_graph_run_equals_eager_and_itself_with_slots_permuted(dev):
    """k 40, top_p 0.95, temp 0.8, repeat 1.1 (the reference's defaults), a seed per sequence: the graph run equals the eager run of the same generator, and sequences 0
    and 1 produce the same tokens in other slots with other prompts beside them at the same B.  Each sequence is admitted by a call of its own (a prompt's prefill
    launches are then the same whoever else is admitted)."""
    from tinychatengine_amd.generate import SamplingParams
    m = _model(dev, SMALL)
    rng = np.random.default_rng(77)
    prompts = [rng.integers(0, VOCAB, n).tolist() for n in (7, 3, 12, 5, 9, 4)]
    seeds = [1001, 1002, 1003, 1004, 1005, 1006]

    def run(layout, graph, free_order=None):  # layout: slot -> sequence number
        gen = m.generator(graph=graph, free_order=free_order)
        for slot, q in layout.items():
            gen.admit(slot, prompts[q], SamplingParams(), seeds[q], 24)
            gen.run(1)  # staggered
        gen.run(30)
        gen.allocator.check_invariants()
        return {q: gen.tokens(slot) for slot, q in layout.items()}

    a = run({0: 0, 1: 1, 2: 2, 3: 3}, True)
    assert all(len(t) == 24 for t in a.values()) and len({tuple(t) for t in a.values()}) == 4
    assert run({0: 0, 1: 1, 2: 2, 3: 3}, False) == a, "graph replay and eager steps disagree"
    c = run({3: 0, 0: 1, 1: 4, 2: 5}, True, free_order=np.random.default_rng(2).permutation(NUM_PAGES).tolist())
    assert c[0] == a[0] and c[1] == a[1], "a sequence's tokens depend on its slot or its neighbours"
    # and sampling is really sampling: another seed draws another sequence from the same prompt
    gen = m.generator(graph=True)
    gen.admit(0, prompts[0], SamplingParams(), 4242, 24)
    gen.run(30)
    assert gen.tokens(0) != a[0]
