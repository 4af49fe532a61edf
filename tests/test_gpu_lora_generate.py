"""Multi-LoRA through the decoders and the generator (tinychatengine_amd/lora.py, batch_decode.py, paged_kv.py, generate.py) on the tiny model shape of
tests/test_gpu_generate.py: 2 layers, hidden 512, 4 query heads over 1 key / value head, head_dim 128, ffn 1408, vocabulary 4096.  Synthetic weights and adapters.

* a decoder step() with a pool equals, bit for bit, the same sequence of public calls issued by hand (7 + 6 launches);
* a generator with a pool and every slot on adapter=None gives the tokens and logits of lora=None bit for bit; a slot on an all-zero adapter gives equal logits (==);
* a (prompt, adapter)'s greedy tokens and its logits at every step do not depend on the other slots (empty, on other adapters, on none) or on the slot it sits in --
  contiguous and paged decoders each compared with themselves;
* the first token (the adapted prefill) and later tokens differ from the base model's; an adapter loaded and admitted after the capture changes the output with the
  same graph object; release() leaves -1; launches_per_token counts the new launches; score(adapter=) scores under the adapter.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HD, VOCAB = 128, 4096
MAX_KEYS, PAGE_KEYS, BATCH, NUM_PAGES = 64, 16, 4, 12
HIDDEN, HEADS, KV_HEADS, FFN, LAYERS = 512, 4, 1, 1408, 2
RANK, MAX_ADAPTERS = 8, 4
STEPS = 4


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


def _adapter(seed, r=RANK, gain=0.5):
    """PEFT-style arrays for every layer and all five projections, strong enough to move the argmax"""
    rng = np.random.default_rng(seed)
    dims = {"q_proj": (HIDDEN, HEADS * HD), "k_proj": (HIDDEN, KV_HEADS * HD), "v_proj": (HIDDEN, KV_HEADS * HD), "o_proj": (HEADS * HD, HIDDEN), "down_proj": (FFN, HIDDEN)}
    return [{nm: ((rng.normal(0, 1, (r, k)) * k ** -0.5).astype(np.float16), (rng.normal(0, 1, (n, r)) * gain).astype(np.float16)) for nm, (k, n) in dims.items()}
            for _ in range(LAYERS)]


class _Model:
    def __init__(self, dev, seed=40 + HIDDEN):
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

    def pool(self):
        """adapters 0 and 1 loaded, 2 left as zeros, 3 free for a later load"""
        from tinychatengine_amd.lora import LoraPool
        pool = LoraPool(self.blocks[0], LAYERS, MAX_ADAPTERS, RANK, self.dev)
        pool.load(0, _adapter(1), alpha=8.0)
        pool.load(1, _adapter(2, r=4), alpha=8.0)
        return pool

    def generator(self, paged, pool=None, graph=True, max_new=STEPS + 2):
        from tinychatengine_amd.batch_decode import BatchedDecoder
        from tinychatengine_amd.generate import BatchedGenerator
        from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchedDecoder
        view = (lambda i: None) if pool is None else pool.layer
        if paged:
            alloc = PageAllocator(NUM_PAGES, PAGE_KEYS, BATCH, MAX_KEYS // PAGE_KEYS, self.dev)
            decs = [PagedBatchedDecoder(b, alloc, lora=view(i)) for i, b in enumerate(self.blocks)]
        else:
            decs = [BatchedDecoder(b, BATCH, lora=view(i)) for i, b in enumerate(self.blocks)]
        return BatchedGenerator(decs, self.final_gamma, self.lm_head, self.table, max_new=max_new, graph=graph, lora=pool)


_model_cache = {}


@pytest.fixture(scope="module")
def model(dev):
    if "m" not in _model_cache:
        _model_cache["m"] = _Model(dev)
    return _model_cache["m"]


def _greedy():
    from tinychatengine_amd.generate import SamplingParams
    return SamplingParams(temp=0.0, repeat_penalty=1.0)


PROMPTS = {k: np.random.default_rng(100 + k).integers(0, VOCAB, n).tolist() for k, n in {0: 7, 1: 3, 2: 18, 3: 5}.items()}


def _trace(gen, admissions, watch):
    """admissions {slot: (prompt key, adapter)} through ONE admit; STEPS replays.  -> (tokens of `watch`, its logits row after the admission and after every replay, as bits)"""
    adm = [(s, PROMPTS[k], _greedy(), 0, STEPS + 2) for s, (k, _) in admissions.items()]
    kw = {"adapters": {s: a for s, (_, a) in admissions.items() if a is not None}} if gen.lora is not None else {}
    gen.admit(adm, **kw)
    rows = [gen.logits[watch, :VOCAB].clone()]
    for _ in range(STEPS):
        gen.run(1)
        rows.append(gen.logits[watch, :VOCAB].clone())
    toks = gen.tokens(watch)
    for s in admissions:
        gen.release(s)
    return toks, torch.stack(rows).cpu().numpy().view(np.uint16)


def test_decoder_step_equals_the_public_calls_by_hand(dev, model):
    from tinychatengine_amd import capi
    from tinychatengine_amd.batch_decode import BatchedDecoder
    from tinychatengine_amd.linear import _stream, rmsnorm_half
    from tinychatengine_amd.lora import expand_add, shrink
    pool = model.pool()
    blk = model.blocks[0]
    lv = pool.layer(0)
    d_pool, d_hand, d_base = BatchedDecoder(blk, BATCH, lora=lv), BatchedDecoder(blk, BATCH), BatchedDecoder(blk, BATCH)
    assert d_pool.LAUNCHES == 13 and d_hand.LAUNCHES == 7
    pool.row_adapter.copy_(torch.tensor([0, -1, 1, 2], dtype=torch.int32))
    g = torch.Generator(device=dev).manual_seed(3)
    h0 = torch.empty((BATCH, HIDDEN), device=dev).normal_(0, 1, generator=g).half()
    pos = torch.zeros(BATCH, dtype=torch.int32, device=dev)
    h_pool, h_hand, h_base = h0.clone(), h0.clone(), h0.clone()
    d_pool.step(h_pool, pos, MAX_KEYS - 1)
    d_base.step(h_base, pos, MAX_KEYS - 1)
    # by hand, on d_hand's buffers and caches
    st, ra, d = _stream(), pool.row_adapter, d_hand
    t = {k: torch.empty((BATCH, lv.A[k].shape[1]), dtype=torch.float32, device=dev) for k in ("qkv", "o", "down")}
    rmsnorm_half(h_hand, blk.gamma1, blk.eps, out=d.xn)
    shrink(d.xn, lv.A["qkv"], ra, t["qkv"])
    capi.check(capi.w4a16_forward(blk.qkv.desc(d.xn, d.qkv_out), st))
    expand_add(t["qkv"], lv.B["qkv"], pool.scale, ra, d.qkv_out)
    d.attention.step(d.qkv_out, pos, MAX_KEYS - 1, out=d.attn_out)
    shrink(d.attn_out, lv.A["o"], ra, t["o"])
    capi.check(capi.w4a16_forward(blk.o.desc(d.attn_out, h_hand, flags=capi.TCE_W4_ADD_TO_C), st))
    expand_add(t["o"], lv.B["o"], pool.scale, ra, h_hand)
    rmsnorm_half(h_hand, blk.gamma2, blk.eps, out=d.xn)
    d._gate_up(d.xn, st)  # (gate / up are not adapted: the decoder's own launches)
    shrink(d.act, lv.A["down"], ra, t["down"])
    capi.check(capi.w4a16_forward(blk.down.desc(d.act, h_hand, flags=capi.TCE_W4_ADD_TO_C), st))
    expand_add(t["down"], lv.B["down"], pool.scale, ra, h_hand)
    torch.cuda.synchronize()
    assert torch.equal(h_pool.view(torch.int16), h_hand.view(torch.int16)), "step() with a pool differs from the calls issued by hand"
    assert torch.equal(h_pool[1].view(torch.int16), h_base[1].view(torch.int16)), "the row without an adapter must be the base model's, bit for bit"
    assert bool((h_pool[3] == h_base[3]).all()), "the row on the all-zero adapter must equal the base model's"
    for r in (0, 2):
        assert not torch.equal(h_pool[r], h_base[r]), f"row {r}: the adapter changed nothing"


@pytest.mark.parametrize("paged", [True, False], ids=["paged", "contiguous"])
def test_generator_with_a_pool(dev, model, paged):
    pool = model.pool()
    base = model.generator(paged)
    gen = model.generator(paged, pool)
    # (the figure is BatchedDecoder.LAUNCHES' : it assumes the SiLU * mul pairs are accepted, as they are at this shape; where gate / up fall back to three launches
    # a layer issues two more than it says, with or without a pool)
    assert base.launches_per_token == 7 * LAYERS + 5 and gen.launches_per_token == 13 * LAYERS + 5
    graph = gen._graph
    assert graph is not None

    # every slot on adapter=None: the base model bit for bit
    adm = {0: (0, None), 1: (1, None), 2: (2, None), 3: (3, None)}
    for watch in (0, 2):
        tb, lb = _trace(base, adm, watch)
        tg, lg = _trace(gen, adm, watch)
        assert tg == tb and np.array_equal(lg, lb), f"slot {watch}: a pool with every slot on None differs from lora=None"
    base_tokens, base_logits = _trace(base, {1: (0, None)}, 1)

    # an all-zero adapter: numerically equal logits
    tz, lz = _trace(gen, {1: (0, 2)}, 1)
    assert tz == base_tokens and bool((lz.view(np.float16) == base_logits.view(np.float16)).all()), "a slot on an all-zero adapter differs from the base model"

    # (prompt 0, adapter 0): alone, beside other adapters, beside slots on none, in another slot
    want_t, want_l = _trace(gen, {1: (0, 0)}, 1)
    for what, (adm, watch) in {"other slots on other adapters": ({0: (1, 1), 1: (0, 0), 2: (2, 1), 3: (3, 2)}, 1),
                               "other slots on the same adapter": ({0: (1, 0), 1: (0, 0), 2: (2, 0)}, 1),
                               "other slots on none": ({0: (1, None), 1: (0, 0), 3: (3, None)}, 1),
                               "in another slot": ({3: (0, 0), 0: (2, 1)}, 3)}.items():
        got_t, got_l = _trace(gen, adm, watch)
        assert got_t == want_t, f"{what}: tokens differ"
        assert np.array_equal(got_l, want_l), f"{what}: logits differ"

    # the adapter is in the prefill (first token) and in the steps
    assert not np.array_equal(want_l[0], base_logits[0]), "the first token's logits are the base model's: the prefill forgot the adapter"
    assert not np.array_equal(want_l[2], base_logits[2]) and want_t != base_tokens
    other_t, other_l = _trace(gen, {1: (0, 1)}, 1)
    assert not np.array_equal(other_l[0], want_l[0]) and not np.array_equal(other_l[0], base_logits[0])

    # an adapter loaded after the capture, admitted without a new capture
    pool.load(3, _adapter(9), alpha=8.0)
    new_t, new_l = _trace(gen, {1: (0, 3)}, 1)
    assert gen._graph is graph
    assert not np.array_equal(new_l[0], want_l[0]) and not np.array_equal(new_l[2], want_l[2]) and not np.array_equal(new_l[2], base_logits[2])
    pool.unload(3)
    gone_t, gone_l = _trace(gen, {1: (0, 3)}, 1)
    assert gone_t == base_tokens and bool((gone_l.view(np.float16) == base_logits.view(np.float16)).all()), "an unloaded adapter must add 0"

    # the words: written by admit, -1 after release
    gen.admit(2, PROMPTS[1], _greedy(), 0, 3, adapter=1)
    assert pool.row_adapter.tolist() == [-1, -1, 1, -1]
    gen.release(2)
    assert pool.row_adapter.tolist() == [-1] * BATCH

    # refusals
    with pytest.raises(ValueError):
        base.admit(0, PROMPTS[1], _greedy(), 0, 3, adapter=0)
    with pytest.raises(ValueError):
        gen.admit(0, PROMPTS[1], _greedy(), 0, 3, adapter=MAX_ADAPTERS)
    with pytest.raises(ValueError):
        gen.admit([(0, PROMPTS[1], _greedy(), 0, 3)], adapters={1: 0})
    with pytest.raises(ValueError):
        gen.admit(0, PROMPTS[1], _greedy(), 0, 3, adapters={0: 0})
    assert gen.book.live() == [] and pool.row_adapter.tolist() == [-1] * BATCH
    from tinychatengine_amd.generate import BatchedGenerator
    with pytest.raises(ValueError):
        BatchedGenerator(gen.decoders, model.final_gamma, model.lm_head, model.table, max_new=4, graph=False)  # decoders with views, no pool

    if paged:  # score(adapter=): every prompt under the adapter; the words are -1 again
        s_base = gen.score([PROMPTS[0], PROMPTS[2]])
        s_lora = gen.score([PROMPTS[0], PROMPTS[2]], adapter=0)
        s_ref = base.score([PROMPTS[0], PROMPTS[2]])
        assert all(np.array_equal(a, b) for a, b in zip(s_base, s_ref)) and not any(np.array_equal(a, b) for a, b in zip(s_lora, s_base))
        assert pool.row_adapter.tolist() == [-1] * BATCH
        with pytest.raises(ValueError):
            base.score([PROMPTS[0]], adapter=0)


def test_a_failed_chunked_admission_leaves_no_adapter_word_behind(dev, model):
    """Three slots hold 9 of the 12 pages; a 60-token prompt admitted in 16-row chunks with adapter=0 runs out of pages in its fourth chunk.  The generator is as it
    was before the call -- the slot free, its word -1 -- and score() without an adapter scores under the base model whatever a free slot's word holds."""
    from tinychatengine_amd.paged_kv import PagePoolExhausted
    pool = model.pool()
    base, gen = model.generator(True), model.generator(True, pool)
    rng = np.random.default_rng(7)
    long_ids = {s: rng.integers(0, VOCAB, 40).tolist() for s in range(3)}
    gen.admit([(s, long_ids[s], _greedy(), 0, 2) for s in range(3)], adapters={0: 1})
    assert gen.allocator.pages_in_use() == 9 and pool.row_adapter.tolist() == [1, -1, -1, -1]
    with pytest.raises(PagePoolExhausted):
        gen.admit(3, rng.integers(0, VOCAB, 60).tolist(), _greedy(), 0, 2, chunk_rows=16, adapter=0)
    assert pool.row_adapter.tolist() == [1, -1, -1, -1], "the failed admission left its adapter word behind"
    assert gen.allocator.pages_in_use() == 9 and gen.book.pos[3] < 0 and 3 in gen.free_slots()
    want = base.score([PROMPTS[0]])
    assert np.array_equal(gen.score([PROMPTS[0]])[0], want[0])
    pool.row_adapter[3] = 0  # a stale word in the free slot, written from outside: score() writes the word of every slot it uses
    assert np.array_equal(gen.score([PROMPTS[0]])[0], want[0]), "score() without an adapter ran under a free slot's stale word"
    assert pool.row_adapter.tolist() == [1, -1, -1, -1]
    assert not np.array_equal(gen.score([PROMPTS[0]], adapter=0)[0], want[0])
