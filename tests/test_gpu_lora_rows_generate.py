"""Gate/up adapters and adapters on speculative rows through the decoders and the generators (tinychatengine_amd/lora.py, batch_decode.py, speculative.py,
generate.py), on the tiny model of tests/test_gpu_lora_generate.py: 2 layers, hidden 512, 4 query heads over 1 key / value head, ffn 1408, vocabulary 4096.

* a decoder step() with a gate_up=True pool equals, bit for bit, the same public calls issued by hand (7 + 8 launches);
* an adapter that carries only gate_proj / up_proj changes the tokens against the base model; launches_per_token is 15 L + 5;
* a generator with a gate_up=True pool and every slot on adapter=None gives lora=None's tokens at B = 4;
* speculative rows, B = 3 (slots on adapter 0, none, adapter 1), T = 4, fp16 and e4m3 pages, greedy and sampled, scripted drafts all right and half wrong:
  SpeculativeGenerator(lora=pool_T) emits BatchedGenerator(lora=pool)'s tokens id for id; between the runs slots are released and admitted on other adapters under
  the same graph object, and release() leaves -1 in all T words of the slot.
"""
import numpy as np
import pytest

import test_gpu_lora_generate as LG

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HD, VOCAB, HIDDEN, HEADS, KV_HEADS, FFN, LAYERS = LG.HD, LG.VOCAB, LG.HIDDEN, LG.HEADS, LG.KV_HEADS, LG.FFN, LG.LAYERS
MAX_KEYS, PAGE_KEYS, NUM_PAGES = LG.MAX_KEYS, LG.PAGE_KEYS, LG.NUM_PAGES
RANK, MAX_ADAPTERS, T = 8, 4, 4
DIMS = {"q_proj": (HIDDEN, HEADS * HD), "k_proj": (HIDDEN, KV_HEADS * HD), "v_proj": (HIDDEN, KV_HEADS * HD), "o_proj": (HEADS * HD, HIDDEN), "down_proj": (FFN, HIDDEN),
        "gate_proj": (HIDDEN, FFN), "up_proj": (HIDDEN, FFN)}


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    if "m" not in LG._model_cache:
        LG._model_cache["m"] = LG._Model(dev)
    return LG._model_cache["m"]


def _adapter(seed, names=tuple(DIMS), r=RANK, gain=0.5):
    """PEFT-style arrays for every layer, strong enough to move the argmax"""
    rng = np.random.default_rng(seed)
    return [{nm: ((rng.normal(0, 1, (r, DIMS[nm][0])) * DIMS[nm][0] ** -0.5).astype(np.float16), (rng.normal(0, 1, (DIMS[nm][1], r)) * gain).astype(np.float16)) for nm in names}
            for _ in range(LAYERS)]


def _pool(model, rows_per_seq=None):
    """adapter 0: all seven projections; adapter 1: gate_proj / up_proj only, rank 4; adapter 2 left as zeros"""
    from tinychatengine_amd.lora import LoraPool
    pool = LoraPool(model.blocks[0], LAYERS, MAX_ADAPTERS, RANK, model.dev, gate_up=True, rows_per_seq=rows_per_seq)
    pool.load(0, _adapter(1), alpha=8.0)
    pool.load(1, _adapter(2, names=("gate_proj", "up_proj"), r=4), alpha=8.0)
    return pool


def _greedy():
    from tinychatengine_amd.generate import SamplingParams
    return SamplingParams(temp=0.0, repeat_penalty=1.0)


def _sampled():
    from tinychatengine_amd.generate import SamplingParams
    return SamplingParams(temp=0.8, top_k=8, top_p=0.95, repeat_penalty=1.1)


def test_decoder_step_equals_the_public_calls_by_hand(dev, model):
    from tinychatengine_amd import capi
    from tinychatengine_amd.batch_decode import BatchedDecoder
    from tinychatengine_amd.linear import _stream, rmsnorm_half
    from tinychatengine_amd.lora import expand_add, expand_silu_mul, shrink
    B = 4
    pool = _pool(model)
    blk, lv = model.blocks[0], pool.layer(0)
    d_pool, d_hand, d_base = BatchedDecoder(blk, B, lora=lv), BatchedDecoder(blk, B), BatchedDecoder(blk, B)
    assert d_pool.LAUNCHES == 15 and d_hand.LAUNCHES == 7
    pool.row_adapter.copy_(torch.tensor([0, -1, 1, 2], dtype=torch.int32))
    g = torch.Generator(device=dev).manual_seed(3)
    h0 = torch.empty((B, HIDDEN), device=dev).normal_(0, 1, generator=g).half()
    pos = torch.zeros(B, dtype=torch.int32, device=dev)
    h_pool, h_hand, h_base = h0.clone(), h0.clone(), h0.clone()
    d_pool.step(h_pool, pos, MAX_KEYS - 1)
    d_base.step(h_base, pos, MAX_KEYS - 1)
    st, ra, d = _stream(), pool.row_adapter, d_hand
    t = {k: torch.empty((B, lv.A[k].shape[1]), dtype=torch.float32, device=dev) for k in ("qkv", "o", "down", "gate_up")}
    y = torch.empty((B, 2 * FFN), dtype=torch.float16, device=dev)
    rmsnorm_half(h_hand, blk.gamma1, blk.eps, out=d.xn)
    shrink(d.xn, lv.A["qkv"], ra, t["qkv"])
    capi.check(capi.w4a16_forward(blk.qkv.desc(d.xn, d.qkv_out), st))
    expand_add(t["qkv"], lv.B["qkv"], pool.scale, ra, d.qkv_out)
    d.attention.step(d.qkv_out, pos, MAX_KEYS - 1, out=d.attn_out)
    shrink(d.attn_out, lv.A["o"], ra, t["o"])
    capi.check(capi.w4a16_forward(blk.o.desc(d.attn_out, h_hand, flags=capi.TCE_W4_ADD_TO_C), st))
    expand_add(t["o"], lv.B["o"], pool.scale, ra, h_hand)
    rmsnorm_half(h_hand, blk.gamma2, blk.eps, out=d.xn)
    shrink(d.xn, lv.A["gate_up"], ra, t["gate_up"])
    capi.check(capi.w4a16_forward(blk.gate_up.desc(d.xn, y), st))
    expand_silu_mul(t["gate_up"], lv.Bg, lv.Bu, pool.scale, ra, y, d.act)
    shrink(d.act, lv.A["down"], ra, t["down"])
    capi.check(capi.w4a16_forward(blk.down.desc(d.act, h_hand, flags=capi.TCE_W4_ADD_TO_C), st))
    expand_add(t["down"], lv.B["down"], pool.scale, ra, h_hand)
    torch.cuda.synchronize()
    assert torch.equal(h_pool.view(torch.int16), h_hand.view(torch.int16)), "step() with a gate_up pool differs from the calls issued by hand"
    assert bool((h_pool[1] == h_base[1]).all()) and bool((h_pool[3] == h_base[3]).all()), "the rows without an adapter and on the all-zero adapter must equal the base model's"
    for r in (0, 2):
        assert not torch.equal(h_pool[r], h_base[r]), f"row {r}: the adapter changed nothing"


def _run_plain(gen, adm, adapters):
    """one admit, replays until every admitted slot has retired -> {slot: tokens}; the slots are released"""
    retired = gen.admit(adm, adapters=adapters)
    for _ in range(40):
        if len(retired) == len(adm):
            break
        retired += gen.run(1)
    assert sorted(retired) == sorted(s for s, *_ in adm)
    out = {s: gen.tokens(s) for s, *_ in adm}
    for s, *_ in adm:
        gen.release(s)
    return out


def test_gate_up_adapters_through_the_generator(dev, model):
    from tinychatengine_amd.generate import BatchedGenerator
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchedDecoder
    B = 4
    pool = _pool(model)
    alloc = PageAllocator(NUM_PAGES, PAGE_KEYS, B, MAX_KEYS // PAGE_KEYS, dev)
    gen = BatchedGenerator([PagedBatchedDecoder(b, alloc, lora=pool.layer(i)) for i, b in enumerate(model.blocks)], model.final_gamma, model.lm_head, model.table, max_new=8, lora=pool)
    base = model.generator(True, max_new=8)
    assert gen.launches_per_token == 15 * LAYERS + 5 and base.launches_per_token == 7 * LAYERS + 5
    graph = gen._graph
    adm = [(s, LG.PROMPTS[s], _greedy(), s, 8) for s in range(B)]
    want = _run_plain(base, adm, None)
    got = _run_plain(gen, adm, {})
    assert got == want, "a gate_up pool with every slot on adapter=None differs from lora=None"
    only = _run_plain(gen, adm, {0: 1, 2: 1})  # adapter 1 carries gate_proj / up_proj only
    assert only[0] != want[0] and only[2] != want[2], "an adapter on gate / up alone changed no token"
    assert only[1] == want[1] and only[3] == want[3], "slots on None beside adapted slots must decode the base model's tokens"
    zero = _run_plain(gen, adm, {0: 2})
    assert zero == want, "a slot on an all-zero adapter differs from the base model"
    assert gen._graph is graph and pool.row_adapter.tolist() == [-1] * B


@pytest.mark.parametrize("kv_dtype", ["fp16", "fp8_e4m3"])
def test_speculative_rows_with_mixed_adapters_emit_the_plain_tokens(dev, model, kv_dtype):
    from tinychatengine_amd.generate import BatchedGenerator
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchedDecoder
    from tinychatengine_amd.speculative import SpeculativeDecoder, SpeculativeGenerator
    B, MAX_NEW = 3, 11
    kw = dict(kv_dtype=kv_dtype, k_scale_log2=-1, v_scale_log2=-1) if kv_dtype != "fp16" else {}
    pool, pool_t = _pool(model), _pool(model, rows_per_seq=T)
    alloc_p, alloc_s = (PageAllocator(NUM_PAGES, PAGE_KEYS, B, MAX_KEYS // PAGE_KEYS, dev) for _ in range(2))
    plain = BatchedGenerator([PagedBatchedDecoder(b, alloc_p, lora=pool.layer(i), **kw) for i, b in enumerate(model.blocks)], model.final_gamma, model.lm_head, model.table,
                             max_new=MAX_NEW, lora=pool)
    spec = SpeculativeGenerator([SpeculativeDecoder(b, alloc_s, T, lora=pool_t.layer(i), **kw) for i, b in enumerate(model.blocks)], model.final_gamma, model.lm_head,
                                model.table, max_new=MAX_NEW, script=True, lora=pool_t)
    assert spec.launches_per_token == 7 * LAYERS + 7 + 8 * LAYERS and spec.lora is pool_t and pool_t.row_adapter.numel() == B * T
    graph = spec._graph
    assert graph is not None
    for rnd, (params, adapters, wrong) in enumerate([(_greedy, {0: 0, 2: 1}, False), (_greedy, {0: 0, 2: 1}, True), (_sampled, {0: 0, 2: 1}, False), (_sampled, {0: 1, 1: 0}, True)]):
        adm = [(s, LG.PROMPTS[s], params(), 30 + s, MAX_NEW) for s in range(B)]
        want = _run_plain(plain, adm, adapters)
        assert all(len(want[s]) == MAX_NEW for s in range(B))
        for s, ids, *_ in adm:  # the drafts: the plain tokens, every other one wrong in the `wrong` rounds
            spec.set_script(s, [-1] * len(ids) + [(t + 1) % VOCAB if wrong and i % 2 else t for i, t in enumerate(want[s])])
        steps0 = spec._steps
        retired = spec.admit(adm, adapters=adapters)
        words = pool_t.row_adapter.view(B, T).tolist()
        assert words == [[-1 if adapters.get(s) is None else adapters[s]] * T for s in range(B)], "admit writes the slot's word once per row"
        for _ in range(MAX_NEW + 2):
            if len(retired) == B:
                break
            retired += spec.run(1)
        assert sorted(retired) == list(range(B))
        for s in range(B):
            assert spec.tokens(s) == want[s], f"round {rnd} slot {s} (adapter {adapters.get(s)}): the speculative run differs from BatchedGenerator(lora=pool)"
        em = spec.emitted_per_step()[steps0:]
        if wrong:
            assert em.max() <= 2 and em.sum() == B * (MAX_NEW - 1)
        else:
            assert em.max() == T, "no step accepted all its drafts: the scripts were not followed"
        for s in range(B):
            spec.release(s)
            assert pool_t.row_adapter.view(B, T)[s].tolist() == [-1] * T, "release() leaves -1 in all T words"
        assert spec._graph is graph, "an admission on another adapter captured again"
    assert spec.embed_violations() == 0
    # the adapters are in the speculative rows: the same prompts on the base model give other tokens
    adm = [(s, LG.PROMPTS[s], _greedy(), 30 + s, MAX_NEW) for s in range(B)]
    base = _run_plain(plain, adm, {})
    adapted = _run_plain(plain, adm, {0: 0, 2: 1})
    assert adapted[0] != base[0] and adapted[2] != base[2] and adapted[1] == base[1]
