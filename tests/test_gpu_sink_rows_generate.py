"""Attention sinks under speculative decoding, in the closed generation loop: SpeculativeGenerator with T = 4 rows on layers with window = 32 and sinks = 4 over
16-key pages emits, id for id, what BatchedGenerator emits over the same layers (tests/test_gpu_sink_generate.py holds that one against the host-driven loop) -- with
every draft right and with every second draft wrong, on a pool that full attention exhausts, one prompt longer than the pool (admitted with chunk_rows), the slots'
pages within ceil((W + n T) / page_keys) + 2, the sinks' page held throughout.  fp16 and e4m3 pages; one layer with sinks beside one with a plain window."""
import numpy as np
import pytest

from test_gpu_sink_generate import _Model
from test_gpu_window import _allocator
from test_gpu_window_rows import _rows_do_not_depend_on_their_index

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KEYS, PAGE, BATCH, W, S, T, NEW, BURST, CHUNK = 512, 16, 3, 32, 4, 4, 150, 2, 16
VOCAB = 4096
PER_SLOT = (W + BURST * T + PAGE - 1) // PAGE + 2  # ceil((W + n T) / page_keys) + 1 + keep_pages = 5
PAGES = BATCH * PER_SLOT  # 15 pages = 240 keys: fewer than the long prompt alone
LAYERS = {"sinks-sinks": ((W, S), (W, S)), "sinks-window": ((W, S), (W, None))}


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    m = _Model(dev)
    assert _rows_do_not_depend_on_their_index(m), "a row's logits depend on its index in the M = B T launch: plain decoding is no reference for rows t > 0"
    return m


def _prompts():
    rng = np.random.default_rng(77)
    return [rng.integers(0, VOCAB, n).tolist() for n in (300, 3, 21)]  # the first: longer than the pool's 15 pages x 16 keys


def _speculative(model, layers, kv_dtype, pages, graph=True):
    from tinychatengine_amd.speculative import SpeculativeDecoder, SpeculativeGenerator
    alloc = _allocator(model.dev, PAGE, BATCH, KEYS, pages, seed=6)
    decoders = [SpeculativeDecoder(b, alloc, T, kv_dtype=kv_dtype, window=w, sinks=s) for b, (w, s) in zip(model.blocks, layers)]
    return SpeculativeGenerator(decoders, model.final_gamma, model.lm_head, model.table, max_new=NEW, script=True, graph=graph)


_PLAIN = {}


def _plain_tokens(model, layers_id, kv_dtype):
    """The reference, computed once per (layers, pool type): BatchedGenerator over the same layers, greedy, the sequences in slots 0, T, 2 T of B T slots -- its linears
    then run at M = B T like the speculative generator's, the same kernels row for row (tests/test_gpu_window_rows.py says why that is needed for "id for id")."""
    key = (layers_id, kv_dtype)
    if key not in _PLAIN:
        from tinychatengine_amd.generate import BatchedGenerator, SamplingParams
        from tinychatengine_amd.paged_kv import PagedBatchedDecoder
        greedy = SamplingParams(temp=0.0, repeat_penalty=1.0)
        alloc = _allocator(model.dev, PAGE, BATCH * T, KEYS, BATCH * ((W + 8 + PAGE - 1) // PAGE + 2) + 1, seed=7)
        gen = BatchedGenerator([PagedBatchedDecoder(b, alloc, kv_dtype=kv_dtype, window=w, sinks=s) for b, (w, s) in zip(model.blocks, LAYERS[layers_id])],
                               model.final_gamma, model.lm_head, model.table, max_new=NEW)
        gen.admit([(s * T, ids, greedy, 0, NEW) for s, ids in enumerate(_prompts())], chunk_rows=CHUNK)
        while gen.book.live():
            gen.run(8)
        _PLAIN[key] = [gen.tokens(s * T) for s in range(BATCH)]
        assert all(len(t) == NEW for t in _PLAIN[key])
    return _PLAIN[key]


@pytest.mark.parametrize("drafts", ["all_correct", "half_wrong"])
@pytest.mark.parametrize("layers_id", list(LAYERS))
@pytest.mark.parametrize("kv_dtype", ["fp16", "fp8_e4m3"])
def test_speculative_generation_with_sinks_on_a_small_pool(dev, model, kv_dtype, layers_id, drafts):
    from tinychatengine_amd.generate import SamplingParams
    from tinychatengine_amd.paged_kv import PagePoolExhausted
    layers = LAYERS[layers_id]
    greedy = SamplingParams(temp=0.0, repeat_penalty=1.0)
    prompts = _prompts()
    adm = [(s, prompts[s], greedy, 0, NEW) for s in range(BATCH)]
    plain = _plain_tokens(model, layers_id, kv_dtype)

    # full attention: the long prompt alone does not fit this pool, chunked or not
    full = _speculative(model, ((None, None), (None, None)), kv_dtype, PAGES, graph=False)
    with pytest.raises(PagePoolExhausted):
        full.admit(adm, chunk_rows=CHUNK)
    assert full.allocator.pages_in_use() == 0
    del full

    spec = _speculative(model, layers, kv_dtype, PAGES)
    assert [(d.window, d.sinks, d.rows_per_seq) for d in spec.decoders] == [(w, s, T) for w, s in layers]
    assert all(d.attention.sinks == s and d.attention._entry("x") == ("x_sink" if s else "x_window") for d, (_, s) in zip(spec.decoders, layers))
    for s in range(BATCH):
        wrong = set(range(1, NEW, 2)) if drafts == "half_wrong" else set()
        spec.set_script(s, [-1] * len(prompts[s]) + [(t + 1) % VOCAB if i in wrong else t for i, t in enumerate(plain[s])])
    spec.admit(adm, chunk_rows=CHUNK)
    assert spec.allocator.kept[0] and spec.allocator.gone[0] >= 10, "the long prompt's pages did not come back"
    retired, runs = [], 0
    while len(retired) < BATCH:
        try:
            retired += spec.run(BURST)
        except PagePoolExhausted as e:  # (stated, not left to the traceback: this is the claim under test)
            pytest.fail(f"run() on {PAGES} pages after {runs} bursts: {e}")
        runs += 1
        spec.allocator.check_invariants()
        for s in spec.book.live():
            held = len(spec.allocator.kept[s]) + len(spec.allocator.pages[s])
            assert held <= PER_SLOT, f"slot {s} holds {held} pages"
            assert spec.allocator.holds(s, 0, S), f"slot {s} gave its sinks' page back"
        assert spec.allocator.pages_in_use() <= BATCH * PER_SLOT and runs <= NEW
    for s in range(BATCH):
        assert spec.tokens(s) == plain[s], f"slot {s} ({drafts}): the speculative run differs from BatchedGenerator over the same layers"
    em = spec.emitted_per_step()
    if drafts == "all_correct":
        assert em.max() == T and runs * BURST < NEW // 2, "the drafts were not accepted: the run proves nothing about rows t > 0"
    else:
        assert em.max() == 2 and (em == 2).sum() > NEW // 4, "every other draft should have been accepted"
    assert spec.embed_violations() == 0
    for s in range(BATCH):
        spec.release(s)
    assert spec.allocator.pages_in_use() == 0
    spec.allocator.check_invariants()
