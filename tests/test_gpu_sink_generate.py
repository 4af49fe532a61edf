"""Attention sinks in the closed generation loop: BatchedGenerator on layers with window = 32 and sinks = 4 over 16-key pages produces, id for id, what the
host-driven loop produces on a pool that holds everything and never gives a page back -- on a pool that full attention exhausts, with one prompt longer than the pool
(admitted with chunk_rows), the slots' pages within ceil((W + N) / page_keys) + 2.  fp16 and e4m3 pages; one layer with sinks beside one with a plain window."""
import numpy as np
import pytest

from test_gpu_window import _allocator, _tables

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KEYS, PAGE, BATCH, PAGES, W, S, NEW, BURST, CHUNK = 512, 16, 3, 16, 32, 4, 150, 8, 16
VOCAB = 4096


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


class _Model:
    """hidden 512, heads 4 / 1, ffn 1408, two layers, synthetic weights (tests/test_gpu_window.py's small model on a 512-key table)."""

    def __init__(self, dev, seed=40):
        from tinychatengine_amd.decoder_block import DecoderBlock
        from tinychatengine_amd.linear import Linear_half_int4
        hidden, heads, kv_heads, ffn, layers = 512, 4, 1, 1408, 2
        cos, sin = _tables(KEYS, seed, dev)
        self.dev = dev
        self.blocks = [DecoderBlock(hidden, heads, ffn, KEYS, dev, cos, sin, seed=seed + i, kv_heads=kv_heads) for i in range(layers)]
        g = torch.Generator(device=dev).manual_seed(seed + 100)
        self.final_gamma = (1.0 + 0.1 * torch.empty(hidden, device=dev).normal_(0, 1, generator=g)).float()
        self.lm_head = Linear_half_int4.from_float(torch.empty(VOCAB, hidden, device=dev).normal_(0.0, hidden ** -0.5, generator=g)).prepack()
        self.table = torch.empty(VOCAB, hidden, device=dev).normal_(0.0, 1.0, generator=g).half()

    def decoders(self, layers, kv_dtype, pages):
        """layers: (window, sinks) per layer over ONE allocator of `pages` pages"""
        from tinychatengine_amd.paged_kv import PagedBatchedDecoder
        alloc = _allocator(self.dev, PAGE, BATCH, KEYS, pages, seed=6)
        return [PagedBatchedDecoder(b, alloc, kv_dtype=kv_dtype, window=w, sinks=s) for b, (w, s) in zip(self.blocks, layers)]


@pytest.fixture(scope="module")
def model(dev):
    return _Model(dev)


def _host_admit_chunked(host, adm, chunk_rows):
    """HostDrivenLoop.admit with the prompts fed in BatchedGenerator's chunks (generate.admission_chunks) -- the same prefill launches -- and no page given back."""
    from tinychatengine_amd.generate import admission_chunks
    last = torch.zeros_like(host.hidden)
    for rnd in admission_chunks([len(ids) for _, ids, _ in adm], chunk_rows):
        chunk = [(adm[i][0], host.table_host[torch.tensor(adm[i][1][c0:c0 + m], dtype=torch.int64)].to(host.device).contiguous(), c0) for i, c0, m in rnd["segments"]]
        for d in host.decoders:
            d.prefill_many(chunk)
        for slot, rows, _ in chunk:
            last[slot].copy_(rows[-1])
    tok = host._argmax(last)
    for s, ids, mn in adm:
        host.out[s], host.max_new[s] = [], mn
        host.pos_host[s] = len(ids) - 1
        host._take(s, int(tok[s]))


@pytest.mark.parametrize("layers", [((W, S), (W, S)), ((W, S), (W, None))], ids=["sinks-sinks", "sinks-window"])
@pytest.mark.parametrize("kv_dtype", ["fp16", "fp8_e4m3"])
def test_a_sink_generator_runs_where_full_attention_exhausts_the_pool(dev, model, kv_dtype, layers):
    from tinychatengine_amd.generate import BatchedGenerator, HostDrivenLoop, SamplingParams
    from tinychatengine_amd.paged_kv import PagePoolExhausted
    greedy = SamplingParams(temp=0.0, repeat_penalty=1.0)
    rng = np.random.default_rng(77)
    prompts = [rng.integers(0, VOCAB, n).tolist() for n in (300, 3, 21)]  # the first: longer than the pool's 16 pages x 16 keys
    adm = [(s, prompts[s], greedy, 0, NEW) for s in range(BATCH)]

    # full attention: the long prompt alone does not fit, chunked or not
    full = BatchedGenerator(model.decoders(((None, None), (None, None)), kv_dtype, PAGES), model.final_gamma, model.lm_head, model.table, max_new=NEW)
    with pytest.raises(PagePoolExhausted):
        full.admit(adm, chunk_rows=CHUNK)
    assert full.allocator.pages_in_use() == 0
    del full

    gen = BatchedGenerator(model.decoders(layers, kv_dtype, PAGES), model.final_gamma, model.lm_head, model.table, max_new=NEW)
    host = HostDrivenLoop(model.decoders(layers, kv_dtype, BATCH * (KEYS // PAGE)), model.final_gamma, model.lm_head, model.table)
    assert [(d.window, d.sinks) for d in gen.decoders] == list(layers)
    gen.admit(adm, chunk_rows=CHUNK)
    _host_admit_chunked(host, [(s, prompts[s], NEW) for s in range(BATCH)], CHUNK)
    per_slot = (W + max(BURST, CHUNK) + PAGE - 1) // PAGE + 2
    assert gen.allocator.kept[0] and gen.allocator.gone[0] >= 10, "the long prompt's pages did not come back"
    retired = []
    while len(retired) < BATCH:
        for s in gen.book.live():
            assert len(gen.allocator.kept[s]) + len(gen.allocator.pages[s]) <= per_slot
        retired += gen.run(BURST)
        gen.allocator.check_invariants()
        for s in gen.book.live():
            held = len(gen.allocator.kept[s]) + len(gen.allocator.pages[s])
            assert held <= per_slot, f"slot {s} holds {held} pages"
            assert gen.allocator.holds(s, 0, S), f"slot {s} gave its sinks' page back"
        assert gen.allocator.pages_in_use() <= BATCH * per_slot
    for _ in range(NEW):
        host.step()  # (the host-driven loop never gives anything back)
    for s in range(BATCH):
        toks = gen.tokens(s)
        assert len(toks) == NEW and toks == host.out[s], f"slot {s}: the graph run and the host-driven loop that kept every page disagree"
    assert gen.embed_violations() == 0
    for s in range(BATCH):
        gen.release(s)
    assert gen.allocator.pages_in_use() == 0
    gen.allocator.check_invariants()
