"""The paged prefill (tce_attention_prefill_paged_f16, PagedBatchDecodeAttention.prefill, PagedBatchedDecoder.prefill_many): prompts straight into pages, several
sequences per launch.

Contract: only a row's address changes.  Every segment's output rows and appended cache rows are BIT-IDENTICAL to tce_attention_prefill_f16 for that sequence alone
on a contiguous cache with the same contents; no pool row other than rows pos .. pos + m - 1 of each segment changes; table words behind (pos + m - 1) // page_keys
are never followed.  The yardstick throughout is the contiguous path -- DecodeAttention.prefill, rows moved with tce_kv_pages_scatter_f16 / gather -- and every
comparison but the float64 guard at the end is for equal bits.  No test hands the kernel a page number outside the pool (canary words name in-range pages full of
NaN bits): a wrong kernel fails an assertion, not an address."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HD = 128
INF_BITS, NAN_BITS = 0x7C00, 0xFE00


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


def _tables(n, seed):
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, (n, HD // 2))
    cos = np.concatenate([np.cos(ang), np.cos(ang)], axis=1).astype(np.float16)
    sin = np.concatenate([np.sin(ang), np.sin(ang)], axis=1).astype(np.float16)
    return cos, sin


def _bits(t):
    return t.contiguous().view(torch.int16)


def _pattern(shape, bits, dev):
    return torch.full(shape, bits - 0x10000 if bits >= 0x8000 else bits, dtype=torch.int16, device=dev).view(torch.float16)


class _World:
    """`batch` sequences two ways: a contiguous DecodeAttention per slot (the yardstick; rows [0, pos) random, everything behind +inf / NaN bits) and one layer's
    pools behind a PageAllocator whose pages come in a seeded permuted order, pre-filled with the same bit patterns."""

    def __init__(self, dev, heads, kv_heads, page_keys, batch, max_keys, rope, seed, spare_pages=4):
        from tinychatengine_amd.attention_ops import DecodeAttention
        from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchDecodeAttention
        self.dev, self.heads, self.kv_heads, self.page_keys, self.batch, self.max_keys = dev, heads, kv_heads, page_keys, batch, max_keys
        self.g = torch.Generator(device=dev).manual_seed(seed)
        tc = ts = None
        if rope:
            cos, sin = _tables(max_keys, seed)
            tc, ts = torch.from_numpy(cos).to(dev), torch.from_numpy(sin).to(dev)
        self.cont = [DecodeAttention(heads, HD, max_keys, dev, tc, ts, kv_heads=kv_heads) for _ in range(batch)]
        for a in self.cont:
            a.k_cache.copy_(_pattern(a.k_cache.shape, INF_BITS, dev))
            a.v_cache.copy_(_pattern(a.v_cache.shape, NAN_BITS, dev))
        stride = max_keys // page_keys
        assert stride * page_keys == max_keys
        self.spare = spare_pages
        num_pages = batch * stride + spare_pages
        order = np.random.default_rng(seed + 1).permutation(num_pages).tolist()
        self.canaries = order[-spare_pages:]  # handed out last: with batch * stride pages for the slots they are never handed out at all
        self.alloc = PageAllocator(num_pages, page_keys, batch, stride, dev, free_order=order)
        self.P = PagedBatchDecodeAttention(self.alloc, heads, kv_heads, dev, tc, ts)
        self.P.k_pool.copy_(_pattern(self.P.k_pool.shape, INF_BITS, dev))
        self.P.v_pool.copy_(_pattern(self.P.v_pool.shape, NAN_BITS, dev))

    def rand(self, *shape, scale=0.9):
        return (torch.randn(shape, generator=self.g, device=self.dev) * scale).half()

    def context(self, slot, pos):
        """`pos` random cached keys in the contiguous cache of `slot`, scattered into freshly reserved pages."""
        if pos == 0:
            return
        a = self.cont[slot]
        a.k_cache[:, :pos].copy_(self.rand(self.kv_heads, pos, HD, scale=0.8))
        a.v_cache[:, :pos].copy_(self.rand(self.kv_heads, pos, HD, scale=0.8))
        self.alloc.reserve(slot, pos - 1)
        self.P.admit(slot, a, 0, pos)

    def plant_canaries(self, slot, upto_pos):
        """Every table word of `slot` behind the one that holds key `upto_pos` names a canary page (in range, never handed out, full of NaN bits)."""
        first = upto_pos // self.page_keys + 1
        n = self.alloc.table.shape[1] - first
        if n > 0:
            words = [self.canaries[i % self.spare] for i in range(n)]
            self.alloc.table[slot, first:].copy_(torch.tensor(words, dtype=torch.int32))

    def expected_pools(self, k0, v0, segments):
        """The pools as they must be after a launch: the clones taken before it with rows pos .. pos + m - 1 of each segment from the contiguous caches."""
        ek, ev = k0.clone(), v0.clone()
        pk = self.page_keys
        for slot, pos, m in segments:
            key = pos
            while key < pos + m:  # page by page
                n = min(pk - key % pk, pos + m - key)
                page = self.alloc.pages[slot][key // pk]
                ek[page, :, key % pk:key % pk + n] = self.cont[slot].k_cache[:, key:key + n]
                ev[page, :, key % pk:key % pk + n] = self.cont[slot].v_cache[:, key:key + n]
                key += n
        return ek, ev

    def launch(self, segments, causal, what):
        """One paged launch of `segments` [(slot, pos, m)] against the contiguous launch of each sequence alone: output rows, the whole pools, the gathered caches."""
        total = sum(m for _, _, m in segments)
        qkv = self.rand(total, (self.heads + 2 * self.kv_heads) * HD)
        for slot, pos, m in segments:
            self.alloc.reserve(slot, pos + m - 1)
            self.plant_canaries(slot, pos + m - 1)
        torch.cuda.synchronize()
        k0, v0 = self.P.k_pool.clone(), self.P.v_pool.clone()
        out_p = self.P.prefill(segments, qkv, causal=causal)
        torch.cuda.synchronize()
        row0 = 0
        for slot, pos, m in segments:
            out_c = self.cont[slot].prefill(qkv[row0:row0 + m], pos, causal=causal)
            torch.cuda.synchronize()
            assert torch.isfinite(out_p[row0:row0 + m].float()).all(), f"{what}: slot {slot} (pos {pos}, m {m}): output not finite"
            assert torch.equal(_bits(out_p[row0:row0 + m]), _bits(out_c)), f"{what}: slot {slot} (pos {pos}, m {m}): output rows differ from the contiguous launch"
            row0 += m
        ek, ev = self.expected_pools(k0, v0, segments)
        assert torch.equal(_bits(self.P.k_pool), _bits(ek)), f"{what}: the K pool is not (what it was + the appended rows)"
        assert torch.equal(_bits(self.P.v_pool), _bits(ev)), f"{what}: the V pool is not (what it was + the appended rows)"
        for slot, pos, m in segments:
            k, v = self.P.read_back(slot, pos + m)
            a = self.cont[slot]
            assert torch.equal(_bits(k), _bits(a.k_cache[:, :pos + m])) and torch.equal(_bits(v), _bits(a.v_cache[:, :pos + m])), f"{what}: slot {slot}: gathered caches differ"
        return qkv, out_p


CASES = [(0, 2), (5, 17), (64, 64), (100, 130), (37, 300), (0, 1024), (1, 129)]  # pos = 0 / inside a page / on a boundary; m below a block, ragged, several blocks, >= 1024


# ---- 1 + 2: one segment equals the contiguous launch; nothing else is written, nothing else is followed ----
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("page_keys", [16, 64, 256])
@pytest.mark.parametrize("heads,kv_heads", [(32, 8), (8, 8), (4, 1)])
def test_one_segment_equals_the_contiguous_launch(dev, heads, kv_heads, page_keys, rope, causal):
    from tinychatengine_amd import capi
    capi.check(capi.lib().tce_w4a16_set_debug_mode(2950))
    w = _World(dev, heads, kv_heads, page_keys, len(CASES), 1280, rope, seed=heads * 100 + page_keys)
    for slot, (pos, m) in enumerate(CASES):
        w.context(slot, pos)
        w.launch([(slot, pos, m)], causal, f"pos {pos} m {m}")
    w.alloc.check_invariants()


@pytest.mark.parametrize("mode", [2954, 2958, 2964, 2968, 2700, 2704, 2708, 2800, 2804, 2808])
@pytest.mark.parametrize("page_keys", [16, 128])
def test_forced_forms_equal_the_contiguous_launch_in_the_same_form(dev, page_keys, mode):
    """4 / 8 waves x 1 row tile (2954 / 2958), x 2 (2964 / 2968), pairing forced on (27xx) and off (28xx): the mode holds for both sides."""
    from tinychatengine_amd import capi
    L = capi.lib()
    capi.check(L.tce_w4a16_set_debug_mode(mode))
    try:
        w = _World(dev, 8, 2, page_keys, len(CASES), 1280, True, seed=mode + page_keys)
        for slot, (pos, m) in enumerate(CASES):
            w.context(slot, pos)
            w.launch([(slot, pos, m)], True, f"mode {mode} pos {pos} m {m}")
        w2 = _World(dev, 8, 2, page_keys, 3, 512, True, seed=mode)  # and a ragged launch in that form
        for slot, pos in enumerate((70, 0, 33)):
            w2.context(slot, pos)
        w2.launch([(2, 33, 300), (0, 70, 3), (1, 0, 129)], True, f"mode {mode} ragged")
    finally:
        capi.check(L.tce_w4a16_set_debug_mode(2950))


# ---- 3: chunks, then decode steps on the same pages ----
@pytest.mark.parametrize("page_keys", [16, 64])
def test_chunked_prompt_then_paged_decode_steps(dev, page_keys):
    """A 300-row prompt as 128 + 128 + 44 straight onto pages equals the contiguous cache fed the same chunks; ten paged decode steps afterwards equal the batched
    step on the contiguous copy."""
    from tinychatengine_amd.batch_decode import BatchDecodeAttention
    heads, kv_heads, max_keys = 32, 8, 512
    w = _World(dev, heads, kv_heads, page_keys, 2, max_keys, True, seed=300 + page_keys)
    pos = 0
    for m in (128, 128, 44):
        w.launch([(1, pos, m)], True, f"chunk at {pos}")
        pos += m
    A = BatchDecodeAttention(2, heads, max_keys, dev, w.P.cos, w.P.sin, kv_heads=kv_heads)
    A.k_cache[1].copy_(w.cont[1].k_cache)
    A.v_cache[1].copy_(w.cont[1].v_cache)
    for step in range(10):
        pos_t = torch.tensor([-1, pos], dtype=torch.int32, device=dev)
        w.alloc.reserve(1, pos)
        qkv = w.rand(2, (heads + 2 * kv_heads) * HD)
        assert w.P.table_violations(pos_t, max_keys - 1) == 0
        out_p = w.P.step(qkv, pos_t, max_keys - 1)
        out_c = A.step(qkv, pos_t, max_keys - 1)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out_p), _bits(out_c)), f"decode step {step} at {pos}"
        pos += 1
    k, v = w.P.read_back(1, pos)
    assert torch.equal(_bits(k), _bits(A.k_cache[1, :, :pos])) and torch.equal(_bits(v), _bits(A.v_cache[1, :, :pos]))


# ---- 4: a shared prefix, two suffixes in one launch ----
@pytest.mark.parametrize("page_keys", [16, 64])
def test_forked_sequences_prefill_their_suffixes_in_one_launch(dev, page_keys):
    heads, kv_heads = 8, 2
    w = _World(dev, heads, kv_heads, page_keys, 3, 8 * page_keys, True, seed=40 + page_keys)
    prefix = 3 * page_keys + 5
    w.launch([(0, 0, prefix)], True, "the prefix")
    for src, dst, rows in w.alloc.fork(0, 2, prefix):
        w.P.copy_rows(src, dst, rows)
    w.cont[2].k_cache.copy_(w.cont[0].k_cache)
    w.cont[2].v_cache.copy_(w.cont[0].v_cache)
    shared = w.alloc.pages[0][:3]
    assert w.alloc.pages[2][:3] == shared and w.alloc.pages[2][3] != w.alloc.pages[0][3]
    assert not w.alloc.writable(0, prefix - 6, 10) and w.alloc.writable(0, prefix, 11) and w.alloc.writable(2, prefix, 7)
    k_shared, v_shared = w.P.k_pool[shared].clone(), w.P.v_pool[shared].clone()
    w.launch([(2, prefix, 7), (0, prefix, 40)], True, "two suffixes")  # (launch() holds each output to the contiguous evaluation of that sequence alone)
    assert torch.equal(_bits(w.P.k_pool[shared]), _bits(k_shared)) and torch.equal(_bits(w.P.v_pool[shared]), _bits(v_shared)), "a shared page changed"
    with pytest.raises(AssertionError):
        w.P.prefill([(2, prefix - 6, 10)], w.rand(10, (heads + 2 * kv_heads) * HD))  # starts inside a shared page: refused before any launch
    w.alloc.check_invariants()


# ---- 5: ragged launches ----
RAGGED = {2: [(1, 40, 300), (0, 0, 2)],
          5: [(3, 100, 1), (0, 0, 300), (4, 17, 3), (1, 64, 64), (2, 5, 130)],
          16: [(15 - i, p, m) for i, (p, m) in enumerate([(0, 1), (3, 2), (16, 3), (0, 300), (100, 130), (37, 64), (64, 65), (1, 129), (200, 17), (0, 64), (63, 1), (128, 128), (5, 5),
                                                          (250, 40), (0, 200), (77, 33)])]}


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("page_keys", [16, 64, 256])
@pytest.mark.parametrize("nseg", [2, 5, 16])
def test_ragged_launch_equals_its_segments_one_at_a_time(dev, nseg, page_keys, causal):
    """One launch of 2 / 5 / 16 segments (m = 1 .. 3 beside m = 300, listed in another order than slot order) under the default rule against (a) the contiguous launch
    of each sequence alone and (b) the same segments through the paged call one at a time -- output rows and whole pools.  A ragged launch may pick another block form
    than a lone segment does: a key tile wholly behind a row's causal bound leaves that row's state bit-unchanged, so the forms agree bit for bit."""
    from tinychatengine_amd import capi
    capi.check(capi.lib().tce_w4a16_set_debug_mode(2950))
    heads, kv_heads = (32, 8) if nseg != 16 else (8, 2)
    segments = RAGGED[nseg]
    worlds = [_World(dev, heads, kv_heads, page_keys, nseg, 512, True, seed=nseg * 10 + page_keys) for _ in range(2)]  # the same seed: the same contents
    for w in worlds:
        for slot, pos, _ in sorted(segments):
            w.context(slot, pos)
    qkv, out_all = worlds[0].launch(segments, causal, f"{nseg} segments")
    w = worlds[1]
    for slot, pos, m in segments:
        w.alloc.reserve(slot, pos + m - 1)
    row0 = 0
    for slot, pos, m in segments:
        out_one = w.P.prefill([(slot, pos, m)], qkv[row0:row0 + m].contiguous(), causal=causal)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out_one), _bits(out_all[row0:row0 + m])), f"slot {slot}: one launch for all differs from a launch of its own"
        row0 += m
    assert worlds[0].alloc.pages == w.alloc.pages
    assert torch.equal(_bits(worlds[0].P.k_pool), _bits(w.P.k_pool)) and torch.equal(_bits(worlds[0].P.v_pool), _bits(w.P.v_pool))


# ---- 6: whole blocks ----
def _blocks(dev, hidden, heads, kv_heads, ffn, layers, max_keys, seed):
    from tinychatengine_amd.decoder_block import DecoderBlock
    cos, sin = _tables(max_keys, seed)
    tc, ts = torch.from_numpy(cos).to(dev), torch.from_numpy(sin).to(dev)
    return [DecoderBlock(hidden, heads, ffn, max_keys, dev, tc, ts, seed=seed + i, kv_heads=kv_heads) for i in range(layers)]


def _reference_prefill(dec, rows, segments):
    """BatchedDecoder.prefill's launches at M = all rows, composed here, with DecodeAttention.prefill per sequence on its row slice in the middle (contiguous caches)."""
    from tinychatengine_amd import capi
    from tinychatengine_amd.linear import _stream, rmsnorm_half
    blk = dec.block
    m = rows.shape[0]
    st = _stream()
    e = lambda n: torch.empty((m, n), dtype=torch.float16, device=rows.device)
    xn, qkv, attn, g, u = e(blk.hidden), e((blk.heads + 2 * blk.kv_heads) * 128), e(blk.hidden), e(blk.ffn), e(blk.ffn)
    rmsnorm_half(rows, blk.gamma1, blk.eps, out=xn)
    capi.check(capi.w4a16_forward(blk.qkv.desc(xn, qkv), st))
    row0 = 0
    for slot, pos, n in segments:
        dec.attention.slot(slot).prefill(qkv[row0:row0 + n], pos, out=attn[row0:row0 + n], causal=True)
        row0 += n
    capi.check(capi.w4a16_forward(blk.o.desc(attn, rows, flags=capi.TCE_W4_ADD_TO_C), st))
    rmsnorm_half(rows, blk.gamma2, blk.eps, out=xn)
    if m > 128 and blk.gate_up.packed is not None:
        capi.check(capi.w4a16_forward(blk.gate_up.desc(xn, g, flags=capi.TCE_W4_SILU_MUL_PAIRS), st))
    else:
        capi.check(capi.w4a16_forward(blk.gate.desc(xn, g), st))
        capi.check(capi.w4a16_forward(blk.up.desc(xn, u), st))
        capi.check(capi.lib().tce_silu_mul_half(g.data_ptr(), u.data_ptr(), g.numel(), st))
    capi.check(capi.w4a16_forward(blk.down.desc(g, rows, flags=capi.TCE_W4_ADD_TO_C), st))


@pytest.mark.parametrize("hidden,heads,kv_heads,ffn,layers", [(512, 4, 1, 1408, 2), (4096, 32, 8, 14336, 1)])
def test_prefill_many_equals_the_composed_reference_then_decodes(dev, hidden, heads, kv_heads, ffn, layers):
    from tinychatengine_amd.batch_decode import BatchedDecoder
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchedDecoder, PagePoolExhausted
    batch, max_keys, page_keys = 4, 128, 16
    blocks = _blocks(dev, hidden, heads, kv_heads, ffn, layers, max_keys, 90 + hidden)
    cont = [BatchedDecoder(b, batch) for b in blocks]
    num_pages = 20
    alloc = PageAllocator(num_pages, page_keys, batch, max_keys // page_keys, dev, free_order=np.random.default_rng(17).permutation(num_pages).tolist())
    paged = [PagedBatchedDecoder(b, alloc) for b in blocks]
    rng = np.random.default_rng(hidden)
    prompts = [(2, 30), (0, 2), (3, 45), (1, 7)]  # (slot, rows): listed in another order than slot order
    xs = [torch.from_numpy(rng.standard_normal((m, hidden)).astype(np.float16)).to(dev) for _, m in prompts]
    # all or nothing: 16 sequences' worth of pages do not fit -- nothing changes
    with pytest.raises(PagePoolExhausted):
        paged[0].prefill_many([(s, torch.zeros((100, hidden), dtype=torch.float16, device=dev), 0) for s in range(4)])
    assert alloc.pages_in_use() == 0 and all(not p for p in alloc.pages)
    ref_rows = torch.cat(xs)
    segments = [(slot, 0, m) for slot, m in prompts]
    for d in cont:
        _reference_prefill(d, ref_rows, segments)
    mine = [x.clone() for x in xs]
    for d in paged:
        d.prefill_many([(slot, rows, 0) for (slot, _), rows in zip(prompts, mine)])
        assert d.attention._staging is None, "prefill created a staging cache"
    torch.cuda.synchronize()
    row0 = 0
    for (slot, m), rows in zip(prompts, mine):
        assert torch.equal(_bits(rows), _bits(ref_rows[row0:row0 + m])), f"slot {slot}: prefill_many's rows differ from the composed reference"
        row0 += m
    alloc.check_invariants()
    pos = np.zeros(batch, np.int32)
    for slot, m in prompts:
        pos[slot] = m
    pos_t = torch.from_numpy(pos).to(dev)
    h_c = torch.zeros((batch, hidden), dtype=torch.float16, device=dev)
    h_p = torch.zeros_like(h_c)
    for t in range(20):
        for b in range(batch):
            alloc.reserve(b, int(pos[b]))
        x = torch.from_numpy(rng.standard_normal((batch, hidden)).astype(np.float16)).to(dev)
        h_c.copy_(x)
        h_p.copy_(x)
        pos_t.copy_(torch.from_numpy(pos))
        assert paged[0].attention.table_violations(pos_t, max_keys - 1) == 0
        for d in cont:
            d.step(h_c, pos_t, max_keys - 1)
        for d in paged:
            d.step(h_p, pos_t, max_keys - 1)
        torch.cuda.synchronize()
        assert torch.equal(_bits(h_c), _bits(h_p)), f"decode step {t}: hidden rows differ"
        pos += 1
    for dc, dp in zip(cont, paged):
        for b in range(batch):
            k, v = dp.attention.read_back(b, int(pos[b]))
            assert torch.equal(_bits(k), _bits(dc.attention.k_cache[b, :, :pos[b]])) and torch.equal(_bits(v), _bits(dc.attention.v_cache[b, :, :pos[b]]))


def test_prefill_is_prefill_many_of_one_and_uses_no_staging_cache(dev):
    """PagedBatchedDecoder.prefill on top of cached keys (a second chunk): bit-identical to BatchedDecoder.prefill on the contiguous cache, no staging cache made."""
    from tinychatengine_amd.batch_decode import BatchedDecoder
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchedDecoder
    hidden, heads, kv_heads, ffn = 512, 4, 1, 1408
    blocks = _blocks(dev, hidden, heads, kv_heads, ffn, 2, 256, 5)
    cont = [BatchedDecoder(b, 2) for b in blocks]
    alloc = PageAllocator(20, 16, 2, 16, dev, free_order=np.random.default_rng(3).permutation(20).tolist())
    paged = [PagedBatchedDecoder(b, alloc) for b in blocks]
    rng = np.random.default_rng(8)
    pos = 0
    for m in (70, 150, 3):
        x = torch.from_numpy(rng.standard_normal((m, hidden)).astype(np.float16)).to(dev)
        rows_c, rows_p = x.clone(), x.clone()
        for d in cont:
            d.prefill(1, rows_c, pos)
        for d in paged:
            d.prefill(1, rows_p, pos)
        torch.cuda.synchronize()
        assert torch.equal(_bits(rows_c), _bits(rows_p)), f"chunk at {pos}"
        pos += m
    assert all(d.attention._staging is None for d in paged)


# ---- 7: float64, a guard against both sides of the bit comparisons being wrong together ----
def test_ragged_launch_against_float64(dev, oracle):
    """The project's bound for prefill (tests/test_gpu_attention.py): |out - ref| <= 2e-3 max|ref| per head and row + 2^-11 |ref|."""
    heads, kv_heads, page_keys, max_keys = 8, 2, 32, 512
    rep = heads // kv_heads
    w = _World(dev, heads, kv_heads, page_keys, 4, max_keys, True, seed=64)
    cos, sin = w.P.cos.cpu().numpy(), w.P.sin.cpu().numpy()
    segments = [(2, 37, 130), (0, 0, 3), (3, 100, 1), (1, 64, 65)]
    for slot, pos, _ in segments:
        w.context(slot, pos)
    before = {slot: (w.cont[slot].k_cache.cpu().numpy().copy(), w.cont[slot].v_cache.cpu().numpy().copy()) for slot, _, _ in segments}
    qkv_t, out = w.launch(segments, True, "float64 case")
    qkv, got_all = qkv_t.cpu().numpy(), out.cpu().numpy().astype(np.float64)
    alpha = float(np.float16(1.0 / np.sqrt(HD)))
    row0 = 0
    for slot, pos, m in segments:
        x = qkv[row0:row0 + m]
        q = np.ascontiguousarray(x[:, :heads * HD].reshape(m, heads, HD).transpose(1, 0, 2))
        k = np.ascontiguousarray(x[:, heads * HD:(heads + kv_heads) * HD].reshape(m, kv_heads, HD).transpose(1, 0, 2))
        v = x[:, (heads + kv_heads) * HD:].reshape(m, kv_heads, HD).transpose(1, 0, 2)
        q_rot, _ = oracle.rope_half(q, q, cos, sin, pos)
        _, k_rot = oracle.rope_half(k, k, cos, sin, pos)
        Kc, Vc = before[slot]
        Kc[:, pos:pos + m] = k_rot
        Vc[:, pos:pos + m] = v
        k_pages, v_pages = w.P.read_back(slot, pos + m)
        assert np.array_equal(k_pages.cpu().numpy().view(np.uint16), Kc[:, :pos + m].view(np.uint16)), "the pages do not hold the reference's rotated keys"
        assert np.array_equal(v_pages.cpu().numpy().view(np.uint16), Vc[:, :pos + m].view(np.uint16))
        Kr, Vr = np.repeat(Kc[:, :pos + m], rep, axis=0).astype(np.float64), np.repeat(Vc[:, :pos + m], rep, axis=0).astype(np.float64)
        got = got_all[row0:row0 + m].reshape(m, heads, HD)
        for r in range(m):
            s = alpha * np.einsum("hd,hkd->hk", q_rot[:, r].astype(np.float64), Kr)
            s[:, pos + r + 1:] = -np.inf
            s = s - s.max(axis=1, keepdims=True)
            p = np.exp(s)
            p /= p.sum(axis=1, keepdims=True)
            ref = np.einsum("hk,hkd->hd", p, Vr)
            tol = 2e-3 * np.abs(ref).max(axis=1, keepdims=True) + 2.0 ** -11 * np.abs(ref)
            err = (np.abs(got[r] - ref) / tol).max()
            assert err <= 1.0, f"slot {slot} row {r}: worst |err| / tol = {err:.3f}"
        row0 += m
