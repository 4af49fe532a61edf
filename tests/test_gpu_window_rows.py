"""Sliding windows on the multi-row (speculative) step and on admission (csrc/attention_fast.hip: attn_decode_fast_kernel with ROWS && WINDOW;
tinychatengine_amd/speculative.py, generate.py).

(a) tce_attention_decode_step_paged_rows_window_f16 / _fp8: row (b, t) and the appended pool rows are BIT-IDENTICAL to t + 1 successive calls of the windowed single
    step on a copy of the same pools; every other pool byte is unchanged.  W from 1 to 2 * page_keys + 3, T = 1, 2, 5, 8, start positions where the window's first
    key crosses a group of four or a page, where the window lies inside the call's own rows, where it does not bind yet, and 0; one sequence inactive, one with a
    prefix of n < T rows; a window of several chunk slots (the combine, a workspace slice per virtual row).
(b) a window that never binds: the unwindowed rows step, bit for bit.
(c) released pages: the words below the window's first name no page and the released pages hold NaNs -- the outputs do not change.
(d) SpeculativeGenerator over windowed layers on a pool smaller than the sequences: BatchedGenerator's tokens, id for id, all drafts right and half of them wrong.
(e) admit(..., chunk_rows=N): a prompt longer than the pool is admitted, and generates what the same chunking generates on a pool that holds everything.
There is no tolerance anywhere in this file."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HD, HEADS, KV_HEADS, PAGE_KEYS, B = 128, 8, 2, 16, 3
MAX_KEYS = 128
BOUND = MAX_KEYS - 1
WINDOWS = (1, 2, 3, 5, 8, PAGE_KEYS, PAGE_KEYS + 1, 2 * PAGE_KEYS + 3)
ROWS = (1, 2, 5, 8)
NAN16 = [0x7E00, 0x7D55, -512 + 1, 0x7FFF]


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


def _raw(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.uint8)


def _rope_tables(n, seed, dev):
    ang = np.random.default_rng(seed).uniform(0, 2 * np.pi, (n, HD // 2))
    cos = np.concatenate([np.cos(ang), np.cos(ang)], axis=1).astype(np.float16)
    sin = np.concatenate([np.sin(ang), np.sin(ang)], axis=1).astype(np.float16)
    return torch.from_numpy(cos).to(dev), torch.from_numpy(sin).to(dev)


def _lo(pos, W):
    return max(0, pos - W + 1)


def start_positions(W: int) -> list[int]:
    """Row 0's position for the cases of (a), by the property the rows then have (lo_t = max(0, p + t - W + 1)):
        0                 the first token; with W <= t the window lies wholly inside the call's rows
        W - 2             p < W: the window starts to bind inside the call (W >= 2)
        W + 2             lo_0 = 3, lo_1 = 4: lo crosses a group of four, base_t moves
        W + PAGE_KEYS - 2 lo_0 = 15, lo_1 = 16: lo crosses a page, the first followed table word moves
        2 * PAGE_KEYS - 2 the rows themselves cross a page (two appends in one page, the rest in the next)"""
    return sorted({0, max(0, W - 2), W + 2, W + PAGE_KEYS - 2, 2 * PAGE_KEYS - 2})


def test_the_start_positions_have_the_properties_they_are_chosen_for():
    for W in WINDOWS:
        ps = start_positions(W)
        assert 0 in ps and any(p < W for p in ps)
        assert any(_lo(p, W) % 4 == 3 and _lo(p + 1, W) % 4 == 0 for p in ps), W
        assert any(_lo(p, W) // PAGE_KEYS != _lo(p + 1, W) // PAGE_KEYS for p in ps), W
        assert max(ps) + max(ROWS) - 1 <= BOUND
    assert any(W <= t for W in WINDOWS for t in range(max(ROWS))), "no case with the window inside the call"


def _fill(R, g, fp8, dev):
    if fp8:
        fill = torch.randint(0, 256, R.k_pool.shape, generator=g, device=dev, dtype=torch.int32)
        fill = torch.where((fill & 0x7F) == 0x7F, fill - 1, fill).to(torch.uint8)  # (no NaN bytes among the cached rows)
        R.k_pool.copy_(fill)
        R.v_pool.copy_(fill.flip(0))
    else:
        R.k_pool.copy_((torch.randn(R.k_pool.shape, generator=g, device=dev) * 0.8).half())
        R.v_pool.copy_((torch.randn(R.v_pool.shape, generator=g, device=dev) * 0.8).half())


def _poison(pools, page, fp8, dev):
    for pool in pools:
        if fp8:
            pool[page].fill_(0x7F)
        else:
            v = pool.view(torch.int16)[page]
            v.copy_(torch.tensor(NAN16, dtype=torch.int16, device=dev).repeat(v.numel() // 4).view(v.shape))


class _Case:
    """One launch of (a): slot 0 runs T rows from p0, slot 1 is inactive, slot 2 a prefix of max(1, T - 1) rows from p2.  R: the rows-window attention; S: the
    windowed single step (unwindowed_rows: the UNWINDOWED rows step, for (b)) with pools of its own, made a copy of R's by sync_pools."""

    def __init__(self, dev, kv_dtype, W, T, p0, p2, seed, max_keys=MAX_KEYS, unwindowed_rows=False, rope=True):
        from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchDecodeAttention
        from tinychatengine_amd.speculative import PagedRowsDecodeAttention
        self.fp8 = fp8 = kv_dtype == "fp8_e4m3"
        scales = dict(kv_dtype=kv_dtype, k_scale_log2=-1, v_scale_log2=-2) if fp8 else {}
        self.dev, self.W, self.T, self.bound = dev, W, T, max_keys - 1
        cos, sin = _rope_tables(max_keys, max_keys + W, dev) if rope else (None, None)
        stride = max_keys // PAGE_KEYS
        g = torch.Generator(device=dev).manual_seed(seed)
        num_pages = B * stride + 3
        self.alloc = alloc = PageAllocator(num_pages, PAGE_KEYS, B, stride, dev, free_order=np.random.default_rng(seed).permutation(num_pages).tolist())
        self.R = PagedRowsDecodeAttention(alloc, HEADS, KV_HEADS, dev, cos, sin, rows_per_seq=T, window=W, **scales)
        if unwindowed_rows:
            self.S = PagedRowsDecodeAttention(alloc, HEADS, KV_HEADS, dev, cos, sin, rows_per_seq=T, **scales)
        else:
            self.S = PagedBatchDecodeAttention(alloc, HEADS, KV_HEADS, dev, cos, sin, window=W, **scales)
        _fill(self.R, g, fp8, dev)
        self.n_act = [T, 0, max(1, T - 1)]
        self.pos = np.full((B, T), -1, np.int32)
        for b, p in ((0, p0), (2, p2)):
            self.pos[b, :self.n_act[b]] = p + np.arange(self.n_act[b])
            alloc.reserve(b, p + self.n_act[b] - 1)
        # a page of NaNs behind every table word the slots do not hold
        self.canary = alloc.free[0]
        _poison((self.R.k_pool, self.R.v_pool), self.canary, fp8, dev)
        table = torch.full_like(alloc.table, self.canary)
        for b, ps in enumerate(alloc.pages):
            if ps:
                table[b, :len(ps)] = torch.tensor(ps, dtype=torch.int32, device=dev)
        alloc.table.copy_(table)
        self.qkv = (torch.randn((B * T, (HEADS + 2 * KV_HEADS) * HD), generator=g, device=dev) * 0.9).half()
        self.pos_t = torch.from_numpy(self.pos.reshape(-1)).to(dev)

    def sync_pools(self):
        self.S.k_pool.copy_(self.R.k_pool)
        self.S.v_pool.copy_(self.R.v_pool)

    def successive(self):
        """The yardstick: T successive windowed single steps on S's pools."""
        want = torch.empty((B, self.T, HEADS * HD), dtype=torch.float16, device=self.dev)
        for t in range(self.T):
            pt = torch.from_numpy(self.pos[:, t].copy()).to(self.dev)
            want[:, t] = self.S.step(self.qkv.view(B, self.T, -1)[:, t].contiguous(), pt, self.bound)
        return want

    def rows(self):
        out = torch.full((B * self.T, HEADS * HD), 3.0, dtype=torch.float16, device=self.dev)
        self.R.step(self.qkv, self.pos_t, self.bound, out=out)
        return out.view(B, self.T, -1)

    def appended(self):
        allowed = torch.zeros(self.R.k_pool.shape[:3], dtype=torch.bool, device=self.dev)  # [page][head][row]
        for b in (0, 2):
            for t in range(self.n_act[b]):
                p = int(self.pos[b, t])
                allowed[self.alloc.pages[b][p // PAGE_KEYS - self.alloc.gone[b]], :, p % PAGE_KEYS] = True
        return allowed


def _check_bit_identity(c, what):
    c.sync_pools()
    k0, v0 = c.R.k_pool.clone(), c.R.v_pool.clone()
    assert c.R.table_violations(c.pos_t, c.bound) == 0, f"{what}: the block table is not sound: no launch"
    want = c.successive()
    out = c.rows()
    torch.cuda.synchronize()
    assert not torch.isnan(out.float()).any(), f"{what}: a NaN page leaked into an output"
    assert torch.equal(_raw(out), _raw(want)), f"{what}: output rows differ from the successive windowed steps'"
    assert torch.equal(_raw(out[1]), torch.zeros_like(_raw(out[1]))), f"{what}: the inactive sequence's rows are not zero"
    assert torch.equal(_raw(c.R.k_pool), _raw(c.S.k_pool)) and torch.equal(_raw(c.R.v_pool), _raw(c.S.v_pool)), f"{what}: the pools differ from the single steps'"
    changed = (_raw(c.R.k_pool) != _raw(k0)).any(-1) | (_raw(c.R.v_pool) != _raw(v0)).any(-1)
    assert not (changed & ~c.appended()).any(), f"{what}: a pool row other than the appended ones changed"


# =====================================================================================================================================================
# (a) the rows-window step against successive windowed steps
# =====================================================================================================================================================
@pytest.mark.parametrize("kv_dtype", ["fp16", "fp8_e4m3"])
@pytest.mark.parametrize("T", ROWS)
def test_rows_window_step_equals_successive_windowed_steps(dev, T, kv_dtype):
    from tinychatengine_amd import capi
    for W in WINDOWS:
        assert capi.describe_attention_paged_window(B, HEADS, KV_HEADS, BOUND, PAGE_KEYS, W)["chunks"] == 1
        ps = start_positions(W)
        for i, p0 in enumerate(ps):
            p2 = ps[(i + 2) % len(ps)]  # each sequence of the batch a different case
            c = _Case(dev, kv_dtype, W, T, p0, p2, seed=1000 * W + 10 * T + i)
            _check_bit_identity(c, f"{kv_dtype} W={W} T={T} starts=({p0}, {p2})")
            del c


@pytest.mark.parametrize("kv_dtype", ["fp16", "fp8_e4m3"])
def test_rows_window_step_over_several_chunk_slots(dev, kv_dtype):
    """W + 3 = 403 keys: four chunk slots, so every virtual row's partial states go through its own workspace slice and the last workgroup combines them; the first
    start leaves the later chunk slots of the early rows without keys, the second has lo > 0 in every row."""
    from tinychatengine_amd import capi
    W, max_keys = 400, 1024
    cut = capi.describe_attention_paged_window(B, HEADS, KV_HEADS, max_keys - 1, PAGE_KEYS, W)
    assert cut["chunks"] == 4 and cut["combine"] == "yes"
    for T, p0, p2 in ((5, 110, 398), (8, 637, 1003), (2, 1022, 401)):
        c = _Case(dev, kv_dtype, W, T, p0, p2, seed=W + T, max_keys=max_keys)
        _check_bit_identity(c, f"{kv_dtype} W={W} T={T} starts=({p0}, {p2})")
        _check_bit_identity(c, f"{kv_dtype} W={W} T={T} starts=({p0}, {p2}), the same workspace again")  # (the arrival counters went back to zero)
        del c


def test_rows_window_step_without_rope_and_with_one_row(dev):
    """No cos / sin tables (the keys enter the pool unrotated), and rows_per_seq = 1: the windowed step itself."""
    for W, T, p0, p2 in ((5, 5, 7, 20), (PAGE_KEYS + 1, 1, 31, 2)):
        c = _Case(dev, "fp16", W, T, p0, p2, seed=77 + W, rope=False)
        _check_bit_identity(c, f"no rope W={W} T={T}")
        del c


# =====================================================================================================================================================
# (b) a window that never binds
# =====================================================================================================================================================
@pytest.mark.parametrize("kv_dtype", ["fp16", "fp8_e4m3"])
def test_a_rows_step_with_a_window_that_never_binds_is_the_rows_step(dev, kv_dtype):
    for T, p0, p2 in ((1, 0, 127), (2, 14, 61), (5, 30, 0), (8, 120, 63)):  # (120 + 7 = the bound: the last row still active)
        c = _Case(dev, kv_dtype, BOUND + 1, T, p0, p2, seed=500 + T, unwindowed_rows=True)
        c.sync_pools()
        want = torch.full((B * T, HEADS * HD), 5.0, dtype=torch.float16, device=dev)
        c.S.step(c.qkv, c.pos_t, BOUND, out=want)
        out = c.rows()
        torch.cuda.synchronize()
        what = f"{kv_dtype} T={T} starts=({p0}, {p2})"
        assert torch.equal(_raw(out), _raw(want.view(B, T, -1))), f"{what}: window = pos_bound + 1 is not the unwindowed rows step"
        assert torch.equal(_raw(c.R.k_pool), _raw(c.S.k_pool)) and torch.equal(_raw(c.R.v_pool), _raw(c.S.v_pool)), what
        del c


# =====================================================================================================================================================
# (c) released pages
# =====================================================================================================================================================
@pytest.mark.parametrize("kv_dtype", ["fp16", "fp8_e4m3"])
def test_released_pages_and_the_words_below_the_window_are_never_followed(dev, kv_dtype):
    """W = page_keys + 1 at starts 46 and 78: lo_0 = 30 and 62, so words 0 (and 0 .. 2) lie below every row's window.  Their pages are given back and filled with NaNs
    and the words are set to num_pages, which is no page: the contract says they never become addresses, so the outputs are those of the untouched table."""
    W, T, p0, p2 = PAGE_KEYS + 1, 5, 46, 78
    c = _Case(dev, kv_dtype, W, T, p0, p2, seed=4242)
    c.sync_pools()
    want = c.successive()
    torch.cuda.synchronize()
    below = {0: _lo(p0, W) // PAGE_KEYS, 2: _lo(p2, W) // PAGE_KEYS}
    assert below == {0: 1, 2: 3}
    for b, n in below.items():
        gone = c.alloc.release_behind(b, n * PAGE_KEYS)
        assert len(gone) == n
        for page in gone:
            _poison((c.R.k_pool, c.R.v_pool), page, c.fp8, dev)
        c.alloc.table[b, :n] = c.alloc.num_pages
    c.alloc.check_invariants()
    assert c.R.table_violations(c.pos_t, c.bound) == 0, "the check counts a word no row follows"
    out = c.rows()
    torch.cuda.synchronize()
    assert not torch.isnan(out.float()).any(), "a released page was weighted"
    assert torch.equal(_raw(out), _raw(want)), "the outputs changed with the words below the window"


# =====================================================================================================================================================
# (d), (e) generation
# =====================================================================================================================================================
VOCAB, GEN_KEYS, GEN_W, GEN_T, GEN_BURST, GEN_NEW = 4096, 256, 24, 4, 2, 150
GEN_PER_SLOT = (GEN_W + GEN_BURST * GEN_T + PAGE_KEYS - 1) // PAGE_KEYS + 1  # ceil((W + n T) / page_keys) + 1 = 3
GEN_PAGES = B * GEN_PER_SLOT  # 9 pages = 144 keys: fewer than one finished sequence (prompt + 150)


class _Model:
    """hidden 1024, heads 8 / 2, ffn 1408, two layers, synthetic weights on a 256-key table (tests/test_gpu_generate.py's small model with this file's heads)."""

    def __init__(self, dev, seed=52):
        from tinychatengine_amd.decoder_block import DecoderBlock
        from tinychatengine_amd.linear import Linear_half_int4
        hidden, ffn, layers = HEADS * HD, 1408, 2
        cos, sin = _rope_tables(GEN_KEYS, seed, dev)
        self.dev = dev
        self.blocks = [DecoderBlock(hidden, HEADS, ffn, GEN_KEYS, dev, cos, sin, seed=seed + i, kv_heads=KV_HEADS) for i in range(layers)]
        g = torch.Generator(device=dev).manual_seed(seed + 100)
        self.final_gamma = (1.0 + 0.1 * torch.empty(hidden, device=dev).normal_(0, 1, generator=g)).float()
        self.lm_head = Linear_half_int4.from_float(torch.empty(VOCAB, hidden, device=dev).normal_(0.0, hidden ** -0.5, generator=g)).prepack()
        self.table = torch.empty(VOCAB, hidden, device=dev).normal_(0.0, 1.0, generator=g).half()

    def allocator(self, num_pages, batch=B):
        from tinychatengine_amd.paged_kv import PageAllocator
        return PageAllocator(num_pages, PAGE_KEYS, batch, GEN_KEYS // PAGE_KEYS, self.dev, free_order=np.random.default_rng(num_pages).permutation(num_pages).tolist())

    def plain(self, num_pages, window=GEN_W, max_new=GEN_NEW, batch=B):
        from tinychatengine_amd.generate import BatchedGenerator
        from tinychatengine_amd.paged_kv import PagedBatchedDecoder
        alloc = self.allocator(num_pages, batch)
        return BatchedGenerator([PagedBatchedDecoder(b, alloc, window=window) for b in self.blocks], self.final_gamma, self.lm_head, self.table, max_new=max_new)

    def speculative(self, num_pages, T=GEN_T, window=GEN_W, max_new=GEN_NEW):
        from tinychatengine_amd.speculative import SpeculativeDecoder, SpeculativeGenerator
        alloc = self.allocator(num_pages)
        return SpeculativeGenerator([SpeculativeDecoder(b, alloc, T, window=window) for b in self.blocks], self.final_gamma, self.lm_head, self.table, max_new=max_new,
                                    script=True)


@pytest.fixture(scope="module")
def model(dev):
    return _Model(dev)


def _rows_do_not_depend_on_their_index(m):
    """w4a16_forward on the model's linears at M = B T with the rows permuted gives the permuted bits (tests/test_gpu_speculative.py's check, at this file's M)."""
    from tinychatengine_amd import capi
    from tinychatengine_amd.linear import _stream
    M = B * GEN_T
    g = torch.Generator(device=m.dev).manual_seed(3)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(M)).to(m.dev)
    blk = m.blocks[0]
    for lin in (m.lm_head, blk.qkv, blk.o, blk.gate, blk.up, blk.down):
        x = torch.randn((M, lin.in_features), generator=g, device=m.dev).half()
        y1 = torch.empty((M, lin.out_features), dtype=torch.float16, device=m.dev)
        y2 = torch.empty_like(y1)
        capi.check(capi.w4a16_forward(lin.desc(x, y1), _stream()))
        capi.check(capi.w4a16_forward(lin.desc(x[perm].contiguous(), y2), _stream()))
        torch.cuda.synchronize()
        if not torch.equal(_raw(y2), _raw(y1[perm])):
            return False
    return True


@pytest.fixture(scope="module")
def plain_run(model):
    """The reference of (d), computed once: BatchedGenerator over the same windowed layers, greedy, the B sequences in slots 0, T, 2 T of B T slots.
    Why B T slots: "id for id" needs the linears of both generators to compute a row with the same arithmetic, and the dispatcher picks the kernel by M -- at this
    model's shapes the int8 GEMV up to M = 4 and the small-batch kernel above, whose rows differ in the last bits (measured on an MI355X: qkv, o, down and lm_head
    at M = 3 against the same rows at M = 12 differ; with a 3-slot BatchedGenerator slot 0's token 16 of 150 came out 459 instead of 2286, with and without drafts
    and with every attention contract of this file holding; with 12 slots all 3 x 150 tokens agree).  The speculative generator runs its linears at M = B T = 12,
    so the plain one is given 12 slots: the same launches, the same kernels, three live sequences."""
    from tinychatengine_amd.generate import SamplingParams
    assert _rows_do_not_depend_on_their_index(model), "a row's logits depend on its index in the M = B T launch: plain decoding is no reference for rows t > 0"
    greedy = SamplingParams(temp=0.0, repeat_penalty=1.0)
    rng = np.random.default_rng(91)
    prompts = [rng.integers(0, VOCAB, n).tolist() for n in (10, 3, 21)]
    adm = [(s, prompts[s], greedy, 0, GEN_NEW) for s in range(B)]
    gen = model.plain(GEN_PAGES, batch=B * GEN_T)
    gen.admit([(s * GEN_T, ids, p, sd, mn) for s, ids, p, sd, mn in adm])
    while gen.book.live():
        gen.run(8)
        gen.allocator.check_invariants()
    tokens = [gen.tokens(s * GEN_T) for s in range(B)]
    assert all(len(t) == GEN_NEW for t in tokens)
    return adm, prompts, tokens


@pytest.mark.parametrize("drafts", ["all_correct", "half_wrong"])
def test_speculative_generation_with_windows_on_a_small_pool(dev, model, plain_run, drafts):
    from tinychatengine_amd.paged_kv import PagePoolExhausted
    adm, prompts, plain = plain_run
    assert GEN_PAGES * PAGE_KEYS < min(len(p) for p in prompts) + GEN_NEW, "the pool must be smaller than every finished sequence"
    spec = model.speculative(GEN_PAGES)
    assert all(d.window == GEN_W and d.rows_per_seq == GEN_T for d in spec.decoders)
    for s in range(B):
        wrong = set(range(1, GEN_NEW, 2)) if drafts == "half_wrong" else set()
        spec.set_script(s, [-1] * len(prompts[s]) + [(t + 1) % VOCAB if i in wrong else t for i, t in enumerate(plain[s])])
    spec.admit(adm)
    retired, runs = [], 0
    while len(retired) < B:
        try:
            retired += spec.run(GEN_BURST)
        except PagePoolExhausted as e:  # (stated, not left to the traceback: this is the claim under test)
            pytest.fail(f"run() on {GEN_PAGES} pages after {runs} bursts: {e}")
        runs += 1
        spec.allocator.check_invariants()
        for s in spec.book.live():
            assert len(spec.allocator.pages[s]) <= GEN_PER_SLOT, f"slot {s} holds {len(spec.allocator.pages[s])} pages"
        assert runs <= GEN_NEW
    for s in range(B):
        assert spec.tokens(s) == plain[s], f"slot {s} ({drafts}): the speculative run differs from BatchedGenerator over the same windowed layers"
    em = spec.emitted_per_step()
    if drafts == "all_correct":
        assert em.max() == GEN_T and runs * GEN_BURST < GEN_NEW // 2, "the drafts were not accepted: the run proves nothing about rows t > 0"
    else:
        assert em.max() == 2 and (em == 2).sum() > GEN_NEW // 4, "every other draft should have been accepted"
    assert spec.embed_violations() == 0
    for s in range(B):
        spec.release(s)
    assert spec.allocator.pages_in_use() == 0
    spec.allocator.check_invariants()


CHUNK = GEN_W // 2 + 1  # 13
PROMPT = 3 * GEN_W + 5  # 77 tokens: five pages
ADMIT_PER_SLOT = (GEN_W + CHUNK + PAGE_KEYS - 1) // PAGE_KEYS + 1  # 4


@pytest.mark.parametrize("front", ["batched", "speculative"])
def test_chunked_admission_takes_a_prompt_longer_than_the_pool(dev, model, front):
    from tinychatengine_amd.generate import SamplingParams
    from tinychatengine_amd.paged_kv import PagePoolExhausted
    greedy = SamplingParams(temp=0.0, repeat_penalty=1.0)
    prompt = np.random.default_rng(17).integers(0, VOCAB, PROMPT).tolist()
    small_pages = ADMIT_PER_SLOT
    assert small_pages < (PROMPT + PAGE_KEYS - 1) // PAGE_KEYS, "the pool must hold fewer pages than the prompt needs"
    make = (lambda n: model.plain(n, max_new=16)) if front == "batched" else (lambda n: model.speculative(n, max_new=16))
    burst = 8 if front == "batched" else 1  # (speculative, an all -1 script: one token per replay, and a replay reserves T keys ahead)

    def tokens(gen):
        """the first token and 8 steps' tokens"""
        out = []
        while len(out) < 9 and gen.book.live():
            gen.run(burst)
            gen.allocator.check_invariants()
            out = gen.tokens(0)
        return out[:9]

    small = make(small_pages)
    with pytest.raises(PagePoolExhausted):
        small.admit(0, prompt, greedy, 0, 16)
    assert small.allocator.pages_in_use() == 0 and small.book.live() == []
    assert small.admit(0, prompt, greedy, 0, 16, chunk_rows=CHUNK) == []
    assert len(small.allocator.pages[0]) <= ADMIT_PER_SLOT, f"{len(small.allocator.pages[0])} pages right after admit"
    assert small.allocator.gone[0] >= 1 and small.book.pos[0] == PROMPT
    small.allocator.check_invariants()
    got = tokens(small)

    big = make(B * (GEN_KEYS // PAGE_KEYS))
    assert big.admit(0, prompt, greedy, 0, 16, chunk_rows=CHUNK) == []
    want = tokens(big)
    assert len(want) == 9 and got == want, f"{front}: the small pool's tokens differ from the same chunked admission on a pool that holds everything"

    # a later chunk that finds no page: the slots of the call are released, everything else is as before
    held = small.allocator.pages_in_use()
    free_before, pos_before = sorted(small.allocator.free), small.pos.clone()
    with pytest.raises(PagePoolExhausted):
        small.admit(1, prompt, greedy, 0, 16, chunk_rows=CHUNK)
    assert small.allocator.pages_in_use() == held and small.allocator.pages[1] == [] and small.allocator.gone[1] == 0
    assert sorted(small.allocator.free) == free_before and torch.equal(small.pos, pos_before) and small.book.live() == [0]
    small.allocator.check_invariants()
