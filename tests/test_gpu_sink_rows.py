"""Attention sinks on the multi-row (speculative) step (csrc/attention_rows_sink.hip: attn_decode_fast_kernel with ROWS && WINDOW && SINK; include/tce_matmul.h,
"ATTENTION SINKS", rows).

(a) tce_attention_decode_step_paged_rows_sink_f16 / _fp8: row (b, t) and the appended pool rows are BIT-IDENTICAL to t + 1 successive calls of the one-row sink step on
    a copy of the same pools; every other pool byte is unchanged.  T = 1, 2, 5, 8; W = 8, 9, 16, 17, 35; S = 1, 4, 5, 16; start positions where the rows straddle the
    bind threshold, where every row binds and the window abuts the sinks, where the window's first key crosses a group of four and a page, where the rows cross a
    page, and 0; one sequence inactive, one with a prefix of n < T rows; a cut of several chunk slots (the combine, a workspace slice per virtual row); no RoPE.
(b) sinks + window that never bind: the unwindowed rows step, bit for bit.
(c) released pages: the words between word 0 and the window's first name a page of NaNs and the released pages hold NaNs -- the outputs do not change.
(d) one captured rows-sink step replayed while release_behind(..., keep_pages=1) gives pages back.
There is no tolerance anywhere in this file."""
import numpy as np
import pytest

from test_gpu_window import _Pair
from test_gpu_window_rows import _fill, _poison, _raw, _rope_tables

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HD, HEADS, KV_HEADS, PAGE_KEYS, B = 128, 8, 2, 16, 3
MAX_KEYS = 128
BOUND = MAX_KEYS - 1
WINDOWS = (8, 9, 16, 17, 35)
SINKS = (1, 4, 5, 16)
ROWS = (1, 2, 5, 8)


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


def _binds(pos, W, S):
    return pos >= S + W


def _lo(pos, W, S):
    """the first window key a row at `pos` weighs (0: the row does not bind and weighs every key)"""
    return pos - W + 1 if _binds(pos, W, S) else 0


def start_positions(W: int, S: int) -> list[int]:
    """Row 0's position for the cases of (a), by the property the rows then have:
        0                     the first token: no row binds, every key comes from the call itself
        S + W - 2             rows 0 and 1 do not bind, row 2 does: the threshold lies inside one call (T >= 3; with T = 2 the call ends at the last row that does not bind)
        S + W                 every row binds, and the window abuts the sinks: lo_0 = S + 1, the first key behind them that weighs nothing is S alone.  S = 5: lo_0 = 6,
                              the window's first group of four (4 .. 7) starts below S4 = 8 -- the virtual sequence is longer than pos + 1
        W - 1 + 15 (or + 31)  lo_0 = 15 (31 where S > 14), lo_1 = 16 (32): lo crosses a group of four AND a page -- base2 and the first followed window word move
        the first p >= S + W with p % 16 == 14   binding rows that cross a page themselves (two appends in one page, the rest in the next)"""
    edge = 15 if S <= 14 else 31
    cross = next(p for p in range(S + W, S + W + PAGE_KEYS) if p % PAGE_KEYS == PAGE_KEYS - 2)
    return sorted({0, S + W - 2, S + W, W - 1 + edge, cross})


def test_the_start_positions_have_the_properties_they_are_chosen_for():
    for W in WINDOWS:
        assert W >= max(ROWS), "the shape rule: window >= rows_per_seq"
        for S in SINKS:
            ps = start_positions(W, S)
            assert 0 in ps
            assert any(not _binds(p, W, S) and not _binds(p + 1, W, S) and _binds(p + 2, W, S) for p in ps), (W, S)  # straddles the threshold inside one call
            assert any(_binds(p, W, S) and _lo(p, W, S) == S + 1 for p in ps), (W, S)  # every row binds, the window abuts the sinks
            assert any(_binds(p, W, S) and _lo(p, W, S) % 4 == 3 and _lo(p + 1, W, S) % 4 == 0 for p in ps), (W, S)  # lo crosses a group of four
            assert any(_binds(p, W, S) and _lo(p, W, S) // PAGE_KEYS != _lo(p + 1, W, S) // PAGE_KEYS for p in ps), (W, S)  # lo crosses a page
            assert any(_binds(p, W, S) and p // PAGE_KEYS != (p + 2) // PAGE_KEYS and p % PAGE_KEYS == PAGE_KEYS - 2 for p in ps), (W, S)  # the rows cross a page
            assert max(ps) + max(ROWS) - 1 <= BOUND
    # S = 5 with lo = 6: the window's first group of four starts below S4 = 8
    assert all(any(_binds(p, W, 5) and _lo(p, W, 5) == 6 and (_lo(p, W, 5) & ~3) < ((5 + 3) & ~3) for p in start_positions(W, 5)) for W in WINDOWS)
    # a small window puts in-call rows into the wave's first block (the sink form of the key loop): virtual index of row 0's own key < 16
    assert any(((S + 3) & ~3) + (p - (_lo(p, W, S) & ~3)) < 16 for W in WINDOWS for S in SINKS for p in start_positions(W, S) if _binds(p, W, S))


class _Case:
    """One launch of (a): slot 0 runs T rows from p0, slot 1 is inactive, slot 2 a prefix of max(1, T - 1) rows from p2.  R: the rows-sink attention; S1: the one-row
    sink step (unwindowed_rows: the UNWINDOWED rows step, for (b)) with pools of its own, made a copy of R's by sync_pools."""

    def __init__(self, dev, kv_dtype, W, S, T, p0, p2, seed, max_keys=MAX_KEYS, unwindowed_rows=False, rope=True):
        from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchDecodeAttention
        from tinychatengine_amd.speculative import PagedRowsDecodeAttention
        self.fp8 = fp8 = kv_dtype == "fp8_e4m3"
        scales = dict(kv_dtype=kv_dtype, k_scale_log2=-1, v_scale_log2=-2) if fp8 else {}
        self.dev, self.W, self.S, self.T, self.bound = dev, W, S, T, max_keys - 1
        cos, sin = _rope_tables(max_keys, max_keys + W + S, dev) if rope else (None, None)
        stride = max_keys // PAGE_KEYS
        g = torch.Generator(device=dev).manual_seed(seed)
        num_pages = B * stride + 3
        self.alloc = alloc = PageAllocator(num_pages, PAGE_KEYS, B, stride, dev, free_order=np.random.default_rng(seed).permutation(num_pages).tolist())
        self.R = PagedRowsDecodeAttention(alloc, HEADS, KV_HEADS, dev, cos, sin, rows_per_seq=T, window=W, sinks=S, **scales)
        assert (self.R.window, self.R.sinks) == (W, S)
        if unwindowed_rows:
            self.S1 = PagedRowsDecodeAttention(alloc, HEADS, KV_HEADS, dev, cos, sin, rows_per_seq=T, **scales)
        else:
            self.S1 = PagedBatchDecodeAttention(alloc, HEADS, KV_HEADS, dev, cos, sin, window=W, sinks=S, **scales)
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
        self.S1.k_pool.copy_(self.R.k_pool)
        self.S1.v_pool.copy_(self.R.v_pool)

    def successive(self):
        """The yardstick: T successive one-row sink steps on S1's pools."""
        want = torch.empty((B, self.T, HEADS * HD), dtype=torch.float16, device=self.dev)
        for t in range(self.T):
            pt = torch.from_numpy(self.pos[:, t].copy()).to(self.dev)
            want[:, t] = self.S1.step(self.qkv.view(B, self.T, -1)[:, t].contiguous(), pt, self.bound)
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
    assert torch.equal(_raw(out), _raw(want)), f"{what}: output rows differ from the successive one-row sink steps'"
    assert torch.equal(_raw(out[1]), torch.zeros_like(_raw(out[1]))), f"{what}: the inactive sequence's rows are not zero"
    assert torch.equal(_raw(c.R.k_pool), _raw(c.S1.k_pool)) and torch.equal(_raw(c.R.v_pool), _raw(c.S1.v_pool)), f"{what}: the pools differ from the single steps'"
    changed = (_raw(c.R.k_pool) != _raw(k0)).any(-1) | (_raw(c.R.v_pool) != _raw(v0)).any(-1)
    assert not (changed & ~c.appended()).any(), f"{what}: a pool row other than the appended ones changed"


# =====================================================================================================================================================
# (a) the rows-sink step against successive one-row sink steps
# =====================================================================================================================================================
@pytest.mark.parametrize("kv_dtype", ["fp16", "fp8_e4m3"])
@pytest.mark.parametrize("T", ROWS)
def test_rows_sink_step_equals_successive_sink_steps(dev, T, kv_dtype):
    from tinychatengine_amd import capi
    for W in WINDOWS:
        for S in SINKS:
            assert capi.describe_attention_paged_sink(B, HEADS, KV_HEADS, BOUND, PAGE_KEYS, W, S)["chunks"] == 1
            ps = start_positions(W, S)
            for i, p0 in enumerate(ps):
                p2 = ps[(i + 2) % len(ps)]  # each sequence of the batch a different case
                c = _Case(dev, kv_dtype, W, S, T, p0, p2, seed=1000 * W + 50 * S + 10 * T + i)
                _check_bit_identity(c, f"{kv_dtype} W={W} S={S} T={T} starts=({p0}, {p2})")
                del c


@pytest.mark.parametrize("kv_dtype", ["fp16", "fp8_e4m3"])
def test_rows_sink_step_over_several_chunk_slots(dev, kv_dtype):
    """S4 + W + 3 = 407 virtual keys: four chunk slots, so every virtual row's partial states go through its own workspace slice and the last workgroup combines
    them.  The first start straddles the threshold (the rows that do not bind leave the later chunk slots' tails without keys), the others bind in every row."""
    from tinychatengine_amd import capi
    W, S, max_keys = 400, 4, 1024
    cut = capi.describe_attention_paged_sink(B, HEADS, KV_HEADS, max_keys - 1, PAGE_KEYS, W, S)
    assert cut["chunks"] == 4 and cut["combine"] == "yes", cut
    for T, p0, p2 in ((5, S + W - 2, 110), (8, 637, 1003), (2, 1022, S + W)):
        c = _Case(dev, kv_dtype, W, S, T, p0, p2, seed=W + T, max_keys=max_keys)
        _check_bit_identity(c, f"{kv_dtype} W={W} S={S} T={T} starts=({p0}, {p2})")
        _check_bit_identity(c, f"{kv_dtype} W={W} S={S} T={T} starts=({p0}, {p2}), the same workspace again")  # (the arrival counters went back to zero)
        del c


def test_rows_sink_step_without_rope(dev):
    """No cos / sin tables: both queries are the raw q and the keys enter the pool unrotated."""
    for W, S, T, p0, p2 in ((8, 5, 5, 11, 13), (17, 16, 8, 33, 60), (9, 1, 1, 10, 9)):
        c = _Case(dev, "fp16", W, S, T, p0, p2, seed=77 + W, rope=False)
        _check_bit_identity(c, f"no rope W={W} S={S} T={T}")
        del c
    c = _Case(dev, "fp8_e4m3", 16, 4, 5, 18, 40, seed=78, rope=False)
    _check_bit_identity(c, "no rope e4m3")


# =====================================================================================================================================================
# (b) sinks + window that never bind
# =====================================================================================================================================================
@pytest.mark.parametrize("kv_dtype", ["fp16", "fp8_e4m3"])
def test_a_rows_sink_step_that_never_binds_is_the_rows_step(dev, kv_dtype):
    for T, S, p0, p2 in ((1, 1, 0, 127), (2, 4, 14, 61), (5, 16, 30, 0), (8, 5, 120, 63)):  # (120 + 7 = the bound: the last row still active)
        W = BOUND + 1 - S  # S + W = pos_bound + 1
        c = _Case(dev, kv_dtype, W, S, T, p0, p2, seed=500 + T, unwindowed_rows=True)
        c.sync_pools()
        want = torch.full((B * T, HEADS * HD), 5.0, dtype=torch.float16, device=dev)
        c.S1.step(c.qkv, c.pos_t, BOUND, out=want)
        out = c.rows()
        torch.cuda.synchronize()
        what = f"{kv_dtype} T={T} S={S} starts=({p0}, {p2})"
        assert torch.equal(_raw(out), _raw(want.view(B, T, -1))), f"{what}: sinks + window = pos_bound + 1 is not the unwindowed rows step"
        assert torch.equal(_raw(c.R.k_pool), _raw(c.S1.k_pool)) and torch.equal(_raw(c.R.v_pool), _raw(c.S1.v_pool)), what
        del c


# =====================================================================================================================================================
# (c) released pages
# =====================================================================================================================================================
@pytest.mark.parametrize("kv_dtype", ["fp16", "fp8_e4m3"])
def test_released_pages_between_the_sinks_and_the_window_are_never_followed(dev, kv_dtype):
    """W = page_keys + 1, S = 4 at starts 78 and 110: lo_0 = 62 and 94, so words 1 .. 2 (and 1 .. 4) lie between the sinks' word and every row's window.  Their pages
    are given back (keep_pages = 1 holds word 0's) and filled with NaNs and the words are pointed at the NaN page: the contract says they never become addresses."""
    W, S, T, p0, p2 = PAGE_KEYS + 1, 4, 5, 78, 110
    c = _Case(dev, kv_dtype, W, S, T, p0, p2, seed=4242)
    c.sync_pools()
    want = c.successive()
    torch.cuda.synchronize()
    first = {0: _lo(p0, W, S) // PAGE_KEYS, 2: _lo(p2, W, S) // PAGE_KEYS}
    assert first == {0: 3, 2: 5}
    for b, n in first.items():
        word0 = int(c.alloc.table[b, 0])
        gone = c.alloc.release_behind(b, n * PAGE_KEYS, keep_pages=1)
        assert len(gone) == n - 1 and word0 not in gone and c.alloc.kept[b] == [word0]
        for page in gone:
            _poison((c.R.k_pool, c.R.v_pool), page, c.fp8, dev)
        c.alloc.table[b, 1:n] = c.canary
    c.alloc.check_invariants()
    assert c.R.table_violations(c.pos_t, c.bound) == 0, "the check counts a word no row follows"
    out = c.rows()
    torch.cuda.synchronize()
    assert not torch.isnan(out.float()).any(), "a released page was weighted"
    assert torch.equal(_raw(out), _raw(want)), "the outputs changed with the words between the sinks and the window"
    # words that are no page numbers: between the sinks and the window nobody looks, at word 0 every binding row does
    good = c.alloc.table.clone()
    c.alloc.table[0, 1:3] = c.alloc.num_pages
    assert c.R.table_violations(c.pos_t, c.bound) == 0
    c.alloc.table[0, 0] = c.alloc.num_pages
    assert c.R.table_violations(c.pos_t, c.bound) > 0, "a broken word 0 was not counted"
    c.alloc.table.copy_(good)
    c.alloc.table[2, 0] = -1
    assert c.R.table_violations(c.pos_t, c.bound) > 0
    c.alloc.table.copy_(good)


# =====================================================================================================================================================
# (d) life cycle
# =====================================================================================================================================================
@pytest.mark.parametrize("kv_dtype", ["fp16", "fp8_e4m3"])
def test_one_captured_rows_sink_step_replayed_while_pages_come_back(dev, kv_dtype):
    """The graph holds one rows-sink step of T = 4 rows; between replays the sequence moves on by 1 .. 4 positions (rejected drafts leave rows behind, the next call
    writes over them), the host gives the pages between the sinks' page and the window back (release_behind(..., keep_pages=1)), fills them with NaN and hands them to
    another slot.  The eager twin keeps every page.  Same outputs, bit for bit."""
    from tinychatengine_amd.paged_kv import PageAllocator
    from tinychatengine_amd.speculative import PagedRowsDecodeAttention
    fp8 = kv_dtype == "fp8_e4m3"
    scales = dict(kv_dtype=kv_dtype, k_scale_log2=1, v_scale_log2=0) if fp8 else {}
    S, W, T, keys = 4, PAGE_KEYS + 3, 4, 512
    n0, replays = 2 * PAGE_KEYS + 1, 40
    cos, sin = _rope_tables(keys, 21, dev)
    # (the squatter keeps every page that comes back, so the pool holds what the sequence ever touches: up to key n0 + replays * T + T - 1, and one to spare)
    small = (n0 + replays * T + T - 1) // PAGE_KEYS + 2
    alloc = PageAllocator(small, PAGE_KEYS, B, keys // PAGE_KEYS, dev, free_order=np.random.default_rng(1).permutation(small).tolist())
    big = PageAllocator(keys // PAGE_KEYS, PAGE_KEYS, B, keys // PAGE_KEYS, dev)
    P = PagedRowsDecodeAttention(alloc, HEADS, KV_HEADS, dev, cos, sin, rows_per_seq=T, window=W, sinks=S, **scales)
    E = PagedRowsDecodeAttention(big, HEADS, KV_HEADS, dev, cos, sin, rows_per_seq=T, window=W, sinks=S, **scales)
    g = torch.Generator(device=dev).manual_seed(5)
    lin = _Pair(np.zeros((KV_HEADS, 1, HD), np.float16), np.zeros((KV_HEADS, 1, HD), np.float16), dev)
    lin.k_cache = (torch.randn((KV_HEADS, n0, HD), generator=g, device=dev) * 0.7).half()
    lin.v_cache = (torch.randn((KV_HEADS, n0, HD), generator=g, device=dev) * 0.7).half()
    lin.k_cache[:, :S] *= 3  # (the sinks carry weight)
    for A, al in ((P, alloc), (E, big)):
        _fill(A, torch.Generator(device=dev).manual_seed(2), fp8, dev)
        al.reserve(0, n0 - 1)
        A.admit(0, lin, 0, n0)
    rows = (torch.randn((replays, T, (HEADS + 2 * KV_HEADS) * HD), generator=g, device=dev) * 0.9).half()
    qkv = torch.zeros((B * T, (HEADS + 2 * KV_HEADS) * HD), dtype=torch.float16, device=dev)
    pos_t = torch.full((B * T,), -1, dtype=torch.int32, device=dev)
    pos_t[:T] = torch.arange(n0, n0 + T, dtype=torch.int32, device=dev)
    out = torch.zeros((B * T, HEADS * HD), dtype=torch.float16, device=dev)
    alloc.reserve(0, n0 + T - 1)
    P.step(qkv, pos_t, keys - 1, out=out)  # warm-up (all-zero rows appended at n0 ..; the first replay appends the real ones over them)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        P.step(qkv, pos_t, keys - 1, out=out)
    squatted, p = 0, n0
    advance = np.random.default_rng(9).integers(1, T + 1, replays)
    for i in range(replays):
        freed = alloc.release_behind(0, p - W + 1, keep_pages=1)
        for page in freed:  # what came back is overwritten and handed to another slot
            _poison((P.k_pool, P.v_pool), page, fp8, dev)
        if freed:
            squatted += len(alloc.reserve(1, (squatted + len(freed)) * PAGE_KEYS - 1))
        alloc.reserve(0, p + T - 1)
        big.reserve(0, p + T - 1)
        alloc.check_invariants()
        assert len(alloc.kept[0]) + len(alloc.pages[0]) <= (W + T + PAGE_KEYS - 1) // PAGE_KEYS + 2
        qkv[:T].copy_(rows[i])
        pos_t[:T] = torch.arange(p, p + T, dtype=torch.int32, device=dev)
        assert P.table_violations(pos_t, keys - 1) == 0
        graph.replay()
        want = E.step(qkv, pos_t, keys - 1)
        torch.cuda.synchronize()
        assert torch.isfinite(out.float()).all(), f"position {p}: a freed page was read"
        assert torch.equal(_raw(out), _raw(want)), f"position {p}: the replay differs from the eager run that kept every page"
        p += int(advance[i])
    assert squatted >= 2 and alloc.gone[0] >= 3 and len(alloc.kept[0]) == 1, "no page came back"
    assert p > S + W + 3 * PAGE_KEYS
