"""The paged batched decode step (tce_attention_decode_step_paged_f16, tinychatengine_amd/paged_kv.py): the batched step with its caches in pages.

Contract: every active row's output and appended rows are BIT-IDENTICAL to tce_attention_decode_step_batch_f16 on contiguous caches with the same contents; no
page other than the ones that hold an active row's index `pos` changes, and in those only that row; table words beyond pos // page_keys and every word of an
inactive row are never followed.  Every comparison here is for equal bits; there is no tolerance.  Every paged launch is preceded by tce_kv_block_table_check with
its count asserted 0, and no test hands the step a page number outside the pool: a wrong kernel fails an assertion, not an address."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HD = 128


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


def _ragged(rng, batch, bound):  # (as tests/test_gpu_batch_decode.py makes them)
    pos = rng.integers(0, bound + 1, batch)
    pos[0] = 0
    if batch > 1:
        pos[-1] = bound
    if batch > 2:
        pos[1] = bound  # two rows at the bound
    return pos.astype(np.int32)


def _contiguous(dev, batch, heads, kv_heads, max_keys, rope, seed):
    """The yardstick: a BatchDecodeAttention with random caches, a q/k/v batch, the generator."""
    from tinychatengine_amd.batch_decode import BatchDecodeAttention
    g = torch.Generator(device=dev).manual_seed(seed)
    tc = ts = None
    if rope:
        cos, sin = _tables(max_keys, seed)
        tc, ts = torch.from_numpy(cos).to(dev), torch.from_numpy(sin).to(dev)
    A = BatchDecodeAttention(batch, heads, max_keys, dev, tc, ts, kv_heads=kv_heads)
    A.k_cache.copy_((torch.randn(A.k_cache.shape, generator=g, device=dev) * 0.8).half())
    A.v_cache.copy_((torch.randn(A.v_cache.shape, generator=g, device=dev) * 0.8).half())
    qkv = (torch.randn((batch, (heads + 2 * kv_heads) * HD), generator=g, device=dev) * 0.9).half()
    return A, qkv, g


def _paged(A, page_keys, extra_pages, seed, dev):
    """An allocator with a seeded permutation of a pool of (pages a full batch needs) + extra_pages, and a layer's pools filled with random bits."""
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchDecodeAttention
    stride = A.max_keys // page_keys
    assert stride * page_keys == A.max_keys
    num_pages = A.batch * stride + extra_pages
    order = np.random.default_rng(seed).permutation(num_pages).tolist()
    alloc = PageAllocator(num_pages, page_keys, A.batch, stride, dev, free_order=order)
    P = PagedBatchDecodeAttention(alloc, A.heads, A.kv_heads, dev, A.cos, A.sin)
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    P.k_pool.copy_((torch.randn(P.k_pool.shape, generator=g, device=dev) * 0.7).half())
    P.v_pool.copy_((torch.randn(P.v_pool.shape, generator=g, device=dev) * 0.7).half())
    return alloc, P


class _Slot:
    """Slot b of a BatchDecodeAttention as a contiguous cache pair (what admit / gather_into take)."""

    def __init__(self, A, b):
        self.k_cache, self.v_cache = A.k_cache[b], A.v_cache[b]


def _fill(alloc, P, A, pos, bound):
    """Give every active slot exactly the pages its position needs and scatter the contiguous caches' rows 0 .. pos into them."""
    for b, p in enumerate(pos.tolist()):
        if 0 <= p <= bound:
            alloc.reserve(b, p)
            P.admit(b, _Slot(A, b), 0, p + 1)


def _expected_pools(alloc, P, A, pos, bound, k0, v0):
    """The pools as they must be after the step: the clones taken before it, with row pos of each active sequence (from the contiguous caches after THEIR step)."""
    ek, ev = k0.clone(), v0.clone()
    pk = alloc.page_keys
    for b, p in enumerate(pos.tolist()):
        if 0 <= p <= bound:
            page = alloc.pages[b][p // pk]
            ek[page, :, p % pk] = A.k_cache[b, :, p]
            ev[page, :, p % pk] = A.v_cache[b, :, p]
    return ek, ev


def _checked_step(P, qkv, pos_t, bound, out=None):
    assert P.table_violations(pos_t, bound) == 0, "the block table is not sound: no launch"
    return P.step(qkv, pos_t, bound, out=out)


def _assert_gathered(P, A, pos, bound, what):
    for b, p in enumerate(pos.tolist()):
        if 0 <= p <= bound:
            k, v = P.read_back(b, p + 1)
            assert torch.equal(_bits(k), _bits(A.k_cache[b, :, :p + 1])) and torch.equal(_bits(v), _bits(A.v_cache[b, :, :p + 1])), f"{what}: slot {b} gathered caches differ"


# ---- 5: bit-identity with the contiguous batched step ----
@pytest.mark.parametrize("page_keys", [16, 64, 256])
@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("heads,kv_heads", [(32, 8), (8, 8), (4, 1)])
def test_paged_step_is_bit_identical_to_the_batched_step(dev, heads, kv_heads, rope, page_keys):
    for batch in (1, 3, 8, 16):
        for bound in (63, 319, 320, 1023, 2047, 4095):
            rng = np.random.default_rng(batch * 10000 + bound)
            max_keys = (bound // page_keys + 1) * page_keys
            A, qkv, _ = _contiguous(dev, batch, heads, kv_heads, max_keys, rope, seed=batch + bound)
            alloc, P = _paged(A, page_keys, 9, seed=bound + page_keys, dev=dev)
            pos = _ragged(rng, batch, bound)
            pos_t = torch.from_numpy(pos).to(dev)
            _fill(alloc, P, A, pos, bound)
            k0, v0 = P.k_pool.clone(), P.v_pool.clone()
            out = _checked_step(P, qkv, pos_t, bound)
            want = A.step(qkv, pos_t, bound)
            torch.cuda.synchronize()
            what = f"B={batch} bound={bound} page_keys={page_keys} pos={pos.tolist()}"
            assert torch.equal(_bits(out), _bits(want)), f"{what}: outputs differ"
            _assert_gathered(P, A, pos, bound, what)
            ek, ev = _expected_pools(alloc, P, A, pos, bound, k0, v0)
            assert torch.equal(_bits(P.k_pool), _bits(ek)) and torch.equal(_bits(P.v_pool), _bits(ev)), f"{what}: a pool row other than the appended ones changed"
            touched = {alloc.pages[b][int(p) // page_keys] for b, p in enumerate(pos)}
            rest = torch.tensor(sorted(set(range(alloc.num_pages)) - touched), dtype=torch.long, device=dev)
            assert torch.equal(_bits(P.k_pool[rest]), _bits(k0[rest])) and torch.equal(_bits(P.v_pool[rest]), _bits(v0[rest])), f"{what}: an untouched page changed"
            del A, P, k0, v0, ek, ev


# ---- 6: unused table words are never followed ----
NAN_BITS = [0x7E00, 0x7D55, -512 + 1, 0x7FFF]  # quiet / signalling-style NaNs of both signs (0xFE01 as int16)


def _canary(alloc, P, dev):
    """A page of the pool that no sequence owns (the LAST one the allocator would hand out), filled with NaN bits in both pools."""
    page = alloc.free[0]
    nan = torch.tensor(NAN_BITS, dtype=torch.int16, device=dev)
    for pool in (P.k_pool, P.v_pool):
        v = pool.view(torch.int16)[page]
        v.copy_(nan.repeat(v.numel() // 4).view(v.shape))
    return page


@pytest.mark.parametrize("page_keys", [16, 64, 256])
@pytest.mark.parametrize("heads,kv_heads,rope", [(32, 8, True), (4, 1, False)])
def test_unused_table_words_are_never_followed(dev, heads, kv_heads, rope, page_keys):
    for batch, bound in ((3, 63), (8, 320), (16, 1023), (8, 4095)):
        rng = np.random.default_rng(batch + bound)
        max_keys = (bound // page_keys + 2) * page_keys  # a table row longer than any sequence needs
        A, qkv, _ = _contiguous(dev, batch, heads, kv_heads, max_keys, rope, seed=3 * batch + bound)
        alloc, P = _paged(A, page_keys, 5, seed=bound + page_keys + 1, dev=dev)
        pos = _ragged(rng, batch, bound)
        if batch > 3:
            pos[2], pos[3] = -1, bound + 1  # two inactive rows
        pos_t = torch.from_numpy(pos).to(dev)
        _fill(alloc, P, A, pos, bound)
        canary = _canary(alloc, P, dev)
        assert all(canary not in ps for ps in alloc.pages)
        table = torch.full_like(alloc.table, canary)  # every word the step must not follow points at the canary -- a VALID page number
        for b, ps in enumerate(alloc.pages):
            if 0 <= pos[b] <= bound:
                n = int(pos[b]) // page_keys + 1
                assert n == len(ps)
                table[b, :n] = torch.tensor(ps, dtype=torch.int32, device=dev)
        alloc.table.copy_(table)
        k0, v0 = P.k_pool.clone(), P.v_pool.clone()
        out = _checked_step(P, qkv, pos_t, bound)
        want = A.step(qkv, pos_t, bound)
        torch.cuda.synchronize()
        what = f"B={batch} bound={bound} page_keys={page_keys} pos={pos.tolist()}"
        assert not torch.isnan(out.float()).any(), f"{what}: the canary leaked into an output"
        assert torch.equal(_bits(out), _bits(want)), f"{what}: outputs differ"
        assert torch.equal(_bits(P.k_pool[canary]), _bits(k0[canary])) and torch.equal(_bits(P.v_pool[canary]), _bits(v0[canary])), f"{what}: the canary page was written"
        ek, ev = _expected_pools(alloc, P, A, pos, bound, k0, v0)
        assert torch.equal(_bits(P.k_pool), _bits(ek)) and torch.equal(_bits(P.v_pool), _bits(ev)), what
        del A, P


# ---- 7: inactive rows ----
@pytest.mark.parametrize("bound,page_keys", [(63, 16), (1023, 64), (1023, 256)])
def test_inactive_rows_write_zeros_and_touch_nothing(dev, bound, page_keys):
    heads, kv_heads, batch = 32, 8, 6
    max_keys = (bound // page_keys + 1) * page_keys
    A, qkv, _ = _contiguous(dev, batch, heads, kv_heads, max_keys, True, seed=31 + bound)
    alloc, P = _paged(A, page_keys, 4, seed=bound, dev=dev)
    # first every row inactive: zeros, and NOTHING else written anywhere
    pos = np.array([-1, bound + 1, -7, bound + 100, -1, bound + 1], np.int32)
    pos_t = torch.from_numpy(pos).to(dev)
    k0, v0, w0 = P.k_pool.clone(), P.v_pool.clone(), P.workspace.clone()
    out = torch.full((batch, heads * HD), 3.0, dtype=torch.float16, device=dev)
    _checked_step(P, qkv, pos_t, bound, out=out)
    torch.cuda.synchronize()
    assert torch.count_nonzero(out) == 0
    assert torch.equal(_bits(P.k_pool), _bits(k0)) and torch.equal(_bits(P.v_pool), _bits(v0)) and torch.equal(P.workspace, w0)
    # then a mix: the inactive rows' table words all point at the canary
    pos = np.array([5, -1, bound, -7, bound + 1, 0], np.int32)
    inactive = [1, 3, 4]
    pos_t.copy_(torch.from_numpy(pos))
    _fill(alloc, P, A, pos, bound)
    canary = _canary(alloc, P, dev)
    for b in inactive:
        alloc.table[b].fill_(canary)
    k0, v0 = P.k_pool.clone(), P.v_pool.clone()
    out = _checked_step(P, qkv, pos_t, bound)
    want = A.step(qkv, pos_t, bound)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want))
    sw = P.slot_workspace_bytes
    for b in range(batch):
        if b in inactive:
            assert torch.count_nonzero(out[b]) == 0 and not torch.isnan(out[b]).any(), f"row {b}: inactive row not zero"
            assert torch.count_nonzero(P.workspace[b * sw:(b + 1) * sw]) == 0, f"row {b}: inactive workspace touched"
        else:
            assert torch.count_nonzero(P.workspace[b * sw:b * sw + 256]) == 0, f"row {b}: a counter was left non-zero"
    ek, ev = _expected_pools(alloc, P, A, pos, bound, k0, v0)
    assert torch.equal(_bits(P.k_pool), _bits(ek)) and torch.equal(_bits(P.v_pool), _bits(ev))
    _assert_gathered(P, A, pos, bound, "mixed launch")


# ---- 8: shared pages ----
@pytest.mark.parametrize("page_keys,full_pages", [(64, 3), (16, 5)])
def test_sequences_that_share_pages(dev, page_keys, full_pages):
    heads, kv_heads, batch = 32, 8, 4
    shared = full_pages * page_keys
    bound = shared + 3 * page_keys - 1
    A, qkv, _ = _contiguous(dev, batch, heads, kv_heads, bound + 1, True, seed=8 + page_keys)
    alloc, P = _paged(A, page_keys, 3, seed=80 + page_keys, dev=dev)
    # slot 0 owns the prompt (+ 11 keys of a partial page); slots 1, 2 fork at the page boundary, slot 3 eight keys into the partial page (one page copy)
    fork_keys = [None, shared, shared, shared + 8]
    pos = np.array([shared + 11, shared, shared + page_keys + 5, bound], np.int32)
    alloc.reserve(0, int(pos[0]))
    P.admit(0, _Slot(A, 0), 0, int(pos[0]) + 1)
    prompt_pages = list(alloc.pages[0][:full_pages])
    for b in (1, 2, 3):
        A.k_cache[b, :, :fork_keys[b]] = A.k_cache[0, :, :fork_keys[b]]  # the contiguous form holds four copies
        A.v_cache[b, :, :fork_keys[b]] = A.v_cache[0, :, :fork_keys[b]]
        for src, dst, rows in alloc.fork(0, b, fork_keys[b]):
            P.copy_rows(src, dst, rows)
        alloc.reserve(b, int(pos[b]))
        P.admit(b, _Slot(A, b), fork_keys[b], int(pos[b]) + 1 - fork_keys[b])
        assert alloc.pages[b][:full_pages] == prompt_pages
    assert all(alloc.refcount[p] == 4 for p in prompt_pages)
    assert len({ps[full_pages] for ps in alloc.pages}) == 4  # private tails
    alloc.check_invariants()
    pos_t = torch.from_numpy(pos).to(dev)
    k0, v0 = P.k_pool.clone(), P.v_pool.clone()
    out = _checked_step(P, qkv, pos_t, bound)
    want = A.step(qkv, pos_t, bound)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want))
    _assert_gathered(P, A, pos, bound, "shared pages")
    idx = torch.tensor(prompt_pages, dtype=torch.long, device=dev)
    assert torch.equal(_bits(P.k_pool[idx]), _bits(k0[idx])) and torch.equal(_bits(P.v_pool[idx]), _bits(v0[idx])), "a shared page changed"
    ek, ev = _expected_pools(alloc, P, A, pos, bound, k0, v0)
    assert torch.equal(_bits(P.k_pool), _bits(ek)) and torch.equal(_bits(P.v_pool), _bits(ev))


# ---- 9: walking across page boundaries under one captured graph ----
def test_captured_paged_step_walks_across_pages(dev):
    heads, kv_heads, batch, page_keys, bound = 8, 4, 3, 16, 79  # five pages per sequence
    A, qkv, g = _contiguous(dev, batch, heads, kv_heads, bound + 1, True, seed=9)
    alloc, P = _paged(A, page_keys, 6, seed=90, dev=dev)
    A.k_cache.zero_()
    A.v_cache.zero_()
    start = np.array([0, 0, -20], np.int32)  # slot 2 joins twenty tokens later
    pos_e = torch.full((batch,), -1, dtype=torch.int32, device=dev)
    pos_g = pos_e.clone()
    out_g = torch.empty((batch, heads * HD), dtype=torch.float16, device=dev)
    _checked_step(P, qkv, pos_g, bound, out=out_g)  # the warm-up launch: every row inactive
    torch.cuda.synchronize()
    pos_e.copy_(torch.from_numpy(start))
    pos_g.copy_(pos_e)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        P.step(qkv, pos_g, bound, out=out_g)
        pos_g.add_(1)
    # (a capture does not run its launches: nothing has been appended yet)
    pos = start.copy()
    crossings = 0
    for t in range(bound + 1):
        qkv.copy_((torch.randn(qkv.shape, generator=g, device=dev) * 0.9).half())
        for b in range(batch):
            if 0 <= pos[b] <= bound:
                crossings += len(alloc.reserve(b, int(pos[b])))
        assert P.table_violations(pos_g, bound) == 0
        graph.replay()
        want = A.step(qkv, pos_e, bound)
        pos_e.add_(1)
        torch.cuda.synchronize()
        assert torch.equal(pos_e, pos_g)
        assert torch.equal(_bits(out_g), _bits(want)), f"token {t}: the replay differs from the contiguous step (pos {pos.tolist()})"
        pos += 1
    assert crossings == 5 + 5 + 4  # slots 0, 1 reached key 79, slot 2 key 59
    last = np.minimum(pos - 1, bound).astype(np.int32)
    _assert_gathered(P, A, last, bound, "after the walk")


# ---- 10: scatter and gather ----
@pytest.mark.parametrize("page_keys", [16, 64, 256])
def test_scatter_and_gather_round_trip(dev, page_keys):
    from tinychatengine_amd import capi
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchDecodeAttention
    L = capi.lib()
    kv_heads, src_keys = 2, 1100
    stride = (src_keys + page_keys - 1) // page_keys
    num_pages = stride + 5
    alloc = PageAllocator(num_pages, page_keys, 2, stride, dev, free_order=np.random.default_rng(page_keys).permutation(num_pages).tolist())
    alloc.reserve(1, src_keys - 1)
    P = PagedBatchDecodeAttention(alloc, 4, kv_heads, dev)
    pages = torch.tensor(alloc.pages[1], dtype=torch.long, device=dev)
    g = torch.Generator(device=dev).manual_seed(page_keys)
    rnd = lambda shape: torch.randint(-32768, 32767, shape, generator=g, device=dev, dtype=torch.int16).view(torch.float16)
    src = _Slot.__new__(_Slot)
    src.k_cache, src.v_cache = rnd((kv_heads, src_keys, HD)), rnd((kv_heads, src_keys, HD))
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for key0 in (0, 1, 63, 64, 65):
        for nkeys in (1, 15, 64, 129, 1000):
            P.k_pool.copy_(rnd(P.k_pool.shape))
            P.v_pool.copy_(rnd(P.v_pool.shape))
            k0, v0 = P.k_pool.clone(), P.v_pool.clone()
            P.admit(1, src, key0, nkeys)
            keys = torch.arange(key0, key0 + nkeys, device=dev)
            pg, row = pages[keys // page_keys], keys % page_keys
            k0[pg, :, row] = src.k_cache[:, keys].permute(1, 0, 2)
            v0[pg, :, row] = src.v_cache[:, keys].permute(1, 0, 2)
            torch.cuda.synchronize()
            what = f"page_keys={page_keys} key0={key0} nkeys={nkeys}"
            assert torch.equal(_bits(P.k_pool), _bits(k0)) and torch.equal(_bits(P.v_pool), _bits(v0)), f"{what}: scatter wrote other rows, or not these"
            dst = _Slot.__new__(_Slot)
            dst.k_cache, dst.v_cache = rnd((kv_heads, src_keys, HD)), rnd((kv_heads, src_keys, HD))
            dk, dv = dst.k_cache.clone(), dst.v_cache.clone()
            P.gather_into(1, dst, key0, nkeys)
            dk[:, keys], dv[:, keys] = src.k_cache[:, keys], src.v_cache[:, keys]
            torch.cuda.synchronize()
            assert torch.equal(_bits(dst.k_cache), _bits(dk)) and torch.equal(_bits(dst.v_cache), _bits(dv)), f"{what}: gather wrote other rows, or not these"
            assert torch.equal(_bits(P.k_pool), _bits(k0)) and torch.equal(_bits(P.v_pool), _bits(v0)), f"{what}: gather wrote the pool"
    # a table word outside the pool copies nothing (and is not followed): the copy kernels' own guard, on a private table
    bad = torch.full((stride,), num_pages, dtype=torch.int32, device=dev)
    k0 = P.k_pool.clone()
    assert L.tce_kv_pages_scatter_f16(p(src.k_cache), p(src.v_cache), p(P.k_pool), p(P.v_pool), p(bad), stride, page_keys, num_pages, kv_heads, HD, src_keys, 0, 100, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(P.k_pool), _bits(k0))


# ---- 11: 200 launches on one workspace ----
def test_two_hundred_launches_reset_their_counters(dev):
    heads, kv_heads, batch, bound, page_keys = 32, 8, 4, 1023, 64
    A, qkv, g = _contiguous(dev, batch, heads, kv_heads, bound + 1, True, seed=200)
    alloc, P = _paged(A, page_keys, 7, seed=201, dev=dev)
    full = np.full(batch, bound, np.int32)
    _fill(alloc, P, A, full, bound)
    rng = np.random.default_rng(200)
    pos_t = torch.zeros(batch, dtype=torch.int32, device=dev)
    for it in range(200):
        pos = rng.integers(0, bound + 1, batch).astype(np.int32)
        if it % 5 == 0:
            pos[it % batch] = rng.integers(0, 64)  # short contexts beside long ones (one live chunk next to eight)
        pos_t.copy_(torch.from_numpy(pos))
        qkv.copy_((torch.randn(qkv.shape, generator=g, device=dev) * 0.9).half())
        out = _checked_step(P, qkv, pos_t, bound)
        want = A.step(qkv, pos_t, bound)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(want)), f"launch {it}: outputs differ (pos {pos.tolist()})"
    _assert_gathered(P, A, full, bound, "after 200 launches")
    assert torch.count_nonzero(P.workspace.view(batch, -1)[:, :256]) == 0


# ---- 12: the table check ----
def test_block_table_check_counts_planted_violations(dev):
    """These tables go to the check kernel only, never to the step."""
    from tinychatengine_amd import capi
    L = capi.lib()
    batch, stride, page_keys, num_pages, bound = 4, 8, 16, 10, 200
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    viol = torch.full((1,), 77, dtype=torch.int32, device=dev)

    def count(table, pos):
        tt, pt = torch.tensor(table, dtype=torch.int32, device=dev), torch.tensor(pos, dtype=torch.int32, device=dev)
        assert L.tce_kv_block_table_check(p(tt), stride, page_keys, num_pages, batch, p(pt), bound, p(viol), st) == capi.TCE_OK
        return int(viol.item())

    good = [[(3 * b + e) % num_pages for e in range(stride)] for b in range(batch)]
    pos = [40, -1, 100, 120]  # needed words: rows 0: 0 .. 2, 2: 0 .. 6, 3: 0 .. 7; row 1 inactive
    assert count(good, pos) == 0
    t = [r[:] for r in good]
    t[0][1] = num_pages      # an entry equal to num_pages
    assert count(t, pos) == 1
    t[2][3] = -5             # a negative entry inside the needed range
    assert count(t, pos) == 2
    t[2][0] = 99
    assert count(t, pos) == 3
    assert count(t, [40, -1, 100, 130]) == 4   # 130 // 16 = 8 reaches table_stride: one more, its eight words are sound
    assert count(good, [40, -1, 100, 130]) == 1
    assert count(good, [40, -1, 100, bound]) == 1
    # the same words beyond the needed range, or in inactive rows: nothing
    t = [r[:] for r in good]
    t[0][3] = num_pages
    t[0][7] = -1
    t[2][7] = -5
    t[1] = [-1, num_pages, 99, -7, 1 << 30, -(1 << 31), num_pages, -1]
    assert count(t, pos) == 0
    assert count(t, [40, bound + 1, 100, 120]) == 0
    t[3] = [num_pages] * stride
    assert count(t, [40, -1, 100, bound + 1]) == 0  # a position past the bound is an inactive row, whatever page index it has
    assert count(t, [40, -1, 100, 0]) == 1


# ---- 13: whole blocks ----
def _blocks(dev, hidden, heads, kv_heads, ffn, layers, max_keys, seed):
    from tinychatengine_amd.decoder_block import DecoderBlock
    cos, sin = _tables(max_keys, seed)
    tc, ts = torch.from_numpy(cos).to(dev), torch.from_numpy(sin).to(dev)
    return [DecoderBlock(hidden, heads, ffn, max_keys, dev, tc, ts, seed=seed + i, kv_heads=kv_heads) for i in range(layers)]


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("hidden,heads,kv_heads,ffn,layers", [(512, 4, 1, 1408, 2), (4096, 32, 8, 14336, 1)])
def test_paged_blocks_equal_contiguous_blocks(dev, hidden, heads, kv_heads, ffn, layers, graph):
    """Four slots, staggered admission by prefill, 40 steps, slot 0 retired at step 15 (its pages released) and a new sequence admitted into it at step 20 that
    reuses released pages: the hidden rows of every active slot are bit-identical between PagedBatchedDecoder and BatchedDecoder at every step."""
    from tinychatengine_amd.batch_decode import BatchedDecoder
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchedDecoder
    batch, max_keys, page_keys = 4, 64, 16
    blocks = _blocks(dev, hidden, heads, kv_heads, ffn, layers, max_keys, 70 + hidden)
    cont = [BatchedDecoder(b, batch) for b in blocks]
    num_pages = 12  # fewer than 4 slots x 4 pages: the run only fits because pages follow the tokens and come back
    alloc = PageAllocator(num_pages, page_keys, batch, max_keys // page_keys, dev, free_order=np.random.default_rng(13).permutation(num_pages).tolist())
    paged = [PagedBatchedDecoder(b, alloc) for b in blocks]
    rng = np.random.default_rng(hidden + ffn)
    bound = max_keys - 1
    pos = np.full(batch, -1, np.int32)
    pos_t = torch.from_numpy(pos).to(dev)
    h_c = torch.zeros((batch, hidden), dtype=torch.float16, device=dev)
    h_p = torch.zeros_like(h_c)
    # step -> [(slot, prompt rows)].  Slot 0 holds 45 keys = three pages when it retires; slots 1 and 2 cross a page boundary at steps 15 and 16 and take two of
    # them (the free list hands a released page out first), the sequence admitted at step 20 takes the third
    admit = {0: [(0, 30), (3, 2)], 2: [(1, 3)], 4: [(2, 4)], 20: [(0, 6)]}
    retire = {15: 0}
    released, replay = [], None
    if graph:
        for d in paged:  # the warm-up: every row inactive (nothing is appended; the gate/up form is settled)
            d.step(h_p, pos_t, bound)
        torch.cuda.synchronize()
        replay = torch.cuda.CUDAGraph()
        with torch.cuda.graph(replay):
            for d in paged:
                d.step(h_p, pos_t, bound)
    for t in range(40):
        if t in retire:
            released = alloc.release(retire[t])
            assert len(released) == 3
            pos[retire[t]] = -1
        for slot, m in admit.get(t, []):
            x = torch.from_numpy(rng.standard_normal((m, hidden)).astype(np.float16)).to(dev)
            rows_c, rows_p = x.clone(), x.clone()
            for d in cont:
                d.prefill(slot, rows_c, 0)
            for d in paged:
                d.prefill(slot, rows_p, 0)
            torch.cuda.synchronize()
            assert torch.equal(_bits(rows_c), _bits(rows_p)), f"step {t}: prefill of slot {slot} differs"
            pos[slot] = m
            if t == 20:
                assert set(alloc.pages[slot]) & set(released), "the new sequence reuses none of the released pages"
        for b in range(batch):
            if pos[b] >= 0:
                alloc.reserve(b, int(pos[b]))
        alloc.check_invariants()
        x = torch.from_numpy(rng.standard_normal((batch, hidden)).astype(np.float16)).to(dev)
        h_c.copy_(x)
        h_p.copy_(x)
        pos_t.copy_(torch.from_numpy(pos))
        assert paged[0].attention.table_violations(pos_t, bound) == 0
        for d in cont:
            d.step(h_c, pos_t, bound)
        if graph:
            replay.replay()
        else:
            for d in paged:
                d.step(h_p, pos_t, bound)
        torch.cuda.synchronize()
        for b in range(batch):
            if pos[b] >= 0:
                assert torch.equal(_bits(h_c[b]), _bits(h_p[b])), f"step {t} slot {b} pos {pos[b]}: hidden rows differ"
                pos[b] += 1
    assert alloc.pages_in_use() <= num_pages and max(pos) == 42
    for dc, dp in zip(cont, paged):  # and the caches: every live slot's keys, gathered, are the contiguous ones
        for b in range(batch):
            k, v = dp.attention.read_back(b, int(pos[b]))
            assert torch.equal(_bits(k), _bits(dc.attention.k_cache[b, :, :pos[b]])) and torch.equal(_bits(v), _bits(dc.attention.v_cache[b, :, :pos[b]]))
