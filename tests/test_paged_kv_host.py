"""CPU (no GPU): the paged KV cache's C ABI -- exports, pool size, argument validation before any HIP call, the cut it describes -- and PageAllocator's bookkeeping
on a host table."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def capi():
    from tinychatengine_amd import build as B
    B.build()
    from tinychatengine_amd import capi
    return capi


NAMES = ("tce_kv_pages_pool_bytes", "tce_attention_decode_step_paged_f16", "tce_attention_decode_describe_paged", "tce_kv_pages_scatter_f16", "tce_kv_pages_gather_f16",
         "tce_kv_block_table_check")


def test_paged_symbols_are_exported(capi):
    L = capi.lib()
    for n in NAMES:
        assert n in capi.EXPORTS
        assert hasattr(L, n)


def test_pool_bytes(capi):
    L = capi.lib()
    for num_pages, kv_heads, page_keys in ((1, 1, 16), (100, 8, 64), (4096, 8, 256), (7, 3, 32), (5, 4, 128)):
        assert int(L.tce_kv_pages_pool_bytes(num_pages, kv_heads, page_keys, 128)) == num_pages * kv_heads * page_keys * 128 * 2
    assert int(L.tce_kv_pages_pool_bytes(100, 8, 64, 64)) == 0
    for bad in (0, 8, 15, 17, 48, 96, 512, -64):
        assert int(L.tce_kv_pages_pool_bytes(100, 8, bad, 128)) == 0, bad
    assert int(L.tce_kv_pages_pool_bytes(0, 8, 64, 128)) == 0
    assert int(L.tce_kv_pages_pool_bytes(-3, 8, 64, 128)) == 0
    assert int(L.tce_kv_pages_pool_bytes(100, 0, 64, 128)) == 0
    assert int(L.tce_kv_pages_pool_bytes(100, -1, 64, 128)) == 0


def _host():
    buf = (C.c_char * 8192)()
    return buf, (C.addressof(buf) + 15) & ~15


def _shared_faults(p):
    """The faults the contiguous batched step knows too, as changes to a valid call on the host buffer p."""
    return [dict(batch=0), dict(batch=-1), dict(kv=3), dict(kv=0), dict(bound=-1), dict(bound=64), dict(cos=p), dict(sin=p), dict(hd=64), dict(batch=65536),
            dict(qkv=p + 8), dict(kp=p + 8), dict(vpool=p + 8), dict(cos=p + 2, sin=p), dict(cos=p, sin=p + 4), dict(pos=p + 2), dict(heads=0)]


def test_paged_step_argument_validation_needs_no_gpu(capi):
    """Every refusal happens before a HIP call: host buffers stand in for the device pointers and are never dereferenced.  The shared faults return the batched
    step's codes."""
    L = capi.lib()
    keep, p = _host()
    vp = C.c_void_p

    def step(**kw):
        g = lambda k, d: kw[k] if k in kw else d
        return L.tce_attention_decode_step_paged_f16(vp(g("qkv", p)), vp(g("kp", p)), vp(g("vpool", p)), vp(g("tab", p)), g("stride", 4), g("pk", 16), g("np", 8),
                                                     vp(g("cos", None)), vp(g("sin", None)), vp(g("out", p)), vp(g("ws", p)), g("batch", 2), g("heads", 4), g("kv", 2),
                                                     g("hd", 128), vp(g("pos", p)), g("bound", 10), 0x2DA8, None)

    def batch(**kw):  # the contiguous batched step with 64 = 4 * 16 keys per slot
        g = lambda k, d: kw[k] if k in kw else d
        return L.tce_attention_decode_step_batch_f16(vp(g("qkv", p)), vp(g("kp", p)), vp(g("vpool", p)), vp(g("cos", None)), vp(g("sin", None)), vp(g("out", p)),
                                                     vp(g("ws", p)), g("batch", 2), g("heads", 4), g("kv", 2), g("hd", 128), 64, vp(g("pos", p)), g("bound", 10), 0x2DA8, None)

    for name in ("qkv", "kp", "vpool", "tab", "out", "ws", "pos"):
        assert step(**{name: None}) == capi.TCE_ERR_BAD_ARG, name
    assert "null pointer" in capi.last_error()
    # the faults the batched step knows: the same codes
    for kw in _shared_faults(p):
        assert step(**kw) == batch(**kw), kw
        assert step(**kw) in (capi.TCE_ERR_BAD_ARG, capi.TCE_ERR_UNSUPPORTED_SHAPE), kw
    assert step(kv=3) == capi.TCE_ERR_BAD_ARG and "do not divide" in capi.last_error()
    assert step(hd=64) == capi.TCE_ERR_UNSUPPORTED_SHAPE
    assert step(batch=65536) == capi.TCE_ERR_UNSUPPORTED_SHAPE and "65535" in capi.last_error()
    assert step(qkv=p + 8) == capi.TCE_ERR_UNSUPPORTED_SHAPE
    # the new ones
    for pk in (0, 8, 15, 24, 48, 512, -16):
        assert step(pk=pk) == capi.TCE_ERR_BAD_ARG and "page_keys" in capi.last_error(), pk
    assert step(stride=0) == capi.TCE_ERR_BAD_ARG
    assert step(stride=-4) == capi.TCE_ERR_BAD_ARG
    assert step(np=0) == capi.TCE_ERR_BAD_ARG
    assert step(bound=64) == capi.TCE_ERR_BAD_ARG and "table_stride * page_keys" in capi.last_error()  # 4 pages of 16 keys hold indices 0 .. 63
    assert step(stride=1, pk=16, bound=16) == capi.TCE_ERR_BAD_ARG
    assert step(tab=p + 2) == capi.TCE_ERR_UNSUPPORTED_SHAPE and "block_table" in capi.last_error()


def test_paged_rows_step_argument_validation_needs_no_gpu(capi):
    """The multi-row step's two entry points refuse before any HIP call (host buffers, never dereferenced): the single-row step's code for every shared fault, then
    the rows' own -- the row count, `out` in 16-byte pieces -- and the e4m3 exponents."""
    L = capi.lib()
    keep, p = _host()
    vp = C.c_void_p
    BAD, SHAPE = capi.TCE_ERR_BAD_ARG, capi.TCE_ERR_UNSUPPORTED_SHAPE

    def args(kw, rows):
        g = lambda k, d: kw[k] if k in kw else d
        return [vp(g("qkv", p)), vp(g("kp", p)), vp(g("vpool", p)), vp(g("tab", p)), g("stride", 4), g("pk", 16), g("np", 8), vp(g("cos", None)), vp(g("sin", None)),
                vp(g("out", p)), vp(g("ws", p)), g("batch", 2)] + ([g("rows", 3)] if rows else []) + [g("heads", 4), g("kv", 2), g("hd", 128), vp(g("pos", p)), g("bound", 10), 0x2DA8]

    step = lambda **kw: L.tce_attention_decode_step_paged_f16(*args(kw, False), None)
    forms = {"tce_attention_decode_step_paged_rows_f16": lambda **kw: L.tce_attention_decode_step_paged_rows_f16(*args(kw, True), None),
             "tce_attention_decode_step_paged_rows_fp8": lambda **kw: L.tce_attention_decode_step_paged_rows_fp8(*args(kw, True), kw.get("k_e", 0), kw.get("v_e", 0), None)}
    for name, rows in forms.items():
        for ptr in ("qkv", "kp", "vpool", "tab", "out", "ws", "pos"):
            assert rows(**{ptr: None}) == BAD and name in capi.last_error() and "null pointer" in capi.last_error(), (name, ptr)
        for kw in _shared_faults(p):
            want = step(**kw)
            assert want in (BAD, SHAPE), kw
            assert rows(**kw) == want, (name, kw)
        for pk in (0, 8, 15, 24, 48, 512, -16):
            assert rows(pk=pk) == BAD and "page_keys" in capi.last_error(), (name, pk)
        for kw in (dict(stride=0), dict(stride=-4), dict(np=0), dict(bound=64), dict(stride=1, pk=16, bound=16)):
            assert rows(**kw) == BAD == step(**kw), (name, kw)
        assert rows(tab=p + 2) == SHAPE and "block_table" in capi.last_error()
        # the rows' own
        for n in (0, 9):
            assert rows(rows=n) == SHAPE and "rows_per_seq" in capi.last_error(), (name, n)
        assert rows(out=p + 8) == SHAPE and "out" in capi.last_error() and "16-byte" in capi.last_error(), name
        assert rows(rows=0, batch=0) == BAD and rows(out=p + 8, kv=3) == BAD, name  # an argument fault wins over a shape fault
    fp8 = forms["tce_attention_decode_step_paged_rows_fp8"]
    for e in (-9, 8):
        assert fp8(k_e=e) == BAD and "k_scale_log2" in capi.last_error() and str(e) in capi.last_error(), e
        assert fp8(v_e=e) == BAD and "v_scale_log2" in capi.last_error() and str(e) in capi.last_error(), e
        assert fp8(k_e=e, hd=64) == BAD, e
    del keep


def test_scatter_gather_and_check_validation_needs_no_gpu(capi):
    L = capi.lib()
    keep, p = _host()
    vp = C.c_void_p
    for fn in (L.tce_kv_pages_scatter_f16, L.tce_kv_pages_gather_f16):
        def call(**kw):
            g = lambda k, d: kw[k] if k in kw else d
            return fn(vp(g("a", p)), vp(g("b", p)), vp(g("c", p)), vp(g("d", p)), vp(g("row", p)), g("stride", 4), g("pk", 16), g("np", 8), g("kv", 2), g("hd", 128),
                      g("mk", 64), g("key0", 3), g("nkeys", 20), None)
        for name in ("a", "b", "c", "d", "row"):
            assert call(**{name: None}) == capi.TCE_ERR_BAD_ARG, name
        for pk in (0, 8, 24, 512):
            assert call(pk=pk) == capi.TCE_ERR_BAD_ARG, pk
        assert call(stride=0) == capi.TCE_ERR_BAD_ARG
        assert call(np=0) == capi.TCE_ERR_BAD_ARG
        assert call(kv=0) == capi.TCE_ERR_BAD_ARG
        assert call(key0=-1) == capi.TCE_ERR_BAD_ARG
        assert call(nkeys=0) == capi.TCE_ERR_BAD_ARG
        assert call(key0=50, nkeys=15) == capi.TCE_ERR_BAD_ARG         # past the contiguous cache's 64 keys
        assert call(mk=128, key0=60, nkeys=5) == capi.TCE_ERR_BAD_ARG  # past the table row's 4 * 16 keys
        assert call(hd=64) == capi.TCE_ERR_UNSUPPORTED_SHAPE
        for name in ("a", "b", "c", "d"):
            assert call(**{name: p + 8}) == capi.TCE_ERR_UNSUPPORTED_SHAPE, name
        assert call(row=p + 2) == capi.TCE_ERR_UNSUPPORTED_SHAPE

    def check(**kw):
        g = lambda k, d: kw[k] if k in kw else d
        return L.tce_kv_block_table_check(vp(g("tab", p)), g("stride", 4), g("pk", 16), g("np", 8), g("batch", 2), vp(g("pos", p)), g("bound", 10), vp(g("viol", p)), None)
    for name in ("tab", "pos", "viol"):
        assert check(**{name: None}) == capi.TCE_ERR_BAD_ARG, name
        assert check(**{name: p + 2}) == capi.TCE_ERR_UNSUPPORTED_SHAPE, name
    for kw in (dict(pk=20), dict(pk=8), dict(stride=0), dict(np=0), dict(batch=0), dict(bound=-1)):
        assert check(**kw) == capi.TCE_ERR_BAD_ARG, kw


@pytest.mark.parametrize("heads,kv_heads", [(32, 8), (32, 32), (4, 1)])
@pytest.mark.parametrize("pos_bound", [0, 319, 320, 1023, 4095])
def test_describe_paged_is_describe_batch_plus_the_page_size(capi, heads, kv_heads, pos_bound):
    L = capi.lib()
    for b in (1, 3, 16):
        for pk in (16, 64, 256):
            a, c = C.create_string_buffer(192), C.create_string_buffer(192)
            assert L.tce_attention_decode_describe_batch(b, heads, kv_heads, pos_bound, a, 192) == capi.TCE_OK
            assert L.tce_attention_decode_describe_paged(b, heads, kv_heads, pos_bound, pk, c, 192) == capi.TCE_OK
            assert c.value.decode() == a.value.decode() + f" page-keys={pk}"
            got = capi.describe_attention_paged(b, heads, kv_heads, pos_bound, pk)
            assert got["page-keys"] == pk and got["batch"] == b and got["waves"] == 4


def test_describe_paged_validates_and_ignores_the_threads_tuning(capi):
    L = capi.lib()
    buf = C.create_string_buffer(192)
    for args in ((0, 32, 8, 10, 64), (2, 32, 5, 10, 64), (2, 0, 1, 10, 64), (2, 32, 8, -1, 64), (2, 32, 8, 10, 48), (2, 32, 8, 10, 8), (2, 32, 8, 10, 512)):
        assert L.tce_attention_decode_describe_paged(*args, buf, 192) == capi.TCE_ERR_BAD_ARG, args
    assert L.tce_attention_decode_describe_paged(2, 32, 8, 10, 64, None, 192) == capi.TCE_ERR_BAD_ARG
    base = capi.describe_attention_paged(2, 32, 8, 2047, 64)
    try:
        assert L.tce_w4a16_set_debug_mode(3000 + 1024) == 0
        assert capi.describe_attention_step(32, 2048, 8)["chunks"] != base["chunks"]  # the setting acts on the single step
        assert capi.describe_attention_paged(2, 32, 8, 2047, 64) == base
        assert L.tce_w4a16_set_debug_mode(2908) == 0
        assert capi.describe_attention_paged(2, 32, 8, 2047, 64) == base
    finally:
        L.tce_w4a16_set_debug_mode(3000)
        L.tce_w4a16_set_debug_mode(2900)
        L.tce_w4a16_set_debug_mode(0)


# ---- PageAllocator on a host table ----
@pytest.fixture()
def PA(capi):
    from tinychatengine_amd.paged_kv import PageAllocator
    return PageAllocator


def _row(a, slot):
    return a.table[slot].tolist()


def test_reserve_grows_by_exactly_the_pages_needed(PA):
    a = PA(32, 16, 4, 8, "cpu")
    assert a.reserve(0, 0) == [0] and a.pages[0] == [0]
    assert a.reserve(0, 15) == [] and a.pages_in_use() == 1
    assert a.reserve(0, 16) == [1]
    assert a.reserve(0, 16) == []
    assert a.reserve(1, 47) == [2, 3, 4]
    assert a.reserve(0, 79) == [5, 6, 7]
    assert a.pages[0] == [0, 1, 5, 6, 7] and a.pages[1] == [2, 3, 4] and a.pages_in_use() == 8
    assert _row(a, 0)[:5] == [0, 1, 5, 6, 7] and _row(a, 1)[:3] == [2, 3, 4]  # the table words are the pages handed out
    assert a.refcount[:8] == [1] * 8 and sum(a.refcount) == 8
    with pytest.raises(ValueError):
        a.reserve(0, 8 * 16)  # past max_pages_per_seq
    with pytest.raises(ValueError):
        a.reserve(0, -1)
    with pytest.raises(IndexError):
        a.reserve(4, 0)
    a.check_invariants()


def test_seeded_page_order_and_table_words(PA):
    order = np.random.default_rng(5).permutation(64).tolist()
    a = PA(64, 64, 2, 16, "cpu", free_order=order)
    got = a.reserve(1, 64 * 5 - 1)
    assert got == order[:5] and _row(a, 1)[:5] == order[:5]
    with pytest.raises(ValueError):
        PA(8, 64, 2, 4, "cpu", free_order=[0, 1, 2, 3, 4, 5, 6, 6])
    with pytest.raises(ValueError):
        PA(8, 48, 2, 4, "cpu")


def test_release_returns_pages_and_a_later_reserve_reuses_them(PA):
    a = PA(8, 16, 3, 4, "cpu")
    a.reserve(0, 40)
    a.reserve(1, 20)
    assert a.pages_in_use() == 5
    freed = a.release(0)
    assert sorted(freed) == [0, 1, 2] and a.pages[0] == [] and a.pages_in_use() == 2
    assert all(a.refcount[p] == 0 for p in freed)
    again = a.reserve(2, 33)
    assert set(again) == set(freed)  # the released pages come back before untouched ones
    assert a.release(0) == []  # an empty slot
    a.check_invariants()


def test_fork_shares_full_pages_and_gives_a_private_last_page(PA):
    a = PA(16, 16, 4, 8, "cpu")
    a.reserve(0, 16 * 3 + 4)  # four pages, the last one holds 5 keys
    src = list(a.pages[0])
    copies = a.fork(0, 1, 16 * 3 + 5)
    assert a.pages[1][:3] == src[:3] and a.pages[1][3] not in src
    assert copies == [(src[3], a.pages[1][3], 5)]
    assert [a.refcount[p] for p in src] == [2, 2, 2, 1] and a.refcount[a.pages[1][3]] == 1
    assert _row(a, 1)[:4] == a.pages[1]
    assert a.appendable_pages(1) == [a.pages[1][3]] and a.appendable_pages(0) == [src[3]]
    # a fork at a page boundary shares everything and copies nothing; the next reserve gives the private page
    assert a.fork(0, 2, 32) == [] and a.pages[2] == src[:2] and [a.refcount[p] for p in src] == [3, 3, 2, 1]
    new = a.reserve(2, 32)
    assert len(new) == 1 and a.refcount[new[0]] == 1 and a.pages[2] == src[:2] + new
    # an append into a shared page is refused by the assertion
    with pytest.raises(AssertionError):
        a.reserve(1, 20)
    with pytest.raises(ValueError):
        a.fork(0, 1, 16)      # destination not empty
    with pytest.raises(ValueError):
        a.fork(0, 3, 16 * 4 + 1)  # more keys than the source's pages hold
    a.check_invariants()


def test_releasing_one_of_two_sharers_frees_nothing_shared(PA):
    a = PA(16, 16, 2, 8, "cpu")
    a.reserve(0, 16 * 3 + 4)
    src = list(a.pages[0])
    a.fork(0, 1, 16 * 3 + 5)
    private = a.pages[1][3]
    assert a.release(1) == [private]
    assert [a.refcount[p] for p in src] == [1, 1, 1, 1] and a.pages[0] == src
    a.fork(0, 1, 40)
    tail = a.pages[1][2]
    freed = a.release(0)  # the source goes first: only its unshared pages are freed
    assert sorted(freed) == sorted(src[2:]) and [a.refcount[p] for p in src[:2]] == [1, 1] and a.pages[1] == src[:2] + [tail]
    assert sorted(a.release(1)) == sorted(src[:2] + [tail])
    assert a.pages_in_use() == 0
    a.check_invariants()


def test_exhaustion_raises_and_changes_nothing(PA):
    from tinychatengine_amd.paged_kv import PagePoolExhausted
    assert issubclass(PagePoolExhausted, MemoryError)
    a = PA(6, 16, 3, 8, "cpu")
    a.reserve(0, 16 * 4 - 1)
    a.reserve(1, 3)

    def snap():
        return ([list(p) for p in a.pages], list(a.free), list(a.refcount), list(a.frozen), a.table.clone())

    before = snap()
    with pytest.raises(MemoryError):
        a.reserve(1, 16 * 3)  # needs 3 more, 1 free
    after = snap()
    assert before[:4] == after[:4] and bool((before[4] == after[4]).all())
    a.reserve(1, 16)  # takes the last page
    before = snap()
    with pytest.raises(PagePoolExhausted):
        a.fork(0, 2, 20)  # the partial page needs a fresh one
    after = snap()
    assert before[:4] == after[:4] and bool((before[4] == after[4]).all())
    assert a.fork(0, 2, 32) == []  # nothing fresh needed: works on an exhausted pool
    a.check_invariants()


def test_two_thousand_random_operations_keep_the_invariants(PA):
    from tinychatengine_amd.paged_kv import PagePoolExhausted
    rng = np.random.default_rng(20260)
    batch, page_keys, max_pages = 8, 16, 12
    a = PA(40, page_keys, batch, max_pages, "cpu", free_order=rng.permutation(40).tolist())
    length = [0] * batch  # keys each slot holds (the model of the caller)
    done = {"reserve": 0, "release": 0, "fork": 0, "exhausted": 0}
    for it in range(2000):
        op = rng.choice(["reserve", "reserve", "reserve", "release", "fork"])
        s = int(rng.integers(0, batch))
        try:
            if op == "reserve":
                grow = int(rng.integers(1, 40))
                upto = min(length[s] + grow, max_pages * page_keys) - 1
                if upto < length[s]:
                    continue
                a.reserve(s, upto)
                length[s] = upto + 1
            elif op == "release":
                a.release(s)
                length[s] = 0
            else:
                d = int(rng.integers(0, batch))
                if d == s or length[d] or not length[s]:
                    continue
                keys = int(rng.integers(1, length[s] + 1))
                copies = a.fork(s, d, keys)
                assert len(copies) == (1 if keys % page_keys else 0)
                for sp, dp, rows in copies:
                    assert rows == keys % page_keys and a.refcount[dp] == 1 and sp == a.pages[s][keys // page_keys] and dp == a.pages[d][-1]
                length[d] = keys
            done[op] += 1
        except PagePoolExhausted:
            done["exhausted"] += 1
        # the invariants, spelled out here as well as in check_invariants
        a.check_invariants()
        held = [p for ps in a.pages for p in ps]
        assert not set(held) & set(a.free), "a page is both free and referenced"
        assert sorted(set(held) | set(a.free)) == list(range(40)), "a page was lost"
        for p in range(40):
            assert a.refcount[p] == held.count(p)
        for slot in range(batch):
            assert len(a.pages[slot]) * page_keys >= length[slot]
            for p in a.pages[slot][length[slot] // page_keys:]:
                assert a.refcount[p] == 1, "a page at or behind the append point is shared"
    assert min(done.values()) > 20, done  # every kind of operation, and exhaustion, happened
