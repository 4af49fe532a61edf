"""CPU (no GPU): sliding-window attention on the paged cache -- PageAllocator.release_behind's bookkeeping on a host table, every refusal of the *_window entry points
(before any HIP call: host buffers stand in for device pointers and are never dereferenced), the cut the windowed step describes and its identity with the unwindowed
step of the re-based launch, and SpeculativeGenerator's refusal of a windowed decoder."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")

import attention_cases as ac  # noqa: E402


@pytest.fixture(scope="module")
def capi():
    from tinychatengine_amd import build as B
    B.build()
    from tinychatengine_amd import capi
    return capi


NAMES = ("tce_attention_decode_describe_paged_window", "tce_attention_decode_step_paged_window_f16", "tce_attention_decode_step_paged_window_fp8",
         "tce_attention_prefill_paged_window_f16", "tce_attention_prefill_paged_window_fp8", "tce_kv_block_table_check_window")
BAD_ARG, UNSUPPORTED = -1, -3


def test_window_symbols_are_exported(capi):
    assert (capi.TCE_ERR_BAD_ARG, capi.TCE_ERR_UNSUPPORTED_SHAPE) == (BAD_ARG, UNSUPPORTED)
    L = capi.lib()
    for n in NAMES:
        assert n in capi.EXPORTS and hasattr(L, n)


# ---- release_behind ----
def _alloc(num_pages=12, page_keys=16, batch=3, stride=8):
    from tinychatengine_amd.paged_kv import PageAllocator
    return PageAllocator(num_pages, page_keys, batch, stride, "cpu")


def test_release_behind_drops_the_pages_wholly_below_the_key_and_nothing_else():
    a = _alloc()
    a.reserve(0, 70)  # pages for keys 0 .. 79: five
    held = list(a.pages[0])
    table0 = a.table.clone()
    assert a.release_behind(0, 0) == [] and a.release_behind(0, -5) == [] and a.release_behind(0, 15) == []
    assert a.pages[0] == held and a.pages_in_use() == 5
    assert a.release_behind(0, 16) == held[:1]  # key 16 is the first of page 1: page 0 lies wholly below
    assert a.release_behind(0, 47) == held[1:2]  # key 47 is in page 2
    assert a.release_behind(0, 47) == [] and a.release_behind(0, 33) == [] and a.release_behind(0, 3) == [], "idempotent, and never backwards"
    assert a.pages[0] == held[2:] and a.gone[0] == 2 and a.pages_in_use() == 3
    assert torch.equal(a.table, table0), "the table words stay as they are"
    a.check_invariants()
    # the freed pages are handed out again, the first page dropped first
    assert a.reserve(1, 20) == [held[1], held[0]]
    a.check_invariants()
    # what the slot still holds is writable and extendable; what it gave back is not
    assert a.writable(0, 32, 48) and not a.writable(0, 31, 2) and not a.writable(0, 0, 1)
    assert a.holds(0, 32, 48) and not a.holds(0, 31, 1) and not a.holds(0, 32, 49)
    added = a.reserve(0, 100)
    assert len(added) == 2 and a.pages[0] == held[2:] + added and a.table[0, 5:7].tolist() == added
    assert a.writable(0, 80, 21)
    with pytest.raises(ValueError):
        a.reserve(0, 31)
    with pytest.raises(ValueError):
        a.reserve_many([(0, 5)])
    a.check_invariants()
    # never more than the slot holds; the slot stays usable for release
    assert len(a.release_behind(0, 10 ** 6)) == 5 and a.pages[0] == [] and a.gone[0] == 7
    a.check_invariants()
    assert a.release(0) == [] and a.gone[0] == 0 and a.pages_in_use() == 2
    assert len(a.reserve(0, 0)) == 1  # a fresh life from key 0
    a.check_invariants()


def test_release_behind_reserve_many_counts_only_missing_pages():
    a = _alloc(num_pages=6, page_keys=16, batch=2, stride=8)
    a.reserve(0, 63)  # 4 pages
    a.reserve(1, 15)  # 1 page
    a.release_behind(0, 32)  # 2 back: 3 free
    from tinychatengine_amd.paged_kv import PagePoolExhausted
    with pytest.raises(PagePoolExhausted):
        a.reserve_many([(0, 111), (1, 31)])  # 3 + 1 needed
    assert a.pages_in_use() == 3 and a.gone == [2, 0]
    added = a.reserve_many([(0, 95), (1, 31)])  # 2 + 1
    assert [len(x) for x in added] == [2, 1] and a.pages_in_use() == 6
    a.check_invariants()


def test_a_shared_page_survives_until_its_last_holder_lets_go():
    a = _alloc()
    a.reserve(0, 40)  # 3 pages
    a.fork(0, 1, 32)  # pages 0 and 1 shared
    shared = a.pages[0][:2]
    assert a.pages[1] == shared and [a.refcount[p] for p in shared] == [2, 2]
    a.reserve(1, 40)
    assert a.release_behind(1, 32) == [], "slot 1 lets go: slot 0 still holds both"
    assert [a.refcount[p] for p in shared] == [1, 1] and a.pages[0][:2] == shared
    a.check_invariants()
    assert a.release_behind(0, 16) == shared[:1]
    assert a.release_behind(0, 32) == shared[1:]
    assert all(a.refcount[p] == 0 for p in shared)
    a.check_invariants()
    assert a.release(1) and a.release(0)
    assert a.pages_in_use() == 0
    a.check_invariants()


def test_fork_is_refused_from_a_slot_whose_leading_pages_are_gone():
    a = _alloc()
    a.reserve(0, 40)
    a.release_behind(0, 16)
    before = (list(a.free), list(a.refcount), [list(p) for p in a.pages])
    with pytest.raises(ValueError):
        a.fork(0, 1, 32)
    assert (list(a.free), list(a.refcount), [list(p) for p in a.pages]) == before
    a.reserve(2, 20)
    a.fork(2, 1, 16)  # an untouched slot forks as ever
    a.check_invariants()


# ---- the C ABI's refusals ----
def _host():
    buf = (C.c_char * 8192)()
    return buf, (C.addressof(buf) + 15) & ~15


def _step_call(L, p, fp8, **kw):
    g = lambda k, d: kw[k] if k in kw else d
    vp = C.c_void_p
    fn = L.tce_attention_decode_step_paged_window_fp8 if fp8 else L.tce_attention_decode_step_paged_window_f16
    scales = (g("ke", 0), g("ve", 0)) if fp8 else ()
    return fn(vp(g("qkv", p)), vp(g("kp", p)), vp(g("vpool", p)), vp(g("table", p)), g("stride", 4), g("pk", 16), g("pages", 8), vp(g("cos", 0)), vp(g("sin", 0)),
              vp(g("out", p)), vp(g("ws", p)), g("batch", 2), g("heads", 4), g("kv", 1), g("hd", 128), vp(g("pos", p)), g("bound", 63), 0x2DA8, *scales, g("window", 8),
              vp(0))


@pytest.mark.parametrize("fp8", [False, True])
def test_windowed_step_refusals_need_no_gpu(capi, fp8):
    L = capi.lib()
    keep, p = _host()
    for w in (0, -1, -2 ** 31):
        assert _step_call(L, p, fp8, window=w) == BAD_ARG and b"window" in L.tce_last_error(), w
    # the unwindowed step's refusals, with its codes
    for fault, code in ((dict(qkv=0), BAD_ARG), (dict(table=0), BAD_ARG), (dict(pk=48), BAD_ARG), (dict(stride=0), BAD_ARG), (dict(batch=0), BAD_ARG),
                        (dict(bound=64), BAD_ARG), (dict(kv=3), BAD_ARG), (dict(cos=p), BAD_ARG), (dict(hd=64), UNSUPPORTED), (dict(batch=65536), UNSUPPORTED),
                        (dict(qkv=p + 8), UNSUPPORTED), (dict(pos=p + 2), UNSUPPORTED)):
        assert _step_call(L, p, fp8, **fault) == code, fault
    if fp8:
        assert _step_call(L, p, True, ke=8) == BAD_ARG and _step_call(L, p, True, ve=-9) == BAD_ARG
    # order: a BAD_ARG rule wins over an UNSUPPORTED_SHAPE rule, whichever argument carries it
    assert _step_call(L, p, fp8, window=0, hd=64) == BAD_ARG and b"window" in L.tce_last_error()
    assert _step_call(L, p, fp8, window=0, qkv=p + 8) == BAD_ARG
    assert _step_call(L, p, fp8, window=0, batch=65536) == BAD_ARG
    # and the pages' own rules come first, as in every entry point of the family
    assert _step_call(L, p, fp8, window=0, pk=48) == BAD_ARG and b"page_keys" in L.tce_last_error()
    del keep


def _prefill_call(L, p, fp8, segs, **kw):
    g = lambda k, d: kw[k] if k in kw else d
    vp = C.c_void_p
    fn = L.tce_attention_prefill_paged_window_fp8 if fp8 else L.tce_attention_prefill_paged_window_f16
    scales = (g("ke", 0), g("ve", 0)) if fp8 else ()
    return fn(vp(g("qkv", p)), 0, vp(g("kp", p)), vp(g("vpool", p)), vp(g("table", p)), g("rows", 2), g("stride", 4), g("pk", 16), g("pages", 8), vp(g("cos", 0)),
              vp(g("sin", 0)), g("causal", 1), vp(g("out", p)), 0, vp(g("ws", p)), g("heads", 4), g("kv", 1), g("hd", 128), C.cast(segs, vp), g("nseg", 1),
              g("total", 5), 0x2DA8, *scales, g("window", 8), vp(0))


@pytest.mark.parametrize("fp8", [False, True])
def test_windowed_prefill_refusals_need_no_gpu(capi, fp8):
    L = capi.lib()
    keep, p = _host()
    segs, total = capi.prefill_segments([(0, 3, 5)])
    assert total == 5
    for w in (0, -1):
        assert _prefill_call(L, p, fp8, segs, window=w) == BAD_ARG and b"window" in L.tce_last_error(), w
    assert _prefill_call(L, p, fp8, segs, causal=0) == BAD_ARG and b"causal" in L.tce_last_error()
    for fault, code in ((dict(qkv=0), BAD_ARG), (dict(pk=48), BAD_ARG), (dict(rows=0), BAD_ARG), (dict(kv=3), BAD_ARG), (dict(nseg=17), BAD_ARG), (dict(total=4), BAD_ARG),
                        (dict(hd=64), UNSUPPORTED), (dict(qkv=p + 8), UNSUPPORTED), (dict(ws=p + 8), UNSUPPORTED)):
        assert _prefill_call(L, p, fp8, segs, **fault) == code, fault
    assert _prefill_call(L, p, fp8, segs, window=0, hd=64) == BAD_ARG and _prefill_call(L, p, fp8, segs, causal=0, qkv=p + 8) == BAD_ARG
    assert _prefill_call(L, p, fp8, segs, causal=0, ws=p + 8) == BAD_ARG
    del keep


def test_table_check_and_describe_refusals_need_no_gpu(capi):
    L = capi.lib()
    keep, p = _host()
    vp = C.c_void_p
    chk = lambda **kw: L.tce_kv_block_table_check_window(vp(kw.get("table", p)), kw.get("stride", 4), kw.get("pk", 16), 8, kw.get("batch", 2), vp(kw.get("pos", p)),
                                                        kw.get("bound", 63), vp(kw.get("viol", p)), kw.get("window", 8), vp(0))
    for fault, code in ((dict(window=0), BAD_ARG), (dict(window=-3), BAD_ARG), (dict(table=0), BAD_ARG), (dict(pos=0), BAD_ARG), (dict(viol=0), BAD_ARG), (dict(pk=8), BAD_ARG),
                        (dict(batch=0), BAD_ARG), (dict(bound=-1), BAD_ARG), (dict(pos=p + 2), UNSUPPORTED), (dict(window=0, pos=p + 2), BAD_ARG)):
        assert chk(**fault) == code, fault
    buf = C.create_string_buffer(192)
    d = lambda **kw: L.tce_attention_decode_describe_paged_window(kw.get("batch", 2), kw.get("heads", 4), kw.get("kv", 1), kw.get("bound", 63), kw.get("pk", 16),
                                                                  kw.get("window", 8), kw.get("buf", buf), kw.get("len", 192))
    assert d() == 0
    for fault in (dict(window=0), dict(window=-1), dict(batch=0), dict(kv=3), dict(bound=-1), dict(pk=24), dict(buf=None), dict(len=0)):
        assert d(**fault) == BAD_ARG, fault
    del keep


# ---- the cut ----
WINDOWS = (1,) + tuple(n - 3 for n in ac.SIZES if n > 3)


def test_the_window_sizes_are_the_chunk_rules():
    assert WINDOWS == (1, 2, 14, 125, 317, 318, 638, 1022)


@pytest.mark.parametrize("heads,kv_heads", [(4, 1), (8, 8), (32, 8)])
def test_describe_window_follows_the_window_not_the_bound(capi, heads, kv_heads):
    for pk in (16, 64):
        for W in WINDOWS:
            # B's identity: the windowed launch with bound 2047 and the unwindowed launch with bound W + 2 are cut alike
            win = capi.describe_attention_paged_window(3, heads, kv_heads, 2047, pk, W)
            ref = capi.describe_attention_paged(3, heads, kv_heads, W + 2, pk)
            assert win == ref, (W, win, ref)
            assert win["chunks"] * win["keys-per-chunk"] >= W + 3 and win["waves"] == 4
        for bound in (0, 63, 319, 320, 1023, 2047):
            # never binding: today's cut
            for W in (bound + 1, bound + 2, 2 ** 30, 2 ** 31 - 1):
                assert capi.describe_attention_paged_window(3, heads, kv_heads, bound, pk, W) == capi.describe_attention_paged(3, heads, kv_heads, bound, pk), (bound, W)
            # binding by less than three keys: still the bound's cut (the span cannot exceed pos_bound + 1)
            for W in (bound, bound - 1, bound - 2):
                if W >= 1:
                    assert capi.describe_attention_paged_window(3, heads, kv_heads, bound, pk, W) == capi.describe_attention_paged(3, heads, kv_heads, bound, pk), (bound, W)
    far = capi.describe_attention_paged_window(16, heads, kv_heads, 32767, 64, 4096)
    near = capi.describe_attention_paged(16, heads, kv_heads, 4098, 64)
    assert far == near and far["workgroups"] < capi.describe_attention_paged(16, heads, kv_heads, 32767, 64)["workgroups"]


# ---- python fronts ----
def test_speculative_generator_refuses_a_windowed_decoder():
    from tinychatengine_amd.speculative import SpeculativeGenerator

    class _Windowed:
        window, rows_per_seq = 32, 2

    with pytest.raises(ValueError, match="window"):
        SpeculativeGenerator([_Windowed()], None, None, None, max_new=4)


def test_window_argument_is_validated(capi):
    from tinychatengine_amd.paged_kv import PagedBatchDecodeAttention
    from tinychatengine_amd.speculative import PagedRowsDecodeAttention
    a = _alloc()
    for bad in (0, -1, 1.5, 2 ** 31):
        with pytest.raises(ValueError):
            PagedBatchDecodeAttention(a, 4, 1, "cpu", window=bad)
    with pytest.raises(ValueError, match="window"):
        PagedRowsDecodeAttention(a, 4, 1, "cpu", rows_per_seq=2, window=8)
