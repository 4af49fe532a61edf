"""CPU (no GPU): the paged prefill's C ABI -- exports, workspace size, every refusal before any HIP call (host buffers stand in for device pointers and are never
dereferenced), the cut it describes -- and the allocator's side of admission on a host table: PageAllocator.writable and the all-or-nothing reservation
PagedBatchedDecoder.prefill_many rests on (PageAllocator.reserve_many)."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def capi():
    from tinychatengine_amd import build as B
    B.build()
    from tinychatengine_amd import capi
    return capi


NAMES = ("tce_attention_prefill_paged_workspace_bytes", "tce_attention_prefill_paged_f16", "tce_attention_prefill_describe_paged")


def test_paged_prefill_symbols_are_exported(capi):
    L = capi.lib()
    for n in NAMES:
        assert n in capi.EXPORTS
        assert hasattr(L, n)
    assert L.tce_version() == 113
    assert capi.TCE_PREFILL_MAX_SEGMENTS == 16 and C.sizeof(capi.PrefillSegment) == 16


def test_workspace_bytes(capi):
    L = capi.lib()
    for heads, rows in ((32, 100), (4, 1), (8, 4096), (32, 8192)):
        assert int(L.tce_attention_prefill_paged_workspace_bytes(heads, rows, 128)) == heads * rows * 128 * 2
    assert int(L.tce_attention_prefill_paged_workspace_bytes(32, 100, 64)) == 0
    assert int(L.tce_attention_prefill_paged_workspace_bytes(0, 100, 128)) == 0
    assert int(L.tce_attention_prefill_paged_workspace_bytes(32, 0, 128)) == 0


def _host():
    buf = (C.c_char * 8192)()
    return buf, (C.addressof(buf) + 15) & ~15


def _segs(capi, quads):
    arr = (capi.PrefillSegment * max(len(quads), 1))()
    for i, q in enumerate(quads):
        arr[i] = capi.PrefillSegment(*q)
    return arr


def test_paged_prefill_argument_validation_needs_no_gpu(capi):
    L = capi.lib()
    keep, p = _host()
    vp = C.c_void_p
    BAD, SHAPE = capi.TCE_ERR_BAD_ARG, capi.TCE_ERR_UNSUPPORTED_SHAPE
    good = [(0, 0, 8, 0), (1, 5, 4, 8)]  # (slot, pos, m, row0): 12 rows

    def call(**kw):
        g = lambda k, d: kw[k] if k in kw else d
        quads = g("segs", good)
        arr = _segs(capi, quads)
        seg_ptr = kw["seg_ptr"] if "seg_ptr" in kw else C.cast(arr, vp)
        return L.tce_attention_prefill_paged_f16(vp(g("qkv", p)), g("ld_qkv", 0), vp(g("kp", p)), vp(g("vpool", p)), vp(g("tab", p)), g("rows", 2), g("stride", 4), g("pk", 16),
                                                 g("np", 8), vp(g("cos", None)), vp(g("sin", None)), g("causal", 1), vp(g("out", p)), g("ld_out", 0), vp(g("ws", p)),
                                                 g("heads", 4), g("kv", 2), g("hd", 128), seg_ptr, g("n", len(quads)), g("total", 12), 0x2DA8, None)

    # null pointers
    for k in ("qkv", "kp", "vpool", "tab", "out", "ws"):
        assert call(**{k: None}) == BAD and "null pointer" in capi.last_error(), k
    assert call(seg_ptr=None) == BAD
    assert call(cos=p) == BAD and "come together" in capi.last_error()
    # misaligned pointers: tce_attention_prefill_f16's codes
    assert call(qkv=p + 2) == SHAPE
    assert call(kp=p + 8) == SHAPE and call(vpool=p + 8) == SHAPE and call(ws=p + 8) == SHAPE
    assert call(out=p + 4) == SHAPE                      # 8-byte stores
    assert call(ld_out=4 * 128 + 2) == SHAPE
    assert call(ld_qkv=100) == BAD                       # shorter than a row
    assert call(ld_qkv=8 * 128 + 4) == SHAPE             # 16-byte pieces
    assert call(tab=p + 2) == SHAPE and "int32-aligned" in capi.last_error()
    # shapes
    assert call(hd=64) == SHAPE
    assert call(kv=3) == BAD and "do not divide" in capi.last_error()
    assert call(heads=0) == BAD
    for pk in (0, 8, 15, 48, 512, -16):
        assert call(pk=pk) == BAD and "page_keys" in capi.last_error(), pk
    assert call(stride=0) == BAD and call(np=0) == BAD and call(rows=0) == BAD
    assert call(total=0) == BAD
    # the segment list
    assert call(n=0) == BAD and call(n=17, segs=[(i, 0, 1, i) for i in range(17)], rows=32, total=17) == BAD and "num_segments" in capi.last_error()
    assert call(segs=[(0, 0, 0, 0)], total=4) == BAD and "segment 0" in capi.last_error()            # m < 1
    assert call(segs=[(0, 0, 4, 0), (1, -1, 4, 4)]) == BAD and "segment 1" in capi.last_error()      # pos < 0
    assert call(segs=[(0, 60, 5, 0)]) == BAD and "segment 0" in capi.last_error()                    # pos + m > 4 * 16
    assert call(segs=[(0, 0, 4, 0), (2, 0, 4, 4)]) == BAD and "segment 1" in capi.last_error() and "slot" in capi.last_error()
    assert call(segs=[(-1, 0, 4, 0)]) == BAD and "slot" in capi.last_error()
    assert call(segs=[(0, 0, 4, 9)]) == BAD and "rows" in capi.last_error()                          # rows 9 .. 12 of 12
    assert call(segs=[(0, 0, 4, -1)]) == BAD
    assert call(segs=[(0, 0, 4, 0), (0, 0, 4, 4)]) == BAD and "segment 1" in capi.last_error() and "race" in capi.last_error()   # the same slot twice
    assert call(segs=[(0, 0, 6, 0), (1, 0, 4, 5)]) == BAD and "overlap" in capi.last_error()
    assert call(segs=[(0, 0, 4, 4), (1, 0, 6, 0)]) == BAD and "overlap" in capi.last_error()
    del keep


def _rule(heads, ms, causal):
    """The rule of launch_attention_prefill (csrc/attention_prefill.hip), restated: blocks of 128 rows (8 waves) once there are 512 of them over all heads, else 64
    rows (4 waves); causal launches pair blocks while the blocks still number 512."""
    blocks = lambda rows: sum((m + rows - 1) // rows for m in ms) * heads
    form = 8 if blocks(128) >= 512 else 4
    rows = 128 if form == 8 else 64
    pair = bool(causal) and blocks(rows) >= 512
    nb = blocks(rows) // heads
    return {"form": form, "rows-per-block": rows, "pair": "yes" if pair else "no", "blocks": nb, "workgroups": ((nb + 1) // 2 if pair else nb) * heads, "segments": len(ms)}


@pytest.mark.parametrize("heads,kv_heads", [(32, 8), (8, 8), (4, 1)])
@pytest.mark.parametrize("causal", [True, False])
def test_describe_names_the_contiguous_launchs_form_for_one_segment(capi, heads, kv_heads, causal):
    capi.check(capi.lib().tce_w4a16_set_debug_mode(2950))
    for m in (1, 2, 17, 64, 65, 130, 300, 512, 1023, 1024, 1025, 2048, 4096, 8192):
        for pos in (0, 37, 7680):
            assert capi.describe_prefill_paged(heads, kv_heads, causal, [(0, pos, m)]) == _rule(heads, [m], causal), (m, pos)


def test_describe_ragged_launches_and_forced_forms(capi):
    L = capi.lib()
    capi.check(L.tce_w4a16_set_debug_mode(2950))
    ms = [64] * 8 + [30] * 4
    assert capi.describe_prefill_paged(32, 8, True, [(i, 0, m) for i, m in enumerate(ms)]) == _rule(32, ms, True)
    ms = [2048, 1, 3, 300, 2048, 1024]
    d = capi.describe_prefill_paged(32, 8, True, [(i, 5, m) for i, m in enumerate(ms)])
    assert d == _rule(32, ms, True) and d["form"] == 8 and d["pair"] == "yes"
    try:
        for mode, form, rows in ((2954, 4, 64), (2958, 8, 128), (2964, 14, 128), (2968, 18, 256)):
            capi.check(L.tce_w4a16_set_debug_mode(mode))
            d = capi.describe_prefill_paged(8, 2, True, [(0, 0, 300), (1, 9, 40)])
            assert (d["form"], d["rows-per-block"], d["blocks"]) == (form, rows, -(-300 // rows) + 1), mode
        capi.check(L.tce_w4a16_set_debug_mode(2704))
        assert capi.describe_prefill_paged(8, 2, True, [(0, 0, 300)]) == {"form": 4, "rows-per-block": 64, "pair": "yes", "blocks": 5, "workgroups": 3 * 8, "segments": 1}
        capi.check(L.tce_w4a16_set_debug_mode(2808))
        assert capi.describe_prefill_paged(32, 8, True, [(0, 0, 4096)])["pair"] == "no"
    finally:
        capi.check(L.tce_w4a16_set_debug_mode(2950))
    # refused lists: NULL and a message
    with pytest.raises(capi.TceError, match="segment 1"):
        capi.describe_prefill_paged(8, 2, True, [(0, 0, 4), (1, 0, 0)])
    with pytest.raises(capi.TceError, match="do not divide"):
        capi.describe_prefill_paged(8, 3, True, [(0, 0, 4)])
    with pytest.raises(capi.TceError, match="at most 1024"):
        capi.describe_prefill_paged(8, 2, True, [(i, 0, 16384) for i in range(16)])  # 16 x 128 blocks of 128 rows
    assert capi.describe_prefill_paged(8, 2, True, [(i, 0, 8192) for i in range(16)])["blocks"] == 1024


def _alloc(num_pages=12, page_keys=16, batch=4, stride=6, order=None):
    import torch
    from tinychatengine_amd.paged_kv import PageAllocator
    return PageAllocator(num_pages, page_keys, batch, stride, torch.device("cpu"), free_order=order)


def test_writable_over_fork_reserve_release():
    a = _alloc()
    assert not a.writable(0, 0, 1)                      # nothing reserved
    a.reserve(0, 52)                                    # 53 keys: pages 0 .. 3 of slot 0
    assert a.writable(0, 0, 53) and a.writable(0, 0, 64) and a.writable(0, 63, 1)
    assert not a.writable(0, 0, 65) and not a.writable(0, 64, 1)   # the fifth page does not exist
    assert not a.writable(0, -1, 2) and not a.writable(0, 0, 0)
    with pytest.raises(IndexError):
        a.writable(4, 0, 1)
    # fork after 3 full pages + 4 rows of a partial one: the full pages become read-only for both, the partial page is each slot's own
    copies = a.fork(0, 1, 52)
    assert len(copies) == 1 and copies[0][2] == 4
    for slot in (0, 1):
        assert not a.writable(slot, 0, 1) and not a.writable(slot, 47, 1) and not a.writable(slot, 40, 20)   # inside / starting inside the shared prefix
        assert a.writable(slot, 48, 16) and a.writable(slot, 52, 12)
    # the gap reserve() leaves: a chunk that STARTS in a shared page and ends in an own one passes reserve's check of the last key's page only
    a.reserve(1, 70)
    assert not a.writable(1, 40, 31) and a.writable(1, 48, 23)
    # release the source: the pages are the fork's alone now, but they stay behind its frozen prefix (they were shared: never the target of an append)
    a.release(0)
    assert not a.writable(0, 0, 1)
    assert all(a.refcount[p] == 1 for p in a.pages[1]) and not a.writable(1, 0, 48) and a.writable(1, 48, 23)
    # release and reuse: a fresh owner writes everything
    a.release(1)
    a.reserve(2, 20)
    assert a.writable(2, 0, 21) and a.writable(2, 0, 32) and not a.writable(2, 0, 33)
    a.check_invariants()


def test_reserve_many_is_all_or_nothing_on_a_host_table():
    from tinychatengine_amd.paged_kv import PagePoolExhausted
    order = [5, 2, 7, 0, 1, 3, 4, 6]
    a = _alloc(num_pages=8, page_keys=16, batch=4, stride=6, order=order)
    a.reserve(3, 20)                                    # two pages in use, six free
    before = ([list(p) for p in a.pages], list(a.free), list(a.refcount), a.table.clone())

    def unchanged():
        return [list(p) for p in a.pages] == before[0] and a.free == before[1] and a.refcount == before[2] and bool((a.table == before[3]).all())

    # 3 + 2 + 2 = 7 pages wanted, 6 free: the first two would fit on their own, and still nothing may change
    with pytest.raises(PagePoolExhausted):
        a.reserve_many([(0, 40), (1, 17), (2, 31)])
    assert unchanged()
    # counts what a slot already holds: slot 3 needs one more page for key 40, 1 + 3 + 3 = 7 > 6
    with pytest.raises(PagePoolExhausted):
        a.reserve_many([(3, 40), (0, 40), (1, 40)])
    assert unchanged()
    # bad arguments are found before anything changes as well
    with pytest.raises(ValueError):
        a.reserve_many([(0, 10), (1, 6 * 16)])          # past a slot's table row
    with pytest.raises(ValueError):
        a.reserve_many([(0, 10), (0, 20)])              # a slot twice
    with pytest.raises(IndexError):
        a.reserve_many([(0, 10), (4, 10)])
    assert unchanged()
    # exactly what is free: 1 + 3 + 2 = 6
    added = a.reserve_many([(3, 40), (0, 40), (1, 17)])
    assert [len(x) for x in added] == [1, 3, 2] and not a.free
    assert added[0] + added[1] + added[2] == order[2:]  # handed out in free_order, entry by entry
    assert a.table[0, :3].tolist() == added[1] and a.table[1, :2].tolist() == added[2] and a.table[3, :3].tolist() == order[:2] + added[0]
    assert a.writable(0, 0, 41) and a.writable(1, 0, 18) and a.writable(3, 0, 41)
    a.check_invariants()
