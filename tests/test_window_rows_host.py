"""CPU (no GPU): sliding windows on the multi-row step and on admission -- every refusal of tce_attention_decode_step_paged_rows_window_f16 / _fp8 (before any HIP
call: host buffers stand in for device pointers and are never dereferenced), the table-check identity the rows form uses instead of an entry point of its own, the
chunk / reserve / release schedule of admit(..., chunk_rows=N) against a brute-force run on a PageAllocator, and the constructors that used to refuse a window."""
import ctypes as C
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def capi():
    from tinychatengine_amd import build as B
    B.build()
    from tinychatengine_amd import capi
    return capi


NAMES = ("tce_attention_decode_step_paged_rows_window_f16", "tce_attention_decode_step_paged_rows_window_fp8")
BAD_ARG, UNSUPPORTED = -1, -3
PAGE_KEYS = 16
WINDOWS = (1, 2, 3, 5, 8, PAGE_KEYS, PAGE_KEYS + 1, 2 * PAGE_KEYS + 3)  # tests/test_gpu_window_rows.py's
ROWS = (1, 2, 5, 8)


def test_rows_window_symbols_are_exported(capi):
    assert (capi.TCE_ERR_BAD_ARG, capi.TCE_ERR_UNSUPPORTED_SHAPE) == (BAD_ARG, UNSUPPORTED)
    L = capi.lib()
    for n in NAMES:
        assert n in capi.EXPORTS and hasattr(L, n)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tce_matmul.h")).read()
    assert all(n + "(" in header for n in NAMES)
    assert "NOT BUILT: the multi-row" not in header


# ---- the C ABI's refusals ----
def _host():
    buf = (C.c_char * 8192)()
    return buf, (C.addressof(buf) + 15) & ~15


def _call(L, p, fp8, **kw):
    g = lambda k, d: kw[k] if k in kw else d
    vp = C.c_void_p
    fn = L.tce_attention_decode_step_paged_rows_window_fp8 if fp8 else L.tce_attention_decode_step_paged_rows_window_f16
    scales = (g("ke", 0), g("ve", 0)) if fp8 else ()
    return fn(vp(g("qkv", p)), vp(g("kp", p)), vp(g("vpool", p)), vp(g("table", p)), g("stride", 4), g("pk", 16), g("pages", 8), vp(g("cos", 0)), vp(g("sin", 0)),
              vp(g("out", p)), vp(g("ws", p)), g("batch", 2), g("rows", 4), g("heads", 4), g("kv", 1), g("hd", 128), vp(g("pos", p)), g("bound", 63), 0x2DA8, *scales,
              g("window", 8), vp(0))


@pytest.mark.parametrize("fp8", [False, True])
def test_rows_window_step_refusals_need_no_gpu(capi, fp8):
    L = capi.lib()
    keep, p = _host()
    for w in (0, -1, -2 ** 31):
        assert _call(L, p, fp8, window=w) == BAD_ARG and b"window" in L.tce_last_error(), w
    for r in (0, 9, -1):
        assert _call(L, p, fp8, rows=r) == UNSUPPORTED and b"rows_per_seq" in L.tce_last_error(), r
    # the two parents' refusals, with their codes
    for fault, code in ((dict(qkv=0), BAD_ARG), (dict(kp=0), BAD_ARG), (dict(vpool=0), BAD_ARG), (dict(table=0), BAD_ARG), (dict(out=0), BAD_ARG), (dict(ws=0), BAD_ARG),
                        (dict(pos=0), BAD_ARG), (dict(pk=48), BAD_ARG), (dict(pk=8), BAD_ARG), (dict(pk=512), BAD_ARG), (dict(stride=0), BAD_ARG), (dict(pages=0), BAD_ARG),
                        (dict(batch=0), BAD_ARG), (dict(bound=64), BAD_ARG), (dict(bound=-1), BAD_ARG), (dict(kv=3), BAD_ARG), (dict(cos=p), BAD_ARG),
                        (dict(hd=64), UNSUPPORTED), (dict(batch=65536), UNSUPPORTED), (dict(qkv=p + 8), UNSUPPORTED), (dict(pos=p + 2), UNSUPPORTED),
                        (dict(out=p + 8), UNSUPPORTED)):  # (out: the rows form stores it in 16-byte pieces)
        assert _call(L, p, fp8, **fault) == code, fault
    if fp8:
        assert _call(L, p, True, ke=8) == BAD_ARG and _call(L, p, True, ve=-9) == BAD_ARG
    # order: a BAD_ARG rule wins over an UNSUPPORTED_SHAPE rule, whichever argument carries it
    assert _call(L, p, fp8, window=0, rows=9) == BAD_ARG and b"window" in L.tce_last_error()
    assert _call(L, p, fp8, window=0, rows=0) == BAD_ARG
    assert _call(L, p, fp8, bound=64, rows=9) == BAD_ARG
    assert _call(L, p, fp8, window=0, hd=64) == BAD_ARG and _call(L, p, fp8, window=-1, out=p + 8) == BAD_ARG
    assert _call(L, p, fp8, rows=9, kp=0) == BAD_ARG
    # and the pages' own rules come first, as in every entry point of the family
    assert _call(L, p, fp8, window=0, pk=48) == BAD_ARG and b"page_keys" in L.tce_last_error()
    assert _call(L, p, fp8, rows=9, pk=48) == BAD_ARG and b"page_keys" in L.tce_last_error()
    del keep


# ---- the table check the rows form uses ----
def _words(pos, W):
    """the table words a windowed row at `pos` follows"""
    return set(range(max(0, pos - W + 1) // PAGE_KEYS, pos // PAGE_KEYS + 1))


def _start_positions(W):
    return sorted({0, max(0, W - 2), W + 2, W + PAGE_KEYS - 2, 2 * PAGE_KEYS - 2})  # tests/test_gpu_window_rows.py's


def test_rows_follow_the_words_of_the_last_row_with_a_window_wider_by_the_rows_in_front():
    """A sequence's active rows p .. p + n - 1 with window W follow exactly the words tce_kv_block_table_check_window follows for position p + n - 1 with window
    W + n - 1: by enumeration, for the GPU test's windows and starts and every p up to 200 besides."""
    for W in WINDOWS + (400,):
        for p in sorted(set(_start_positions(W)) | set(range(200))):
            for n in range(1, 9):
                union = set().union(*(_words(p + t, W) for t in range(n)))
                assert union == _words(p + n - 1, W + n - 1), (W, p, n)


def test_rows_check_calls_cover_every_sequence_once():
    from tinychatengine_amd.speculative import rows_check_calls
    # unwindowed: one call at the last positions
    assert rows_check_calls([4, 0, 3], [13, -1, 40], 4, None) == [(None, [13, -1, 40])]
    # windowed: one call per distinct row count, the window wider by n - 1, the other sequences inactive in it
    calls = rows_check_calls([4, 0, 3, 4, 1], [13, -1, 40, 7, 99], 4, 8)
    assert calls == [(8, [-1, -1, -1, -1, 99]), (10, [-1, -1, 40, -1, -1]), (11, [13, -1, -1, 7, -1])]
    assert rows_check_calls([0, 0], [-1, -1], 8, 5) == []
    rng = np.random.default_rng(3)
    for _ in range(200):
        T, W = int(rng.integers(1, 9)), int(rng.integers(1, 40))
        n = rng.integers(0, T + 1, 6).tolist()
        last = [int(rng.integers(m - 1, 300)) if m else -1 for m in n]
        seen = [0] * 6
        for w, words in rows_check_calls(n, last, T, W):
            for b, q in enumerate(words):
                if q >= 0:
                    seen[b] += 1
                    assert q == last[b] and w == W + n[b] - 1
        assert seen == [1 if m else 0 for m in n]
    with pytest.raises(ValueError):
        rows_check_calls([1], [0], 9, 4)


# ---- the admission schedule ----
def _alloc(num_pages, batch=3, stride=64):
    from tinychatengine_amd.paged_kv import PageAllocator
    return PageAllocator(num_pages, PAGE_KEYS, batch, stride, "cpu")


def _state(a):
    """What the allocator's behaviour depends on, but for the ORDER of the free stack (pages that went out and came back may lie in another order) and the table
    words of slots that hold nothing (never followed)."""
    return (sorted(a.free), list(a.refcount), [list(p) for p in a.pages], list(a.gone), list(a.frozen))


def _run_plan(a, slots, plan):
    """admit's loop on the allocator alone; returns the peak pages per slot.  On PagePoolExhausted the slots are released, as admit does, and the error passes on."""
    from tinychatengine_amd.paged_kv import PagePoolExhausted
    peak = [0] * len(slots)
    try:
        for rnd in plan:
            a.reserve_many([(slots[i], upto) for i, upto in rnd["reserve"]])
            for i, c0, m in rnd["segments"]:
                assert a.writable(slots[i], c0, m), "a chunk's rows are not in pages of the slot's own"
                peak[i] = max(peak[i], len(a.pages[slots[i]]))
            for i, key in rnd["release"]:
                a.release_behind(slots[i], key)
            a.check_invariants()
    except PagePoolExhausted:
        for s in slots:
            a.release(s)
        raise
    return peak


def test_admission_chunks_is_the_brute_force_schedule():
    from tinychatengine_amd.generate import admission_chunks
    for lengths, N, W in (([77], 13, 24), ([77, 5, 40], 13, 24), ([1], 1, 1), ([30, 31, 32], 16, None), ([100], 7, 3), ([64, 65], 64, 16), ([9], 100, 4)):
        plan = admission_chunks(lengths, N, W)
        # brute force: walk every prompt row by row
        covered = [[] for _ in lengths]
        for r, rnd in enumerate(plan):
            want_segs = [(i, r * N, min(N, n - r * N)) for i, n in enumerate(lengths) if n > r * N]
            assert rnd["segments"] == want_segs
            assert rnd["reserve"] == [(i, c0 + m - 1) for i, c0, m in want_segs]
            assert rnd["release"] == ([] if W is None else [(i, c0 + m - W) for i, c0, m in want_segs])
            for i, c0, m in rnd["segments"]:
                assert 1 <= m <= N
                covered[i] += list(range(c0, c0 + m))
        assert covered == [list(range(n)) for n in lengths] and len(plan) == (max(lengths) + N - 1) // N
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError):
            admission_chunks([5], bad, 4)
    with pytest.raises(ValueError):
        admission_chunks([5], 2, 0)
    with pytest.raises(ValueError):
        admission_chunks([], 2, 4)


def test_a_windowed_slots_pages_stay_within_the_bound_whatever_the_prompt_length():
    """Every key a later chunk or step weighs is still held: the release after a chunk that ends at key e - 1 keeps key e - W + 1, the first one the row at e weighs."""
    from tinychatengine_amd.generate import admission_chunks
    from tinychatengine_amd.paged_kv import PagePoolExhausted
    for W in (1, 5, 16, 24, 35, 100):
        for N in (1, 7, 13, 16, 50):
            bound = (W + N + PAGE_KEYS - 1) // PAGE_KEYS + 1
            for lengths in ([3 * W + 5], [1], [250, 17, 3 * W + 5]):
                a = _alloc(num_pages=bound * len(lengths))  # exactly the bound per slot: the schedule must fit
                peak = _run_plan(a, list(range(len(lengths))), admission_chunks(lengths, N, W))
                assert max(peak) <= bound, (W, N, lengths, peak)
                for s, n in enumerate(lengths):
                    first = max(0, n - W + 1)  # the first key the first generated token's row (position n) weighs; its own it appends itself
                    assert (first == n or a.holds(s, first, n - first)) and len(a.pages[s]) <= bound
            # one-shot admission of the long prompt does not fit the same pool
            if (3 * W + 5 + PAGE_KEYS - 1) // PAGE_KEYS > bound:
                with pytest.raises(PagePoolExhausted):
                    _alloc(num_pages=bound).reserve_many([(0, 3 * W + 4)])
    # without windows nothing is released: the pages are the prompt's
    a = _alloc(num_pages=8)
    assert _run_plan(a, [0], admission_chunks([100], 13, None)) == [7] and a.gone[0] == 0


def test_exhaustion_in_a_later_chunk_leaves_the_allocator_as_it_was():
    from tinychatengine_amd.generate import admission_chunks
    from tinychatengine_amd.paged_kv import PagePoolExhausted
    W, N = 24, 32
    plan = admission_chunks([3 * N], N, None)  # three chunks of two pages, nothing released in between
    assert len(plan) == 3
    a = _alloc(num_pages=7)
    a.reserve(2, 3 * PAGE_KEYS - 1)  # another sequence holds three of the seven pages: chunk 0 and chunk 1 fit, chunk 2 does not
    a.release_behind(2, PAGE_KEYS)
    a.reserve(2, 4 * PAGE_KEYS - 1)
    before = _state(a)
    with pytest.raises(PagePoolExhausted):
        _run_plan(a, [0], plan)
    assert _state(a) == before, "the failed admission left something behind"
    a.check_invariants()
    # exhaustion in chunk 2 of 3 with windows, two admissions in the round: all or nothing across them, and both slots come back empty
    plan = admission_chunks([3 * N, 3 * N], N, 2 * N)
    b = _alloc(num_pages=11)
    b.reserve(2, 0)
    before = _state(b)
    with pytest.raises(PagePoolExhausted):
        _run_plan(b, [0, 1], plan)  # rounds 0 and 1 take 2 x 4 of the 10 free pages and give none back (keys 32 - 64, 64 - 64); round 2 needs 2 x 2 more
    assert _state(b) == before
    b.check_invariants()


# ---- python fronts ----
def test_rows_attention_validates_rows_and_window_without_a_device(capi):
    """The "not built" refusal is gone.  What a host table still meets with a window is the rule that the windowed form is a device form (the unwindowed one may be
    built over a host table); the windowed object itself is built in tests/test_gpu_window_rows.py."""
    from tinychatengine_amd.speculative import PagedRowsDecodeAttention
    a = _alloc(12, stride=8)
    R = PagedRowsDecodeAttention(a, 8, 2, "cpu", rows_per_seq=4)
    assert R.window is None and R._entry("tce_attention_decode_step_paged_rows") == "tce_attention_decode_step_paged_rows"
    need = int(capi.lib().tce_attention_decode_batch_workspace_bytes(a.batch * 4, 8, a.max_keys, 128))
    assert R.workspace.numel() == need > 0, "a workspace slice per virtual row"
    R.window = 8  # (what the constructor sets on a device table)
    assert R._entry("tce_attention_decode_step_paged_rows") == "tce_attention_decode_step_paged_rows_window" and R._window() == (8,)
    with pytest.raises(ValueError, match="on the device") as e:
        PagedRowsDecodeAttention(a, 8, 2, "cpu", rows_per_seq=4, window=8)
    assert "not built" not in str(e.value)
    for bad in (0, 9, -1):
        with pytest.raises(ValueError, match="rows_per_seq"):
            PagedRowsDecodeAttention(a, 8, 2, "cpu", rows_per_seq=bad, window=8)


def test_speculative_generator_validates_rows_and_no_longer_refuses_a_window():
    from tinychatengine_amd.speculative import SpeculativeGenerator

    class _Windowed:
        window = 32

        def __init__(self, rows_per_seq, attention_window=32):
            self.rows_per_seq, self.attention = rows_per_seq, types.SimpleNamespace(window=attention_window)

    # a decoder whose attention object does not carry its window would run the unwindowed rows step
    with pytest.raises(ValueError, match="window") as e:
        SpeculativeGenerator([_Windowed(2, attention_window=None)], None, None, None, max_new=4)
    assert "not built" not in str(e.value)

    for bad in (0, 9):
        with pytest.raises(ValueError, match="rows_per_seq"):
            SpeculativeGenerator([_Windowed(bad)], None, None, None, max_new=4)
    with pytest.raises(ValueError, match="ngram"):
        SpeculativeGenerator([_Windowed(2)], None, None, None, max_new=4, ngram=5)
    with pytest.raises(AssertionError, match="one T"):
        SpeculativeGenerator([_Windowed(2), _Windowed(4)], None, None, None, max_new=4)
    # a windowed decoder passes every check of the constructor's own: what stops this stand-in is only that it is no decoder
    with pytest.raises(AttributeError):
        SpeculativeGenerator([_Windowed(2)], None, None, None, max_new=4)


def test_admit_validates_chunk_rows_before_anything_changes():
    """admit's own checks, on a generator that is nothing but what they read (no device, no decoder)."""
    from tinychatengine_amd.generate import SlotBook, _GeneratorBase
    g = object.__new__(_GeneratorBase)
    g.batch, g.vocab, g.max_keys = 2, 100, 64
    g.book, g.sampler = SlotBook(2, 64), types.SimpleNamespace(top_k_bound=40, log_stride=8)
    g.allocator = _alloc(4, batch=2, stride=4)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="chunk_rows"):
            g.admit(0, [1, 2, 3], None, 0, 4, chunk_rows=bad)
    assert g.allocator.pages_in_use() == 0 and g.book.live() == []
    g.allocator = None
    with pytest.raises(ValueError, match="paged"):
        g.admit(0, [1, 2, 3], None, 0, 4, chunk_rows=2)
