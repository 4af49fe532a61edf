"""CPU (no GPU): attention sinks on the multi-row (speculative) step -- every refusal of tce_attention_decode_step_paged_rows_sink_f16 / _fp8 (before any HIP call: host
buffers stand in for device pointers and are never dereferenced), their order, the table-check identity the rows form uses instead of an entry point of its own
(rows_check_calls with sinks, against an enumeration), the Python rules, and the page bound's arithmetic."""
import ctypes as C
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

NAMES = ("tce_attention_decode_step_paged_rows_sink_f16", "tce_attention_decode_step_paged_rows_sink_fp8")
BAD_ARG, UNSUPPORTED = -1, -3
PAGE_KEYS = 16
WINDOWS, SINKS = (8, 17, 35), (1, 5, 16)


@pytest.fixture(scope="module")
def capi():
    from tinychatengine_amd import build as B
    B.build()
    from tinychatengine_amd import capi
    return capi


def test_rows_sink_symbols_are_exported_and_the_abi_number_stays(capi):
    assert (capi.TCE_ERR_BAD_ARG, capi.TCE_ERR_UNSUPPORTED_SHAPE) == (BAD_ARG, UNSUPPORTED)
    L = capi.lib()
    assert L.tce_version() == 113 == capi.TCE_ABI_VERSION
    for n in NAMES:
        assert n in capi.EXPORTS and hasattr(L, n)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tce_matmul.h")).read()
    assert all(n + "(" in header for n in NAMES)
    assert "attention sinks on the multi-row step" not in header, "the NOT BUILT sentence still lists the form"


def test_the_new_unit_is_built_with_the_spill_check(capi):
    from tinychatengine_amd import build as B
    assert "attention_rows_sink.hip" in B.HIP_SOURCES and B.NO_VGPR_SPILL["attention_rows_sink.hip"]
    kernels = [ln for ln in open(B.LIB_PATH + ".kernels.txt") if ln.startswith("attention_rows_sink:")]
    assert len(kernels) == 2 and all("attn_decode_fast_kernel" in k for k in kernels), kernels


# ---- the C ABI's refusals ----
def _host():
    buf = (C.c_char * 8192)()
    return buf, (C.addressof(buf) + 15) & ~15


def _call(L, p, fp8, **kw):
    g = lambda k, d: kw[k] if k in kw else d
    vp = C.c_void_p
    fn = L.tce_attention_decode_step_paged_rows_sink_fp8 if fp8 else L.tce_attention_decode_step_paged_rows_sink_f16
    scales = (g("ke", 0), g("ve", 0)) if fp8 else ()
    return fn(vp(g("qkv", p)), vp(g("kp", p)), vp(g("vpool", p)), vp(g("table", p)), g("stride", 4), g("pk", 16), g("pages", 8), vp(g("cos", 0)), vp(g("sin", 0)),
              vp(g("out", p)), vp(g("ws", p)), g("batch", 2), g("rows", 4), g("heads", 4), g("kv", 1), g("hd", 128), vp(g("pos", p)), g("bound", 63), 0x2DA8, *scales,
              g("window", 8), g("sinks", 4), vp(0))


@pytest.mark.parametrize("fp8", [False, True])
def test_rows_sink_step_refusals_need_no_gpu(capi, fp8):
    L = capi.lib()
    keep, p = _host()
    for s in (0, 17, -1, 2 ** 31 - 1):
        assert _call(L, p, fp8, sinks=s) == BAD_ARG and b"sinks" in L.tce_last_error(), s
    for w in (0, -1, -2 ** 31):
        assert _call(L, p, fp8, window=w) == BAD_ARG and b"window" in L.tce_last_error(), w
    for r in (0, 9, -1):
        assert _call(L, p, fp8, rows=r) == UNSUPPORTED and b"rows_per_seq" in L.tce_last_error(), r
    # the rule of the pair: window >= rows_per_seq, the message names both
    for w, r in ((3, 4), (7, 8), (1, 2)):
        assert _call(L, p, fp8, window=w, rows=r) == UNSUPPORTED, (w, r)
        assert b"window" in L.tce_last_error() and b"rows_per_seq" in L.tce_last_error(), L.tce_last_error()
    # the windowed rows entry point's refusals, with their codes
    for fault, code in ((dict(qkv=0), BAD_ARG), (dict(kp=0), BAD_ARG), (dict(vpool=0), BAD_ARG), (dict(table=0), BAD_ARG), (dict(out=0), BAD_ARG), (dict(ws=0), BAD_ARG),
                        (dict(pos=0), BAD_ARG), (dict(pk=48), BAD_ARG), (dict(pk=8), BAD_ARG), (dict(pk=512), BAD_ARG), (dict(stride=0), BAD_ARG), (dict(pages=0), BAD_ARG),
                        (dict(batch=0), BAD_ARG), (dict(bound=64), BAD_ARG), (dict(bound=-1), BAD_ARG), (dict(kv=3), BAD_ARG), (dict(cos=p), BAD_ARG),
                        (dict(hd=64), UNSUPPORTED), (dict(batch=65536), UNSUPPORTED), (dict(qkv=p + 8), UNSUPPORTED), (dict(pos=p + 2), UNSUPPORTED),
                        (dict(out=p + 8), UNSUPPORTED)):  # (out: the rows form stores it in 16-byte pieces)
        assert _call(L, p, fp8, **fault) == code, fault
    if fp8:
        assert _call(L, p, True, ke=8) == BAD_ARG and _call(L, p, True, ve=-9) == BAD_ARG
    # order 1: the windowed rows entry point's BAD_ARG rules come in front of the sinks rule, in their order
    assert _call(L, p, fp8, sinks=0, window=0) == BAD_ARG and b"window" in L.tce_last_error()
    assert _call(L, p, fp8, sinks=0, pk=48) == BAD_ARG and b"page_keys" in L.tce_last_error()
    assert _call(L, p, fp8, sinks=0, bound=64) == BAD_ARG and b"sinks" not in L.tce_last_error()
    assert _call(L, p, fp8, sinks=17, kv=3) == BAD_ARG and b"sinks" not in L.tce_last_error()
    assert _call(L, p, fp8, sinks=0, qkv=0) == BAD_ARG and b"sinks" not in L.tce_last_error()
    # order 2: the sinks rule is a BAD_ARG rule, and those win over every UNSUPPORTED_SHAPE rule, whichever argument carries it
    for fault in (dict(hd=64), dict(batch=65536), dict(rows=9), dict(rows=0), dict(qkv=p + 8), dict(out=p + 8), dict(pos=p + 2), dict(window=3)):
        assert _call(L, p, fp8, sinks=0, **fault) == BAD_ARG and b"sinks" in L.tce_last_error(), fault
    assert _call(L, p, fp8, window=0, rows=9) == BAD_ARG and b"window" in L.tce_last_error()
    assert _call(L, p, fp8, rows=9, kp=0) == BAD_ARG
    # order 3: window < rows_per_seq comes last -- behind the windowed rows entry point's UNSUPPORTED_SHAPE rules
    assert _call(L, p, fp8, window=3, hd=64) == UNSUPPORTED and b"head_dim" in L.tce_last_error()
    assert _call(L, p, fp8, window=3, rows=9) == UNSUPPORTED and b"1 .. 8" in L.tce_last_error()
    assert _call(L, p, fp8, window=3, qkv=p + 8) == UNSUPPORTED and b"16-byte" in L.tce_last_error()
    assert _call(L, p, fp8, window=3, pos=p + 2) == UNSUPPORTED and b"int32" in L.tce_last_error()
    # window == rows_per_seq is allowed: what stops this call is nothing of the entry point's own (host memory is no device memory: it must not be launched here)
    assert _call(L, p, fp8, window=4, rows=4, sinks=0) == BAD_ARG and b"sinks" in L.tce_last_error()
    del keep


# ---- the table check the rows form uses ----
def _row_words(pos, W, S):
    """the table words a sink row at `pos` follows (include/tce_matmul.h, "trust")"""
    if pos >= S + W:
        return {0} | set(range((pos - W + 1) // PAGE_KEYS, pos // PAGE_KEYS + 1))
    return set(range(pos // PAGE_KEYS + 1))


def _starts(W, S, n):
    """around 0, the threshold as the last row meets it (S + W - n), the threshold (S + W), and the page edges"""
    near = lambda x: range(max(0, x - 2), x + 3)
    ps = set(near(0)) | set(near(S + W - n)) | set(near(S + W))
    for edge in range(PAGE_KEYS, 8 * PAGE_KEYS, PAGE_KEYS):
        ps |= set(near(edge)) | set(near(edge + W - 1)) | set(near(max(0, edge - n)))
    return sorted(ps)


def test_rows_with_sinks_are_covered_by_the_sink_check_of_the_last_row():
    """Rows p .. p + n - 1 against tce_kv_block_table_check_sink at position p + n - 1 with window W + n - 1 and sinks S: exactly the rows' words when p >= S + W,
    else words 0 .. (p + n - 1) // page_keys -- a superset, and a sound one: before position S + W release_behind gives nothing back but what lies behind page 0."""
    exact = superset = 0
    for W in WINDOWS:
        for S in SINKS:
            for n in range(1, 9):
                assert W >= n
                for p in _starts(W, S, n):
                    union = set().union(*(_row_words(p + t, W, S) for t in range(n)))
                    check = _row_words(p + n - 1, W + n - 1, S)
                    binds = p + n - 1 >= S + W + n - 1
                    assert binds == (p >= S + W) == all(p + t >= S + W for t in range(n)), (W, S, n, p)
                    if binds:
                        assert check == union, (W, S, n, p)
                        exact += 1
                    else:
                        assert check == set(range((p + n - 1) // PAGE_KEYS + 1)) and check >= union, (W, S, n, p)
                        superset += 1
                        # sound: the words beyond the rows' own name pages the slot still holds -- at the synced position p < S + W the generator has released
                        # behind key p - W + 1 <= S <= page_keys at the most, which is page 0 alone, and page 0 is kept for the sinks
                        assert p - W + 1 <= S <= PAGE_KEYS
    # (with S <= 16, n <= 8 and pages of 16 keys or more a binding row of such a call has lo <= S + 7 < 2 pages: the superset is in fact the rows' own words)
    assert exact > 1000 and superset > 1000, "the enumeration did not reach the cases it is for"


def test_rows_check_calls_with_sinks(capi):
    from tinychatengine_amd.speculative import rows_check_calls
    # the windowed calls: one per distinct row count, the window wider by n - 1 -- sinks do not change the calls, only the entry point they go to
    calls = rows_check_calls([4, 0, 3, 4, 1], [13, -1, 40, 7, 99], 4, 8, 4)
    assert calls == [(8, [-1, -1, -1, -1, 99]), (10, [-1, -1, 40, -1, -1]), (11, [13, -1, -1, 7, -1])] == rows_check_calls([4, 0, 3, 4, 1], [13, -1, 40, 7, 99], 4, 8)
    assert rows_check_calls([0, 0], [-1, -1], 8, 8, 16) == []
    with pytest.raises(AssertionError, match="sinks"):
        rows_check_calls([1], [0], 2, None, 4)
    rng = np.random.default_rng(5)
    for _ in range(100):
        T = int(rng.integers(1, 9))
        W, S = int(rng.integers(T, 40)), int(rng.integers(1, 17))
        n = rng.integers(0, T + 1, 6).tolist()
        last = [int(rng.integers(m - 1, 300)) if m else -1 for m in n]
        seen = [0] * 6
        for w, words in rows_check_calls(n, last, T, W, S):
            for b, q in enumerate(words):
                if q >= 0:
                    seen[b] += 1
                    assert q == last[b] and w == W + n[b] - 1
        assert seen == [1 if m else 0 for m in n]


# ---- python fronts ----
def _alloc(num_pages=12, batch=3, stride=8):
    from tinychatengine_amd.paged_kv import PageAllocator
    return PageAllocator(num_pages, PAGE_KEYS, batch, stride, "cpu")


def test_rows_attention_with_sinks_names_its_rules(capi):
    from tinychatengine_amd.speculative import PagedRowsDecodeAttention, SpeculativeDecoder
    a = _alloc()
    # window < rows_per_seq beside sinks: both are named, and the rule comes before the device-table rule
    for ctor in (lambda **kw: PagedRowsDecodeAttention(a, 8, 2, "cpu", **kw), lambda **kw: SpeculativeDecoder(None, a, kw.pop("rows_per_seq"), **kw)):
        with pytest.raises(ValueError, match=r"window 3 < rows_per_seq 4") as e:
            ctor(rows_per_seq=4, window=3, sinks=4)
        assert "sinks" in str(e.value)
        # a window needs the table on the device; with sinks the message names them, and SpeculativeDecoder says so before it touches `block` (None here)
        with pytest.raises(ValueError, match="on the device") as e:
            ctor(rows_per_seq=4, window=4, sinks=4)
        assert "sinks" in str(e.value) and "not built" not in str(e.value)
    with pytest.raises(ValueError, match="on the device") as e:
        PagedRowsDecodeAttention(a, 8, 2, "cpu", rows_per_seq=4, window=8)
    assert "sinks" not in str(e.value)
    # sinks without a window, and counts outside 1 .. 16: PagedBatchDecodeAttention's rule
    with pytest.raises(ValueError, match="sinks"):
        PagedRowsDecodeAttention(a, 8, 2, "cpu", rows_per_seq=4, sinks=4)
    # what the constructor sets on a device table: the entry point and its two arguments
    R = PagedRowsDecodeAttention(a, 8, 2, "cpu", rows_per_seq=4)
    R.window, R.sinks = 8, 4
    assert R._entry("tce_attention_decode_step_paged_rows") == "tce_attention_decode_step_paged_rows_sink" and R._window() == (8, 4)
    assert R._entry("tce_kv_block_table_check") == "tce_kv_block_table_check_sink"


def test_speculative_generator_accepts_sinks_and_refuses_a_mismatched_count():
    from tinychatengine_amd.speculative import SpeculativeGenerator

    class _Layer:
        def __init__(self, rows_per_seq, window, sinks, attention_window, attention_sinks):
            self.rows_per_seq, self.window, self.sinks = rows_per_seq, window, sinks
            self.attention = types.SimpleNamespace(window=attention_window, sinks=attention_sinks)

    # the attention object does not carry the count the decoder reports: it would run the windowed rows step.  The sinks rule comes before the window rule
    for att_w, att_s in ((32, None), (32, 5), (None, None)):
        with pytest.raises(ValueError, match="sinks 4") as e:
            SpeculativeGenerator([_Layer(2, 32, 4, att_w, att_s)], None, None, None, max_new=4)
        assert "not built" not in str(e.value)
    with pytest.raises(ValueError, match="window 32"):
        SpeculativeGenerator([_Layer(2, 32, None, None, None)], None, None, None, max_new=4)
    # a layer with sinks passes every check of the constructor's own -- rows, n-gram, one T --: what stops this stand-in is only that it is no decoder
    with pytest.raises(ValueError, match="rows_per_seq"):
        SpeculativeGenerator([_Layer(9, 32, 4, 32, 4)], None, None, None, max_new=4)
    with pytest.raises(AssertionError, match="one T"):
        SpeculativeGenerator([_Layer(2, 32, 4, 32, 4), _Layer(4, 32, None, 32, None)], None, None, None, max_new=4)
    with pytest.raises(AttributeError):
        SpeculativeGenerator([_Layer(2, 32, 4, 32, 4), _Layer(2, 32, None, 32, None)], None, None, None, max_new=4)


# ---- the page bound ----
def test_a_speculative_slot_with_sinks_stays_within_the_bound():
    """SpeculativeGenerator.run(n) on the allocator alone: reserve up to p + n T - 1 (SpecSlotBook.wanted), advance by 1 .. T per step, release behind the window
    with keep_pages = 1 (the base class's _release_behind).  A slot never holds more than ceil((W + n T) / page_keys) + 1 + keep_pages pages, the sinks' page is
    held throughout and every key a later row weighs is still there."""
    from tinychatengine_amd.speculative import SpecSlotBook
    for W, S, T, n in ((32, 4, 4, 2), (8, 16, 8, 1), (17, 5, 5, 3), (35, 1, 2, 8)):
        assert W >= T
        keep = -(-S // PAGE_KEYS)
        bound = -(-(W + n * T) // PAGE_KEYS) + 1 + keep
        assert keep == 1
        stride = 64
        a = _alloc(num_pages=bound, batch=1, stride=stride)  # exactly the bound: the schedule must fit
        book = SpecSlotBook(1, stride * PAGE_KEYS, T)
        rng = np.random.default_rng(W + S)
        p = 3
        a.reserve(0, p - 1)
        book.pos[0] = p
        worst = 0
        while p + n * T < 700:
            a.release_behind(0, p - W + 1, keep_pages=keep)
            a.reserve_many(book.wanted(n))
            worst = max(worst, len(a.kept[0]) + len(a.pages[0]))
            assert a.holds(0, 0, S), f"W={W} S={S}: the sinks' page was given back at position {p}"
            lo = p - W + 1 if p >= S + W else 0
            assert a.holds(0, lo, p + n * T - lo), f"W={W} S={S}: a key the rows at {p} weigh is not held"
            p += int(rng.integers(n, n * T + 1))  # n replays of 1 .. T tokens
            book.pos[0] = p
            a.check_invariants()
        assert worst <= bound and a.gone[0] > 2, (W, S, T, n, worst, bound)
        a.release(0)
        assert a.pages_in_use() == 0 and a.kept[0] == []
