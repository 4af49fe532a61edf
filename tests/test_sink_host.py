"""CPU (no GPU): attention sinks beside the sliding window (include/tce_matmul.h, "ATTENTION SINKS").

    1  the definition (two rotations of q, keys rotated at their absolute positions) IS StreamingLLM (keys compacted and rotated at positions inside the cache), in float64
    2  on a designed case the sinks matter: the float64 sink reference and the window-only reference differ by far more than the kernels' bound
    3  PageAllocator.release_behind(..., keep_pages=k): semantics, a seeded walk under check_invariants, keep_pages=0 equal to the allocator as it was, the page bound
    4  every refusal of the six new entry points (before any HIP call: host buffers stand in for device pointers), their order, and the Python ValueErrors"""
import ctypes as C
import os

import numpy as np
import pytest

import attention_cases as ac
import sink_cases as sc

torch = pytest.importorskip("torch")
BAD_ARG, UNSUPPORTED = -1, -3
NAMES = ("tce_attention_decode_describe_paged_sink", "tce_attention_decode_step_paged_sink_f16", "tce_attention_decode_step_paged_sink_fp8",
         "tce_attention_prefill_paged_sink_f16", "tce_attention_prefill_paged_sink_fp8", "tce_kv_block_table_check_sink")


@pytest.fixture(scope="module")
def capi():
    from tinychatengine_amd import build as B
    B.build()
    from tinychatengine_amd import capi
    return capi


def test_sink_symbols_are_exported(capi):
    L = capi.lib()
    for n in NAMES:
        assert n in capi.EXPORTS and hasattr(L, n)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tce_matmul.h")).read()
    assert all(n + "(" in header for n in NAMES)
    assert "would have to be re-rotated" not in header


# ---- 1. the definition is StreamingLLM ----
def _rope64(x, pos, theta):
    """x [..][hd] rotated by the true RoPE angles theta_i * pos, the pairs (i, i + hd / 2), in float64."""
    ang = theta * float(pos)
    c, s = np.cos(ang), np.sin(ang)
    lo, hi = x[..., : ac.HD // 2], x[..., ac.HD // 2:]
    return np.concatenate([lo * c - hi * s, hi * c + lo * s], axis=-1)


def _softmax_out(s, V):
    w = np.exp(s - s.max())
    return (w / w.sum()) @ V


@pytest.mark.parametrize("W,S", [(1, 1), (5, 4), (5, 5), (61, 16), (400, 3), (1100, 16)])
def test_the_definition_is_streaming_llm(W, S):
    theta = 10000.0 ** (-np.arange(ac.HD // 2) / (ac.HD // 2))
    rng = np.random.default_rng([W, S])
    for p in (S + W - 1, S + W, S + W + 1, S + W + 2, S + W + 3, 2 * (S + W) + 7, 2047):
        q, k, V = rng.standard_normal(ac.HD), rng.standard_normal((p + 1, ac.HD)), rng.standard_normal((p + 1, ac.HD))
        pool = np.stack([_rope64(k[j], j, theta) for j in range(p + 1)])  # what the pools hold: a function of the tokens alone
        sk, wk = sc.weighed_keys(p, W, S)
        # the definition: the pool's keys, q rotated with row S + W - 1 for the sinks and with row p for the window
        s_def = np.concatenate([pool[sk] @ _rope64(q, S + W - 1, theta), pool[wk] @ _rope64(q, p, theta)]) * ac.ALPHA
        got = _softmax_out(s_def, np.concatenate([V[sk], V[wk]]))
        # StreamingLLM: the UN-rotated keys of the cache [0, S) ++ [lo, p], rotated at their positions inside the cache; q at the cache's last position
        cache = np.concatenate([sk, wk])
        kc = np.stack([_rope64(k[j], i, theta) for i, j in enumerate(cache)])
        want = _softmax_out(kc @ _rope64(q, len(cache) - 1, theta) * ac.ALPHA, V[cache])
        assert len(cache) == (S + W if p >= S + W else p + 1)
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), (W, S, p)


# ---- 2. the sinks are not optional ----
@pytest.mark.parametrize("heads,kv_heads", [(4, 2), (8, 8)])
@pytest.mark.parametrize("W,S", [(5, 1), (61, 4), (400, 5), (1100, 16)])
def test_on_sink_first_the_sink_row_is_not_the_windowed_row(heads, kv_heads, W, S):
    cos, sin = ac.rope_tables(2048, 5)
    for p in (S + W, S + W + 3, 2047):
        c = sc.compact_case("sink_first", heads, kv_heads, p, W, S, cos, sin, seed=p)
        ref, win = c.reference(cos, sin), c.window_only(cos, sin)
        assert (np.abs(ref - win) > 10.0 * ac.bound(ref)).any(), (W, S, p)
        assert (np.abs(ref - win) / ac.bound(ref)).max() > 10.0
        # and the row is what the family says: the first sink's value row, on the heads that look along the pilot
        up = c.case.a[0] > 0
        _, Vr = c.repeated()
        assert np.abs(ref - Vr[:, 0].astype(np.float64))[up].max() < 0.02
    # a row that does not bind is the unwindowed row
    p = S + W - 1
    c = sc.compact_case("sink_first", heads, kv_heads, p, W, S, cos, sin, seed=p)
    Kr, Vr = c.repeated()
    assert np.array_equal(c.reference(cos, sin), ac.reference_f64(sc.rotate_half(c.q_raw, cos, sin, p), Kr, Vr))


# ---- 3. the allocator ----
def _alloc(num_pages=40, batch=3, stride=32, pk=16):
    from tinychatengine_amd.paged_kv import PageAllocator
    return PageAllocator(num_pages, pk, batch, stride, "cpu")


def _state(a):
    return (list(a.free), list(a.refcount), [list(p) for p in a.pages], list(a.gone), list(a.frozen), a.table.clone())


def _same(x, y):
    return x[:5] == y[:5] and torch.equal(x[5], y[5])


def test_keep_pages_keeps_the_first_pages_and_frees_the_hole():
    a = _alloc()
    a.reserve(0, 16 * 10 - 1)
    first = list(a.pages[0])
    assert a.release_behind(0, 16, keep_pages=1) == [] and a.gone[0] == 0 and a.kept[0] == []  # nothing behind the kept page yet
    freed = a.release_behind(0, 16 * 5 + 3, keep_pages=1)
    assert freed == first[1:5] and a.kept[0] == first[:1] and a.pages[0] == first[5:] and a.gone[0] == 5
    assert a.pages_in_use() == 6
    a.check_invariants()
    assert a.holds(0, 0, 16) and a.holds(0, 3, 5) and a.holds(0, 16 * 5, 16 * 5)
    assert not a.holds(0, 0, 17) and not a.holds(0, 16, 1) and not a.holds(0, 16 * 4, 17) and not a.holds(0, 8, 16 * 5)
    assert a.release_behind(0, 16 * 5 + 3, keep_pages=1) == []  # idempotent
    assert a.release_behind(0, 16 * 7, keep_pages=0) == first[5:7] and a.kept[0] == first[:1]  # asking for fewer keeps what is kept
    with pytest.raises(ValueError, match="keep_pages"):
        a.release_behind(0, 16 * 8, keep_pages=2)
    with pytest.raises(ValueError, match="keep_pages"):
        a.release_behind(0, 0, keep_pages=-1)
    with pytest.raises(ValueError, match="gave its leading pages back"):
        a.fork(0, 1, 16)
    added = a.reserve(0, 16 * 12)
    a.check_invariants()
    freed = a.release(0)
    assert len(added) == 3 and sorted(freed) == sorted(first[:1] + first[7:] + added) and a.pages_in_use() == 0 and a.kept[0] == [] and a.gone[0] == 0
    a.check_invariants()
    # kept pages can only be established by the first release
    a.reserve(1, 16 * 6)
    a.release_behind(1, 16 * 2)
    with pytest.raises(ValueError, match="keep_pages"):
        a.release_behind(1, 16 * 4, keep_pages=1)
    # two kept pages; a shared kept page only loses this slot's reference
    b = _alloc()
    b.reserve(0, 16 * 6)
    b.fork(0, 1, 16 * 3)
    shared = b.pages[0][:3]
    assert b.release_behind(1, 16 * 3, keep_pages=2) == [] and b.kept[1] == shared[:2] and b.gone[1] == 3
    b.check_invariants()
    assert b.release(1) == []  # (it holds no page of its own: the kept ones are the source's too)
    b.check_invariants()
    assert all(b.refcount[p] == 1 for p in shared)


def test_a_seeded_walk_keeps_the_invariants_and_keep_zero_is_the_allocator_as_it_was():
    from tinychatengine_amd.paged_kv import PagePoolExhausted
    for seed in range(6):
        rng = np.random.default_rng(seed)
        a, z = _alloc(24, 4, 16), _alloc(24, 4, 16)  # z: the same walk with keep_pages never given (today's calls)
        pos = [-1] * 4
        for _ in range(300):
            op, s = rng.integers(0, 10), int(rng.integers(0, 4))
            try:
                if op < 4:
                    if a.gone[s] + len(a.pages[s]) < 16:
                        upto = min(16 * 16 - 1, max(pos[s], a.gone[s] * 16) + int(rng.integers(1, 40)))
                        a.reserve(s, upto), z.reserve(s, upto)
                        pos[s] = upto
                elif op < 7 and pos[s] >= 0:
                    key = int(rng.integers(0, pos[s] + 2))
                    keep = int(rng.integers(0, 3)) if seed % 2 else 0
                    try:
                        a.release_behind(s, key, keep_pages=keep)
                    except ValueError:
                        assert a.gone[s] and keep > len(a.kept[s])
                    z.release_behind(s, key)
                elif op == 7:
                    a.release(s), z.release(s)
                    pos[s] = -1
                elif op >= 8 and pos[s] >= 0:
                    d = int(rng.integers(0, 4))
                    if d != s and not a.pages[d] and not a.gone[d] and not a.gone[s]:
                        keys = int(rng.integers(0, len(a.pages[s]) * 16 + 1))
                        a.fork(s, d, keys), z.fork(s, d, keys)
                        pos[d] = keys - 1 if keys % 16 else (keys - 1 if keys else -1)
            except PagePoolExhausted:
                pass
            a.check_invariants()
            assert a.pages_in_use() == sum(1 for c in a.refcount if c)
            for t in range(4):
                assert len(a.kept[t]) <= a.gone[t]
            if seed % 2 == 0:
                assert _same(_state(a), _state(z)) and all(k == [] for k in a.kept)
        for s in range(4):
            a.release(s)
        a.check_invariants()
        assert a.pages_in_use() == 0


def test_admission_chunks_with_sinks_and_the_page_bound():
    from tinychatengine_amd.generate import admission_chunks
    assert admission_chunks([100, 7], 16, 32, sinks=4) == admission_chunks([100, 7], 16, 32)
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match="sinks"):
            admission_chunks([100], 16, 32, sinks=bad)
    with pytest.raises(ValueError, match="sinks"):
        admission_chunks([100], 16, None, sinks=4)
    # the schedule carried out with keep_pages = 1: a slot never holds more than ceil((W + N) / page_keys) + 2 pages, whatever the prompt's length
    for pk, W, N, S in ((16, 32, 16, 4), (16, 5, 7, 16), (64, 100, 130, 1), (16, 61, 1, 5)):
        a = _alloc(num_pages=64, batch=2, stride=4096 // pk, pk=pk)
        limit = -(-(W + N) // pk) + 2
        lengths = [1500, 333]
        worst = 0
        for rnd in admission_chunks(lengths, N, W, sinks=S):
            a.reserve_many(rnd["reserve"])
            for i, c0, m in rnd["segments"]:
                lo = c0 - W + 1 if c0 >= S + W else 0  # the first key the chunk's first row weighs; and word 0's page when a row binds
                assert a.holds(i, max(lo, 0), c0 + m - max(lo, 0)) and a.holds(i, 0, S)
            worst = max(worst, max(len(a.kept[i]) + len(a.pages[i]) for i in range(2)))
            for i, key in rnd["release"]:
                a.release_behind(i, key, keep_pages=-(-S // pk))
            a.check_invariants()
        assert worst <= limit, (pk, W, N, S, worst, limit)
        # and the decode loop's releases behind it
        for pos in range(lengths[0], lengths[0] + 200):
            a.reserve(0, pos)
            assert a.holds(0, pos - W + 1, W) and a.holds(0, 0, S)
            a.release_behind(0, pos - W + 1, keep_pages=1)
            assert len(a.kept[0]) + len(a.pages[0]) <= limit


# ---- 4. refusals ----
def _host():
    buf = (C.c_char * 8192)()
    return buf, (C.addressof(buf) + 15) & ~15


def _step_call(L, p, fp8, **kw):
    g = lambda k, d: kw[k] if k in kw else d
    vp = C.c_void_p
    fn = L.tce_attention_decode_step_paged_sink_fp8 if fp8 else L.tce_attention_decode_step_paged_sink_f16
    scales = (g("ke", 0), g("ve", 0)) if fp8 else ()
    return fn(vp(g("qkv", p)), vp(g("kp", p)), vp(g("vpool", p)), vp(g("table", p)), g("stride", 4), g("pk", 16), g("pages", 8), vp(g("cos", 0)), vp(g("sin", 0)),
              vp(g("out", p)), vp(g("ws", p)), g("batch", 2), g("heads", 4), g("kv", 1), g("hd", 128), vp(g("pos", p)), g("bound", 63), 0x2DA8, *scales, g("window", 8),
              g("sinks", 4), vp(0))


@pytest.mark.parametrize("fp8", [False, True])
def test_sink_step_refusals_need_no_gpu(capi, fp8):
    L = capi.lib()
    keep, p = _host()
    for s in (0, 17, -1, 2 ** 31 - 1):
        assert _step_call(L, p, fp8, sinks=s) == BAD_ARG and b"sinks" in L.tce_last_error(), s
    for w in (0, -1, -2 ** 31):
        assert _step_call(L, p, fp8, window=w) == BAD_ARG and b"window" in L.tce_last_error(), w
    # the windowed step's refusals, with its codes
    for fault, code in ((dict(qkv=0), BAD_ARG), (dict(kp=0), BAD_ARG), (dict(table=0), BAD_ARG), (dict(out=0), BAD_ARG), (dict(ws=0), BAD_ARG), (dict(pos=0), BAD_ARG),
                        (dict(pk=48), BAD_ARG), (dict(stride=0), BAD_ARG), (dict(pages=0), BAD_ARG), (dict(batch=0), BAD_ARG), (dict(bound=64), BAD_ARG), (dict(bound=-1), BAD_ARG),
                        (dict(kv=3), BAD_ARG), (dict(cos=p), BAD_ARG), (dict(hd=64), UNSUPPORTED), (dict(batch=65536), UNSUPPORTED), (dict(qkv=p + 8), UNSUPPORTED),
                        (dict(pos=p + 2), UNSUPPORTED)):
        assert _step_call(L, p, fp8, **fault) == code, fault
    if fp8:
        assert _step_call(L, p, True, ke=8) == BAD_ARG and _step_call(L, p, True, ve=-9) == BAD_ARG
    # order: every refusal of the windowed entry point comes first, in its order, then sinks
    assert _step_call(L, p, fp8, sinks=0, window=0) == BAD_ARG and b"window" in L.tce_last_error()
    assert _step_call(L, p, fp8, sinks=0, pk=48) == BAD_ARG and b"page_keys" in L.tce_last_error()
    assert _step_call(L, p, fp8, sinks=0, bound=64) == BAD_ARG and b"sinks" not in L.tce_last_error()
    assert _step_call(L, p, fp8, sinks=0, hd=64) == UNSUPPORTED and _step_call(L, p, fp8, sinks=17, qkv=p + 8) == UNSUPPORTED
    assert _step_call(L, p, fp8, sinks=0, pos=p + 2) == UNSUPPORTED
    del keep


def _prefill_call(L, p, fp8, segs, **kw):
    g = lambda k, d: kw[k] if k in kw else d
    vp = C.c_void_p
    fn = L.tce_attention_prefill_paged_sink_fp8 if fp8 else L.tce_attention_prefill_paged_sink_f16
    scales = (g("ke", 0), g("ve", 0)) if fp8 else ()
    return fn(vp(g("qkv", p)), 0, vp(g("kp", p)), vp(g("vpool", p)), vp(g("table", p)), g("rows", 2), g("stride", 4), g("pk", 16), g("pages", 8), vp(g("cos", 0)),
              vp(g("sin", 0)), g("causal", 1), vp(g("out", p)), 0, vp(g("ws", p)), g("heads", 4), g("kv", 1), g("hd", 128), C.cast(segs, vp), g("nseg", 1),
              g("total", 5), 0x2DA8, *scales, g("window", 8), g("sinks", 4), vp(0))


@pytest.mark.parametrize("fp8", [False, True])
def test_sink_prefill_refusals_need_no_gpu(capi, fp8):
    L = capi.lib()
    keep, p = _host()
    segs, total = capi.prefill_segments([(0, 3, 5)])
    assert total == 5
    for s in (0, 17, -5):
        assert _prefill_call(L, p, fp8, segs, sinks=s) == BAD_ARG and b"sinks" in L.tce_last_error(), s
    for w in (0, -1):
        assert _prefill_call(L, p, fp8, segs, window=w) == BAD_ARG and b"window" in L.tce_last_error(), w
    assert _prefill_call(L, p, fp8, segs, causal=0) == BAD_ARG and b"causal" in L.tce_last_error()
    for fault, code in ((dict(qkv=0), BAD_ARG), (dict(pk=48), BAD_ARG), (dict(rows=0), BAD_ARG), (dict(kv=3), BAD_ARG), (dict(nseg=17), BAD_ARG), (dict(total=4), BAD_ARG),
                        (dict(hd=64), UNSUPPORTED), (dict(qkv=p + 8), UNSUPPORTED), (dict(ws=p + 8), UNSUPPORTED)):
        assert _prefill_call(L, p, fp8, segs, **fault) == code, fault
    if fp8:
        assert _prefill_call(L, p, True, segs, ke=8) == BAD_ARG
    # order: the windowed prefill's refusals first
    assert _prefill_call(L, p, fp8, segs, sinks=0, window=0) == BAD_ARG and b"window" in L.tce_last_error()
    assert _prefill_call(L, p, fp8, segs, sinks=0, causal=0) == BAD_ARG and b"causal" in L.tce_last_error()
    assert _prefill_call(L, p, fp8, segs, sinks=0, hd=64) == UNSUPPORTED and _prefill_call(L, p, fp8, segs, sinks=17, ws=p + 8) == UNSUPPORTED
    del keep


def test_sink_table_check_and_describe_refusals_need_no_gpu(capi):
    L = capi.lib()
    keep, p = _host()
    vp = C.c_void_p
    chk = lambda **kw: L.tce_kv_block_table_check_sink(vp(kw.get("table", p)), kw.get("stride", 4), kw.get("pk", 16), 8, kw.get("batch", 2), vp(kw.get("pos", p)),
                                                      kw.get("bound", 63), vp(kw.get("viol", p)), kw.get("window", 8), kw.get("sinks", 4), vp(0))
    for fault, code in ((dict(sinks=0), BAD_ARG), (dict(sinks=17), BAD_ARG), (dict(window=0), BAD_ARG), (dict(window=-3), BAD_ARG), (dict(table=0), BAD_ARG),
                        (dict(pos=0), BAD_ARG), (dict(viol=0), BAD_ARG), (dict(pk=8), BAD_ARG), (dict(batch=0), BAD_ARG), (dict(bound=-1), BAD_ARG),
                        (dict(pos=p + 2), UNSUPPORTED), (dict(sinks=0, pos=p + 2), UNSUPPORTED), (dict(sinks=0, window=0), BAD_ARG)):
        assert chk(**fault) == code, fault
    assert chk(sinks=0, window=0) == BAD_ARG and b"window" in L.tce_last_error()
    buf = C.create_string_buffer(192)
    d = lambda **kw: L.tce_attention_decode_describe_paged_sink(kw.get("batch", 2), kw.get("heads", 4), kw.get("kv", 1), kw.get("bound", 63), kw.get("pk", 16),
                                                                kw.get("window", 8), kw.get("sinks", 4), kw.get("buf", buf), kw.get("len", 192))
    assert d() == 0
    for fault in (dict(sinks=0), dict(sinks=17), dict(window=0), dict(window=-1), dict(batch=0), dict(kv=3), dict(bound=-1), dict(pk=24), dict(buf=None), dict(len=0)):
        assert d(**fault) == BAD_ARG, fault
    del keep


def test_the_sink_cut(capi):
    for heads, kv in ((4, 2), (8, 8), (32, 8)):
        for pk in (16, 64):
            for W in (1, 5, 61, 400, 1100, 4096):
                for S in (1, 3, 4, 5, 16):
                    s4 = (S + 3) & ~3
                    far = capi.describe_attention_paged_sink(3, heads, kv, 32767, pk, W, S)
                    assert far == capi.describe_attention_paged(3, heads, kv, s4 + W + 2, pk), (W, S)
                    assert far["chunks"] * far["keys-per-chunk"] >= s4 + W + 3
                    # no row can bind: the unwindowed step's cut
                    for bound in (S + W - 1, max(S + W - 9, 0)):
                        assert capi.describe_attention_paged_sink(3, heads, kv, bound, pk, W, S) == capi.describe_attention_paged(3, heads, kv, bound, pk)
                    # some row can: the slots cover the longest virtual sequence of any position
                    for bound in range(S + W, S + W + 9):
                        cut = capi.describe_attention_paged_sink(3, heads, kv, bound, pk, W, S)
                        longest = max(s4 + p - ((p - W + 1) & ~3) + 1 for p in range(S + W, bound + 1))
                        assert cut["chunks"] * cut["keys-per-chunk"] >= max(longest, S + W), (W, S, bound)


def test_python_refuses_bad_sinks(capi):
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchDecodeAttention
    from tinychatengine_amd.speculative import PagedRowsDecodeAttention, SpeculativeDecoder, SpeculativeGenerator
    a = PageAllocator(8, 16, 2, 4, "cpu")
    for bad in (0, 17, -1, 2.5):
        with pytest.raises(ValueError, match="sinks"):
            PagedBatchDecodeAttention(a, 4, 1, "cpu", window=8, sinks=bad)
    with pytest.raises(ValueError, match="sinks"):
        PagedBatchDecodeAttention(a, 4, 1, "cpu", sinks=4)
    att = PagedBatchDecodeAttention(a, 4, 1, "cpu", window=8, sinks=4)
    assert (att.sinks, att._window(), att._entry("x")) == (4, (8, 4), "x_sink")
    plain = PagedBatchDecodeAttention(a, 4, 1, "cpu", window=8)
    assert (plain.sinks, plain._window(), plain._entry("x")) == (None, (8,), "x_window")
    none = PagedBatchDecodeAttention(a, 4, 1, "cpu")
    assert (none.sinks, none._window(), none._entry("x")) == (None, (), "x")
    with pytest.raises(ValueError, match="sinks"):
        PagedRowsDecodeAttention(a, 4, 1, "cpu", rows_per_seq=2, window=8, sinks=4)
    with pytest.raises(ValueError, match="sinks"):
        SpeculativeDecoder(None, a, 2, window=8, sinks=4)

    class _D:
        window, sinks, rows_per_seq = 32, 4, 2

    with pytest.raises(ValueError, match="sinks"):
        SpeculativeGenerator([_D()], None, None, None, 8)
