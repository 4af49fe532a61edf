"""The attention kernels on designed rows (tests/attention_cases.py) against float64: peaked, ramping and out-of-range scores, subnormal values.

Every other attention test draws Gaussian q, K and V, whose score rows span 2 - 5 nats: there the running maximum never moves, every merge weight is near 1, no score
leaves binary16's range and no value is subnormal, so a kernel that got any of that wrong would pass.  tests/test_attention_adversarial_host.py shows on an fp32
emulation of the decode step that these families tell such kernels from a correct one; here the real entry points are held to the same bound
(attention_cases.bound: the project's 2e-3 max|ref| + 2^-11 |ref|, plus 2^-25 for a subnormal output's final rounding) -- the single step with its kept forms, the
batched, paged and e4m3-paged steps, both prefills, and o_proj's deferred combine.  Each test prints its worst |err| / bound per family (pytest -s).

Shapes are the smallest that reach every path: (heads, kv_heads) in {(4, 1), (4, 2), (2, 2)}, contexts of attention_cases.SIZES keys (one chunk up to 320 keys,
four up to 640 or 1024, eight slots beyond; 128, 320, 641 and 1025 give a wave at least two 16-key blocks, which a staircase needs to make a slot's maximum move)."""
import numpy as np
import pytest

import attention_cases as ac
from deferred_pair import deferred as _deferred, plain as _plain

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HD = ac.HD
SHAPES = [(4, 1), (4, 2), (2, 2)]
FORM_FAMILIES = ("stairs_up", "two_peaks", "out_of_range")
INF_BITS = 0x7C00


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int16)


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _report(entry, worst):
    print(f"adversarial {entry}: " + " ".join(f"{k}:{v:.3f}" for k, v in worst.items()))


class _Mode:
    """tce_w4a16_set_debug_mode(mode) for a block, the family's neutral value restored on the way out whatever happens."""

    def __init__(self, mode, neutral):
        self.mode, self.neutral = mode, neutral

    def __enter__(self):
        from tinychatengine_amd import capi
        capi.check(capi.lib().tce_w4a16_set_debug_mode(self.mode))

    def __exit__(self, *exc):
        from tinychatengine_amd import capi
        capi.check(capi.lib().tce_w4a16_set_debug_mode(self.neutral))


# ---------------------------------------------------------------------------------------------------------------------------------
# the single step
# ---------------------------------------------------------------------------------------------------------------------------------
def _single_step(dev, case, mask=None, tables=None, raw_row=None):
    """DecodeAttention.step at position n - 1 on a cache that holds the case's first n - 1 keys (the row at n - 1: inf bits until the step writes it)."""
    from tinychatengine_amd.attention_ops import DecodeAttention
    n = case.n
    cos, sin = (None, None) if tables is None else (_t(tables[0], dev), _t(tables[1], dev))
    att = DecodeAttention(case.heads, HD, n, dev, cos, sin, kv_heads=case.kv_heads)
    K, V = case.K.copy(), case.V.copy()
    K[:, n - 1] = V[:, n - 1] = np.array([INF_BITS], np.uint16).view(np.float16)[0]
    att.k_cache.copy_(_t(K, dev))
    att.v_cache.copy_(_t(V, dev))
    row = case.qkv_row() if raw_row is None else raw_row
    out = att.step(_t(row, dev), n - 1, mask=None if mask is None else _t(mask, dev))
    torch.cuda.synchronize()
    assert np.array_equal(att.k_cache.cpu().numpy().view(np.uint16), case.K.view(np.uint16)), "the appended key (or another cache row) is not what it must be"
    assert np.array_equal(att.v_cache.cpu().numpy().view(np.uint16), case.V.view(np.uint16))
    return out.cpu().numpy().astype(np.float64)


def _blocks_per_wave(heads, kv_heads, keys):
    from tinychatengine_amd import capi
    d = capi.describe_attention_step(heads, keys, kv_heads)
    return -(-(d["keys-per-chunk"] // d["waves"]) // 16), d  # (a wave's run is a multiple of 4 keys: its last block may be partial)


@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("heads,kv_heads", SHAPES)
def test_single_step_against_float64(dev, heads, kv_heads, family):
    worst = {}
    for n in ac.SIZES:
        if family in ("stairs_up", "stairs_down") and n in (128, 320, 641, 1025):
            blocks, d = _blocks_per_wave(heads, kv_heads, n)
            assert blocks >= 2, f"{n} keys: {d}: a wave holds one block, no slot's maximum would move"
        case = ac.make_case(family, n, heads, kv_heads, seed=1)
        worst[n] = ac.error_ratio(_single_step(dev, case), case.reference())
    _report(f"step {heads}/{kv_heads} {family}", worst)
    assert max(worst.values()) <= 1.0, worst


def test_the_chunk_rule_puts_the_sizes_where_they_are_meant(dev):
    from tinychatengine_amd import capi
    for heads, kv_heads in SHAPES:
        chunks = [capi.describe_attention_step(heads, n, kv_heads)["chunks"] for n in ac.SIZES]
        assert chunks[:6] == [1, 1, 1, 1, 1, 4] and chunks[6] in (4, 7) and chunks[7] == 8, (heads, kv_heads, chunks)


@pytest.mark.parametrize("family", ["sink_first", "sink_last", "sink_own", "two_peaks", "stairs_up"])
@pytest.mark.parametrize("heads,kv_heads", SHAPES)
def test_single_step_with_rope(dev, oracle, heads, kv_heads, family):
    """The projection's row holds the UN-rotated q and key; the scores are designed for the q the oracle's RotaryPosEmb makes of it (the family's property is asserted
    again on that q and on the rotated own key), and the appended key must be the oracle's, bit for bit."""
    worst = {}
    for n in (17, 320, 321, 1025):
        case = ac.make_case(family, n, heads, kv_heads, seed=2)
        cos, sin = ac.rope_tables(n, seed=n)
        q_raw = ac.unrotate(case.q[0], cos[n - 1], sin[n - 1])
        k_raw = ac.unrotate(case.K[:, n - 1], cos[n - 1], sin[n - 1])
        q_rot, _ = oracle.rope_half(q_raw[:, None, :], q_raw[:, None, :], cos, sin, n - 1)
        _, k_rot = oracle.rope_half(k_raw[:, None, :], k_raw[:, None, :], cos, sin, n - 1)
        case.q[0] = q_rot[:, 0]
        case.K[:, n - 1] = k_rot[:, 0]
        case.check()
        row = np.concatenate([q_raw.reshape(-1), k_raw.reshape(-1), case.V[:, n - 1].reshape(-1)])
        got = _single_step(dev, case, tables=(cos, sin), raw_row=row)  # (asserts the appended key == the oracle's k_rot)
        worst[n] = ac.error_ratio(got, case.reference())
    _report(f"step+rope {heads}/{kv_heads} {family}", worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("heads,kv_heads", SHAPES)
def test_single_step_with_the_sink_masked_off(dev, heads, kv_heads):
    """An additive mask of -65504 on the sink (40 - 65504 is IN range: no clamp): the rest of the row takes over; on `two_peaks` with key 3 masked the other peak wins."""
    worst = {}
    for family in ("sink_first", "sink_last", "two_peaks"):
        for n in (17, 321, 1025):
            case = ac.make_case(family, n, heads, kv_heads, seed=3)
            if family == "two_peaks":
                mask = np.zeros(n, np.float16)
                mask[3] = np.float16(-65504.0)
            else:
                mask, _ = ac.masked_sink(case)
            ref = case.reference(mask=mask)
            worst[f"{family}/{n}"] = ac.error_ratio(_single_step(dev, case, mask=mask), ref)
            if family == "two_peaks":  # head 0 (a = 1): all the weight on key n - 2
                assert np.abs(ref[0] - case.V[0, n - 2].astype(np.float64)).max() < 1e-6
            else:
                assert np.abs(ref[0] - case.reference()[0]).max() > 0.1  # the mask changes the answer
    _report(f"step+mask {heads}/{kv_heads}", worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("mode,neutral,heads,kv_heads", [(2908, 2900, 4, 1), (2916, 2900, 4, 2), (2922, 2920, 4, 2), (2922, 2920, 4, 1), (2924, 2920, 4, 1), (3080, 3000, 4, 1)])
def test_single_step_kept_forms(dev, mode, neutral, heads, kv_heads):
    """8 / 16 waves per workgroup (2908 / 2916), two / four query heads per workgroup (2922 / 2924), and a cut for 80 workgroups (3080: 4 heads x 20 chunk slots of 64
    keys, 17 of them live at 1025 keys -- the combine's one-by-one tail past 16)."""
    from tinychatengine_amd import capi
    worst = {}
    with _Mode(mode, neutral):
        for family in FORM_FAMILIES:
            for n in (320, 321, 1025):
                if mode == 3080 and n == 1025:
                    assert capi.describe_attention_step(heads, n, kv_heads)["chunks"] > 16
                case = ac.make_case(family, n, heads, kv_heads, seed=4)
                worst[f"{family}/{n}"] = ac.error_ratio(_single_step(dev, case), case.reference())
    _report(f"step form {mode} {heads}/{kv_heads}", worst)
    assert max(worst.values()) <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------------------------------
# the batched, the paged and the e4m3-paged step
# ---------------------------------------------------------------------------------------------------------------------------------
PAGE_SIZES = [16, 256]
BOUND, MAX_KEYS = 640, 768  # the cut is made for 641 keys; 768 = 3 pages of 256


def _batch_rows(heads, kv_heads, which):
    """Three slots: two families on the two sides of the first chunk's end under one bound, or one of those and one at the bound; one slot inactive (-1)."""
    from tinychatengine_amd import capi
    chunk = capi.describe_attention_batch(3, heads, kv_heads, BOUND)["keys-per-chunk"]
    plans = {0: [("stairs_up", chunk), None, ("two_peaks", BOUND + 1)],          # n keys: the last key of chunk 0 is the own row / the whole bound
             1: [("out_of_range", chunk + 1), ("stairs_down", BOUND + 1), None],  # one key into chunk 1
             2: [None, ("sink_own", chunk + 1), ("all_out_of_range", chunk)],
             3: [("subnormal_v", chunk + 1), ("flat", 5), None],
             4: [("ramp_up", BOUND + 1), None, ("sink_last", chunk)]}
    return plans[which]


def _make_rows(plan, heads, kv_heads, seed, **kw):
    return [None if p is None else ac.make_case(p[0], p[1], heads, kv_heads, seed=seed + i, **kw) for i, p in enumerate(plan)]


def _contiguous_batch(dev, cases, heads, kv_heads):
    """A BatchDecodeAttention whose slot b holds cases[b]'s first n - 1 keys (inf bits from there on), the q/k/v rows and the position words (-1: inactive)."""
    from tinychatengine_amd.batch_decode import BatchDecodeAttention
    B = len(cases)
    A = BatchDecodeAttention(B, heads, MAX_KEYS, dev, None, None, kv_heads=kv_heads)
    inf = np.array([INF_BITS], np.uint16).view(np.float16)[0]
    K = np.full((B, kv_heads, MAX_KEYS, HD), inf, np.float16)
    V = np.full((B, kv_heads, MAX_KEYS, HD), inf, np.float16)
    qkv = np.zeros((B, (heads + 2 * kv_heads) * HD), np.float16)
    pos = np.full(B, -1, np.int32)
    for b, c in enumerate(cases):
        if c is not None:
            K[b, :, :c.n - 1], V[b, :, :c.n - 1] = c.K[:, :c.n - 1], c.V[:, :c.n - 1]
            qkv[b] = c.qkv_row()
            pos[b] = c.n - 1
    A.k_cache.copy_(_t(K, dev))
    A.v_cache.copy_(_t(V, dev))
    return A, _t(qkv, dev), _t(pos, dev), pos


@pytest.mark.parametrize("which", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("heads,kv_heads", SHAPES)
def test_batched_step_against_float64_and_the_single_step(dev, heads, kv_heads, which):
    plan = _batch_rows(heads, kv_heads, which)
    cases = _make_rows(plan, heads, kv_heads, seed=10 * which)
    A, qkv, pos_t, pos = _contiguous_batch(dev, cases, heads, kv_heads)
    S, _, _, _ = _contiguous_batch(dev, cases, heads, kv_heads)  # the same slots for the single step, one sequence at a time
    out = A.step(qkv, pos_t, BOUND)
    torch.cuda.synchronize()
    worst = {}
    for b, c in enumerate(cases):
        if c is None:
            assert not out[b].any(), f"slot {b}: an inactive row is not zeros"
            assert torch.equal(_bits(A.k_cache[b]), _bits(S.k_cache[b])) and torch.equal(_bits(A.v_cache[b]), _bits(S.v_cache[b])), f"slot {b}: an inactive row's cache changed"
            continue
        worst[c.family] = ac.error_ratio(out[b].cpu().numpy().astype(np.float64).reshape(heads, HD), c.reference())
        one = S.slot(b).step(qkv[b], BOUND, pos_device=pos_t[b:b + 1])
        torch.cuda.synchronize()
        assert torch.equal(_bits(out[b].view(heads, HD)), _bits(one)), f"slot {b} ({c.family}): the batched row differs from the single step on the same data"
        assert np.array_equal(A.k_cache[b, :, :c.n].cpu().numpy().view(np.uint16), c.K.view(np.uint16)), f"slot {b}: appended key"
    _report(f"batch {heads}/{kv_heads}", worst)
    assert max(worst.values()) <= 1.0, worst


NAN_BITS = [0x7E00, 0x7D55, -512 + 1, 0x7FFF]


def _paged_from(dev, A, pos, page_keys, seed, kv_dtype="fp16", ke=0, ve=0, alloc=None):
    """One layer's pools behind an allocator with a permuted free order: every active slot gets exactly the pages its position needs and the contiguous rows
    0 .. pos - 1 scattered into them (the row at pos is the step's to write)."""
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchDecodeAttention
    fresh = alloc is None
    if fresh:
        stride = MAX_KEYS // page_keys
        num_pages = A.batch * stride + 5
        alloc = PageAllocator(num_pages, page_keys, A.batch, stride, dev, free_order=np.random.default_rng(seed).permutation(num_pages).tolist())
    P = PagedBatchDecodeAttention(alloc, A.heads, A.kv_heads, dev, None, None, kv_dtype=kv_dtype, k_scale_log2=ke, v_scale_log2=ve)

    class _Slot:
        def __init__(self, b):
            self.k_cache, self.v_cache = A.k_cache[b], A.v_cache[b]

    for b, p in enumerate(pos.tolist()):
        if p >= 0:
            if fresh:
                alloc.reserve(b, p)
            if p > 0:
                P.admit(b, _Slot(b), 0, p)
    return alloc, P


def _plant_canaries(alloc, pools, pos, dev):
    """Every table word no active row owns names a page nobody owns, full of NaN (fp16 pools: NaN bit patterns; byte pools: 0x7f)."""
    canary = alloc.free[0]
    for pool in pools:
        if pool.dtype == torch.uint8:
            pool[canary].fill_(0x7F)
        else:
            v = pool.view(torch.int16)[canary]
            v.copy_(torch.tensor(NAN_BITS, dtype=torch.int16, device=dev).repeat(v.numel() // 4).view(v.shape))
    table = torch.full_like(alloc.table, canary)
    for b, ps in enumerate(alloc.pages):
        if pos[b] >= 0:
            assert len(ps) == int(pos[b]) // alloc.page_keys + 1 and canary not in ps
            table[b, :len(ps)] = torch.tensor(ps, dtype=torch.int32, device=dev)
    alloc.table.copy_(table)


@pytest.mark.parametrize("which", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("page_keys", PAGE_SIZES)
@pytest.mark.parametrize("heads,kv_heads", SHAPES)
def test_paged_step_is_the_batched_step_bit_for_bit(dev, heads, kv_heads, page_keys, which):
    plan = _batch_rows(heads, kv_heads, which)
    cases = _make_rows(plan, heads, kv_heads, seed=10 * which)
    A, qkv, pos_t, pos = _contiguous_batch(dev, cases, heads, kv_heads)
    alloc, P = _paged_from(dev, A, pos, page_keys, seed=which + page_keys)
    _plant_canaries(alloc, (P.k_pool, P.v_pool), pos, dev)
    assert P.table_violations(pos_t, BOUND) == 0, "the block table is not sound: no launch"
    out = P.step(qkv, pos_t, BOUND)
    want = A.step(qkv, pos_t, BOUND)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all(), "a canary page leaked into an output"
    assert torch.equal(_bits(out), _bits(want))
    worst = {}
    for b, c in enumerate(cases):
        if c is not None:
            worst[c.family] = ac.error_ratio(out[b].cpu().numpy().astype(np.float64).reshape(heads, HD), c.reference())
            k, v = P.read_back(b, c.n)
            assert np.array_equal(k.cpu().numpy().view(np.uint16), c.K.view(np.uint16)) and np.array_equal(v.cpu().numpy().view(np.uint16), c.V.view(np.uint16)), f"slot {b}: pages"
    _report(f"paged {heads}/{kv_heads} page_keys {page_keys}", worst)
    assert max(worst.values()) <= 1.0, worst


FP8_FAMILIES = tuple(f for f in ac.FAMILIES if f != "ramp_up")  # (on the e4m3 grid the rounding of K moves a score of t by ~0.004 t: more than the ramp's half nat per key)
FP8_STEP = 200.0  # a stair on the e4m3 grid: see attention_cases.make_case


@pytest.mark.parametrize("ve", [0, -8])
@pytest.mark.parametrize("page_keys", PAGE_SIZES)
@pytest.mark.parametrize("heads,kv_heads", SHAPES)
def test_fp8_paged_step_against_the_fp16_paged_step_and_float64(dev, heads, kv_heads, page_keys, ve):
    """Per family one launch: the family at two positions (one chunk's worth of keys, and 321 keys under the bound's cut) and an inactive slot; K on the e4m3 grid of
    the smallest exponent that holds both rows, V on the grid of `ve`.  The e4m3 step equals the fp16 paged step on the dequantised pools bit for bit and float64 on
    what read_back returns.  `subnormal_v` exists at ve = -8 only (e4m3's smallest value at exponent 0 is 2^-9)."""
    from tinychatengine_amd import capi
    chunk = capi.describe_attention_batch(3, heads, kv_heads, BOUND)["keys-per-chunk"]
    worst = {}
    for i, family in enumerate(FP8_FAMILIES):
        if family == "subnormal_v" and ve != -8:
            continue
        sizes = [chunk, None, 321]
        mk = lambda ke: [None if n is None else ac.make_case(family, n, heads, kv_heads, seed=50 + i + b, e4m3=True, ke=ke, ve=ve, step=FP8_STEP) for b, n in enumerate(sizes)]
        ke = max(c.ke for c in mk(None) if c is not None)
        cases = mk(ke)
        A, qkv, pos_t, pos = _contiguous_batch(dev, cases, heads, kv_heads)
        alloc, P16 = _paged_from(dev, A, pos, page_keys, seed=i + page_keys)
        _, P8 = _paged_from(dev, A, pos, page_keys, seed=0, kv_dtype="fp8_e4m3", ke=ke, ve=ve, alloc=alloc)
        _plant_canaries(alloc, (P16.k_pool, P16.v_pool, P8.k_pool, P8.v_pool), pos, dev)
        assert P8.table_violations(pos_t, BOUND) == 0
        out8 = P8.step(qkv, pos_t, BOUND)
        out16 = P16.step(qkv, pos_t, BOUND)
        torch.cuda.synchronize()
        assert torch.isfinite(out8.float()).all(), family
        assert torch.equal(_bits(out8), _bits(out16)), f"{family}: the e4m3 step differs from the fp16 step on the dequantised pools"
        for b, c in enumerate(cases):
            if c is None:
                assert not out8[b].any()
                continue
            k, v = P8.read_back(b, c.n)
            k, v = k.cpu().numpy(), v.cpu().numpy()
            assert np.array_equal(k.view(np.uint16), c.K.view(np.uint16)) and np.array_equal(v.view(np.uint16), c.V.view(np.uint16)), f"{family} slot {b}: the pages do not hold the case"
            ref = ac.reference_f64(c.q[0], np.repeat(k, c.rep, axis=0), np.repeat(v, c.rep, axis=0))
            r = ac.error_ratio(out8[b].cpu().numpy().astype(np.float64).reshape(heads, HD), ref)
            worst[family] = max(worst.get(family, 0.0), r)
    _report(f"fp8 step {heads}/{kv_heads} page_keys {page_keys} ve {ve}", worst)
    assert max(worst.values()) <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------------------------------
# prefill
# ---------------------------------------------------------------------------------------------------------------------------------
PREFILL_FAMILIES = ("sink_first", "two_peaks", "stairs_up", "stairs_down", "out_of_range", "all_out_of_range", "subnormal_v")
SEGMENT_SETS = [[(0, 0, 30)], [(2, 17, 64)], [(2, 17, 64), (0, 0, 30), (1, 5, 1)]]  # (slot, cached keys, new rows): tests/test_gpu_fp8_kv.py's
PREFILL_FORMS = [2954, 2958, 2704]  # 4 / 8 waves x one row tile; 4 waves with pairing forced on
PREFILL_KEYS, PREFILL_PAGE = 128, 16


def _prefill_reference(case, pos, m, causal):
    """[m][heads][hd]: row r is query row r over keys 0 .. pos + m - 1, of which it sees 0 .. pos + r when causal."""
    keys = np.arange(pos + m)
    return np.stack([case.reference(row=r, visible=(keys <= pos + r) if causal else None) for r in range(m)])


def _prefill_qkv(case, pos, m):
    heads, kvh = case.heads, case.kv_heads
    return np.concatenate([case.q.reshape(m, heads * HD), case.K[:, pos:].transpose(1, 0, 2).reshape(m, kvh * HD), case.V[:, pos:].transpose(1, 0, 2).reshape(m, kvh * HD)], axis=1)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("mode", PREFILL_FORMS)
@pytest.mark.parametrize("heads,kv_heads", SHAPES)
def test_prefill_contiguous_and_paged_against_float64(dev, heads, kv_heads, mode, causal):
    """Without RoPE: prefill rotates every row by its own position, and a score designed as a . t does not survive a per-row rotation (the rotated forms are covered
    on Gaussian rows by tests/test_gpu_attention.py and on the single step above).  The new rows' keys are designed like the cached ones; EVERY output row is compared.
    The paged launch serves all segments of a set at once and equals the contiguous launches bit for bit.
    A family's property is asserted on all pos + m keys of each query row; a causal row sees a prefix of them (of `two_peaks` only the first peak until the last two
    rows, of a staircase the stairs up to its own), and the float64 reference is taken over exactly that prefix."""
    from tinychatengine_amd.attention_ops import DecodeAttention
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchDecodeAttention
    worst = {}
    with _Mode(mode, 2950):
        for fi, family in enumerate(PREFILL_FAMILIES):
            for si, segments in enumerate(SEGMENT_SETS):
                stride = PREFILL_KEYS // PREFILL_PAGE
                num_pages = 3 * stride + 4
                alloc = PageAllocator(num_pages, PREFILL_PAGE, 3, stride, dev, free_order=np.random.default_rng(mode + fi + si).permutation(num_pages).tolist())
                P = PagedBatchDecodeAttention(alloc, heads, kv_heads, dev, None, None)
                nan = torch.tensor(NAN_BITS, dtype=torch.int16, device=dev)
                for pool in (P.k_pool, P.v_pool):  # every row nobody writes holds NaN bits
                    pool.view(torch.int16).copy_(nan.repeat(pool.numel() // 4).view(pool.shape))
                cases, conts, rows = [], [], []
                for slot, pos, m in segments:
                    case = ac.make_case(family, pos + m, heads, kv_heads, seed=100 + slot + si, rows=m)
                    cont = DecodeAttention(heads, HD, PREFILL_KEYS, dev, None, None, kv_heads=kv_heads)
                    cont.k_cache.view(torch.int16).fill_(INF_BITS)
                    cont.v_cache.view(torch.int16).fill_(INF_BITS)
                    alloc.reserve(slot, pos + m - 1)
                    if pos:
                        cont.k_cache[:, :pos].copy_(_t(case.K[:, :pos], dev))
                        cont.v_cache[:, :pos].copy_(_t(case.V[:, :pos], dev))
                        P.admit(slot, cont, 0, pos)
                    cases.append(case); conts.append(cont); rows.append(_prefill_qkv(case, pos, m))
                qkv = _t(np.concatenate(rows), dev)
                out_p = P.prefill(segments, qkv, causal=causal)
                torch.cuda.synchronize()
                row0 = 0
                for (slot, pos, m), case, cont in zip(segments, cases, conts):
                    out_c = cont.prefill(qkv[row0:row0 + m].contiguous(), pos, causal=causal)
                    torch.cuda.synchronize()
                    what = f"{family} segment {(slot, pos, m)}"
                    assert np.array_equal(cont.k_cache[:, :pos + m].cpu().numpy().view(np.uint16), case.K.view(np.uint16)), f"{what}: appended keys"
                    assert torch.equal(_bits(out_p[row0:row0 + m]), _bits(out_c)), f"{what}: the paged rows differ from the contiguous launch"
                    k, v = P.read_back(slot, pos + m)
                    assert torch.equal(_bits(k), _bits(cont.k_cache[:, :pos + m])) and torch.equal(_bits(v), _bits(cont.v_cache[:, :pos + m])), f"{what}: pages"
                    got = out_c.cpu().numpy().astype(np.float64).reshape(m, heads, HD)
                    worst[family] = max(worst.get(family, 0.0), ac.error_ratio(got, _prefill_reference(case, pos, m, causal)))
                    row0 += m
    _report(f"prefill {heads}/{kv_heads} form {mode} causal {causal}", worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("ve", [0, -8])
@pytest.mark.parametrize("mode", PREFILL_FORMS)
@pytest.mark.parametrize("heads,kv_heads", SHAPES)
def test_fp8_paged_prefill_against_float64(dev, heads, kv_heads, mode, ve):
    """The e4m3 pages: cached and new rows on the grid (K: one exponent for the launch's segments), every output row against float64 on what read_back returns."""
    from tinychatengine_amd.attention_ops import DecodeAttention
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchDecodeAttention
    worst = {}
    with _Mode(mode, 2950):
        for fi, family in enumerate(PREFILL_FAMILIES):
            if family == "subnormal_v" and ve != -8:
                continue
            for causal, segments in [(c, segs) for segs in SEGMENT_SETS for c in (True, False)]:
                mk = lambda ke: [ac.make_case(family, pos + m, heads, kv_heads, seed=200 + slot, rows=m, e4m3=True, ke=ke, ve=ve, step=FP8_STEP) for slot, pos, m in segments]
                ke = max(c.ke for c in mk(None))
                cases = mk(ke)
                stride = PREFILL_KEYS // PREFILL_PAGE
                num_pages = 3 * stride + 4
                alloc = PageAllocator(num_pages, PREFILL_PAGE, 3, stride, dev, free_order=np.random.default_rng(mode + fi).permutation(num_pages).tolist())
                P = PagedBatchDecodeAttention(alloc, heads, kv_heads, dev, None, None, kv_dtype="fp8_e4m3", k_scale_log2=ke, v_scale_log2=ve)
                P.k_pool.fill_(0x7F)
                P.v_pool.fill_(0x7F)
                rows = []
                for (slot, pos, m), case in zip(segments, cases):
                    alloc.reserve(slot, pos + m - 1)
                    if pos:
                        cont = DecodeAttention(heads, HD, PREFILL_KEYS, dev, None, None, kv_heads=kv_heads)
                        cont.k_cache[:, :pos].copy_(_t(case.K[:, :pos], dev))
                        cont.v_cache[:, :pos].copy_(_t(case.V[:, :pos], dev))
                        P.admit(slot, cont, 0, pos)
                    rows.append(_prefill_qkv(case, pos, m))
                out = P.prefill(segments, _t(np.concatenate(rows), dev), causal=causal)
                torch.cuda.synchronize()
                row0 = 0
                for (slot, pos, m), case in zip(segments, cases):
                    k, v = P.read_back(slot, pos + m)
                    assert np.array_equal(k.cpu().numpy().view(np.uint16), case.K.view(np.uint16)) and np.array_equal(v.cpu().numpy().view(np.uint16), case.V.view(np.uint16)), \
                        f"{family} segment {(slot, pos, m)}: the pages do not hold the case"
                    got = out[row0:row0 + m].cpu().numpy().astype(np.float64).reshape(m, heads, HD)
                    worst[family] = max(worst.get(family, 0.0), ac.error_ratio(got, _prefill_reference(case, pos, m, causal)))
                    row0 += m
    _report(f"fp8 prefill {heads}/{kv_heads} form {mode} ve {ve}", worst)
    assert max(worst.values()) <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------------------------------
# o_proj's deferred combine
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FORM_FAMILIES)
def test_deferred_combine_gives_the_same_bits_on_designed_rows(dev, family):
    """The step that stops at its partial states + o_proj combining them in its prologue against the step with its own combine + the plain o_proj: the same bits, as
    tests/test_gpu_deferred_attention.py asserts on Gaussian caches -- here with chunk maxima 100 nats apart, merge weights of exactly 1/2 and clamped scores.  8 query
    heads over 2 (the deferred linear needs heads * 128 to be a multiple of 1024); 321 keys: 4 slots, 1025: 8."""
    from tinychatengine_amd.attention_ops import DecodeAttention
    from tinychatengine_amd.linear import Linear_half_int4
    heads, kv_heads, hidden = 8, 2, 8 * HD
    g = torch.Generator(device=dev).manual_seed(7)
    o = Linear_half_int4.from_float(torch.empty(hidden, hidden, device=dev).normal_(0, hidden ** -0.5, generator=g), 128).prepack()
    res = torch.empty(1, hidden, device=dev).normal_(0, 1, generator=g).to(torch.float16)
    seen, worst = set(), {}
    for n in (321, 1025):
        case = ac.make_case(family, n, heads, kv_heads, seed=6)
        atts = [DecodeAttention(heads, HD, n, dev, None, None, kv_heads=kv_heads) for _ in range(2)]
        for a in atts:
            a.k_cache[:, :n - 1].copy_(_t(case.K[:, :n - 1], dev))
            a.v_cache[:, :n - 1].copy_(_t(case.V[:, :n - 1], dev))
        qkv = _t(case.qkv_row(), dev)
        x0, y0 = _plain(atts[0], o, qkv, res, n - 1)
        x1, y1, slots = _deferred(atts[1], o, qkv, res, n - 1)
        torch.cuda.synchronize()
        seen.add(slots)
        assert torch.isfinite(y0.float()).all()
        assert torch.equal(y0, y1), f"{family}, {n} keys ({slots} slots): o_proj + residual differs"
        assert torch.equal(atts[0].k_cache, atts[1].k_cache) and torch.equal(atts[0].v_cache, atts[1].v_cache)
        worst[n] = ac.error_ratio(x0.cpu().numpy().astype(np.float64).reshape(heads, HD), case.reference())
    _report(f"deferred {family}", worst)
    assert seen == {4, 8}, seen
    assert max(worst.values()) <= 1.0, worst
