"""Sliding-window attention on the paged cache (include/tce_matmul.h, "SLIDING-WINDOW"): the windowed step and prefill, fp16 and e4m3 pages, and the pages they give back.

    A  a window that never binds IS today's kernel: `out` and every pool byte, no tolerance
    B  where lo is a multiple of page_keys the windowed step equals the EXISTING step of the re-based launch (bound W + 2, position W - 1, the table row from word
       lo / page_keys, cos / sin advanced by lo rows), no tolerance
    C  everywhere else: float64 over keys lo .. p (attention_cases.reference_f64 with `visible`) within the project's bound (attention_cases.bound), on designed rows
       and with a dominant key planted at lo - 1 (must weigh nothing) and at lo (must dominate)
    D  no table word outside lo / page_keys .. pos / page_keys is followed: they point at NaN canary pages -- valid page numbers -- and nothing changes
    E  pages really come back: a captured step replayed with release_behind in between and the freed pages overwritten; a generator on a pool too small for full
       attention

Shapes: heads / kv_heads (4, 1) and (8, 8) throughout, (32, 8) once per contract; page_keys 16 and 64; pos_bound <= 2047; three rows per launch, one of them inactive."""
import numpy as np
import pytest

import attention_cases as ac

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HD = 128
BOUND = 2047
WINDOWS = (1,) + tuple(n - 3 for n in ac.SIZES if n > 3)  # W + 3 = the chunk rule's sizes: 1, 2, 14, 125, 317, 318, 638, 1022
FP8_FAMILIES = tuple(f for f in ac.FAMILIES if f != "ramp_up")  # (the e4m3 grid cannot hold the ramp's half nat per key: tests/test_gpu_attention_adversarial.py)
FP8_STEP = 200.0


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.uint8)


def _tables(n, seed, dev):
    cos, sin = ac.rope_tables(n, seed)
    return torch.from_numpy(cos).to(dev), torch.from_numpy(sin).to(dev)


def _allocator(dev, page_keys, batch, keys, num_pages, seed=0):
    from tinychatengine_amd.paged_kv import PageAllocator
    return PageAllocator(num_pages, page_keys, batch, keys // page_keys, dev, free_order=np.random.default_rng(seed).permutation(num_pages).tolist())


def _attention(alloc, heads, kv_heads, dev, fp8=False, window=None, cos=None, sin=None, ke=0, ve=0):
    from tinychatengine_amd.paged_kv import PagedBatchDecodeAttention
    return PagedBatchDecodeAttention(alloc, heads, kv_heads, dev, cos, sin, kv_dtype="fp8_e4m3" if fp8 else "fp16", k_scale_log2=ke, v_scale_log2=ve, window=window)


_NOISE, _NOISE_LEN = {}, 1 << 24


def _randomise(P, seed):
    """Finite random contents for both pools: a stretch, chosen by the seed, of one Gaussian array per element type made once on the host (e4m3: rounded to the grid,
    so no NaN byte)."""
    if P.fp8 not in _NOISE:
        x = torch.from_numpy(np.random.default_rng(123).standard_normal(_NOISE_LEN, dtype=np.float32) * 0.7)
        _NOISE[P.fp8] = (x.to(torch.float8_e4m3fn).view(torch.uint8) if P.fp8 else x.half()).to(P.k_pool.device)
    n = P.k_pool.numel()
    assert 2 * n <= _NOISE_LEN
    off = (seed * 40503) % (_NOISE_LEN - 2 * n + 1)
    P.k_pool.copy_(_NOISE[P.fp8][off:off + n].view(P.k_pool.shape))
    P.v_pool.copy_(_NOISE[P.fp8][off + n:off + 2 * n].view(P.v_pool.shape))


def _same_pools(dst, src):
    dst.k_pool.copy_(src.k_pool)
    dst.v_pool.copy_(src.v_pool)


def _pools_equal(P, Q):
    return torch.equal(_bits(P.k_pool), _bits(Q.k_pool)) and torch.equal(_bits(P.v_pool), _bits(Q.v_pool))


def _qkv(dev, rows, heads, kv_heads, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn((rows, (heads + 2 * kv_heads) * HD), generator=g, device=dev) * 0.9).half()


class _Pair:
    """A contiguous cache pair [kv_heads][keys][hd] on the device: what PagedBatchDecodeAttention.admit scatters from."""

    def __init__(self, K, V, dev):
        self.k_cache, self.v_cache = torch.from_numpy(np.ascontiguousarray(K)).to(dev), torch.from_numpy(np.ascontiguousarray(V)).to(dev)


def _lo(pos, W):
    return max(0, pos - W + 1)


# =====================================================================================================================================================================
# A  never binding = today's kernels
# =====================================================================================================================================================================
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("heads,kv_heads,page_keys", [(4, 1, 16), (4, 1, 64), (8, 8, 16), (8, 8, 64), (32, 8, 64)])
def test_a_step_with_a_window_that_never_binds_is_todays_step(dev, heads, kv_heads, page_keys, fp8):
    for bound in (63, 1023):
        keys = (bound // page_keys + 1) * page_keys
        for rope in (True, False):
            cos, sin = _tables(keys, bound, dev) if rope else (None, None)
            for W in (bound + 1, 2 ** 30):
                alloc = _allocator(dev, page_keys, 3, keys, 3 * (keys // page_keys) + 2, seed=bound)
                P0 = _attention(alloc, heads, kv_heads, dev, fp8, None, cos, sin, ke=1, ve=-1)
                Pw = _attention(alloc, heads, kv_heads, dev, fp8, W, cos, sin, ke=1, ve=-1)
                _randomise(P0, bound + page_keys)
                _same_pools(Pw, P0)
                pos = np.array([bound, -1, bound * 2 // 3], np.int32)
                for b, p in enumerate(pos.tolist()):
                    if p >= 0:
                        alloc.reserve(b, p)
                pos_t = torch.from_numpy(pos).to(dev)
                qkv = _qkv(dev, 3, heads, kv_heads, bound + W % 7)
                assert Pw.table_violations(pos_t, bound) == 0 and P0.table_violations(pos_t, bound) == 0
                want, got = P0.step(qkv, pos_t, bound), Pw.step(qkv, pos_t, bound)
                torch.cuda.synchronize()
                what = f"bound={bound} rope={rope} W={W}"
                assert torch.equal(_bits(got), _bits(want)), f"{what}: outputs differ"
                assert _pools_equal(Pw, P0), f"{what}: a pool byte differs"
                assert not got[1].any()


SEGMENT_SETS = [[(1, 100, 130)], [(0, 3, 65), (2, 0, 5)], [(3, 0, 64), (0, 100, 1), (4, 3, 130), (1, 0, 5), (2, 100, 65)]]  # (slot, cached keys, new rows)


def _prefill_pair(dev, heads, kv_heads, page_keys, fp8, W, segments, rope, seed):
    """Two attention objects over one allocator with the same random pools -- unwindowed, windowed -- the segments' pages reserved, and packed q/k/v rows."""
    keys, batch = 256, 5
    cos, sin = _tables(keys, seed, dev) if rope else (None, None)
    alloc = _allocator(dev, page_keys, batch, keys, batch * (keys // page_keys), seed=seed)
    P0 = _attention(alloc, heads, kv_heads, dev, fp8, None, cos, sin, ke=1, ve=0)
    Pw = _attention(alloc, heads, kv_heads, dev, fp8, W, cos, sin, ke=1, ve=0)
    _randomise(P0, seed + 1)
    _same_pools(Pw, P0)
    for slot, pos, m in segments:
        alloc.reserve(slot, pos + m - 1)
    return alloc, P0, Pw, _qkv(dev, sum(m for _, _, m in segments), heads, kv_heads, seed + 2)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("heads,kv_heads,page_keys", [(4, 1, 16), (8, 8, 64), (32, 8, 16)])
def test_a_prefill_with_a_window_that_never_binds_is_todays_prefill(dev, heads, kv_heads, page_keys, fp8):
    from tinychatengine_amd import capi
    for i, segments in enumerate(SEGMENT_SETS):
        reach = max(pos + m for _, pos, m in segments)
        for W in (reach, 2 ** 30):
            alloc, P0, Pw, qkv = _prefill_pair(dev, heads, kv_heads, page_keys, fp8, W, segments, rope=i != 1, seed=10 * i + page_keys)
            assert capi.describe_prefill_paged(heads, kv_heads, True, segments)["segments"] == len(segments)  # (one plan serves both launches: form and pairs are its)
            want, got = P0.prefill(segments, qkv), Pw.prefill(segments, qkv)
            torch.cuda.synchronize()
            assert torch.equal(_bits(got), _bits(want)), f"segments {segments} W={W}: outputs differ"
            assert _pools_equal(Pw, P0), f"segments {segments} W={W}: a pool byte differs"


# =====================================================================================================================================================================
# B  the re-based identity
# =====================================================================================================================================================================
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("heads,kv_heads,page_keys", [(4, 1, 16), (4, 1, 64), (8, 8, 16), (8, 8, 64), (32, 8, 16)])
def test_b_windowed_step_equals_the_existing_step_of_the_rebased_launch(dev, heads, kv_heads, page_keys, fp8):
    from tinychatengine_amd import capi
    keys = BOUND + 1
    stride = keys // page_keys
    cos, sin = _tables(keys, 5, dev)
    for W in WINDOWS:
        assert capi.describe_attention_paged_window(3, heads, kv_heads, BOUND, page_keys, W) == capi.describe_attention_paged(3, heads, kv_heads, W + 2, page_keys)
        for lo in (0, page_keys, 5 * page_keys):
            pos_w = lo + W - 1
            need = pos_w // page_keys + 1
            alloc = _allocator(dev, page_keys, 3, keys, 2 * need + 3, seed=W + lo)
            ref_alloc = _allocator(dev, page_keys, 3, keys, 2 * need + 3)  # only its table is used: the same page numbers from word lo / page_keys on
            Pw = _attention(alloc, heads, kv_heads, dev, fp8, W, cos, sin, ke=0, ve=1)
            Pr = _attention(ref_alloc, heads, kv_heads, dev, fp8, None, cos[lo:], sin[lo:], ke=0, ve=1)
            _randomise(Pw, W + lo + page_keys)
            _same_pools(Pr, Pw)
            k0, v0 = Pw.k_pool.clone(), Pw.v_pool.clone()
            for b in (0, 2):
                alloc.reserve(b, pos_w)
            shifted = torch.zeros_like(alloc.table)
            shifted[:, :stride - lo // page_keys] = alloc.table[:, lo // page_keys:]
            ref_alloc.table.copy_(shifted)
            pos = torch.tensor([pos_w, -1, pos_w], dtype=torch.int32, device=dev)
            pos_r = torch.tensor([W - 1, -1, W - 1], dtype=torch.int32, device=dev)
            qkv = _qkv(dev, 3, heads, kv_heads, W + lo)
            assert Pw.table_violations(pos, BOUND) == 0
            got, want = Pw.step(qkv, pos, BOUND), Pr.step(qkv, pos_r, W + 2)
            torch.cuda.synchronize()
            what = f"W={W} lo={lo}"
            assert torch.equal(_bits(got), _bits(want)), f"{what}: outputs differ"
            assert _pools_equal(Pw, Pr), f"{what}: the appended rows differ"
            # nothing but row pos of the two active slots changed
            for pool, before in ((Pw.k_pool, k0), (Pw.v_pool, v0)):
                changed = (_bits(pool) != _bits(before)).reshape(pool.shape[0], kv_heads, page_keys, -1).any(dim=3).any(dim=1)  # [page][row]
                allowed = torch.zeros_like(changed)
                for b in (0, 2):
                    allowed[alloc.pages[b][pos_w // page_keys], pos_w % page_keys] = True
                assert not (changed & ~allowed).any(), f"{what}: a pool row other than the appended ones changed"


# =====================================================================================================================================================================
# C  against float64
# =====================================================================================================================================================================
def _step_positions(capi, heads, kv_heads, page_keys, W, core=False):
    """W - 2 .. W + 3 (lo = 0, 0, 1, 2, 3, 4: every lo % 4), a page edge on either side of lo and of pos, and the positions at which the span meets a chunk edge.
    core: one position of each kind (the e4m3 runs, whose cases cost the host twice as much)."""
    chunk = capi.describe_attention_paged_window(3, heads, kv_heads, BOUND, page_keys, W)["keys-per-chunk"]
    edge = (W // page_keys + 2) * page_keys  # a multiple of page_keys with lo > 0
    if core:
        ps = {W - 1, W, W + 1, W + 2, W + 3, edge - 1, edge + W - 1, 4 + chunk - 1}
    else:
        ps = {W - 2, W - 1, W, W + 1, W + 2, W + 3, edge - 1, edge, edge + W - 1, edge + W - 2, edge + W}
        for base in (4, 64):  # pos - base + 1 = chunk or chunk + 1 with base = lo & ~3
            ps |= {base + chunk - 1, base + chunk, base + chunk - 2}
    return sorted(p for p in ps if 0 <= p <= BOUND)


def _step_cases(dev, heads, kv_heads, page_keys, fp8, W, cases):
    """One windowed launch for two cases (rows 0 and 2; row 1 inactive): their keys 0 .. pos - 1 scattered into pages, the own row in q/k/v.  Returns the outputs."""
    keys = BOUND + 1
    pos = [c.n - 1 for c in cases]
    need = sum(p // page_keys + 1 for p in pos)
    alloc = _allocator(dev, page_keys, 3, keys, need + 2, seed=W + pos[0])
    ke, ve = (cases[0].ke, cases[0].ve) if fp8 else (0, 0)
    P = _attention(alloc, heads, kv_heads, dev, fp8, W, ke=ke, ve=ve)
    _randomise(P, W + pos[1])
    qkv = torch.zeros((3, (heads + 2 * kv_heads) * HD), dtype=torch.float16, device=dev)
    for b, c in zip((0, 2), cases):
        alloc.reserve(b, c.n - 1)
        if c.n > 1:
            P.admit(b, _Pair(c.K[:, :c.n - 1], c.V[:, :c.n - 1], dev), 0, c.n - 1)
        qkv[b].copy_(torch.from_numpy(c.qkv_row()).to(dev))
    pos_t = torch.tensor([pos[0], -1, pos[1]], dtype=torch.int32, device=dev)
    assert P.table_violations(pos_t, BOUND) == 0
    out = P.step(qkv, pos_t, BOUND)
    torch.cuda.synchronize()
    assert not out[1].any()
    return [out[b].cpu().numpy().reshape(heads, HD) for b in (0, 2)]


def _seeded(make, seed):
    """make(seed), with the next seeds tried where make_case's own guard refuses a draw (an `out_of_range` pilot short enough to push a designed key past 40000:
    a property of the draw, asserted by the generator before it hands a case out)."""
    for attempt in range(8):
        try:
            return make(seed + 1000 * attempt)
        except AssertionError as e:
            if "a designed key reaches" not in str(e) or attempt == 7:
                raise


def _make_pair(family, ns, heads, kv_heads, seed, fp8, own=None):
    kw = [dict(own=o) for o in own] if own is not None else [{}, {}]
    if not fp8:
        return [_seeded(lambda sd: ac.make_case(family, n, heads, kv_heads, seed=sd, **k), seed + i) for i, (n, k) in enumerate(zip(ns, kw))]
    ve = -8 if family == "subnormal_v" else 0
    mk = lambda i, ke: _seeded(lambda sd: ac.make_case(family, ns[i], heads, kv_heads, seed=sd, e4m3=True, ke=ke, ve=ve, step=FP8_STEP, **kw[i]), seed + i)
    cases = [mk(0, None), mk(1, None)]
    ke = max(c.ke for c in cases)  # one exponent per launch
    return [c if c.ke == ke else mk(i, ke) for i, c in enumerate(cases)]


def _step_against_float64(dev, family, heads, kv_heads, page_keys, fp8):
    from tinychatengine_amd import capi
    worst = 0.0
    for W in WINDOWS:
        ps = _step_positions(capi, heads, kv_heads, page_keys, W, core=fp8)
        if fp8 and family in ("stairs_up", "stairs_down"):
            # the generator's limit, not the kernel's: rounding K to the e4m3 grid moves a score of t by ~0.004 t, and beyond ~40 stairs of 200 nats that is more than
            # the 90 nats make_case asserts between stairs (tests/test_gpu_attention_adversarial.py builds these families up to 321 keys)
            ps = [p for p in ps if p < 512]
            if not ps:
                continue
        if len(ps) % 2:
            ps.append(ps[0])
        for i in range(0, len(ps), 2):
            cases = _make_pair(family, [ps[i] + 1, ps[i + 1] + 1], heads, kv_heads, 7 * W + i, fp8)
            outs = _step_cases(dev, heads, kv_heads, page_keys, fp8, W, cases)
            for c, got in zip(cases, outs):
                ref = c.reference(visible=np.arange(c.n) >= _lo(c.n - 1, W))
                r = ac.error_ratio(got, ref)
                worst = max(worst, r)
                assert r <= 1.0, f"{family} W={W} pos={c.n - 1} lo={_lo(c.n - 1, W)}: {r:.3f} of the bound"
    print(f"{family} {heads}/{kv_heads} page_keys={page_keys} fp8={fp8}: worst {worst:.3f} of the bound")


@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("heads,kv_heads,page_keys", [(4, 1, 16), (8, 8, 64)])
def test_c_windowed_step_against_float64(dev, family, heads, kv_heads, page_keys):
    _step_against_float64(dev, family, heads, kv_heads, page_keys, False)


@pytest.mark.parametrize("family", FP8_FAMILIES)
@pytest.mark.parametrize("heads,kv_heads,page_keys", [(4, 1, 64), (8, 8, 16)])
def test_c_windowed_step_against_float64_e4m3(dev, family, heads, kv_heads, page_keys):
    _step_against_float64(dev, family, heads, kv_heads, page_keys, True)


@pytest.mark.parametrize("family", ["sink_first", "stairs_up", "out_of_range"])
def test_c_windowed_step_against_float64_llama_heads(dev, family):
    _step_against_float64(dev, family, 32, 8, 64, False)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("heads,kv_heads,page_keys", [(4, 1, 16), (8, 8, 64), (32, 8, 64)])
def test_c_a_dominant_key_just_outside_weighs_nothing_and_just_inside_dominates(dev, heads, kv_heads, page_keys, fp8):
    """`sink_own` with its peak moved: 30 nats above every other key, at lo - 1 and at lo.  An off-by-one at the lower end of the mask is an error of the size of a
    value row here, where Gaussian rows would hide it."""
    for W in WINDOWS:
        for pos in (W + 4, W + 2 * page_keys + 1, min(BOUND, W + 1000)):  # lo = 5, 2 page_keys + 2, and far out
            lo = _lo(pos, W)
            cases = _make_pair("sink_own", [pos + 1, pos + 1], heads, kv_heads, 3 * W + pos, fp8, own=[lo - 1, lo])
            outs = _step_cases(dev, heads, kv_heads, page_keys, fp8, W, cases)
            visible = np.arange(pos + 1) >= lo
            for c, got, where in zip(cases, outs, ("lo - 1", "lo")):
                ref = c.reference(visible=visible)
                assert ac.error_ratio(got, ref) <= 1.0, f"W={W} pos={pos}: dominant key at {where}: {ac.error_ratio(got, ref):.3f} of the bound"
            # the two rows are what they are meant to be, on the heads whose query points along the pilot (a > 0: the designed key is 30 nats ABOVE the rest): with
            # the peak inside, the output is that key's value row; outside, it is not
            up = cases[0].a[0] > 0
            _, Vr = cases[1].repeated()
            assert np.abs(outs[1] - Vr[:, lo].astype(np.float64))[up].max() < 0.02, f"W={W} pos={pos}: the key at lo does not dominate"
            _, Vo = cases[0].repeated()
            assert np.abs(outs[0] - Vo[:, lo - 1].astype(np.float64))[up].max() > 0.1, f"W={W} pos={pos}: the key at lo - 1 was weighed"


PREFILL_M, PREFILL_POS, PREFILL_W = (1, 5, 64, 65, 130), (0, 3, 100), (1, 17, 64, 100)


def _prefill_launch(dev, heads, kv_heads, page_keys, fp8, W, segments, family, seed):
    """One windowed and one unwindowed prefill of the same designed segments; every row of the first against float64, the appended rows of both bit for bit."""
    keys, batch = 256, 5
    ve = -8 if family == "subnormal_v" else 0
    if fp8:
        mk = lambda ke: [ac.make_case(family, pos + m, heads, kv_heads, seed=seed + slot, rows=m, e4m3=True, ke=ke, ve=ve, step=FP8_STEP) for slot, pos, m in segments]
        cases = mk(max(c.ke for c in mk(None)))
        ke = cases[0].ke
    else:
        cases, ke, ve = [ac.make_case(family, pos + m, heads, kv_heads, seed=seed + slot, rows=m) for slot, pos, m in segments], 0, 0
    alloc = _allocator(dev, page_keys, batch, keys, batch * (keys // page_keys), seed=seed)
    Pw, P0 = _attention(alloc, heads, kv_heads, dev, fp8, W, ke=ke, ve=ve), _attention(alloc, heads, kv_heads, dev, fp8, None, ke=ke, ve=ve)
    _randomise(Pw, seed)
    rows = []
    for (slot, pos, m), c in zip(segments, cases):
        alloc.reserve(slot, pos + m - 1)
        if pos:
            Pw.admit(slot, _Pair(c.K[:, :pos], c.V[:, :pos], dev), 0, pos)
        rows += [c.qkv_row(row=i, key=pos + i) for i in range(m)]
    _same_pools(P0, Pw)
    qkv = torch.from_numpy(np.stack(rows)).to(dev)
    out = Pw.prefill(segments, qkv)
    P0.prefill(segments, qkv)
    torch.cuda.synchronize()
    assert _pools_equal(Pw, P0), f"{segments} W={W}: the windowed prefill appended other rows than the unwindowed one"
    got, r0, worst = out.cpu().numpy(), 0, 0.0
    for (slot, pos, m), c in zip(segments, cases):
        for i in range(m):
            p = pos + i
            k = np.arange(c.n)
            ref = c.reference(row=i, visible=(k >= _lo(p, W)) & (k <= p))
            r = ac.error_ratio(got[r0 + i].reshape(heads, HD), ref)
            worst = max(worst, r)
            assert r <= 1.0, f"{family} W={W} segment (slot {slot}, pos {pos}, m {m}) row {i}: {r:.3f} of the bound"
        r0 += m
    return worst


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("W", PREFILL_W)
@pytest.mark.parametrize("heads,kv_heads,page_keys", [(4, 1, 16), (8, 8, 64)])
def test_c_windowed_prefill_against_float64(dev, heads, kv_heads, page_keys, W, fp8):
    worst = 0.0
    lone = [(m, pos) for m in PREFILL_M for pos in PREFILL_POS]
    for i, (m, pos) in enumerate(lone):  # a lone segment: sink_first puts 30 nats on key 0, which most rows must not see
        worst = max(worst, _prefill_launch(dev, heads, kv_heads, page_keys, fp8, W, [(i % 5, pos, m)], ("sink_first", "two_peaks", "stairs_down")[i % 3], 100 + i))
    for i, segments in enumerate(SEGMENT_SETS[1:]):  # ragged: 2 and 5 segments
        worst = max(worst, _prefill_launch(dev, heads, kv_heads, page_keys, fp8, W, segments, ("sink_first", "out_of_range")[i], 200 + i))
    print(f"prefill {heads}/{kv_heads} page_keys={page_keys} W={W} fp8={fp8}: worst {worst:.3f} of the bound")


def test_c_windowed_prefill_against_float64_llama_heads(dev):
    for W in (17, 100):
        _prefill_launch(dev, 32, 8, 64, False, W, SEGMENT_SETS[2], "sink_first", 300 + W)
        _prefill_launch(dev, 32, 8, 16, True, W, SEGMENT_SETS[1], "stairs_up", 310 + W)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("heads,kv_heads,page_keys", [(4, 1, 16), (8, 8, 64)])
def test_c_windowed_prefill_then_windowed_steps(dev, heads, kv_heads, page_keys, fp8):
    W, m, steps, keys = 17, 65, 24, 256
    case = ac.make_case("two_peaks", m + steps, heads, kv_heads, seed=9, rows=m + steps, **(dict(e4m3=True, ve=0) if fp8 else {}))
    alloc = _allocator(dev, page_keys, 3, keys, 3 * (keys // page_keys), seed=4)
    P = _attention(alloc, heads, kv_heads, dev, fp8, W, ke=case.ke or 0, ve=0)
    _randomise(P, 3)
    alloc.reserve(2, m - 1)
    qkv = torch.from_numpy(np.stack([case.qkv_row(row=i, key=i) for i in range(m)])).to(dev)
    out = P.prefill([(2, 0, m)], qkv).cpu().numpy()
    k = np.arange(case.n)
    for i in range(m):
        assert ac.error_ratio(out[i].reshape(heads, HD), case.reference(row=i, visible=(k >= _lo(i, W)) & (k <= i))) <= 1.0, f"prefill row {i}"
    row = torch.zeros((3, qkv.shape[1]), dtype=torch.float16, device=dev)
    for p in range(m, m + steps):
        alloc.release_behind(2, p - W + 1)
        alloc.reserve(2, p)
        row[2].copy_(torch.from_numpy(case.qkv_row(row=p, key=p)).to(dev))
        pos_t = torch.tensor([-1, -1, p], dtype=torch.int32, device=dev)
        assert P.table_violations(pos_t, keys - 1) == 0
        got = P.step(row, pos_t, keys - 1)[2].cpu().numpy().reshape(heads, HD)
        assert ac.error_ratio(got, case.reference(row=p, visible=(k >= _lo(p, W)) & (k <= p))) <= 1.0, f"step at position {p}"
    alloc.check_invariants()
    assert len(alloc.pages[2]) <= (W + page_keys - 1) // page_keys + 1


# =====================================================================================================================================================================
# D  nothing behind the window is touched
# =====================================================================================================================================================================
def _canary_page(alloc, pools, dev):
    """The last page the allocator would hand out, filled with NaN (e4m3: the NaN byte) in every pool given."""
    page = alloc.free[0]
    for pool in pools:
        if pool.dtype == torch.uint8:
            pool[page].fill_(0x7F)
        else:
            pool[page].copy_(torch.full_like(pool[page], float("nan")))
    return page


def _point_unfollowed_words_at(alloc, canary, rows, page_keys):
    """rows: {slot: (first followed key, last followed key)}.  Every other word of the table -- the whole row of the slots not named -- becomes `canary`."""
    t = torch.full_like(alloc.table, canary)
    for slot, (k0, k1) in rows.items():
        t[slot, k0 // page_keys:k1 // page_keys + 1] = alloc.table[slot, k0 // page_keys:k1 // page_keys + 1]
    alloc.table.copy_(t)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("heads,kv_heads,page_keys", [(4, 1, 16), (8, 8, 64), (32, 8, 16)])
def test_d_the_step_follows_no_table_word_outside_its_window(dev, heads, kv_heads, page_keys, fp8):
    keys = BOUND + 1
    cos, sin = _tables(keys, 8, dev)
    for W in WINDOWS:
        for pos in ([W + 3 * page_keys + 2, 2 * W + 5 * page_keys], [BOUND, W + page_keys - 1]):
            pos = [min(p, BOUND) for p in pos]
            alloc = _allocator(dev, page_keys, 3, keys, sum(p // page_keys + 1 for p in pos) + 3, seed=W)
            P, Q = _attention(alloc, heads, kv_heads, dev, fp8, W, cos, sin), _attention(alloc, heads, kv_heads, dev, fp8, W, cos, sin)
            _randomise(P, W + pos[0])
            for b, p in zip((0, 2), pos):
                alloc.reserve(b, p)
            canary = _canary_page(alloc, (P.k_pool, P.v_pool), dev)
            _same_pools(Q, P)
            pos_t = torch.tensor([pos[0], -1, pos[1]], dtype=torch.int32, device=dev)
            qkv = _qkv(dev, 3, heads, kv_heads, W)
            clean = Q.step(qkv, pos_t, BOUND)  # the table as the allocator wrote it
            _point_unfollowed_words_at(alloc, canary, {b: (_lo(p, W), p) for b, p in zip((0, 2), pos)}, page_keys)
            assert P.table_violations(pos_t, BOUND) == 0
            got = P.step(qkv, pos_t, BOUND)
            torch.cuda.synchronize()
            what = f"W={W} pos={pos}"
            assert torch.isfinite(got.float()).all(), f"{what}: a canary leaked into an output"
            assert torch.equal(_bits(got), _bits(clean)), f"{what}: outputs differ from the clean run"
            assert _pools_equal(P, Q), f"{what}: pools differ from the clean run (the canary page included)"


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("heads,kv_heads,page_keys", [(4, 1, 16), (8, 8, 64), (32, 8, 16)])
def test_d_the_prefill_follows_no_table_word_outside_its_window(dev, heads, kv_heads, page_keys, fp8):
    for W in PREFILL_W:
        for segments in SEGMENT_SETS:
            alloc, _, P, qkv = _prefill_pair(dev, heads, kv_heads, page_keys, fp8, W, segments, rope=True, seed=W + len(segments))
            Q = _attention(alloc, heads, kv_heads, dev, fp8, W, P.cos, P.sin, ke=1, ve=0)
            canary = _canary_page(alloc, (P.k_pool, P.v_pool), dev)
            assert all(canary not in ps for ps in alloc.pages)
            _same_pools(Q, P)
            clean = Q.prefill(segments, qkv)
            # followed: from the first key the segment's FIRST row weighs to its last row's own key
            _point_unfollowed_words_at(alloc, canary, {slot: (_lo(pos, W), pos + m - 1) for slot, pos, m in segments}, page_keys)
            got = P.prefill(segments, qkv)
            torch.cuda.synchronize()
            what = f"W={W} segments={segments}"
            assert torch.isfinite(got.float()).all(), f"{what}: a canary leaked into an output"
            assert torch.equal(_bits(got), _bits(clean)), f"{what}: outputs differ from the clean run"
            assert _pools_equal(P, Q), f"{what}: pools differ from the clean run (the canary page included)"


def test_d_the_table_check_counts_what_a_windowed_row_follows(dev):
    page_keys, keys, W = 16, 512, 40
    alloc = _allocator(dev, page_keys, 3, keys, 70)
    P = _attention(alloc, 4, 1, dev, False, W)
    pos = [300, -1, 37]
    for b, p in zip((0, 2), (300, 37)):
        alloc.reserve(b, p)
    pos_t = torch.tensor(pos, dtype=torch.int32, device=dev)
    good = alloc.table.clone()
    first, last = _lo(300, W) // page_keys, 300 // page_keys  # words 16 .. 18 of row 0; row 2 follows words 0 .. 2
    bad = good.clone()
    bad[0, :first] = -1
    bad[0, last + 1:] = alloc.num_pages
    bad[1, :] = -7
    bad[2, 3:] = alloc.num_pages + 5
    alloc.table.copy_(bad)
    assert P.table_violations(pos_t, keys - 1) == 0, "a word outside the followed range was counted"
    for planted in ([(0, first)], [(0, first), (0, last)], [(0, first + 1), (2, 0), (2, 2)]):
        t = bad.clone()
        for b, e in planted:
            t[b, e] = -1 if e % 2 else alloc.num_pages
        alloc.table.copy_(t)
        assert P.table_violations(pos_t, keys - 1) == len(planted), planted
    alloc.table.copy_(good)
    assert _attention(alloc, 4, 1, dev, False, None).table_violations(pos_t, keys - 1) == 0


# =====================================================================================================================================================================
# E  pages really come back
# =====================================================================================================================================================================
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("heads,kv_heads,page_keys", [(4, 1, 16), (8, 8, 64)])
def test_e_one_captured_step_replayed_while_pages_come_back(dev, heads, kv_heads, page_keys, fp8):
    """The graph holds one windowed step; between replays the host gives the pages behind the window back, fills them with NaN and hands them to another slot.  The
    eager twin keeps every page.  Same outputs, bit for bit, and both within the bound of float64 over the window."""
    W, keys = page_keys + 3, 512
    n0, steps = 2 * page_keys + 1, 3 * page_keys + 5
    case = ac.make_case("two_peaks", n0 + steps, heads, kv_heads, seed=21, rows=n0 + steps, **(dict(e4m3=True, ve=0) if fp8 else {}))
    ke = case.ke or 0
    alloc = _allocator(dev, page_keys, 3, keys, 8, seed=1)  # 8 pages: the sequence alone would need 6 by the end, the squatter takes what comes back
    big = _allocator(dev, page_keys, 3, keys, keys // page_keys)
    P, E = _attention(alloc, heads, kv_heads, dev, fp8, W, ke=ke), _attention(big, heads, kv_heads, dev, fp8, W, ke=ke)
    for A, al in ((P, alloc), (E, big)):
        _randomise(A, 2)
        al.reserve(0, n0 - 1)
        A.admit(0, _Pair(case.K[:, :n0], case.V[:, :n0], dev), 0, n0)
    qkv = torch.zeros((3, (heads + 2 * kv_heads) * HD), dtype=torch.float16, device=dev)
    pos_t = torch.tensor([n0, -1, -1], dtype=torch.int32, device=dev)
    out = torch.zeros((3, heads * HD), dtype=torch.float16, device=dev)
    alloc.reserve(0, n0)
    P.step(qkv, pos_t, keys - 1, out=out)  # warm-up (an all-zero row appended at n0; the first replay appends the real one over it)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        P.step(qkv, pos_t, keys - 1, out=out)
    k = np.arange(case.n)
    squatted = 0
    for p in range(n0, n0 + steps):
        freed = alloc.release_behind(0, p - W + 1)
        for page in freed:  # what came back is overwritten and handed to another slot
            for pool in (P.k_pool, P.v_pool):
                pool[page].fill_(0x7F) if fp8 else pool[page].copy_(torch.full_like(pool[page], float("nan")))
        if freed:
            squatted += len(alloc.reserve(1, (squatted + len(freed)) * page_keys - 1))
        alloc.reserve(0, p)
        big.reserve(0, p)
        alloc.check_invariants()
        qkv[0].copy_(torch.from_numpy(case.qkv_row(row=p, key=p)).to(dev))
        pos_t.copy_(torch.tensor([p, -1, -1], dtype=torch.int32))
        assert P.table_violations(pos_t, keys - 1) == 0
        graph.replay()
        want = E.step(qkv, pos_t, keys - 1)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(want)), f"position {p}: the replay differs from the eager run that kept every page"
        r = ac.error_ratio(out[0].cpu().numpy().reshape(heads, HD), case.reference(row=p, visible=(k >= _lo(p, W)) & (k <= p)))
        assert r <= 1.0, f"position {p}: {r:.3f} of the bound"
    assert squatted >= 3 and alloc.gone[0] >= 3, "no page came back"
    assert len(alloc.pages[0]) <= (W + page_keys - 1) // page_keys + 1


GEN_KEYS, GEN_PAGE, GEN_BATCH, GEN_PAGES, GEN_W, GEN_NEW, GEN_BURST = 256, 16, 3, 15, 32, 150, 8
VOCAB = 4096


class _Model:
    """hidden 512, heads 4 / 1, ffn 1408, two layers, synthetic weights (tests/test_gpu_generate.py's small model on a 256-key table)."""

    def __init__(self, dev, seed=40):
        from tinychatengine_amd.decoder_block import DecoderBlock
        from tinychatengine_amd.linear import Linear_half_int4
        hidden, heads, kv_heads, ffn, layers = 512, 4, 1, 1408, 2
        cos, sin = _tables(GEN_KEYS, seed, dev)
        self.dev = dev
        self.blocks = [DecoderBlock(hidden, heads, ffn, GEN_KEYS, dev, cos, sin, seed=seed + i, kv_heads=kv_heads) for i in range(layers)]
        g = torch.Generator(device=dev).manual_seed(seed + 100)
        self.final_gamma = (1.0 + 0.1 * torch.empty(hidden, device=dev).normal_(0, 1, generator=g)).float()
        self.lm_head = Linear_half_int4.from_float(torch.empty(VOCAB, hidden, device=dev).normal_(0.0, hidden ** -0.5, generator=g)).prepack()
        self.table = torch.empty(VOCAB, hidden, device=dev).normal_(0.0, 1.0, generator=g).half()

    def decoders(self, window, kv_dtype):
        from tinychatengine_amd.paged_kv import PagedBatchedDecoder
        alloc = _allocator(self.dev, GEN_PAGE, GEN_BATCH, GEN_KEYS, GEN_PAGES, seed=6)
        return [PagedBatchedDecoder(b, alloc, kv_dtype=kv_dtype, window=window) for b in self.blocks]


@pytest.fixture(scope="module")
def model(dev):
    return _Model(dev)


@pytest.mark.parametrize("kv_dtype", ["fp16", "fp8_e4m3"])
def test_e_a_windowed_generator_runs_where_full_attention_exhausts_the_pool(dev, model, kv_dtype):
    from tinychatengine_amd.generate import BatchedGenerator, HostDrivenLoop, SamplingParams
    from tinychatengine_amd.paged_kv import PagePoolExhausted
    greedy = SamplingParams(temp=0.0, repeat_penalty=1.0)
    rng = np.random.default_rng(77)
    prompts = [rng.integers(0, VOCAB, n).tolist() for n in (40, 3, 21)]
    adm = [(s, prompts[s], greedy, 0, GEN_NEW) for s in range(GEN_BATCH)]

    # full attention: 3 slots x (prompt + 150 tokens) / 16 keys is far more than 15 pages
    full = BatchedGenerator(model.decoders(None, kv_dtype), model.final_gamma, model.lm_head, model.table, max_new=GEN_NEW)
    full.admit(adm)
    with pytest.raises(PagePoolExhausted):
        for _ in range(GEN_NEW // GEN_BURST + 1):
            full.run(GEN_BURST)
    full.allocator.check_invariants()
    del full

    gen = BatchedGenerator(model.decoders(GEN_W, kv_dtype), model.final_gamma, model.lm_head, model.table, max_new=GEN_NEW)
    host = HostDrivenLoop(model.decoders(GEN_W, kv_dtype), model.final_gamma, model.lm_head, model.table)
    assert all(d.window == GEN_W for d in gen.decoders)
    gen.admit(adm)
    host.admit([(s, prompts[s], GEN_NEW) for s in range(GEN_BATCH)])
    per_slot = (GEN_W + GEN_BURST + GEN_PAGE - 1) // GEN_PAGE + 1
    retired = []
    while len(retired) < GEN_BATCH:
        retired += gen.run(GEN_BURST)
        gen.allocator.check_invariants()
        for s in gen.book.live():
            assert len(gen.allocator.pages[s]) <= per_slot, f"slot {s} holds {len(gen.allocator.pages[s])} pages"
        assert gen.allocator.pages_in_use() <= GEN_BATCH * per_slot  # (a retired slot keeps what it held when it retired, until release())
    for _ in range(GEN_NEW):
        for s in range(GEN_BATCH):  # the host-driven loop never gives anything back by itself
            if host.pos_host[s] >= 0:
                host.allocator.release_behind(s, int(host.pos_host[s]) - GEN_W + 1)
        host.step()
        host.allocator.check_invariants()
    for s in range(GEN_BATCH):
        toks = gen.tokens(s)
        assert len(toks) == GEN_NEW and toks == host.out[s], f"slot {s}: the windowed graph run and the host-driven loop disagree"
    assert gen.embed_violations() == 0
    for s in range(GEN_BATCH):
        gen.release(s)
    assert gen.allocator.pages_in_use() == 0
    gen.allocator.check_invariants()
