"""Attention sinks beside the sliding window (include/tce_matmul.h, "ATTENTION SINKS"): the sink step and prefill, fp16 and e4m3 pages.

    A  sinks + window that never bind ARE today's unwindowed kernels: `out` and every pool byte, no tolerance
    B  compaction: without RoPE, S a multiple of 4 and lo % 4 == 0, the sink step at a binding position equals the EXISTING unwindowed step at position S + W - 1 under
       bound S + W + 2 on a pool that holds keys [0, S) ++ [lo, pos), no tolerance
    C  everywhere else: sink_cases.sink_reference_f64 on the pools read back, within attention_cases.bound -- designed families with RoPE (the sink keys re-rotated
       so that the family's scores are what the row sees; tests/test_sink_host.py shows that ignoring the sinks misses the bound tenfold), a dominant key planted at S
       and at lo - 1 that must weigh nothing, and the prefill (all-binding, none-binding, mixed blocks; every forced form)
    D  canaries: every table word other than word 0 and lo / page_keys .. pos / page_keys, rows S .. page_keys - 1 of word 0's page and rows base2 .. lo - 1 hold NaN
    E  one captured step replayed while release_behind(..., keep_pages=1) gives pages back
    F  the pools after prefill plus 40 sink steps are the unwindowed layer's

Shapes: heads / kv_heads (4, 2) and (8, 8); three rows per launch, one of them inactive; pos_bound 2047."""
import numpy as np
import pytest

import attention_cases as ac
import sink_cases as sc
from test_gpu_window import _Pair, _allocator, _bits, _canary_page, _pools_equal, _qkv, _randomise, _same_pools, _tables

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HD = 128
BOUND = 2047
SHAPES = [(4, 2), (8, 8)]
SW = [(1, 5), (4, 61), (5, 400), (16, 1100), (16, 5), (5, 61), (4, 400), (1, 1100)]  # (S, W): every S and every W of the issue, twice each; 1, 4 and 8 chunk slots
FP8_FAMILIES = tuple(f for f in ac.FAMILIES if f != "ramp_up")  # (the e4m3 grid cannot hold the ramp's half nat per key: tests/test_gpu_attention_adversarial.py)
FP8_STEP = 200.0
FORMS = [2950, 2954, 2958, 2964, 2968, 2704, 2708]  # tests/test_gpu_paged_prefill.py's forcing modes: the rule; 4 / 8 waves x 1 row tile, x 2; pairing forced on


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


def _attention(alloc, heads, kv_heads, dev, fp8=False, window=None, sinks=None, cos=None, sin=None, ke=0, ve=0):
    from tinychatengine_amd.paged_kv import PagedBatchDecodeAttention
    return PagedBatchDecodeAttention(alloc, heads, kv_heads, dev, cos, sin, kv_dtype="fp8_e4m3" if fp8 else "fp16", k_scale_log2=ke, v_scale_log2=ve, window=window,
                                     sinks=sinks)


# =====================================================================================================================================================================
# A  never binding = today's kernels
# =====================================================================================================================================================================
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("heads,kv_heads", SHAPES)
@pytest.mark.parametrize("page_keys", [16, 64])
def test_a_a_sink_step_that_never_binds_is_todays_step(dev, heads, kv_heads, page_keys, fp8):
    for bound in (63, 1023):
        keys = (bound // page_keys + 1) * page_keys
        cos, sin = _tables(keys, bound, dev)
        for S, W in ((4, bound - 3), (1, bound), (16, 2 ** 30), (5, bound + 1)):  # S + W >= bound + 1
            alloc = _allocator(dev, page_keys, 3, keys, 3 * (keys // page_keys) + 2, seed=bound)
            P0 = _attention(alloc, heads, kv_heads, dev, fp8, None, None, cos, sin, ke=1, ve=-1)
            Ps = _attention(alloc, heads, kv_heads, dev, fp8, W, S, cos, sin, ke=1, ve=-1)
            _randomise(P0, bound + page_keys)
            _same_pools(Ps, P0)
            pos = np.array([bound, -1, bound * 2 // 3], np.int32)
            for b, p in enumerate(pos.tolist()):
                if p >= 0:
                    alloc.reserve(b, p)
            pos_t = torch.from_numpy(pos).to(dev)
            qkv = _qkv(dev, 3, heads, kv_heads, bound + W % 7)
            assert Ps.table_violations(pos_t, bound) == 0
            want, got = P0.step(qkv, pos_t, bound), Ps.step(qkv, pos_t, bound)
            torch.cuda.synchronize()
            what = f"bound={bound} S={S} W={W}"
            assert torch.equal(_bits(got), _bits(want)), f"{what}: outputs differ"
            assert _pools_equal(Ps, P0), f"{what}: a pool byte differs"
            assert not got[1].any()


SEGMENT_SETS = [[(1, 100, 130)], [(0, 3, 65), (2, 0, 5)], [(3, 0, 64), (0, 100, 1), (4, 3, 130), (1, 0, 5), (2, 100, 65)]]  # (slot, cached keys, new rows)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("heads,kv_heads,page_keys", [(4, 2, 16), (8, 8, 64)])
def test_a_a_sink_prefill_that_never_binds_is_todays_prefill(dev, heads, kv_heads, page_keys, fp8):
    keys, batch = 256, 5
    cos, sin = _tables(keys, 3, dev)
    for segments in SEGMENT_SETS:
        top = max(pos + m for _, pos, m in segments)
        for S, W in ((4, top - 4), (16, top), (1, 2 ** 30)):  # S + W >= pos + m of every segment
            alloc = _allocator(dev, page_keys, batch, keys, batch * (keys // page_keys), seed=top)
            P0 = _attention(alloc, heads, kv_heads, dev, fp8, None, None, cos, sin, ke=1, ve=0)
            Ps = _attention(alloc, heads, kv_heads, dev, fp8, W, S, cos, sin, ke=1, ve=0)
            _randomise(P0, top + S)
            _same_pools(Ps, P0)
            for slot, pos, m in segments:
                alloc.reserve(slot, pos + m - 1)
            qkv = _qkv(dev, sum(m for _, _, m in segments), heads, kv_heads, top)
            want, got = P0.prefill(segments, qkv), Ps.prefill(segments, qkv)
            torch.cuda.synchronize()
            assert torch.equal(_bits(got), _bits(want)), f"{segments} S={S} W={W}: outputs differ"
            assert _pools_equal(Ps, P0), f"{segments} S={S} W={W}: a pool byte differs"


# =====================================================================================================================================================================
# B  compaction
# =====================================================================================================================================================================
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("heads,kv_heads", SHAPES)
@pytest.mark.parametrize("page_keys", [16, 64])
def test_b_the_sink_step_equals_the_existing_step_on_the_compacted_cache(dev, heads, kv_heads, page_keys, fp8):
    from tinychatengine_amd import capi
    keys = BOUND + 1
    for S in (4, 16):
        for W in (5, 61, 317, 400, 1100):
            for lo in (S + 4, 4 * ((S + 70) // 4), 4 * ((BOUND - W + 1) // 4)):  # lo % 4 == 0, lo > S: just behind the sinks, a page or more out, far out
                pos = lo + W - 1
                if pos > BOUND:
                    continue
                n = S + W  # the compacted cache's keys; the row sits at its last, S + W - 1
                cut = capi.describe_attention_paged_sink(3, heads, kv_heads, BOUND, page_keys, W, S)
                assert cut == capi.describe_attention_paged(3, heads, kv_heads, n + 2, page_keys), "the two launches are not cut alike"
                alloc = _allocator(dev, page_keys, 3, keys, 2 * (pos // page_keys + 1) + 2, seed=W + lo)
                small = _allocator(dev, page_keys, 3, (n + 2 + page_keys) // page_keys * page_keys, 2 * ((n + 2) // page_keys + 1) + 2, seed=W)
                P, Q = _attention(alloc, heads, kv_heads, dev, fp8, W, S, ke=1, ve=-1), _attention(small, heads, kv_heads, dev, fp8, None, None, ke=1, ve=-1)
                _randomise(P, W + lo)
                _randomise(Q, W + lo + 1)
                g = torch.Generator(device=dev).manual_seed(lo)
                lin = _Pair(np.zeros((kv_heads, 1, HD), np.float16), np.zeros((kv_heads, 1, HD), np.float16), dev)
                lin.k_cache = (torch.randn((kv_heads, pos, HD), generator=g, device=dev) * 0.7).half()
                lin.v_cache = (torch.randn((kv_heads, pos, HD), generator=g, device=dev) * 0.7).half()
                com = _Pair(np.zeros((kv_heads, 1, HD), np.float16), np.zeros((kv_heads, 1, HD), np.float16), dev)
                com.k_cache = torch.cat([lin.k_cache[:, :S], lin.k_cache[:, lo:pos]], dim=1).contiguous()
                com.v_cache = torch.cat([lin.v_cache[:, :S], lin.v_cache[:, lo:pos]], dim=1).contiguous()
                for b in (0, 2):
                    alloc.reserve(b, pos)
                    small.reserve(b, n - 1)
                    P.admit(b, lin, 0, pos)
                    Q.admit(b, com, 0, n - 1)
                qkv = _qkv(dev, 3, heads, kv_heads, lo + W)
                pos_s, pos_q = torch.tensor([pos, -1, pos], dtype=torch.int32, device=dev), torch.tensor([n - 1, -1, n - 1], dtype=torch.int32, device=dev)
                assert P.table_violations(pos_s, BOUND) == 0
                got, want = P.step(qkv, pos_s, BOUND), Q.step(qkv, pos_q, n + 2)
                torch.cuda.synchronize()
                what = f"S={S} W={W} lo={lo}"
                assert torch.equal(_bits(got), _bits(want)), f"{what}: outputs differ"
                for b in (0, 2):  # the appended rows: key pos of the sink launch, key n - 1 of the compacted one
                    for pool_p, pool_q in ((P.k_pool, Q.k_pool), (P.v_pool, Q.v_pool)):
                        rp = pool_p[alloc.pages[b][pos // page_keys], :, pos % page_keys]
                        rq = pool_q[small.pages[b][(n - 1) // page_keys], :, (n - 1) % page_keys]
                        assert torch.equal(_bits(rp), _bits(rq)), f"{what}: the appended rows differ"


# =====================================================================================================================================================================
# C  float64
# =====================================================================================================================================================================
def _positions(S, W):
    """S + W - 1 (the last row that does not bind), S + W, and four consecutive positions further out: every lo mod 4, with and without a page edge between lo and pos"""
    far = min(BOUND - 3, S + W + 2 * 64 + 1)
    return [S + W - 1, S + W, far, far + 1, far + 2, far + 3]


def _make(family, heads, kv_heads, p, W, S, cos, sin, seed, fp8, ke=None):
    def mk(sd):
        if not fp8:
            return sc.compact_case(family, heads, kv_heads, p, W, S, cos, sin, sd)
        return sc.compact_case(family, heads, kv_heads, p, W, S, cos, sin, sd, e4m3=True, ke=ke, ve=-8 if family == "subnormal_v" else 0, step=FP8_STEP)
    for attempt in range(8):  # (make_case's own guard on a draw: tests/test_gpu_window.py's _seeded)
        try:
            return mk(seed + 1000 * attempt)
        except AssertionError as e:
            if "a designed key reaches" not in str(e) or attempt == 7:
                raise


def _step_cases(dev, heads, kv_heads, page_keys, fp8, W, S, cases, cos_t, sin_t, cos, sin):
    """One sink launch for two cases (rows 0 and 2; row 1 inactive): keys 0 .. pos - 1 scattered into pages, the own row in q/k/v.  Returns the error ratios against
    sink_reference_f64 on the pools READ BACK (e4m3: dequantised)."""
    pos = [c.p for c in cases]
    alloc = _allocator(dev, page_keys, 3, BOUND + 1, sum(p // page_keys + 1 for p in pos) + 2, seed=W + pos[0])
    ke, ve = (cases[0].case.ke, cases[0].case.ve) if fp8 else (0, 0)
    P = _attention(alloc, heads, kv_heads, dev, fp8, W, S, cos_t, sin_t, ke=ke, ve=ve)
    _randomise(P, W + pos[1])
    qkv = torch.zeros((3, (heads + 2 * kv_heads) * HD), dtype=torch.float16, device=dev)
    for b, c in zip((0, 2), cases):
        alloc.reserve(b, c.p)
        if c.p:
            P.admit(b, _Pair(c.K[:, :c.p], c.V[:, :c.p], dev), 0, c.p)
        qkv[b].copy_(torch.from_numpy(c.qkv_row()).to(dev))
    pos_t = torch.tensor([pos[0], -1, pos[1]], dtype=torch.int32, device=dev)
    assert P.table_violations(pos_t, BOUND) == 0
    out = P.step(qkv, pos_t, BOUND)
    torch.cuda.synchronize()
    assert not out[1].any()
    ratios = []
    for b, c in zip((0, 2), cases):
        K, V = (t.cpu().numpy() for t in P.read_back(b, c.p + 1))
        ratios.append(ac.error_ratio(out[b].cpu().numpy().reshape(heads, HD), c.reference(cos, sin, K, V)))
    return ratios


def _step_against_float64(dev, family, heads, kv_heads, page_keys, fp8):
    cos, sin = ac.rope_tables(BOUND + 1, 11)
    cos_t, sin_t = torch.from_numpy(cos).to(dev), torch.from_numpy(sin).to(dev)
    worst = 0.0
    for S, W in SW:
        ps = _positions(S, W)
        if fp8 and family in ("stairs_up", "stairs_down") and S + W > 512:
            continue  # (the generator's limit on the e4m3 grid, not the kernel's: tests/test_gpu_window.py)
        for i in range(0, len(ps), 2):
            cases = [_make(family, heads, kv_heads, p, W, S, cos, sin, 7 * W + S + i + j, fp8) for j, p in enumerate(ps[i:i + 2])]
            if fp8 and cases[0].case.ke != cases[1].case.ke:  # one exponent per launch
                ke = max(c.case.ke for c in cases)
                cases = [c if c.case.ke == ke else _make(family, heads, kv_heads, c.p, W, S, cos, sin, 7 * W + S + i + j, True, ke) for j, c in enumerate(cases)]
            for c, r in zip(cases, _step_cases(dev, heads, kv_heads, page_keys, fp8, W, S, cases, cos_t, sin_t, cos, sin)):
                worst = max(worst, r)
                assert r <= 1.0, f"{family} S={S} W={W} pos={c.p} planted={c.planted}: {r:.3f} of the bound"
    print(f"{family} {heads}/{kv_heads} page_keys={page_keys} fp8={fp8}: worst {worst:.3f} of the bound")


@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("heads,kv_heads,page_keys", [(4, 2, 16), (8, 8, 64)])
def test_c_sink_step_against_float64(dev, family, heads, kv_heads, page_keys):
    _step_against_float64(dev, family, heads, kv_heads, page_keys, False)


@pytest.mark.parametrize("family", FP8_FAMILIES)
@pytest.mark.parametrize("heads,kv_heads,page_keys", [(4, 2, 64), (8, 8, 16)])
def test_c_sink_step_against_float64_e4m3(dev, family, heads, kv_heads, page_keys):
    _step_against_float64(dev, family, heads, kv_heads, page_keys, True)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("heads,kv_heads,page_keys", [(4, 2, 16), (8, 8, 64)])
def test_c_dominant_keys_at_the_four_edges(dev, heads, kv_heads, page_keys, fp8):
    """`sink_own` with its peak moved: 30 nats above every other weighed key at S - 1 and at lo (must dominate: the output is that key's value row), beside
    compact_case's 60-nat plants at S and lo - 1 (must weigh nothing: they would dominate)."""
    cos, sin = ac.rope_tables(BOUND + 1, 12)
    cos_t, sin_t = torch.from_numpy(cos).to(dev), torch.from_numpy(sin).to(dev)
    for S, W in SW:
        for p in (S + W + 5, min(BOUND, S + W + 777)):
            lo = p - W + 1
            cases = []
            for j, own in enumerate((S - 1, S)):  # the family's key S - 1 is the last sink, its key S is pool key lo
                for attempt in range(8):
                    try:
                        kw = dict(e4m3=True, ke=3) if fp8 else {}
                        cases.append(sc.compact_case("sink_own", heads, kv_heads, p, W, S, cos, sin, 3 * W + p + j + 1000 * attempt, own=own, **kw))
                        break
                    except AssertionError as e:
                        if "a designed key reaches" not in str(e) or attempt == 7:
                            raise
            assert all(c.planted == sorted({S, lo - 1}) for c in cases)
            ratios = _step_cases(dev, heads, kv_heads, page_keys, fp8, W, S, cases, cos_t, sin_t, cos, sin)
            assert max(ratios) <= 1.0, f"S={S} W={W} pos={p}: {ratios} of the bound"
            for c, key in zip(cases, (S - 1, lo)):  # and the reference itself says that the designed key dominates, on the heads that look along the pilot
                up = c.case.a[0] > 0
                _, Vr = c.repeated()
                assert np.abs(c.reference(cos, sin) - Vr[:, key].astype(np.float64))[up].max() < 0.05, f"S={S} W={W} pos={p}: key {key} does not dominate the reference"


def _prefill_launch(dev, heads, kv_heads, page_keys, fp8, W, S, segments, seed):
    """One sink prefill of Gaussian rows on Gaussian cached keys whose first S + 3 rows are three times as long (the sinks carry weight; rows S .. S + 2 would, if a
    binding row weighed them); every row against sink_reference_f64 on the pools read back, the appended rows against the unwindowed prefill's bit for bit."""
    keys, batch = 512, 5
    cos, sin = ac.rope_tables(keys, seed)
    cos_t, sin_t = torch.from_numpy(cos).to(dev), torch.from_numpy(sin).to(dev)
    alloc = _allocator(dev, page_keys, batch, keys, batch * (keys // page_keys), seed=seed)
    Ps, P0 = _attention(alloc, heads, kv_heads, dev, fp8, W, S, cos_t, sin_t, ke=2, ve=0), _attention(alloc, heads, kv_heads, dev, fp8, None, None, cos_t, sin_t, ke=2, ve=0)
    _randomise(Ps, seed)
    rng = np.random.default_rng(seed)
    total = sum(m for _, _, m in segments)
    qkv_h = (rng.standard_normal((total, (heads + 2 * kv_heads) * HD)) * 0.9).astype(np.float16)
    r0 = 0
    for slot, pos, m in segments:
        alloc.reserve(slot, pos + m - 1)
        K, V = (rng.standard_normal((kv_heads, max(pos, 1), HD)) * 0.7).astype(np.float16), (rng.standard_normal((kv_heads, max(pos, 1), HD)) * 0.8).astype(np.float16)
        K[:, :S + 3] *= 3
        if pos:
            Ps.admit(slot, _Pair(K[:, :pos], V[:, :pos], dev), 0, pos)
        for i in range(m):  # the new rows' keys among the first S + 3: as long as the cached ones
            if pos + i < S + 3:
                qkv_h[r0 + i, heads * HD:(heads + kv_heads) * HD] *= 3
        r0 += m
    _same_pools(P0, Ps)
    qkv = torch.from_numpy(qkv_h).to(dev)
    out = Ps.prefill(segments, qkv)
    P0.prefill(segments, qkv)
    torch.cuda.synchronize()
    assert _pools_equal(Ps, P0), f"{segments} S={S} W={W}: the sink prefill appended other rows than the unwindowed one"
    got, r0, worst, bound_rows = out.cpu().numpy(), 0, 0.0, 0
    for slot, pos, m in segments:
        K, V = (t.cpu().numpy() for t in Ps.read_back(slot, pos + m))
        Kr, Vr = np.repeat(K, heads // kv_heads, axis=0), np.repeat(V, heads // kv_heads, axis=0)
        for i in range(m):
            p = pos + i
            ref = sc.sink_reference_f64(qkv_h[r0 + i, :heads * HD].reshape(heads, HD), cos, sin, Kr, Vr, p, W, S)
            r = ac.error_ratio(got[r0 + i].reshape(heads, HD), ref)
            worst = max(worst, r)
            bound_rows += sc.binds(p, W, S)
            assert r <= 1.0, f"S={S} W={W} segment (slot {slot}, pos {pos}, m {m}) row {i} (binds: {sc.binds(p, W, S)}): {r:.3f} of the bound"
        r0 += m
    return worst, bound_rows


@pytest.mark.parametrize("mode", FORMS)
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("heads,kv_heads,page_keys", [(4, 2, 16), (8, 8, 64)])
def test_c_sink_prefill_against_float64(dev, heads, kv_heads, page_keys, fp8, mode):
    from tinychatengine_amd import capi
    L = capi.lib()
    capi.check(L.tce_w4a16_set_debug_mode(mode))
    try:
        worst, nbound = 0.0, 0
        for S, W in ((4, 61), (5, 5), (16, 17), (1, 100)) if mode == 2950 else ((4, 61), (16, 17)):  # (a forced form: half the launches)
            n = S + W
            # lone segments: all rows bind; none binds; mixed inside one block; a row count of 1, 17 and 130; then 2 and 5 ragged segments around the threshold
            sets = [[(0, n + 40, 130)], [(1, 0, min(n, 130))], [(2, n - 9, 17)], [(3, n, 1)], [(4, n - 1, 1)], [(0, max(n - 100, 0), 130)],
                    [(0, n - 3, 65), (2, 0, 5)], [(3, 0, 64), (0, n + 30, 1), (4, n - 60 if n > 60 else 0, 130), (1, 0, 5), (2, n + 64, 17)]]
            for i, segments in enumerate(sets if mode == 2950 else sets[0:8:2] + sets[7:]):
                w, nb = _prefill_launch(dev, heads, kv_heads, page_keys, fp8, W, S, segments, 100 * S + W + i)
                worst, nbound = max(worst, w), nbound + nb
        assert nbound > 300
        print(f"prefill {heads}/{kv_heads} page_keys={page_keys} fp8={fp8} mode={mode}: worst {worst:.3f} of the bound, {nbound} binding rows")
    finally:
        capi.check(L.tce_w4a16_set_debug_mode(2950))


# =====================================================================================================================================================================
# D  canaries
# =====================================================================================================================================================================
def _nan_rows(P, page, r0, r1, fp8):
    for pool in (P.k_pool, P.v_pool):
        if r1 > r0:
            pool[page, :, r0:r1].fill_(0x7F) if fp8 else pool[page, :, r0:r1].copy_(torch.full_like(pool[page, :, r0:r1], float("nan")))


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("heads,kv_heads,page_keys", [(4, 2, 16), (8, 8, 64)])
def test_d_a_binding_row_touches_nothing_but_its_sinks_and_its_window(dev, heads, kv_heads, page_keys, fp8):
    keys = BOUND + 1
    cos, sin = _tables(keys, 8, dev)
    for S, W in SW:
        for pos in ([S + W + 3 * page_keys + 2, 2 * (S + W) + 5 * page_keys + 1], [BOUND, S + W + page_keys + 3]):
            pos = [min(p, BOUND) for p in pos]
            alloc = _allocator(dev, page_keys, 3, keys, sum(p // page_keys + 1 for p in pos) + 3, seed=W)
            P, Q = _attention(alloc, heads, kv_heads, dev, fp8, W, S, cos, sin), _attention(alloc, heads, kv_heads, dev, fp8, W, S, cos, sin)
            _randomise(P, W + pos[0])
            for b, p in zip((0, 2), pos):
                alloc.reserve(b, p)
            canary = _canary_page(alloc, (P.k_pool, P.v_pool), dev)
            _same_pools(Q, P)
            pos_t = torch.tensor([pos[0], -1, pos[1]], dtype=torch.int32, device=dev)
            qkv = _qkv(dev, 3, heads, kv_heads, W)
            assert Q.table_violations(pos_t, BOUND) == 0
            clean = Q.step(qkv, pos_t, BOUND)  # the table and the pools as they were
            good = alloc.table.clone()
            t = torch.full_like(alloc.table, canary)
            for b, p in zip((0, 2), pos):
                lo = p - W + 1
                assert p >= S + W
                t[b, 0] = good[b, 0]
                t[b, lo // page_keys:p // page_keys + 1] = good[b, lo // page_keys:p // page_keys + 1]
                # rows S .. page_keys - 1 of word 0's page (unless the window reaches into it), and rows base2 .. lo - 1
                first = int(good[b, 0])
                _nan_rows(P, first, S, min(page_keys, lo) if lo // page_keys == 0 else page_keys, fp8)
                if lo // page_keys > 0:
                    _nan_rows(P, int(good[b, lo // page_keys]), (lo & ~3) % page_keys, lo % page_keys, fp8)
            alloc.table.copy_(t)
            assert P.table_violations(pos_t, BOUND) == 0
            got = P.step(qkv, pos_t, BOUND)
            torch.cuda.synchronize()
            what = f"S={S} W={W} pos={pos}"
            assert torch.isfinite(got.float()).all(), f"{what}: a canary leaked into an output"
            assert torch.equal(_bits(got), _bits(clean)), f"{what}: outputs differ from the clean run"
            for b, p in zip((0, 2), pos):  # the appended rows are the clean run's (the NaN rows planted above are this run's alone)
                page = int(good[b, p // page_keys])
                assert torch.equal(_bits(P.k_pool[page, :, p % page_keys]), _bits(Q.k_pool[page, :, p % page_keys]))
                assert torch.equal(_bits(P.v_pool[page, :, p % page_keys]), _bits(Q.v_pool[page, :, p % page_keys]))
            bad = t.clone()
            bad[0, 0] = alloc.num_pages
            alloc.table.copy_(bad)
            assert P.table_violations(pos_t, BOUND) == 1, f"{what}: a bad word 0 was not counted"
            bad[2, pos[1] // page_keys] = -1
            alloc.table.copy_(bad)
            assert P.table_violations(pos_t, BOUND) == 2
            alloc.table.copy_(good)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("heads,kv_heads,page_keys", [(4, 2, 16), (8, 8, 64)])
def test_d_the_prefill_follows_word_0_and_the_words_of_its_window(dev, heads, kv_heads, page_keys, fp8):
    keys, batch = 512, 5
    cos, sin = _tables(keys, 9, dev)
    for S, W in ((4, 61), (16, 17), (1, 100)):
        n = S + W
        for segments in ([(1, n + 3 * page_keys + 40, 130)], [(0, n + 2 * page_keys, 65), (2, n + 5 * page_keys + 3, 17)]):
            alloc = _allocator(dev, page_keys, batch, keys, batch * (keys // page_keys), seed=W)
            P, Q = _attention(alloc, heads, kv_heads, dev, fp8, W, S, cos, sin, ke=1), _attention(alloc, heads, kv_heads, dev, fp8, W, S, cos, sin, ke=1)
            _randomise(P, W)
            for slot, pos, m in segments:
                alloc.reserve(slot, pos + m - 1)
            canary = _canary_page(alloc, (P.k_pool, P.v_pool), dev)
            _same_pools(Q, P)
            qkv = _qkv(dev, sum(m for _, _, m in segments), heads, kv_heads, W)
            clean = Q.prefill(segments, qkv)
            good = alloc.table.clone()
            t = torch.full_like(alloc.table, canary)
            for slot, pos, m in segments:  # every row binds: word 0, and from the first row's lo to the last row's own key
                lo = pos - W + 1
                t[slot, 0] = good[slot, 0]
                t[slot, lo // page_keys:(pos + m - 1) // page_keys + 1] = good[slot, lo // page_keys:(pos + m - 1) // page_keys + 1]
                _nan_rows(P, int(good[slot, 0]), S, page_keys, fp8)
            alloc.table.copy_(t)
            got = P.prefill(segments, qkv)
            torch.cuda.synchronize()
            alloc.table.copy_(good)
            what = f"S={S} W={W} segments={segments}"
            assert torch.isfinite(got.float()).all(), f"{what}: a canary leaked into an output"
            assert torch.equal(_bits(got), _bits(clean)), f"{what}: outputs differ from the clean run"


# =====================================================================================================================================================================
# E  life cycle
# =====================================================================================================================================================================
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("heads,kv_heads,page_keys", [(4, 2, 16), (8, 8, 64)])
def test_e_one_captured_sink_step_replayed_while_pages_come_back(dev, heads, kv_heads, page_keys, fp8):
    """The graph holds one sink step; between replays the host gives the pages between the sinks' page and the window back (release_behind(..., keep_pages=1)), fills
    them with NaN and hands them to another slot.  The eager twin keeps every page.  Same outputs, bit for bit."""
    S, W, keys = 4, page_keys + 3, 512
    n0, steps = 2 * page_keys + 1, 3 * page_keys + 5
    cos, sin = _tables(keys, 21, dev)
    alloc = _allocator(dev, page_keys, 3, keys, 9, seed=1)  # 9 pages: the sequence alone would need 6 by the end, the squatter takes what comes back
    big = _allocator(dev, page_keys, 3, keys, keys // page_keys)
    P, E = _attention(alloc, heads, kv_heads, dev, fp8, W, S, cos, sin, ke=1), _attention(big, heads, kv_heads, dev, fp8, W, S, cos, sin, ke=1)
    g = torch.Generator(device=dev).manual_seed(5)
    lin = _Pair(np.zeros((kv_heads, 1, HD), np.float16), np.zeros((kv_heads, 1, HD), np.float16), dev)
    lin.k_cache = (torch.randn((kv_heads, n0, HD), generator=g, device=dev) * 0.7).half()
    lin.v_cache = (torch.randn((kv_heads, n0, HD), generator=g, device=dev) * 0.7).half()
    lin.k_cache[:, :S] *= 3  # (the sinks carry weight)
    for A, al in ((P, alloc), (E, big)):
        _randomise(A, 2)
        al.reserve(0, n0 - 1)
        A.admit(0, lin, 0, n0)
    rows = _qkv(dev, steps + 1, heads, kv_heads, 9)
    qkv = torch.zeros((3, (heads + 2 * kv_heads) * HD), dtype=torch.float16, device=dev)
    pos_t = torch.tensor([n0, -1, -1], dtype=torch.int32, device=dev)
    out = torch.zeros((3, heads * HD), dtype=torch.float16, device=dev)
    alloc.reserve(0, n0)
    P.step(qkv, pos_t, keys - 1, out=out)  # warm-up (an all-zero row appended at n0; the first replay appends the real one over it)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        P.step(qkv, pos_t, keys - 1, out=out)
    squatted = 0
    for i, p in enumerate(range(n0, n0 + steps)):
        freed = alloc.release_behind(0, p - W + 1, keep_pages=1)
        for page in freed:  # what came back is overwritten and handed to another slot
            for pool in (P.k_pool, P.v_pool):
                pool[page].fill_(0x7F) if fp8 else pool[page].copy_(torch.full_like(pool[page], float("nan")))
        if freed:
            squatted += len(alloc.reserve(1, (squatted + len(freed)) * page_keys - 1))
        alloc.reserve(0, p)
        big.reserve(0, p)
        alloc.check_invariants()
        qkv[0].copy_(rows[i])
        pos_t.copy_(torch.tensor([p, -1, -1], dtype=torch.int32))
        assert P.table_violations(pos_t, keys - 1) == 0
        graph.replay()
        want = E.step(qkv, pos_t, keys - 1)
        torch.cuda.synchronize()
        assert torch.isfinite(out.float()).all(), f"position {p}: a freed page was read"
        assert torch.equal(_bits(out), _bits(want)), f"position {p}: the replay differs from the eager run that kept every page"
    assert squatted >= 2 and alloc.gone[0] >= 3 and len(alloc.kept[0]) == 1, "no page came back"
    assert len(alloc.kept[0]) + len(alloc.pages[0]) <= (W + page_keys - 1) // page_keys + 2
    # and the last row is the definition's
    K, V = (t.cpu().numpy() for t in E.read_back(0, p + 1))
    ref = sc.sink_reference_f64(rows[steps - 1, :heads * HD].cpu().numpy().reshape(heads, HD), cos.cpu().numpy(), sin.cpu().numpy(), np.repeat(K, heads // kv_heads, axis=0),
                                np.repeat(V, heads // kv_heads, axis=0), p, W, S)
    assert ac.error_ratio(out[0].cpu().numpy().reshape(heads, HD), ref) <= 1.0


# =====================================================================================================================================================================
# F  the pools do not know about sinks
# =====================================================================================================================================================================
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("heads,kv_heads,page_keys", [(4, 2, 16), (8, 8, 64)])
def test_f_the_pools_after_prefill_and_sink_steps_are_the_unwindowed_layers(dev, heads, kv_heads, page_keys, fp8):
    S, W, m, steps, keys = 5, 17, 65, 40, 256
    cos, sin = _tables(keys, 4, dev)
    alloc = _allocator(dev, page_keys, 3, keys, 3 * (keys // page_keys), seed=4)
    Ps, P0 = _attention(alloc, heads, kv_heads, dev, fp8, W, S, cos, sin, ke=1), _attention(alloc, heads, kv_heads, dev, fp8, None, None, cos, sin, ke=1)
    _randomise(Ps, 3)
    _same_pools(P0, Ps)
    alloc.reserve(2, m + steps - 1)
    alloc.reserve(0, steps + 2)
    rows = _qkv(dev, m + 2 + 3 * steps, heads, kv_heads, 12)
    segments = [(2, 0, m), (0, 0, 2)]
    Ps.prefill(segments, rows[:m + 2])
    P0.prefill(segments, rows[:m + 2])
    for i in range(steps):
        pos_t = torch.tensor([2 + i, -1, m + i], dtype=torch.int32, device=dev)
        qkv = rows[m + 2 + 3 * i:m + 5 + 3 * i].contiguous()
        Ps.step(qkv, pos_t, keys - 1)
        P0.step(qkv, pos_t, keys - 1)
    torch.cuda.synchronize()
    assert _pools_equal(Ps, P0), "a pool byte depends on window or sinks"
