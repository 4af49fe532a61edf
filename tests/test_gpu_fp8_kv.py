"""The e4m3 paged KV cache on the GPU (include/tce_matmul.h, "FP8 pages"): conversions, the paged step, the paged prefill, fork, generation.

The contract is stated without a tolerance wherever the format allows it: dequant(byte, e) is exact in binary16 and every arithmetic instruction behind the
conversion is the fp16 kernels', so on pools whose fp16 image holds dequant(byte) the fp8 and the fp16 entry points agree bit for bit; what is appended is
quant(row) byte for byte (paged_kv.fp8_quantize_reference, held to the format's definition for every input by tests/test_fp8_kv_host.py).  Only the cases with RoPE
and off-grid rows carry a bound -- the project's own for these kernels (tests/test_gpu_attention.py) against float64 on the DEQUANTISED pool contents read back
after the launch.  Every paged launch is preceded by tce_kv_block_table_check, and every table word a launch must not follow names an in-range page full of 0x7f
bytes (NaN): a wrong kernel fails an assertion, not an address."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HD = 128
FP8 = "fp8_e4m3"
SCALES = [(0, 0), (3, -4)]


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available()
    capi.lib()
    return torch.device("cuda:0")


def _q(x, e):
    from tinychatengine_amd.paged_kv import fp8_quantize_reference
    return fp8_quantize_reference(x, e)


def _dq(b, e):
    from tinychatengine_amd.paged_kv import fp8_dequantize_reference
    return fp8_dequantize_reference(b, e)


def _tables(n, seed, dev):
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, (n, HD // 2))
    cos = np.concatenate([np.cos(ang), np.cos(ang)], axis=1).astype(np.float16)
    sin = np.concatenate([np.sin(ang), np.sin(ang)], axis=1).astype(np.float16)
    return torch.from_numpy(cos).to(dev), torch.from_numpy(sin).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _finite_bytes(rng, shape):
    """Random e4m3 bytes without the two NaN encodings."""
    b = rng.integers(0, 256, shape, dtype=np.uint8)
    b[(b & 0x7F) == 0x7F] = 0x3C
    return b


def _gaussian_bytes(rng, shape, e):
    """Bytes whose dequantised values are Gaussian, sigma 0.8, whatever the exponent: the data the project's float64 bound was stated for."""
    return _q((rng.standard_normal(shape) * 0.8).astype(np.float16), e)


def _on_grid(x_f16, e):
    return _dq(_q(x_f16, e), e)


# ---- 1: the conversions, exhaustively ----
def _copy_call(fn, first, second, row, stride, page_keys, num_pages, kv_heads, lin_keys, key0, nkeys, ke, ve):
    from tinychatengine_amd import capi
    from tinychatengine_amd.linear import _stream
    p = lambda t: C.c_void_p(t.data_ptr())
    capi.check(fn(p(first[0]), p(first[1]), p(second[0]), p(second[1]), p(row), stride, page_keys, num_pages, kv_heads, HD, lin_keys, key0, nkeys, ke, ve, C.c_void_p(_stream())))


@pytest.mark.parametrize("e", [-8, -3, 0, 4, 7])
def test_scatter_quantises_every_binary16_pattern(dev, e):
    """A contiguous pair [1][512][128] holding all 65536 bit patterns (K ascending, V descending) into 32 pages of 16 keys through a permuted table row; rows 3 ..
    508 only: the pool rows of keys 0 .. 2 and 509 .. 511 and every page the row does not name keep their background."""
    from tinychatengine_amd import capi
    allh = np.arange(65536, dtype=np.uint16)
    k_lin = torch.from_numpy(allh.view(np.float16).reshape(1, 512, HD).copy()).to(dev)
    v_lin = torch.from_numpy(allh[::-1].copy().view(np.float16).reshape(1, 512, HD)).to(dev)
    num_pages, pk = 40, 16
    perm = np.random.default_rng(e + 100).permutation(num_pages)[:32].astype(np.int32)
    row = torch.from_numpy(perm).to(dev)
    k_pool = torch.full((num_pages, 1, pk, HD), 0x5A, dtype=torch.uint8, device=dev)
    v_pool = torch.full_like(k_pool, 0xA5)
    _copy_call(capi.lib().tce_kv_pages_scatter_fp8, (k_lin, v_lin), (k_pool, v_pool), row, 32, pk, num_pages, 1, 512, 3, 506, e, e - 1 if e > -8 else 7)
    torch.cuda.synchronize()
    ve = e - 1 if e > -8 else 7
    for lin, pool, ex, bg in ((k_lin, k_pool, e, 0x5A), (v_lin, v_pool, ve, 0xA5)):
        src = lin.cpu().numpy().reshape(512, HD)
        want = np.full((num_pages, pk, HD), bg, np.uint8)
        ref = _q(src, ex)
        for key in range(3, 509):
            want[perm[key // pk], key % pk] = ref[key]
        got = pool.cpu().numpy().reshape(num_pages, pk, HD)
        nan_in = np.zeros((num_pages, pk, HD), bool)
        for key in range(3, 509):
            nan_in[perm[key // pk], key % pk] = np.isnan(src[key])
        assert ((got[nan_in] & 0x7F) == 0x7F).all(), f"e={ex}: a NaN input did not give a NaN byte"
        bad = (got != want) & ~nan_in
        assert not bad.any(), f"e={ex}: {int(bad.sum())} bytes differ from quant(); first at {np.argwhere(bad)[0].tolist()}: got {got[bad][0]:#x}, want {want[bad][0]:#x}"


@pytest.mark.parametrize("e", list(range(-8, 8)))
def test_gather_dequantises_every_byte_exactly(dev, e):
    """Pages holding every byte value (K: byte = element index mod 256; V: the complement) gathered through a permuted table row into a contiguous fp16 pair
    [2][64][128] with a background pattern; rows 5 .. 58 only."""
    from tinychatengine_amd import capi
    num_pages, pk, kvh = 7, 16, 2
    base = (np.arange(num_pages * kvh * pk * HD) % 256).astype(np.uint8).reshape(num_pages, kvh, pk, HD)
    k_pool, v_pool = torch.from_numpy(base.copy()).to(dev), torch.from_numpy((255 - base).astype(np.uint8)).to(dev)
    perm = np.random.default_rng(e + 50).permutation(num_pages)[:4].astype(np.int32)
    row = torch.from_numpy(perm).to(dev)
    bgbits = 0x1234
    k_lin = torch.full((kvh, 64, HD), bgbits, dtype=torch.int16, device=dev).view(torch.float16)
    v_lin = k_lin.clone()
    ve = -e - 1  # (another exponent of the range for V)
    _copy_call(capi.lib().tce_kv_pages_gather_fp8, (k_pool, v_pool), (k_lin, v_lin), row, 4, pk, num_pages, kvh, 64, 5, 54, e, ve)
    torch.cuda.synchronize()
    for lin, pool, ex in ((k_lin, k_pool, e), (v_lin, v_pool, ve)):
        src = pool.cpu().numpy()
        want = np.full((kvh, 64, HD), bgbits, np.uint16)
        nan_b = np.zeros((kvh, 64, HD), bool)
        for key in range(5, 59):
            bytes_ = src[perm[key // pk], :, key % pk]
            want[:, key] = _dq(bytes_, ex).view(np.uint16)
            nan_b[:, key] = (bytes_ & 0x7F) == 0x7F
        got = lin.cpu().numpy().view(np.uint16)
        assert np.isnan(got.view(np.float16)[nan_b]).all(), f"e={ex}: a NaN byte did not give a NaN"
        bad = (got != want) & ~nan_b
        assert not bad.any(), f"e={ex}: {int(bad.sum())} elements differ from dequant(); first: got {got[bad][0]:#x}, want {want[bad][0]:#x}"
    assert torch.equal(k_pool.cpu(), torch.from_numpy(base)), "gather wrote a pool"


# ---- the decode step ----
POSITIONS = [0, 3, 15, 16, 63, 64, 337, 511]
BOUND = 511


class _StepWorld:
    """B = 3 table rows over fp8 pools and, on the SAME table, fp16 pools holding dequant of the same bytes.  Random finite bytes below each active position (every
    exponent of the format, for the bit comparisons; gaussian=True: quantised Gaussian rows, for the float64 bound), a background byte elsewhere; every table word
    an active row must not follow (and every word of an inactive row) names a canary page of 0x7f bytes."""

    def __init__(self, dev, heads, kv_heads, page_keys, pos, ke, ve, rope, seed, gaussian=False):
        from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchDecodeAttention
        self.dev, self.heads, self.kv_heads, self.pk, self.pos, self.ke, self.ve = dev, heads, kv_heads, page_keys, pos, ke, ve
        rng = np.random.default_rng(seed)
        stride = (BOUND + 1) // page_keys + 1  # a word more than any row needs
        batch = len(pos)
        num_pages = batch * stride + 2
        order = rng.permutation(num_pages).tolist()
        self.alloc = PageAllocator(num_pages, page_keys, batch, stride, dev, free_order=order)
        cos = sin = None
        if rope:
            cos, sin = _tables(stride * page_keys, seed, dev)
        self.P8 = PagedBatchDecodeAttention(self.alloc, heads, kv_heads, dev, cos, sin, kv_dtype=FP8, k_scale_log2=ke, v_scale_log2=ve)
        self.P16 = PagedBatchDecodeAttention(self.alloc, heads, kv_heads, dev, cos, sin)
        kb = np.full((num_pages, kv_heads, page_keys, HD), 0x11, np.uint8)
        vb = np.full_like(kb, 0x91)
        for b, p in enumerate(pos):
            if 0 <= p <= BOUND:
                self.alloc.reserve(b, p)
                for key in range(p):
                    page = self.alloc.pages[b][key // page_keys]
                    kb[page, :, key % page_keys] = _gaussian_bytes(rng, (kv_heads, HD), ke) if gaussian else _finite_bytes(rng, (kv_heads, HD))
                    vb[page, :, key % page_keys] = _gaussian_bytes(rng, (kv_heads, HD), ve) if gaussian else _finite_bytes(rng, (kv_heads, HD))
        self.canary = order[-1]
        assert all(self.canary not in ps for ps in self.alloc.pages)
        kb[self.canary], vb[self.canary] = 0x7F, 0x7F
        table = torch.full_like(self.alloc.table, self.canary)
        for b, ps in enumerate(self.alloc.pages):
            if ps:
                assert len(ps) == pos[b] // page_keys + 1
                table[b, :len(ps)] = torch.tensor(ps, dtype=torch.int32, device=dev)
        self.alloc.table.copy_(table)
        self.kb, self.vb = kb, vb
        self.P8.k_pool.copy_(torch.from_numpy(kb))
        self.P8.v_pool.copy_(torch.from_numpy(vb))
        self.P16.k_pool.copy_(torch.from_numpy(_dq(kb, ke)))
        self.P16.v_pool.copy_(torch.from_numpy(_dq(vb, ve)))
        self.pos_t = torch.tensor(pos, dtype=torch.int32, device=dev)
        self.rng = rng

    def qkv(self, on_grid):
        h, kvh = self.heads, self.kv_heads
        x = (self.rng.standard_normal((len(self.pos), (h + 2 * kvh) * HD)) * 0.9).astype(np.float16)
        if on_grid:
            x[:, h * HD:(h + kvh) * HD] = _on_grid(x[:, h * HD:(h + kvh) * HD], self.ke)
            x[:, (h + kvh) * HD:] = _on_grid(x[:, (h + kvh) * HD:], self.ve)
        return x

    def active(self):
        return [(b, p) for b, p in enumerate(self.pos) if 0 <= p <= BOUND]

    def expect_bytes(self, k_rows, v_rows):
        """The byte pools after a step that appended k_rows / v_rows [batch][kv_heads][128] (uint8) at each active row's position."""
        ek, ev = self.kb.copy(), self.vb.copy()
        for b, p in self.active():
            page = self.alloc.pages[b][p // self.pk]
            ek[page, :, p % self.pk] = k_rows[b]
            ev[page, :, p % self.pk] = v_rows[b]
        return ek, ev


def _position_sets():
    """B = 3 with one row inactive (-1) and one past the bound, the active position running over POSITIONS (the inactive rows change places)."""
    sets = []
    for i, p in enumerate(POSITIONS):
        row = [p, -1, BOUND + 1]
        sets.append(row[i % 3:] + row[:i % 3])
    return sets


@pytest.mark.parametrize("ke,ve", SCALES)
@pytest.mark.parametrize("page_keys", [16, 64])
@pytest.mark.parametrize("heads,kv_heads", [(4, 2), (2, 2)])
def test_step_without_rope_is_bit_identical_to_the_fp16_step_on_dequantised_pools(dev, heads, kv_heads, page_keys, ke, ve):
    for pos in _position_sets() + [[337, 64, 511], [15, 16, 0]]:
        w = _StepWorld(dev, heads, kv_heads, page_keys, pos, ke, ve, rope=False, seed=sum(pos) + page_keys + heads)
        x = w.qkv(on_grid=True)
        qkv = torch.from_numpy(x).to(dev)
        assert w.P8.table_violations(w.pos_t, BOUND) == 0
        out8 = w.P8.step(qkv, w.pos_t, BOUND)
        assert w.P16.table_violations(w.pos_t, BOUND) == 0
        k16_0, v16_0 = w.P16.k_pool.clone(), w.P16.v_pool.clone()
        out16 = w.P16.step(qkv, w.pos_t, BOUND)
        torch.cuda.synchronize()
        what = f"heads={heads}/{kv_heads} page_keys={page_keys} scales=({ke},{ve}) pos={pos}"
        assert not torch.isnan(out8.float()).any(), f"{what}: a canary page leaked into an output"
        assert torch.equal(_bits(out8), _bits(out16)), f"{what}: out differs from the fp16 step on the dequantised pools"
        for b, p in enumerate(pos):
            if not 0 <= p <= BOUND:
                assert not out8[b].any(), f"{what}: inactive row {b} is not zeros"
        # appended bytes = quant of the rows the fp16 step appended; every other byte unchanged
        k16, v16 = w.P16.k_pool.cpu().numpy(), w.P16.v_pool.cpu().numpy()
        k_rows = np.zeros((len(pos), kv_heads, HD), np.uint8)
        v_rows = np.zeros_like(k_rows)
        for b, p in w.active():
            page = w.alloc.pages[b][p // page_keys]
            k_rows[b], v_rows[b] = _q(k16[page, :, p % page_keys], ke), _q(v16[page, :, p % page_keys], ve)
        ek, ev = w.expect_bytes(k_rows, v_rows)
        assert np.array_equal(w.P8.k_pool.cpu().numpy(), ek) and np.array_equal(w.P8.v_pool.cpu().numpy(), ev), f"{what}: the byte pools are not (what they were + quant of the appended rows)"
        # (and the fp16 side appended exactly the on-grid input rows: the comparison above is between equals)
        for b, p in w.active():
            page = w.alloc.pages[b][p // page_keys]
            assert np.array_equal(k16[page, :, p % page_keys].view(np.uint16), x[b, heads * HD:(heads + kv_heads) * HD].reshape(kv_heads, HD).view(np.uint16))
        del w


def _float64_attention(q_rot, K, V, rep, alpha):
    """q_rot [heads][128], K / V [kv_heads][keys][128] (float64-able): softmax(alpha q K^T) V per head, in float64."""
    Kr, Vr = np.repeat(K, rep, axis=0).astype(np.float64), np.repeat(V, rep, axis=0).astype(np.float64)
    s = alpha * np.einsum("hd,hkd->hk", q_rot.astype(np.float64), Kr)
    s = s - s.max(axis=1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=1, keepdims=True)
    return np.einsum("hk,hkd->hd", p, Vr)


def _assert_within_project_bound(got, ref, what):
    """tests/test_gpu_attention.py's bound: |out - ref| <= 2e-3 max|ref| per head + 2^-11 |ref|."""
    tol = 2e-3 * np.abs(ref).max(axis=-1, keepdims=True) + 2.0 ** -11 * np.abs(ref)
    err = (np.abs(got.astype(np.float64) - ref) / tol).max()
    print(f"{what}: worst |err| / tol = {err:.3f}")
    assert err <= 1.0, f"{what}: worst |err| / tol = {err:.3f}"


@pytest.mark.parametrize("ke,ve", SCALES)
@pytest.mark.parametrize("page_keys", [16, 64])
@pytest.mark.parametrize("heads,kv_heads", [(4, 2), (2, 2)])
def test_step_with_rope_appends_exact_bytes_and_meets_the_projects_bound(dev, oracle, heads, kv_heads, page_keys, ke, ve):
    alpha = float(np.float16(1.0 / np.sqrt(HD)))
    rep = heads // kv_heads
    for pos in _position_sets()[::2] + [[337, 64, 511]]:
        w = _StepWorld(dev, heads, kv_heads, page_keys, pos, ke, ve, rope=True, seed=7 + sum(pos) + page_keys + heads, gaussian=True)
        x = w.qkv(on_grid=False)
        qkv = torch.from_numpy(x).to(dev)
        cos, sin = w.P8.cos.cpu().numpy(), w.P8.sin.cpu().numpy()
        assert w.P8.table_violations(w.pos_t, BOUND) == 0
        out = w.P8.step(qkv, w.pos_t, BOUND)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        what = f"heads={heads}/{kv_heads} page_keys={page_keys} scales=({ke},{ve}) pos={pos}"
        k_rows = np.zeros((len(pos), kv_heads, HD), np.uint8)
        v_rows = np.zeros_like(k_rows)
        q_rots = {}
        for b, p in w.active():
            q = x[b, :heads * HD].reshape(heads, 1, HD)
            k = x[b, heads * HD:(heads + kv_heads) * HD].reshape(kv_heads, 1, HD)
            v = x[b, (heads + kv_heads) * HD:].reshape(kv_heads, HD)
            q_rot, _ = oracle.rope_half(q, q, cos, sin, p)
            _, k_rot = oracle.rope_half(k, k, cos, sin, p)
            q_rots[b] = q_rot[:, 0]
            k_rows[b], v_rows[b] = _q(k_rot[:, 0], ke), _q(v, ve)
        ek, ev = w.expect_bytes(k_rows, v_rows)
        assert np.array_equal(w.P8.k_pool.cpu().numpy(), ek), f"{what}: appended K bytes are not quant(rope_half(k)) (or another byte changed)"
        assert np.array_equal(w.P8.v_pool.cpu().numpy(), ev), f"{what}: appended V bytes are not quant(v) (or another byte changed)"
        for b, p in enumerate(pos):
            if not 0 <= p <= BOUND:
                assert not got[b].any(), f"{what}: inactive row {b} is not zeros"
                continue
            K, V = w.P8.read_back(b, p + 1)  # dequantised pool contents after the step, own row included
            ref = _float64_attention(q_rots[b], K.cpu().numpy(), V.cpu().numpy(), rep, alpha)
            _assert_within_project_bound(got[b].reshape(heads, HD), ref, f"{what} row {b}")
        del w


# ---- 4: prefill ----
class _PrefillWorld:
    """A table of `batch` rows over fp8 pools and fp16 pools holding dequant of the same bytes; canary pages behind every row's last needed word."""

    def __init__(self, dev, heads, kv_heads, page_keys, batch, max_keys, ke, ve, rope, seed, gaussian=False):
        from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchDecodeAttention
        self.dev, self.heads, self.kv_heads, self.pk, self.ke, self.ve, self.gaussian = dev, heads, kv_heads, page_keys, ke, ve, gaussian
        self.rng = np.random.default_rng(seed)
        stride = max_keys // page_keys
        num_pages = batch * stride + 2
        order = self.rng.permutation(num_pages).tolist()
        self.canary = order[-1]
        self.alloc = PageAllocator(num_pages, page_keys, batch, stride, dev, free_order=order)
        cos = sin = None
        if rope:
            cos, sin = _tables(max_keys, seed, dev)
        self.P8 = PagedBatchDecodeAttention(self.alloc, heads, kv_heads, dev, cos, sin, kv_dtype=FP8, k_scale_log2=ke, v_scale_log2=ve)
        self.P16 = PagedBatchDecodeAttention(self.alloc, heads, kv_heads, dev, cos, sin)
        # rows nobody has written yet hold NaN bytes (and NaN in the fp16 image): keys at and beyond pos + m must weigh nothing
        self.kb = np.full((num_pages, kv_heads, page_keys, HD), 0x7F, np.uint8)
        self.vb = np.full_like(self.kb, 0xFF)

    def context(self, segments):
        for slot, pos, m in segments:
            self.alloc.reserve(slot, pos + m - 1)
            for key in range(pos):
                page = self.alloc.pages[slot][key // self.pk]
                shape = (self.kv_heads, HD)
                self.kb[page, :, key % self.pk] = _gaussian_bytes(self.rng, shape, self.ke) if self.gaussian else _finite_bytes(self.rng, shape)
                self.vb[page, :, key % self.pk] = _gaussian_bytes(self.rng, shape, self.ve) if self.gaussian else _finite_bytes(self.rng, shape)
            first = (pos + m - 1) // self.pk + 1
            if first < self.alloc.table.shape[1]:
                self.alloc.table[slot, first:] = self.canary
        self.P8.k_pool.copy_(torch.from_numpy(self.kb))
        self.P8.v_pool.copy_(torch.from_numpy(self.vb))
        self.P16.k_pool.copy_(torch.from_numpy(_dq(self.kb, self.ke)))
        self.P16.v_pool.copy_(torch.from_numpy(_dq(self.vb, self.ve)))

    def qkv(self, total, on_grid):
        h, kvh = self.heads, self.kv_heads
        x = (self.rng.standard_normal((total, (h + 2 * kvh) * HD)) * 0.9).astype(np.float16)
        if on_grid:
            x[:, h * HD:(h + kvh) * HD] = _on_grid(x[:, h * HD:(h + kvh) * HD], self.ke)
            x[:, (h + kvh) * HD:] = _on_grid(x[:, (h + kvh) * HD:], self.ve)
        return x

    def expect_bytes(self, segments, k_rows, v_rows):
        """k_rows / v_rows [total][kv_heads][128] uint8 in packed segment order."""
        ek, ev = self.kb.copy(), self.vb.copy()
        row0 = 0
        for slot, pos, m in segments:
            for r in range(m):
                page = self.alloc.pages[slot][(pos + r) // self.pk]
                ek[page, :, (pos + r) % self.pk] = k_rows[row0 + r]
                ev[page, :, (pos + r) % self.pk] = v_rows[row0 + r]
            row0 += m
        return ek, ev


SEGMENT_SETS = [[(0, 0, 1)], [(1, 0, 30)], [(2, 17, 64)], [(2, 17, 64), (0, 0, 30), (1, 5, 1)]]
# the forms (tests/test_gpu_paged_prefill.py's forcing modes): 2954 / 2958 = 4 / 8 waves x 1 row tile; 2704 = 4 waves with pairing forced on
FORMS = [2954, 2958, 2704]


def _with_mode(mode, fn):
    from tinychatengine_amd import capi
    L = capi.lib()
    capi.check(L.tce_w4a16_set_debug_mode(mode))
    try:
        return fn()
    finally:
        capi.check(L.tce_w4a16_set_debug_mode(2950))


@pytest.mark.parametrize("mode", FORMS)
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("heads,kv_heads", [(4, 2), (4, 1)])
@pytest.mark.parametrize("page_keys", [16, 64])
def test_prefill_without_rope_is_bit_identical_to_the_fp16_prefill_on_dequantised_pools(dev, page_keys, heads, kv_heads, causal, mode):
    ke, ve = SCALES[(page_keys // 16 + heads + kv_heads) % 2]
    for i, segments in enumerate(SEGMENT_SETS):
        w = _PrefillWorld(dev, heads, kv_heads, page_keys, 3, 128, ke, ve, rope=False, seed=mode + i + page_keys)
        w.context(segments)
        total = sum(m for _, _, m in segments)
        x = w.qkv(total, on_grid=True)
        qkv = torch.from_numpy(x).to(dev)

        def run():
            o8 = w.P8.prefill(segments, qkv, causal=causal)
            o16 = w.P16.prefill(segments, qkv, causal=causal)
            torch.cuda.synchronize()
            return o8, o16
        out8, out16 = _with_mode(mode, run)
        what = f"mode={mode} page_keys={page_keys} heads={heads}/{kv_heads} causal={causal} scales=({ke},{ve}) segments={segments}"
        assert torch.isfinite(out8.float()).all(), f"{what}: output not finite (a canary or an unwritten row leaked)"
        assert torch.equal(_bits(out8), _bits(out16)), f"{what}: out differs from the fp16 launch on the dequantised pools"
        k_rows = _q(x[:, heads * HD:(heads + kv_heads) * HD].reshape(total, kv_heads, HD), ke)
        v_rows = _q(x[:, (heads + kv_heads) * HD:].reshape(total, kv_heads, HD), ve)
        ek, ev = w.expect_bytes(segments, k_rows, v_rows)
        assert np.array_equal(w.P8.k_pool.cpu().numpy(), ek) and np.array_equal(w.P8.v_pool.cpu().numpy(), ev), f"{what}: the byte pools are not (what they were + quant of the new rows)"
        # the resulting pools are those of the fp16 launch: dequant of the one = the other, bit for bit (NaN rows compared as bytes above)
        fin = (ek & 0x7F) != 0x7F
        assert np.array_equal(_dq(ek, ke).view(np.uint16)[fin], w.P16.k_pool.cpu().numpy().view(np.uint16)[fin]), f"{what}: K pools differ"
        fin = (ev & 0x7F) != 0x7F
        assert np.array_equal(_dq(ev, ve).view(np.uint16)[fin], w.P16.v_pool.cpu().numpy().view(np.uint16)[fin]), f"{what}: V pools differ"
        del w


@pytest.mark.parametrize("mode", FORMS)
@pytest.mark.parametrize("heads,kv_heads", [(4, 2), (4, 1)])
@pytest.mark.parametrize("page_keys", [16, 64])
def test_prefill_with_rope_appends_exact_bytes_and_meets_the_projects_bound(dev, oracle, page_keys, heads, kv_heads, mode):
    alpha = float(np.float16(1.0 / np.sqrt(HD)))
    rep = heads // kv_heads
    ke, ve = SCALES[(page_keys // 16 + kv_heads) % 2]
    for causal, segments in [(True, SEGMENT_SETS[3]), (False, SEGMENT_SETS[2]), (True, SEGMENT_SETS[0])]:
        w = _PrefillWorld(dev, heads, kv_heads, page_keys, 3, 128, ke, ve, rope=True, seed=mode + page_keys + heads, gaussian=True)
        w.context(segments)
        total = sum(m for _, _, m in segments)
        x = w.qkv(total, on_grid=False)
        qkv = torch.from_numpy(x).to(dev)
        cos, sin = w.P8.cos.cpu().numpy(), w.P8.sin.cpu().numpy()
        out = _with_mode(mode, lambda: w.P8.prefill(segments, qkv, causal=causal))
        torch.cuda.synchronize()
        got_all = out.cpu().numpy()
        what = f"mode={mode} page_keys={page_keys} heads={heads}/{kv_heads} causal={causal} segments={segments}"
        k_rows, v_rows, q_rots = np.zeros((total, kv_heads, HD), np.uint8), np.zeros((total, kv_heads, HD), np.uint8), {}
        row0 = 0
        for slot, pos, m in segments:
            xs = x[row0:row0 + m]
            q = np.ascontiguousarray(xs[:, :heads * HD].reshape(m, heads, HD).transpose(1, 0, 2))
            k = np.ascontiguousarray(xs[:, heads * HD:(heads + kv_heads) * HD].reshape(m, kv_heads, HD).transpose(1, 0, 2))
            q_rot, _ = oracle.rope_half(q, q, cos, sin, pos)
            _, k_rot = oracle.rope_half(k, k, cos, sin, pos)
            q_rots[slot] = q_rot
            k_rows[row0:row0 + m] = _q(np.ascontiguousarray(k_rot.transpose(1, 0, 2)), ke)
            v_rows[row0:row0 + m] = _q(xs[:, (heads + kv_heads) * HD:].reshape(m, kv_heads, HD), ve)
            row0 += m
        ek, ev = w.expect_bytes(segments, k_rows, v_rows)
        assert np.array_equal(w.P8.k_pool.cpu().numpy(), ek), f"{what}: appended K bytes are not quant of the oracle-rotated keys (or another byte changed)"
        assert np.array_equal(w.P8.v_pool.cpu().numpy(), ev), f"{what}: appended V bytes are not quant(v) (or another byte changed)"
        row0 = 0
        for slot, pos, m in segments:
            K, V = (t.cpu().numpy() for t in w.P8.read_back(slot, pos + m))
            got = got_all[row0:row0 + m].reshape(m, heads, HD)
            for r in range(m):
                n = pos + r + 1 if causal else pos + m
                ref = _float64_attention(q_rots[slot][:, r], K[:, :n], V[:, :n], rep, alpha)
                _assert_within_project_bound(got[r], ref, f"{what} slot {slot} row {r}")
            row0 += m
        del w


# ---- 5: one cache, two ways in ----
def test_a_prompt_prefilled_and_the_same_rows_decoded_leave_identical_pages(dev):
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchDecodeAttention
    heads, kv_heads, pk, n = 4, 2, 16, 40
    cos, sin = _tables(64, 5, dev)
    rng = np.random.default_rng(55)
    x = torch.from_numpy((rng.standard_normal((n, (heads + 2 * kv_heads) * HD)) * 0.9).astype(np.float16)).to(dev)
    pools = []
    for way in ("prefill", "steps"):
        alloc = PageAllocator(6, pk, 1, 4, dev, free_order=[4, 1, 5, 0, 2, 3])
        P = PagedBatchDecodeAttention(alloc, heads, kv_heads, dev, cos, sin, kv_dtype=FP8, k_scale_log2=1, v_scale_log2=-2)
        P.k_pool.fill_(0x22)
        P.v_pool.fill_(0x22)
        alloc.reserve(0, n - 1)
        if way == "prefill":
            P.prefill([(0, 0, n)], x)
        else:
            pos_t = torch.zeros(1, dtype=torch.int32, device=dev)
            for i in range(n):
                pos_t.fill_(i)
                assert P.table_violations(pos_t, n - 1) == 0
                P.step(x[i:i + 1].contiguous(), pos_t, n - 1)
        torch.cuda.synchronize()
        pools.append((P.k_pool.cpu().numpy(), P.v_pool.cpu().numpy(), alloc.pages[0]))
    (k1, v1, p1), (k2, v2, p2) = pools
    assert p1 == p2 == [4, 1, 5]
    assert np.array_equal(k1, k2) and np.array_equal(v1, v2), "a token that arrived by prefill and one that arrived by a decode step differ in the pages"
    assert (k1[p1[2], :, 8:] == 0x22).all() and (k1[[0, 2, 3]] == 0x22).all(), "a row outside the prompt was written"


# ---- 6: fork ----
def test_forked_sequences_equal_the_same_sequences_alone(dev):
    """Two sequences share the full pages of a 37-key prompt (two pages of 16 shared, 5 rows copied), prefill different suffixes in ONE launch and decode a step:
    each equals the same sequence run alone -- pages byte for byte, outputs bit for bit."""
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchDecodeAttention
    heads, kv_heads, pk, common, ke, ve = 4, 2, 16, 37, 2, -1
    cos, sin = _tables(128, 9, dev)
    rng = np.random.default_rng(66)
    width = (heads + 2 * kv_heads) * HD
    rows = lambda m: torch.from_numpy((rng.standard_normal((m, width)) * 0.9).astype(np.float16)).to(dev)
    prompt, suffix, token = rows(common), {0: rows(9), 1: rows(20)}, {0: rows(1), 1: rows(1)}

    def make(batch):
        alloc = PageAllocator(16, pk, batch, 8, dev)
        return alloc, PagedBatchDecodeAttention(alloc, heads, kv_heads, dev, cos, sin, kv_dtype=FP8, k_scale_log2=ke, v_scale_log2=ve)

    # alone
    alone = {}
    for s in (0, 1):
        alloc, P = make(1)
        alloc.reserve(0, common - 1)
        P.prefill([(0, 0, common)], prompt)
        m = suffix[s].shape[0]
        alloc.reserve(0, common + m)
        o_suffix = P.prefill([(0, common, m)], suffix[s])
        pos_t = torch.tensor([common + m], dtype=torch.int32, device=dev)
        o_tok = P.step(token[s], pos_t, 127)
        torch.cuda.synchronize()
        alone[s] = (o_suffix.clone(), o_tok.clone(), [P.k_pool[p].cpu().numpy() for p in alloc.pages[0]], [P.v_pool[p].cpu().numpy() for p in alloc.pages[0]])
    # forked
    alloc, P = make(2)
    alloc.reserve(0, common - 1)
    P.prefill([(0, 0, common)], prompt)
    for src, dst, n in alloc.fork(0, 1, common):
        P.copy_rows(src, dst, n)
    assert alloc.pages[0][:2] == alloc.pages[1][:2] and alloc.pages[0][2] != alloc.pages[1][2]
    segs = [(0, common, suffix[0].shape[0]), (1, common, suffix[1].shape[0])]
    for slot, pos, m in segs:
        alloc.reserve(slot, pos + m)
    o = P.prefill(segs, torch.cat([suffix[0], suffix[1]]))
    pos_t = torch.tensor([common + 9, common + 20], dtype=torch.int32, device=dev)
    assert P.table_violations(pos_t, 127) == 0
    o_tok = P.step(torch.cat([token[0], token[1]]), pos_t, 127)
    torch.cuda.synchronize()
    alloc.check_invariants()
    row0 = 0
    for s in (0, 1):
        m = suffix[s].shape[0]
        assert torch.equal(_bits(o[row0:row0 + m]), _bits(alone[s][0])), f"sequence {s}: suffix outputs differ from the run alone"
        assert torch.equal(_bits(o_tok[s:s + 1]), _bits(alone[s][1])), f"sequence {s}: the decode step's output differs from the run alone"
        keys = common + m + 1
        for i, page in enumerate(alloc.pages[s]):
            n = min(pk, keys - i * pk)
            assert np.array_equal(P.k_pool[page].cpu().numpy()[:, :n], alone[s][2][i][:, :n]) and np.array_equal(P.v_pool[page].cpu().numpy()[:, :n], alone[s][3][i][:, :n]), \
                f"sequence {s}: page {i} differs from the run alone"
        row0 += m


# ---- 7: generation ----
VOCAB = 4096
MAX_KEYS, PAGE_KEYS, BATCH, NUM_PAGES = 64, 16, 4, 12
SMALL = (512, 4, 1, 1408, 2)


class _Model:
    """tests/test_gpu_generate.py's SMALL model, rebuilt: hidden 512, 4 heads, 1 kv head, 2 layers, vocab 4096, 64 max keys, pages of 16, 12 pages."""

    def __init__(self, dev, hidden, heads, kv_heads, ffn, layers, seed):
        from tinychatengine_amd.decoder_block import DecoderBlock
        from tinychatengine_amd.linear import Linear_half_int4
        rng = np.random.default_rng(seed)
        ang = rng.uniform(0, 2 * np.pi, (MAX_KEYS, HD // 2))
        cos = torch.from_numpy(np.concatenate([np.cos(ang), np.cos(ang)], axis=1).astype(np.float16)).to(dev)
        sin = torch.from_numpy(np.concatenate([np.sin(ang), np.sin(ang)], axis=1).astype(np.float16)).to(dev)
        self.dev, self.hidden = dev, hidden
        self.blocks = [DecoderBlock(hidden, heads, ffn, MAX_KEYS, dev, cos, sin, seed=seed + i, kv_heads=kv_heads) for i in range(layers)]
        g = torch.Generator(device=dev).manual_seed(seed + 100)
        self.final_gamma = (1.0 + 0.1 * torch.empty(hidden, device=dev).normal_(0, 1, generator=g)).float()
        self.lm_head = Linear_half_int4.from_float(torch.empty(VOCAB, hidden, device=dev).normal_(0.0, hidden ** -0.5, generator=g)).prepack()
        self.table = torch.empty(VOCAB, hidden, device=dev).normal_(0.0, 1.0, generator=g).half()

    def decoders(self, free_order=None, **kv):
        from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchedDecoder
        alloc = PageAllocator(NUM_PAGES, PAGE_KEYS, BATCH, MAX_KEYS // PAGE_KEYS, self.dev, free_order=free_order)
        return [PagedBatchedDecoder(b, alloc, **kv) for b in self.blocks]

    def generator(self, stop_ids=(), free_order=None, max_new=40, **kv):
        from tinychatengine_amd.generate import BatchedGenerator
        return BatchedGenerator(self.decoders(free_order, **kv), self.final_gamma, self.lm_head, self.table, max_new=max_new, stop_ids=stop_ids, graph=True)

    def host_loop(self, stop_ids=(), free_order=None, **kv):
        from tinychatengine_amd.generate import HostDrivenLoop
        return HostDrivenLoop(self.decoders(free_order, **kv), self.final_gamma, self.lm_head, self.table, stop_ids=stop_ids)


@pytest.fixture(scope="module")
def model(dev):
    return _Model(dev, *SMALL, seed=40 + SMALL[0])


def test_greedy_generation_over_fp8_pages_equals_the_host_driven_loop(dev, model):
    """BatchedGenerator under the captured graph = HostDrivenLoop over fp8 decoders, id for id: staggered admissions, slot 0 retired and a new prompt admitted into
    it onto reused pages, slot 3 retiring on its budget.  PageAllocator, BatchedGenerator, SlotBook and HostDrivenLoop are used as they are."""
    from tinychatengine_amd.generate import SamplingParams
    kv = dict(kv_dtype=FP8, k_scale_log2=-1, v_scale_log2=-2)
    rng = np.random.default_rng(77)
    greedy = SamplingParams(temp=0.0, repeat_penalty=1.0)
    prompts = {s: rng.integers(0, VOCAB, n).tolist() for s, n in {0: 20, 1: 3, 2: 4, 3: 2, "new": 6}.items()}
    order = np.random.default_rng(13).permutation(NUM_PAGES).tolist()
    gen, host = model.generator(free_order=order, **kv), model.host_loop(free_order=order, **kv)
    assert all(d.attention.k_pool.dtype == torch.uint8 and d.attention.fp8 for d in gen.decoders + host.decoders)
    alloc = gen.allocator

    def both_run(n):
        retired = gen.run(n)
        for _ in range(n):
            host.step()
        alloc.check_invariants()
        for s in range(BATCH):
            assert gen.tokens(s) == host.out[s], f"slot {s}: the graph run and the host-driven loop disagree"
        return retired

    assert gen.admit([(0, prompts[0], greedy, 0, 40), (3, prompts[3], greedy, 0, 12)]) == []
    host.admit([(0, prompts[0], 40), (3, prompts[3], 12)])
    assert both_run(2) == []
    gen.admit(1, prompts[1], greedy, 0, 40)
    host.admit(1, prompts[1], 40)
    assert both_run(2) == []
    gen.admit(2, prompts[2], greedy, 0, 40)
    host.admit(2, prompts[2], 40)
    retired = both_run(3)
    assert 0 not in retired and len(gen.tokens(0)) == 8
    released = gen.release(0)  # retired by the caller: its pages come back
    host.release(0)
    assert len(released) == 2
    gen.admit(0, prompts["new"], greedy, 0, 40)
    host.admit(0, prompts["new"], 40)
    assert set(alloc.pages[0]) & set(released), "the new sequence reuses none of the released pages"
    for _ in range(3):
        retired += both_run(3)
    assert 3 in retired and len(gen.tokens(3)) == 12  # its budget
    assert gen.embed_violations() == 0
    alloc.check_invariants()
    host.allocator.check_invariants()
    assert len(set(map(tuple, (gen.tokens(s) for s in range(BATCH))))) == BATCH, "the slots produced the same ids: the run shows nothing"
    for s in gen.book.live():
        n = gen.book.pos[s]
        assert n == host.pos_host[s]
        for dg, dh in zip(gen.decoders, host.decoders):
            for a, b in zip(dg.attention.read_back(s, n), dh.attention.read_back(s, n)):
                assert a.dtype == torch.float16 and torch.equal(_bits(a), _bits(b)), f"slot {s}: cached keys differ"


def test_the_fp16_default_through_the_new_arguments_gives_the_same_ids(dev, model):
    from tinychatengine_amd.generate import SamplingParams
    greedy = SamplingParams(temp=0.0, repeat_penalty=1.0)
    rng = np.random.default_rng(78)
    prompts = [(2, rng.integers(0, VOCAB, 5).tolist()), (0, rng.integers(0, VOCAB, 9).tolist())]
    ids = []
    for kv in ({}, dict(kv_dtype="fp16", k_scale_log2=0, v_scale_log2=0)):
        gen = model.generator(**kv)
        assert all(d.attention.k_pool.dtype == torch.float16 for d in gen.decoders)
        for s, p in prompts:
            gen.admit(s, p, greedy, 0, 20)
        gen.run(25)
        ids.append([gen.tokens(s) for s, _ in prompts])
        assert all(len(t) == 20 for t in ids[-1])
    assert ids[0] == ids[1]
