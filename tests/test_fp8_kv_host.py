"""CPU (no GPU): the e4m3 KV pages' format (include/tce_matmul.h, "FP8 pages") as the host helpers state it, and the new entry points' refusals.

* fp8_dequantize_reference against the 256-entry table built from sign / exponent / mantissa, exact in binary16 for all 254 finite bytes x 16 exponents;
* fp8_quantize_reference against the definition for every finite binary16 value x every exponent: the chosen byte is a nearest finite value, a tie goes to the even
  byte, values saturate at +-448 (the infinities too), -0 stays 0x80, NaN becomes a NaN byte;
* the fp8 entry points refuse an exponent of -9 or 8, a misaligned pointer and an unsupported pool shape before any HIP call, naming the argument;
* tce_kv_pages_pool_bytes_fp8 is half of tce_kv_pages_pool_bytes."""
import ctypes as C
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

EXPONENTS = list(range(-8, 8))


@pytest.fixture(scope="module")
def capi():
    from tinychatengine_amd import build as B
    B.build()
    from tinychatengine_amd import capi
    return capi


def _table():
    """e4m3fn from the definition, as Python floats (exact): index = byte; NaN for 0x7f / 0xff."""
    t = []
    for b in range(256):
        s, ex, m = b >> 7, (b >> 3) & 15, b & 7
        if ex == 15 and m == 7:
            v = math.nan
        elif ex == 0:
            v = m * 2.0 ** -9
        else:
            v = (1 + m / 8) * 2.0 ** (ex - 7)
        t.append(-v if s else v)
    return np.array(t, np.float64)


def test_format_constants():
    t = _table()
    assert np.nanmax(t) == 448.0 and t[0x7E] == 448.0 and t[0x01] == 2.0 ** -9 and t[0x08] == 2.0 ** -6 and t[0x38] == 1.0
    assert np.isnan(t[0x7F]) and np.isnan(t[0xFF]) and np.isfinite(np.delete(t, [0x7F, 0xFF])).all()
    assert (np.diff(t[:0x7F]) > 0).all(), "the positive bytes are ordered as their values"


def test_dequantize_reference_is_the_table_times_a_power_of_two_exactly():
    from tinychatengine_amd.paged_kv import fp8_dequantize_reference
    t = _table()
    b = np.arange(256, dtype=np.uint8)
    finite = ~np.isnan(t)
    assert finite.sum() == 254
    for e in EXPONENTS:
        got = fp8_dequantize_reference(b, e)
        assert got.dtype == np.float16 and got.shape == b.shape
        want = t * 2.0 ** e
        assert np.array_equal(got[finite].astype(np.float64), want[finite]), f"e={e}: not exact in binary16"
        assert np.array_equal(np.signbit(got[finite]), np.signbit(want[finite]))  # (the zeros' signs)
        assert np.isnan(got[~finite]).all()
    assert np.array_equal(fp8_dequantize_reference(torch.arange(256, dtype=torch.uint8), 3), fp8_dequantize_reference(b, 3), equal_nan=True)
    for bad in (-9, 8):
        with pytest.raises(ValueError):
            fp8_dequantize_reference(b, bad)


def test_quantize_reference_is_nearest_ties_to_even_saturating_for_every_binary16():
    from tinychatengine_amd.paged_kv import fp8_quantize_reference
    t = _table()
    pos = t[:0x7F]  # the 127 finite non-negative values, ascending: index = byte
    allh = np.arange(65536, dtype=np.uint16).view(np.float16)
    isnan = np.isnan(allh)
    assert (~isnan).sum() == 63488 + 2  # the finite values and the two infinities
    for e in EXPONENTS:
        got = fp8_quantize_reference(allh, e)
        assert got.dtype == np.uint8 and got.shape == allh.shape
        assert ((got[isnan] & 0x7F) == 0x7F).all(), "NaN in, NaN byte out"
        x = allh[~isnan].astype(np.float64) * 2.0 ** -e  # exact
        g = got[~isnan]
        assert ((g & 0x7F) != 0x7F).all(), "a number became a NaN byte"
        assert np.array_equal((g & 0x80) != 0, np.signbit(x)), "the sign (of zero too) is the input's"
        a = np.minimum(np.abs(x), 448.0)  # the clamp: saturation, +-inf included
        mag = (g & 0x7F).astype(np.int64)
        err = np.abs(pos[mag] - a)
        # nearest: no neighbour is closer; a tie with a neighbour only where the chosen byte is even
        lo, hi = np.maximum(mag - 1, 0), np.minimum(mag + 1, 0x7E)
        err_lo, err_hi = np.abs(pos[lo] - a), np.abs(pos[hi] - a)
        assert (err <= err_lo).all() and (err <= err_hi).all(), f"e={e}: a neighbouring byte is nearer"
        tie = ((err == err_lo) & (lo != mag)) | ((err == err_hi) & (hi != mag))
        assert (mag[tie] % 2 == 0).all(), f"e={e}: a tie did not go to the even byte"
        # (nearest among the neighbours is nearest among all: the table is monotonic -- test_format_constants)
        assert (g[np.isinf(x)] & 0x7F == 0x7E).all() and (g[np.abs(x) >= 448] & 0x7F == 0x7E).all()
    assert fp8_quantize_reference(np.array([-0.0], np.float16), 0)[0] == 0x80
    h = torch.from_numpy(allh[:1024].copy())
    assert np.array_equal(fp8_quantize_reference(h, -3), fp8_quantize_reference(allh[:1024], -3))


def test_quantize_of_dequantize_is_the_identity_on_finite_bytes():
    from tinychatengine_amd.paged_kv import fp8_dequantize_reference, fp8_quantize_reference
    b = np.delete(np.arange(256, dtype=np.uint8), [0x7F, 0xFF])
    for e in EXPONENTS:
        assert np.array_equal(fp8_quantize_reference(fp8_dequantize_reference(b, e), e), b)


def test_pool_bytes_are_half_of_the_fp16_pools(capi):
    L = capi.lib()
    for shape in [(1, 1, 16, 128), (12, 1, 16, 128), (9399 // 64 + 1, 8, 64, 128), (1000, 8, 256, 128)]:
        full = int(L.tce_kv_pages_pool_bytes(*shape))
        assert full > 0 and int(L.tce_kv_pages_pool_bytes_fp8(*shape)) * 2 == full
    for shape in [(0, 8, 16, 128), (4, 0, 16, 128), (4, 8, 8, 128), (4, 8, 48, 128), (4, 8, 512, 128), (4, 8, 16, 64)]:
        assert int(L.tce_kv_pages_pool_bytes(*shape)) == 0 and int(L.tce_kv_pages_pool_bytes_fp8(*shape)) == 0


class _Args:
    """Host memory standing in for device memory: every refusal below happens before any HIP call, so nothing is ever dereferenced."""

    def __init__(self):
        self.buf = C.create_string_buffer(1 << 16)
        base = C.addressof(self.buf)
        self.a = [(base + 255) // 256 * 256 + 4096 * i for i in range(12)]  # 256-byte aligned, distinct

    def p(self, i, off=0):
        return C.c_void_p(self.a[i] + off)


def _step(L, A, k_e=0, v_e=0, k_off=0, qkv_off=0, page_keys=16, hd=128, batch=2):
    return L.tce_attention_decode_step_paged_fp8(A.p(0, qkv_off), A.p(1, k_off), A.p(2), A.p(3), 4, page_keys, 8, None, None, A.p(4), A.p(5), batch, 4, 2, hd, A.p(6), 63,
                                                 0x2DA8, k_e, v_e, None)


def _prefill(L, A, capi, k_e=0, v_e=0, v_off=0, page_keys=16, hd=128):
    segs, total = capi.prefill_segments([(0, 0, 5)])
    return L.tce_attention_prefill_paged_fp8(A.p(0), 0, A.p(1), A.p(2, v_off), A.p(3), 2, 4, page_keys, 8, None, None, 1, A.p(4), 0, A.p(5), 4, 2, hd,
                                             C.cast(segs, C.c_void_p), 1, total, 0x2DA8, k_e, v_e, None)


def _copy(L, A, which, k_e=0, v_e=0, lin_off=0, pool_off=0, page_keys=16, hd=128):
    fn = L.tce_kv_pages_scatter_fp8 if which == "scatter" else L.tce_kv_pages_gather_fp8
    lin, pool = (A.p(0, lin_off), A.p(1)), (A.p(2, pool_off), A.p(3))
    first, second = (lin, pool) if which == "scatter" else (pool, lin)
    return fn(*first, *second, A.p(4), 4, page_keys, 8, 2, hd, 64, 0, 5, k_e, v_e, None)


def test_the_fp8_entry_points_refuse_bad_exponents_pointers_and_shapes_without_a_device(capi):
    L, A = capi.lib(), _Args()
    err = lambda: L.tce_last_error().decode()
    calls = {"tce_attention_decode_step_paged_fp8": lambda **kw: _step(L, A, **kw), "tce_attention_prefill_paged_fp8": lambda **kw: _prefill(L, A, capi, **kw),
             "tce_kv_pages_scatter_fp8": lambda **kw: _copy(L, A, "scatter", **kw), "tce_kv_pages_gather_fp8": lambda **kw: _copy(L, A, "gather", **kw)}
    for name, call in calls.items():
        for e in (-9, 8):
            assert call(k_e=e) == capi.TCE_ERR_BAD_ARG and name in err() and "k_scale_log2" in err() and str(e) in err(), (name, e, err())
            assert call(v_e=e) == capi.TCE_ERR_BAD_ARG and name in err() and "v_scale_log2" in err() and str(e) in err(), (name, e, err())
        for pk in (8, 48, 512):
            assert call(page_keys=pk) == capi.TCE_ERR_BAD_ARG and name in err() and "page_keys" in err(), (name, pk, err())
        assert call(hd=64) == capi.TCE_ERR_UNSUPPORTED_SHAPE and name in err() and "head_dim" in err(), (name, err())
    # a pointer that is not 16-byte aligned: refused by name
    assert _step(L, A, k_off=8) == capi.TCE_ERR_UNSUPPORTED_SHAPE and "k_pool" in err() and "16-byte" in err()
    assert _step(L, A, qkv_off=2) == capi.TCE_ERR_UNSUPPORTED_SHAPE and "qkv" in err() and "16-byte" in err()
    assert _prefill(L, A, capi, v_off=8) == capi.TCE_ERR_UNSUPPORTED_SHAPE and "v_pool" in err() and "16-byte" in err()
    assert _copy(L, A, "scatter", lin_off=8) == capi.TCE_ERR_UNSUPPORTED_SHAPE and "k_src" in err() and "16-byte" in err()
    assert _copy(L, A, "gather", lin_off=8) == capi.TCE_ERR_UNSUPPORTED_SHAPE and "k_dst" in err() and "16-byte" in err()
    assert _copy(L, A, "gather", pool_off=8) == capi.TCE_ERR_UNSUPPORTED_SHAPE and "k_pool" in err() and "16-byte" in err()
    # null pointers and a batch beyond the grid
    assert L.tce_attention_decode_step_paged_fp8(None, A.p(1), A.p(2), A.p(3), 4, 16, 8, None, None, A.p(4), A.p(5), 2, 4, 2, 128, A.p(6), 63, 0x2DA8, 0, 0, None) == capi.TCE_ERR_BAD_ARG
    assert "null" in err()
    assert _step(L, A, batch=65536) == capi.TCE_ERR_UNSUPPORTED_SHAPE and "batch" in err()


def test_python_front_refuses_bad_kv_dtype_and_exponents():
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchDecodeAttention
    alloc = PageAllocator(4, 16, 2, 2, "cpu")
    with pytest.raises(ValueError, match="kv_dtype"):
        PagedBatchDecodeAttention(alloc, 4, 2, "cpu", kv_dtype="fp8_e5m2")
    for kw in ({"k_scale_log2": 8}, {"v_scale_log2": -9}, {"k_scale_log2": 0.5}):
        with pytest.raises(ValueError, match="exponent"):
            PagedBatchDecodeAttention(alloc, 4, 2, "cpu", kv_dtype="fp8_e4m3", **kw)
