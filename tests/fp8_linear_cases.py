"""The FP8 linears' definition (include/tce_matmul.h, "FP8 linears") restated in numpy, and the designed inputs of tests/test_fp8_linear.py and
tests/test_gpu_fp8_linear.py.  Everything here is from the format's definition: the 256-entry table, nearest-with-ties-to-even by search in it, float64 products."""
import numpy as np


def _table():
    b = np.arange(256)
    ex, m = (b >> 3) & 15, b & 7
    v = np.where(ex == 0, m * 2.0 ** -9, (1 + m / 8) * 2.0 ** (ex.astype(np.float64) - 7))
    v[(b & 0x7F) == 0x7F] = np.nan
    return np.where(b >> 7 == 1, -v, v)


TABLE = _table()  # float64 value of every byte
POS = TABLE[:0x7F]  # the 127 finite non-negative values, ascending: index = byte


def e4m3_rne_sat(f):
    """float32 array -> bytes: the nearest table value of min(|f|, 448), a tie to the even byte; the sign bit is f's; NaN -> 0x7f."""
    f = np.asarray(f, np.float32)
    a = np.minimum(np.abs(f.astype(np.float64)), 448.0)
    hi = np.clip(np.searchsorted(POS, a), 1, 0x7E)
    lo = hi - 1
    dl, dh = a - POS[lo], POS[hi] - a
    mag = np.where((dl < dh) | ((dl == dh) & (lo % 2 == 0)), lo, hi)
    out = (mag | np.where(np.signbit(f), 0x80, 0)).astype(np.uint8)
    return np.where(np.isnan(f), np.uint8(0x7F), out)


def quantize_rows(x):
    """x float16 [M][K] -> (xq uint8 [M][K], sx float32 [M]): one float32 operation per step of the definition."""
    xf = x.astype(np.float32)
    amax = np.abs(xf).max(axis=1)
    zero = amax == 0
    safe = np.where(zero, np.float32(1), amax)
    sx = np.where(zero, np.float32(1), safe / np.float32(448))
    inv = np.where(zero, np.float32(1), np.float32(448) / safe)
    return e4m3_rne_sat(xf * inv[:, None]), sx.astype(np.float32)


def quantiser_rows(K, rng):
    """The rows the quantiser is held on: Gaussian, all zero, with a -0, amax 65504, one-hot, exact ties between e4m3 neighbours (amax 448: inv = 1)."""
    g = rng.standard_normal(K).astype(np.float16)
    neg0 = g.copy()
    neg0[[3, K - 1]] = np.float16(-0.0)
    big = (g * np.float16(100)).astype(np.float16)
    big[K // 2] = np.float16(-65504)
    hot = np.zeros(K, np.float16)
    hot[K - 7] = np.float16(0.3)
    ties = np.array([1.0625, 17, 2.0 ** -10, 3 * 2.0 ** -10, 27, 432, 15 * 2.0 ** -10, 0.0302734375, 1.1875, 200], np.float16)
    tie = np.resize(np.concatenate([ties, -ties]), K)
    tie[5] = np.float16(448)
    zero = np.zeros(K, np.float16)
    zero[1] = np.float16(-0.0)
    return np.stack([g, zero, neg0, big, hot, tie])


def weight_bytes_nk(N, K):
    """Finite positive bytes that name their (n, k): what a one-hot activation row reads back."""
    n, k = np.arange(N)[:, None], np.arange(K)[None, :]
    return ((n * 31 + k * 7 + k // 127) % 127).astype(np.uint8)


def one_hot_rows(M, K, k0):
    """Row 0 one-hot at k0, row m at (k0 + 17 m) % K; the value 448 * 2^-9: sx = 2^-9 and every output 0.875 * e4m3(byte), exact in binary16."""
    x = np.zeros((M, K), np.float16)
    x[np.arange(M), (k0 + 17 * np.arange(M)) % K] = np.float16(0.875)
    return x


def byte_of(v):
    """The byte of values that are exactly representable (integers up to 16, 448)."""
    b = e4m3_rne_sat(np.asarray(v, np.float32))
    assert np.array_equal(TABLE[b], np.asarray(v, np.float64))
    return b


def exact_case(M, N, K, rng):
    """Integer operands whose every partial sum is an integer below 2^16 and whose scaled sum (+ C0) is exact in fp32: |xq| <= 4 with one 448 per row, |wq| <= 8,
    sx = 2^j (j -3 .. 0), sw = 2^i (i -4 .. 0), C0 integers up to 64.  |acc| <= 32 K + 3584 <= 40448."""
    xi = rng.integers(-4, 5, (M, K)).astype(np.float64)
    xi[np.arange(M), rng.integers(0, K, M)] = 448.0
    wi = rng.integers(-8, 9, (N, K)).astype(np.float64)
    sx = (2.0 ** rng.integers(-3, 1, M)).astype(np.float32)
    sw = (2.0 ** rng.integers(-4, 1, N)).astype(np.float32)
    c0 = rng.integers(-64, 65, (M, N)).astype(np.float16)
    return byte_of(xi), sx, byte_of(wi), sw, c0


def reference(xq, sx, wq, sw):
    """float64 on the same bytes and scales: (v [M][N], sum_k |xq wq| [M][N])."""
    a, w = TABLE[xq], TABLE[wq]
    s = sx.astype(np.float64)[:, None] * sw.astype(np.float64)[None, :]
    return (a @ w.T) * s, np.abs(a) @ np.abs(w).T * s


def bound(ref, absprod, K):
    """The issue's bound: the binary16 rounding (2^-11 |ref| + 2^-25), one fp32 unit per product alignment and accumulation step ((K + 128) 2^-23) and the two scale
    multiplies and the add (3 * 2^-24), on sx sw sum_k |xq wq|."""
    return 2.0 ** -11 * np.abs(ref) + 2.0 ** -25 + ((K + 128) * 2.0 ** -23 + 3 * 2.0 ** -24) * absprod
