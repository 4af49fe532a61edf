"""GPU: the FP8 linears (tce_fp8_quantize_rows_f16, tce_w8a8_fp8_forward_f16, linear.Linear_half_fp8) against the numpy restatement of their definition
(tests/fp8_linear_cases.py): the quantiser bit for bit, one-hot rows that read back the weight byte at (n, k) -- the matrix instruction's operand layout --, integer
operands whose result is exact, random operands inside the issue's bound, and the bits' independence of M and of a repeat.  Both forms, forced by their flag bits."""
import numpy as np
import pytest

import fp8_linear_cases as fc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SKINNY, TILED, ADD = 256, 512, 16
FORMS = [pytest.param(SKINNY, id="skinny"), pytest.param(TILED, id="tiled")]
NAN16 = 0x7E00


@pytest.fixture(scope="module")
def dev():
    from tinychatengine_amd import capi
    assert torch.cuda.is_available() and capi.lib()
    return torch.device("cuda:0")


def _quantize(dev, x, pad=0):
    """x float16 [M][K] with ldx = K + pad, ldq = K + 2 pad -> (xq [M][K], sx [M]) as numpy; the bytes between K and ldq must stay as they were."""
    from tinychatengine_amd import capi
    M, K = x.shape
    xb = torch.zeros((M, K + pad), dtype=torch.float16, device=dev)
    xb[:, :K] = torch.from_numpy(x).to(dev)
    xq = torch.full((M, K + 2 * pad), 0xAA, dtype=torch.uint8, device=dev)
    sx = torch.empty(M, dtype=torch.float32, device=dev)
    capi.check(capi.lib().tce_fp8_quantize_rows_f16(xb.data_ptr(), K + pad, xq.data_ptr(), K + 2 * pad, sx.data_ptr(), M, K, None))
    torch.cuda.synchronize()
    q = xq.cpu().numpy()
    assert (q[:, K:] == 0xAA).all()
    return q[:, :K].copy(), sx.cpu().numpy()


def _forward(dev, xq, sx, wq, sw, flags, c0=None):
    """C with ldc = N + 8 -> its bits [M][N] (uint16); the columns past N must stay NaN."""
    from tinychatengine_amd import capi
    (M, K), N = xq.shape, wq.shape[0]
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (xq, sx, wq, sw)]
    c = torch.full((M, N + 8), NAN16, dtype=torch.int16, device=dev)
    if c0 is not None:
        c[:, :N] = torch.from_numpy(c0.view(np.int16)).to(dev)
    capi.check(capi.lib().tce_w8a8_fp8_forward_f16(t[0].data_ptr(), K, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), c.data_ptr(), N + 8, M, N, K, flags, None))
    torch.cuda.synchronize()
    out = c.cpu().numpy().view(np.uint16)
    assert (out[:, N:] == NAN16).all()
    return out[:, :N].copy()


@pytest.mark.parametrize("K", [128, 384, 4096])
def test_quantiser_is_the_definition_bit_for_bit(dev, K):
    x = fc.quantiser_rows(K, np.random.default_rng(K))
    xq, sx = _quantize(dev, x, pad=8)
    want_q, want_s = fc.quantize_rows(x)
    assert np.array_equal(sx.view(np.uint32), want_s.view(np.uint32))
    assert np.array_equal(xq, want_q), np.argwhere(xq != want_q)[:8]


@pytest.mark.parametrize("k0", [0, 1, 15, 16, 31, 32, 63, 64, 127, 128, 255])
@pytest.mark.parametrize("form", FORMS)
def test_one_hot_rows_read_back_the_weight_byte_at_n_k(dev, form, k0):
    M, N, K = (16 if form == SKINNY else 17), 48, 256
    x = fc.one_hot_rows(M, K, k0)
    xq, sx = _quantize(dev, x)
    assert (sx == 2.0 ** -9).all() and np.array_equal(xq, fc.quantize_rows(x)[0])
    wq, sw = fc.weight_bytes_nk(N, K), np.ones(N, np.float32)
    want = np.float16(fc.reference(xq, sx, wq, sw)[0])
    assert np.array_equal(want[0], np.float16(0.875 * fc.TABLE[wq[:, k0]]))  # what the case is about: row 0 names column k0 of the weights
    got = _forward(dev, xq, sx, wq, sw, form)
    assert np.array_equal(got, want.view(np.uint16)), np.argwhere(got != want.view(np.uint16))[:8]


@pytest.mark.parametrize("add", [0, ADD])
@pytest.mark.parametrize("form,M", [(SKINNY, 1), (SKINNY, 15), (SKINNY, 16), (TILED, 1), (TILED, 17), (TILED, 127), (TILED, 128), (TILED, 129), (TILED, 257)])
def test_integer_operands_give_the_float64_value_rounded_once(dev, form, M, add):
    rng = np.random.default_rng(1000 * M + form + add)
    for N in (16, 48, 144, 272):
        for K in (128, 256, 1152):  # 1152: nine K steps, an odd count for the two buffers
            xq, sx, wq, sw, c0 = fc.exact_case(M, N, K, rng)
            want = np.float16(fc.reference(xq, sx, wq, sw)[0] + (c0.astype(np.float64) if add else 0.0))
            got = _forward(dev, xq, sx, wq, sw, form | add, c0 if add else None)
            assert np.array_equal(got, want.view(np.uint16)), (N, K, np.argwhere(got != want.view(np.uint16))[:8])


@pytest.fixture(scope="module")
def random_case(dev):
    """Gaussian rows quantised on the device, random non-NaN weight bytes, 257 rows: (xq, sx, wq, sw, float64 v, float64 sum of |products|)."""
    rng = np.random.default_rng(7)
    N, K = 272, 1152
    xq, sx = _quantize(dev, rng.standard_normal((257, K)).astype(np.float16))
    wq = rng.integers(0, 256, (N, K)).astype(np.uint8)
    wq[(wq & 0x7F) == 0x7F] -= 1
    sw = (rng.uniform(0.5, 1.0, N) * 2.0 ** -6).astype(np.float32)
    return (xq, sx, wq, sw) + fc.reference(xq, sx, wq, sw)


@pytest.mark.parametrize("add", [0, ADD])
@pytest.mark.parametrize("form,M", [(SKINNY, 16), (TILED, 257)])
def test_random_operands_stay_inside_the_bound(dev, random_case, form, M, add):
    xq, sx, wq, sw, v, absprod = random_case
    c0 = np.random.default_rng(8).standard_normal((M, wq.shape[0])).astype(np.float16)
    ref = v[:M] + (c0.astype(np.float64) if add else 0.0)
    got = _forward(dev, xq[:M], sx[:M], wq, sw, form | add, c0 if add else None).view(np.float16).astype(np.float64)
    ratio = np.abs(got - ref) / fc.bound(ref, absprod[:M], xq.shape[1])
    print(f"fp8 linear form={form} add={add}: worst error / bound = {ratio.max():.4f}")
    assert (ratio <= 1.0).all(), (ratio.max(), np.argwhere(ratio > 1.0)[:8])  # every element


def test_bits_do_not_depend_on_a_repeat_or_on_the_rows_beside(dev, random_case):
    xq, sx, wq, sw = random_case[:4]
    s16 = _forward(dev, xq[:16], sx[:16], wq, sw, SKINNY)
    assert np.array_equal(s16, _forward(dev, xq[:16], sx[:16], wq, sw, SKINNY))
    for m in (0, 5, 15):  # a row alone sits in lane row 0 of the operand, not in its own
        assert np.array_equal(_forward(dev, xq[m:m + 1], sx[m:m + 1], wq, sw, SKINNY)[0], s16[m])
    t257 = _forward(dev, xq, sx, wq, sw, TILED)
    assert np.array_equal(t257, _forward(dev, xq, sx, wq, sw, TILED))
    assert np.array_equal(_forward(dev, xq[:129], sx[:129], wq, sw, TILED), t257[:129])
    assert np.array_equal(_forward(dev, xq[:16], sx[:16], wq, sw, 0), s16) and np.array_equal(_forward(dev, xq[:17], sx[:17], wq, sw, 0), t257[:17])  # the dispatcher


def test_linear_half_fp8_is_the_two_launches(dev):
    from tinychatengine_amd.linear import Linear_half_fp8
    rng = np.random.default_rng(9)
    w, x = rng.standard_normal((48, 256)).astype(np.float16), rng.standard_normal((2, 9, 256)).astype(np.float16)
    xq, sx = fc.quantize_rows(x.reshape(18, 256))
    wq, sw = fc.quantize_rows(w)  # (a weight row is quantised by the activation rows' rule)
    lin16 = Linear_half_fp8.from_float(torch.from_numpy(w).to(dev))
    assert np.array_equal(lin16.weight.cpu().numpy(), wq) and np.array_equal(lin16.scale.cpu().numpy(), sw) and lin16.weight_bytes() == 48 * 256 + 4 * 48
    xt = torch.from_numpy(x).to(dev)
    y = lin16(xt)
    res = torch.from_numpy(rng.standard_normal((2, 9, 48)).astype(np.float16)).to(dev)
    c0 = res.cpu().numpy().reshape(18, 48)
    lin16.forward_add(xt, res)
    torch.cuda.synchronize()
    assert y.shape == (2, 9, 48) and np.array_equal(y.cpu().numpy().reshape(18, 48).view(np.uint16), _forward(dev, xq, sx, wq, sw, 0))
    assert np.array_equal(res.cpu().numpy().reshape(18, 48).view(np.uint16), _forward(dev, xq, sx, wq, sw, ADD, c0))
