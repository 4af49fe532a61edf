"""CPU (no GPU): the FP8 linears' host side (include/tce_matmul.h, "FP8 linears") -- the torch load-time quantiser against the numpy restatement of the definition
(tests/fp8_linear_cases.py), and every refusal of the two entry points, which happens before any HIP call and reads through no pointer."""
import ctypes as C

import numpy as np
import pytest

import fp8_linear_cases as fc

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def capi():
    from tinychatengine_amd import build as B
    B.build()
    from tinychatengine_amd import capi
    return capi


@pytest.mark.parametrize("inv", [1.0, 0.37, 448 / 65504, 448 * 2.0 ** 24])
def test_torch_bytes_are_the_definitions_for_every_binary16(inv):
    from tinychatengine_amd import quantize
    with np.errstate(invalid="ignore"):  # (the NaN patterns are inputs too)
        f = np.arange(65536, dtype=np.uint16).view(np.float16).astype(np.float32) * np.float32(inv)
    assert np.array_equal(quantize.e4m3_rne_sat(torch.from_numpy(f)).numpy(), fc.e4m3_rne_sat(f))


def test_channel_quantiser_is_the_row_rule():
    from tinychatengine_amd import quantize
    x = fc.quantiser_rows(384, np.random.default_rng(384))
    wq, sw = quantize.quantize_fp8_channel(torch.from_numpy(x))
    xq, sx = fc.quantize_rows(x)
    assert np.array_equal(wq.numpy(), xq) and np.array_equal(sw.numpy().view(np.uint32), sx.view(np.uint32))
    assert sx[1] == 1.0 and set(xq[1]) == {0x00, 0x80} and sx[5] == 1.0 and xq[5][5] == 0x7E and 0xFE in xq[3]  # the zero row, the tie row's 448, -65504


def _forward(L, p, ldq=256, ldc=48, M=4, N=48, K=256, flags=0, null=None, off=None):
    a = [C.c_void_p(None if null == i else p[i] + (off or {}).get(i, 0)) for i in range(5)]
    return L.tce_w8a8_fp8_forward_f16(a[0], ldq, a[1], a[2], a[3], a[4], ldc, M, N, K, flags, None)


def _quantize(L, p, ldx=256, ldq=256, rows=4, K=256, null=None, off=None):
    a = [C.c_void_p(None if null == i else p[i] + (off or {}).get(i, 0)) for i in range(3)]
    return L.tce_fp8_quantize_rows_f16(a[0], ldx, a[1], ldq, a[2], rows, K, None)


BAD, SHAPE = "TCE_ERR_BAD_ARG", "TCE_ERR_UNSUPPORTED_SHAPE"
REFUSALS = [(_forward, dict(null=i), BAD) for i in range(5)] + [(_quantize, dict(null=i), BAD) for i in range(3)] + [
    (_forward, dict(M=0), BAD), (_forward, dict(N=0), BAD), (_forward, dict(K=0), BAD), (_forward, dict(ldq=240), BAD), (_forward, dict(ldc=32), BAD),
    (_forward, dict(flags=1), BAD), (_forward, dict(flags=1024), BAD), (_forward, dict(flags=256 | 512), BAD),
    (_forward, dict(flags=256 | 512, K=100, ldq=112), BAD),  # arguments before shapes
    (_forward, dict(K=192, ldq=192), SHAPE), (_forward, dict(K=32896, ldq=32896), SHAPE), (_forward, dict(N=40), SHAPE), (_forward, dict(ldq=264), SHAPE),
    (_forward, dict(ldc=52), SHAPE), (_forward, dict(flags=256, M=17), SHAPE), (_forward, dict(M=65535 * 128 + 1), SHAPE),
    (_quantize, dict(rows=0), BAD), (_quantize, dict(K=0), BAD), (_quantize, dict(ldx=248), BAD), (_quantize, dict(ldq=240), BAD),
    (_quantize, dict(K=64, ldx=64, ldq=64), SHAPE), (_quantize, dict(ldx=260), SHAPE), (_quantize, dict(ldq=264), SHAPE),
] + [(_forward, dict(off={i: 8 if i != 1 else 2}), SHAPE) for i in range(5)] + [(_quantize, dict(off={i: 8 if i != 2 else 2}), SHAPE) for i in range(3)]


@pytest.mark.parametrize("call,kw,code", REFUSALS, ids=[f"{c.__name__}-{k}" for c, k, _ in REFUSALS])
def test_refusals_need_no_device_and_name_the_entry_point(capi, call, kw, code):
    L = capi.lib()
    p = [0x10000 * (i + 1) for i in range(5)]  # 16-byte aligned addresses of nothing: a refusal that read through one would fault here
    assert call(L, p, **kw) == getattr(capi, code), L.tce_last_error().decode()
    assert ("tce_fp8_quantize_rows_f16" if call is _quantize else "tce_w8a8_fp8_forward_f16") in L.tce_last_error().decode()


def test_python_front_refuses_wrong_operands():
    from tinychatengine_amd.linear import Linear_half_fp8
    with pytest.raises(ValueError):
        Linear_half_fp8(torch.zeros((16, 96), dtype=torch.uint8), torch.ones(16))
    with pytest.raises(ValueError):
        Linear_half_fp8(torch.zeros((16, 128), dtype=torch.int8), torch.ones(16))
    lin = Linear_half_fp8.from_float(torch.randn(16, 128))
    assert lin.weight_bytes() == 16 * 128 + 64 and lin.weight.dtype == torch.uint8
    with pytest.raises(ValueError):
        lin.quantize_rows(torch.zeros((2, 128), dtype=torch.float32))
