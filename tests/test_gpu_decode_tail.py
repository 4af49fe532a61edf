"""The tail of the int8 decode kernel on the GPU (csrc/w4a16_gemv_i8.hip section 4: the waves' partial rows -> LDS -> wave 0's sum in wave order -> rounding,
epilogue, store; profiles/decode_tail/).  The tail reads exactly the partial rows of the WK waves that exist, chosen by scalar branches, and stores through an address
formed in front of the K reduction's barrier.  What can go wrong there is a wrong slot, a dropped or doubled wave, another order of the sum, a wrong row / member / element
at the store -- none of which an error tolerance is the right yardstick for: every check here is on BITS (`==` on int16 views), through tce_w4a16_forward / _group /
_independent on packed copies, with the dispatch asserted to be the int8 kernel.

  (a) slots: with the activations non-zero only inside one 1024-wide block of K, every other wave's partial row is +0 and the output is that wave's row alone -- it must
      equal, bit for bit, the output of a separately packed linear built from that block's columns (one wave, nothing to add).  For every block of K = 1024 x WK,
      WK = 1, 2, 3, 4, 5, 8, 14, 16, of K = 1152 (a ragged last wave) and of K = 20480 (sixteen units per wave: two blocks per wave).
  (b) order: dense seeded inputs against outputs recorded from the PARENT commit's library on an MI355X (tests/golden/decode_tail_parent.npz, written by
      scripts/decode_tail_record.py, which also defines the cases): the sum's order is unchanged, so no bit may move.
  (c) forms: every form of the body at its smallest shape -- M = 1 .. 4, groups 128 / 64 / 32, zero point 8 and general zero points, the plain / residual / SiLU-pair
      epilogues, two tiles per wave, sixteen units per wave, the NORM prologue, RNORM, a three-member group copy in and out of order, a mixed launch of two K, a
      row holding NaN -- against the same recording; and the NaN row is NaN in whole while its neighbour is finite.
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("decode_tail_record", os.path.join(REPO, "scripts", "decode_tail_record.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

GOLDEN = os.path.join(REPO, "tests", "golden", "decode_tail_parent.npz")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU (they must not silently pass without it)"
    from tinychatengine_amd import capi
    capi.lib()
    capi.set_gemv_config()
    capi.set_gemm_config()
    capi.set_gemv_i8()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("K", R.DENSE_K)
@pytest.mark.parametrize("N", R.DENSE_N)
def test_every_wave_lands_in_its_own_slot(dev, N, K):
    G = 128
    codes, scales, zp = R.arrays(N, K, G, seed=11 + N + K)
    big = R.linear(dev, codes, scales, zp, G).prepack()
    a = R.activations(1, K, seed=12 + K)
    assert (a != 0).all()
    blocks = (K + 1023) // 1024
    for b in range(blocks):
        lo, hi = 1024 * b, min(K, 1024 * (b + 1))
        xb = np.zeros_like(a)
        xb[:, lo:hi] = a[:, lo:hi]
        got = R.bits(R.forward(big, torch.from_numpy(xb).to(dev)))
        sub = R.linear(dev, codes[:, lo:hi], scales[:, lo // G:hi // G], zp[:, lo // G:hi // G], G).prepack()
        want = R.bits(R.forward(sub, torch.from_numpy(np.ascontiguousarray(a[:, lo:hi])).to(dev)))
        assert np.array_equal(got, want), f"N={N} K={K}: block {b} of {blocks} (columns {lo}..{hi - 1}) differs from its own K={hi - lo} linear in {int((got != want).sum())} of {N} outputs"
        assert np.any(want != 0), "a block whose outputs are all zero checks nothing"


@pytest.mark.parametrize("key", [k for k in R.CASES if k.startswith("dense")])
def test_dense_outputs_keep_the_parents_bits(dev, golden, key):
    got = R.run_case(dev, key)
    want = golden[key]
    assert got.shape == want.shape and np.array_equal(got, want), f"{key}: {int((got != want).sum())} of {got.size} outputs differ from the parent commit's"


@pytest.mark.parametrize("key", [k for k in R.CASES if k.startswith("form")])
def test_every_form_keeps_the_parents_bits(dev, golden, key):
    got = R.run_case(dev, key)
    want = golden[key]
    assert got.shape == want.shape and np.array_equal(got, want), f"{key}: {int((got != want).sum())} of {got.size} outputs differ from the parent commit's"
    h = got.view(np.float16)
    if key == "form NaN row":
        assert np.isnan(h[1]).all() and np.isfinite(h[0]).all(), "the row that holds a NaN is NaN in whole, its neighbour is untouched"
    else:
        assert np.isfinite(h).all(), f"{key}: an output is NaN / inf (an element that was not written stays NaN)"


def test_the_recording_covers_the_cases(golden):
    assert set(R.CASES) <= set(golden), sorted(set(R.CASES) - set(golden))
