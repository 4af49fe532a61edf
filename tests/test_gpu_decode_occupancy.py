"""The contraction of the int8 decode kernel with its B operand staged two units deep (csrc/w4a16_gemv_i8.hip section 3; profiles/decode_occupancy/): the plain forms
read the digit planes of a 128-k unit into a ring of two register sets, two units ahead of the MFMAs that consume them, and the lanes of the other units' columns read a
block of zeros -- 64 registers (72 with the RMSNorm prologue) where the parent needed 84, seven waves per SIMD where it ran five.  No floating-point operation moves and
the integer sums are exact, so the yardstick is BITS (`==` on int16 views), not a tolerance:

  (a) every case of scripts/decode_occupancy_record.py against tests/golden/decode_occupancy_parent.npz, recorded from the PARENT commit's library on an MI355X: one
      wave and two passes (K = 1024: the ring wraps once), ragged last waves with 1 and 7 live units (1152, 1920), four and fourteen K-waves (4096, 14336) at one and
      three tiles, rows that are no multiple of 16, zero point 8 and general zero points (their digit-sum MFMAs read the same sets), groups of 64 and 32, M = 2 and 4,
      the SiLU-pair and residual epilogues, the RMSNorm prologue, a two-member group copy -- on seeded normal activations and on DESIGNED ones: one huge entry among
      tiny ones per 1024-wide block and a block of zeros, where a lane that should hold zeros in a reused set and does not moves the sum by far more than a rounding;
  (b) residency: 16 x (7 x 256 + 8) rows at K = 4096 -- more four-wave workgroups than seven per CU, so registers and LDS of finished workgroups are reused by late
      ones -- run twice on one input: both runs identical, and the first and the last 64 rows identical to a launch of those rows alone (a row's bits depend on K and
      the group size only).
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("decode_occupancy_record", os.path.join(REPO, "scripts", "decode_occupancy_record.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)
T = R.T

GOLDEN = os.path.join(REPO, "tests", "golden", "decode_occupancy_parent.npz")


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


@pytest.mark.parametrize("key", list(R.CASES))
def test_every_case_keeps_the_parents_bits(dev, golden, key):
    got = R.run_case(dev, key)
    want = golden[key]
    assert got.shape == want.shape and np.array_equal(got, want), f"{key}: {int((got != want).sum())} of {got.size} outputs differ from the parent commit's"
    h = got.view(np.float16)
    assert np.isfinite(h).all(), f"{key}: an output is NaN / inf (an element that was not written stays NaN)"
    assert np.any(h != 0), "a case whose outputs are all zero checks nothing"


def test_the_recording_covers_the_cases(golden):
    assert set(R.CASES) <= set(golden), sorted(set(R.CASES) - set(golden))


def test_the_designed_activations_are_what_they_say():
    a = R.designed(2, 4096, seed=1, zero_block=2).astype(np.float64)
    for m in range(2):
        for b in range(4):
            blk = np.abs(a[m, 1024 * b:1024 * (b + 1)])
            if b == 2:
                assert not blk.any()
            else:
                assert (blk >= 256).sum() == 1 and np.sort(blk)[-2] < 2.0 ** -7 and blk.min() >= 2.0 ** -10


def test_more_workgroups_than_the_chip_holds_reuse_their_slots_cleanly(dev):
    K, G = 4096, 128
    N = 16 * (7 * 256 + 8)  # 1800 four-wave workgroups: more than seven per CU on 256 CUs
    from tinychatengine_amd import quantize
    from tinychatengine_amd.linear import Linear_half_int4
    rng = np.random.default_rng(77)
    # the q4_6 words drawn directly (code 8 i + e of a row is nibble e of its word i: uniform words are uniform codes) -- at 59 MB the detour over one byte per code
    # (decode_tail_record.linear) costs seconds
    qw = rng.integers(0, 2 ** 32, (N, K // 8), dtype=np.uint32)
    zw = quantize.calculate_zeros_width(K, G)
    scales = np.zeros((N, zw * 8), np.float16)
    scales[:, :K // G] = (rng.uniform(0.5, 1.5, (N, K // G)) * 0.01).astype(np.float16)
    zz = np.full((N, zw), 0x88888888, np.uint32)  # zero point 8 throughout

    def linear(lo, hi):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return Linear_half_int4(t(qw[lo:hi].view(np.int32)), t(scales[lo:hi]), t(zz[lo:hi].view(np.int32)), G).prepack()

    x = torch.from_numpy(R.designed(1, K, seed=78, zero_block=1)).to(dev)
    big = linear(0, N)
    first = T.bits(T.forward(big, x))
    second = T.bits(T.forward(big, x))
    assert first.shape == (1, N) and np.array_equal(first, second), f"two runs on one input differ in {int((first != second).sum())} of {N} outputs"
    for lo in (0, N - 64):
        sub = linear(lo, lo + 64)
        want = T.bits(T.forward(sub, x))
        got = first[:, lo:lo + 64]
        assert np.array_equal(got, want), f"rows {lo}..{lo + 63} of the {N}-row launch differ from a launch of those rows alone in {int((got != want).sum())} of 64 outputs"
        assert np.any(want != 0)
