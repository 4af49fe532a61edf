"""The end of the fp16 GEMV kernels' LDS allocations (run with -m gpu on an MI355X; -s prints the worst ratio per launch).

The row-block GEMV (csrc/w4a16_gemv.hip) allocates its x image and, right behind it, one 16-byte trash slot per thread -- the last bytes of the allocation; with the
fused RMSNorm prologue the first 4 KiB of the slots are the 1024 partial sums.  The stream kernel (csrc/w4a16_gemv_stream.hip) allocates its x image, the ticket
words and the RMSNorm partials.  An LDS access past an allocation fails silently, so these launches are built to reach the last slots and are judged by value:

  * N = 64, groups of 32, `gauss x random` of tests/w4a16_cases.py (general zero points), M = 1, 2, 4;
  * K = 32 -- one chunk: every thread but one writes a surplus piece into its trash slot --, and per geometry the smallest K whose image needs a second batch of x
    pieces (second_batch_k: 4128 ... 32800, none a multiple of 2048: the last batch is ragged and its surplus lands in the slots too);
  * every compiled row-block geometry forced, with and without the prologue (the prologue is a decode feature: M = 1);
  * the stream kernel on the same rule, and at its last admitted step count (T = 18, K = 36832) and one step past it (K = 36896), where describe_dispatch must name the
    row-block kernel.

Judged by w4a16_cases.judge (conftest.w4a16_close, unchanged) against float64 on the stored values; with the prologue the stored activations are what the stand-alone
RMSNorm kernel writes (tests/test_gpu_epilogues.py holds the two forms to identical bits).  The oracle's own sequential fp32 sum must stay within 0.6 of the bound on
every draw used here (asserted where the cases are built; measured on the host: 0.38 - 0.46, the rounding of the outputs to
binary16 alone being up to 0.49).
"""
import functools

import numpy as np
import pytest

import w4a16_cases as wc

torch = pytest.importorskip("torch")

N, G = 64, 32
ORACLE_BOUND = 0.6  # (tests/test_w4a16_adversarial_host.py's)
STREAM_CFGS = ((2, 16, 2), (1, 16, 3), (2, 4, 2))  # (rows per row group, waves, depth)
K_LAST_ADMITTED, K_PAST = 36832, 36896  # 1151 / 1153 chunks of 32: 18 / 19 steps of 64 lanes


def second_batch_k(wn, wk, mb, norm):
    """The smallest K at which a workgroup of 64 * wn * wk threads cannot stage the x image of mb rows in one batch: a batch is 8 pieces per thread (2 with the
    prologue), the image mb * T * 64 * wk * 4 pieces, T steps of 64 * wk chunks of 32."""
    t = (2 if norm else 8) * wn // (4 * mb) + 1
    return 32 * ((t - 1) * 64 * wk + 1)


def stream_second_batch_k(nw):
    """The stream kernel holds 4 pieces per thread across its weight prologue; its image is T * 256 pieces."""
    return 32 * (nw * 64 + 1)


@functools.lru_cache(maxsize=None)
def case_of(M, K):
    """One seeded draw per (M, K), shared by every launch on it; the oracle is held to its bound on it before any kernel is."""
    case = wc.make_case("gauss x random", M, N, K, G)
    _, c16 = _oracle().w4a16_gemv_q4_6(case.a, case.qw, case.sc, case.zp, M, N, K, G)
    r = wc.judge(case, np.asarray(c16, np.float16).reshape(M, N))
    assert r <= ORACLE_BOUND, f"M={M} K={K}: the oracle itself is at {r:.3f} of the bound"
    return case


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oracle import Oracle
    return Oracle()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU (they must not silently pass without it)"
    from tinychatengine_amd import capi
    capi.lib()
    capi.set_gemv_config()
    capi.set_gemv_i8()
    return torch.device("cuda:0")


def _linear(dev, case):
    from tinychatengine_amd.linear import Linear_half_int4
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    lin = Linear_half_int4(t(case.qw.view(np.int32)), t(case.sc), t(case.zp.view(np.int32)), case.G)
    lin.zeros_are_8 = False  # the zero points are read
    return lin


def _launch(dev, case, cfg, kernel, norm):
    """One forced launch on a NaN-filled output -> the worst ratio of wc.judge.  norm: the hidden state is case.a, the kernel stages RMSNorm(a) * gamma."""
    from tinychatengine_amd import capi
    from tinychatengine_amd.linear import forward_group, forward_group_rmsnorm, rmsnorm_half
    lin = _linear(dev, case)
    x = torch.from_numpy(case.a).to(dev)
    out = torch.full((case.M, N), float("nan"), dtype=torch.float16, device=dev)
    try:
        capi.set_gemv_config(*cfg)
        what = capi.describe_dispatch(lin.desc(x, out, flags=capi.TCE_W4_FORCE_GEMV))
        assert what == f"gemv passes={(case.M + 3) // 4} kernel={kernel}", (cfg, case.K, what)
        if norm:
            gamma = torch.from_numpy(1.0 + 0.2 * np.random.default_rng(case.K).standard_normal(case.K).astype(np.float32)).to(dev)
            forward_group_rmsnorm([lin], x, [out], gamma, 1e-6)
        else:
            forward_group([lin], x, [out])
        torch.cuda.synchronize()
    finally:
        capi.set_gemv_config()
    if norm:  # the float64 reference on the activations the prologue stages
        xn = rmsnorm_half(x, gamma, 1e-6).cpu().numpy()
        assert np.isfinite(xn.astype(np.float32)).all()
        case = wc.Case(case.name, xn, case.codes, case.z, case.s, case.G, case.sets)
        _, c16 = _oracle().w4a16_gemv_q4_6(xn, case.qw, case.sc, case.zp, 1, N, case.K, G)
        assert wc.judge(case, np.asarray(c16, np.float16).reshape(1, N)) <= ORACLE_BOUND
    return wc.judge(case, out.cpu().numpy())


def _row_block(dev, M, norm):
    from tinychatengine_amd import capi
    ran, worst = 0, []
    for v in capi.gemv_variants():
        rows, wn, wk, depth = v
        for K in (32, second_batch_k(wn, wk, M, norm)):
            try:
                r = _launch(dev, case_of(M, K), v, "row-block", norm)
            except capi.TceError as e:
                # one step (K = 32) under a geometry whose shallower pipelines are not compiled: refused loudly, nothing ran.  Never at the longer K.
                assert K == 32 and depth > 1 and (e.code == capi.TCE_ERR_UNSUPPORTED_SHAPE or "no kernel variant for this shape" in str(e)), (v, K, str(e))
                continue
            ran += 1
            worst.append((r, v, K))
            print(f"    row-block {v} M={M} K={K:6d} norm={norm}: {r:.3f}")
    assert ran >= 2 * len(capi.gemv_variants()) - 2, f"only {ran} launches ran"
    bad = [w for w in worst if not w[0] <= 1.0]
    assert not bad, f"worst |err| / bound past 1.0: {bad}"


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 2, 4])
def test_row_block_trash_slots(dev, M):
    _row_block(dev, M, norm=False)


@pytest.mark.gpu
def test_row_block_partials_in_the_trash_slots(dev):
    """The fused RMSNorm prologue: part[] is the first 4 KiB of the trash slots, the last thing in the allocation."""
    _row_block(dev, 1, norm=True)


@pytest.mark.gpu
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "rmsnorm"])
def test_stream_kernel_tail_and_gate(dev, norm):
    """Ticket words and RMSNorm partials sit right behind the image; 18 steps are the last the kernel admits, the launch one step past it is the row-block kernel's."""
    bad = []
    for cfg in STREAM_CFGS:
        for K in (32, stream_second_batch_k(cfg[1]), K_LAST_ADMITTED):
            r = _launch(dev, case_of(1, K), (cfg[0], cfg[1], 0, cfg[2]), "persistent", norm)
            print(f"    stream {cfg} K={K:6d} norm={norm}: {r:.3f}")
            if not r <= 1.0:
                bad.append((r, cfg, K))
    r = _launch(dev, case_of(1, K_PAST), (STREAM_CFGS[0][0], STREAM_CFGS[0][1], 0, STREAM_CFGS[0][2]), "row-block", norm)
    print(f"    stream config forced, K={K_PAST} (19 steps): the row-block kernel, {r:.3f}")
    assert not bad and r <= 1.0, (bad, r)
