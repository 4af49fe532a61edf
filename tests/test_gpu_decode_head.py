"""GPU test of the decode kernel's flat, preloadable argument list (csrc/w4a16_gemv_i8.hip; profiles/decode_head/): linear 0 of a launch travels in the leading
parameters, linears 1.. of a grouped launch in the tail's batch and are chosen by scalar selects, the K-split width is an argument.  Every route must give the same bits:
one grouped launch, one launch per linear, and eight row shards of each linear (packed on their own: other N, other tile counts, the same row arithmetic) -- with a
ragged last tile (N % 16 != 0, whole and per shard), K = 14336 (14 waves, the widest K split of the token) beside K = 4096, every position of a group of four, and the
two-row form.  The plain launch is held to the oracle, so the three routes are not merely equal to each other."""
import numpy as np
import pytest

from conftest import w4a16_close

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU (they must not silently pass without it)"
    from tinychatengine_amd import capi
    capi.lib()
    capi.set_gemv_config()
    capi.set_gemm_config()
    capi.set_gemv_i8()
    return torch.device("cuda:0")


def _lin(oracle, dev, N, K, seed):
    from tinychatengine_amd.linear import Linear_half_int4
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((N, K)) * 0.02).astype(np.float32)
    qw, sc, zp, _, _ = oracle.quantize_q4_6(w, 128)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return Linear_half_int4(t(qw.view(np.int32)), t(sc.view(np.float16)), t(zp.view(np.int32)), 128).prepack(), (qw, sc, zp)


def _row_shard(lin, r, world):
    """rows [r N / world, (r + 1) N / world) as a linear of its own (Linear_half_int4.shard keeps to multiples of 16 rows; here the shards' last tiles are ragged too)"""
    from tinychatengine_amd.linear import Linear_half_int4
    n = lin.out_features
    assert n % world == 0
    lo, hi = r * (n // world), (r + 1) * (n // world)
    return Linear_half_int4(lin.weight[lo:hi].contiguous(), lin.scale[lo:hi].contiguous(), lin.zero_point[lo:hi].contiguous(), lin.group_size).prepack()


def _fwd(lin, x):
    from tinychatengine_amd import capi
    out = torch.full((x.shape[0], lin.out_features), float("nan"), dtype=torch.float16, device=x.device)
    d = lin.desc(x, out)
    assert capi.describe_dispatch(d).startswith("gemv-i8"), capi.describe_dispatch(d)
    capi.check(capi.w4a16_forward(d, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("M,K,Ns", [(1, 14336, [4096, 264, 1000, 72]), (1, 4096, [264, 4096, 1000]), (1, 4096, [1000, 520]), (2, 14336, [264, 1000]), (1, 11008, [520, 40, 264, 2048])])
def test_grouped_per_linear_and_row_shards_agree_bit_for_bit(dev, oracle, M, K, Ns):
    from tinychatengine_amd.linear import forward_group
    made = [_lin(oracle, dev, n, K, seed=7 * n + K + i) for i, n in enumerate(Ns)]
    lins = [m[0] for m in made]
    x = torch.randn((M, K), device=dev).to(torch.float16)
    singles = [_fwd(l, x) for l in lins]
    for l, (qw, sc, zp), got in zip(lins, (m[1] for m in made), singles):
        ref32, _ = oracle.w4a16_gemv_q4_6(x.cpu().numpy(), qw, sc, zp, M, l.out_features, K, 128)
        g = got.cpu().numpy()
        assert not np.isnan(g.astype(np.float32)).any(), f"N={l.out_features}: unwritten outputs"
        ok, worst = w4a16_close(g, ref32)
        assert ok, f"N={l.out_features} K={K}: worst |err|/tol = {worst:.3f}"
    # one grouped launch, in the given order and reversed (every linear in the leading parameters once, in the tail's batch once)
    for order in (list(range(len(lins))), list(range(len(lins)))[::-1]):
        outs = [torch.full((M, lins[i].out_features), float("nan"), dtype=torch.float16, device=dev) for i in order]
        forward_group([lins[i] for i in order], x, outs)
        torch.cuda.synchronize()
        for i, o in zip(order, outs):
            assert torch.equal(o.view(torch.int16), singles[i].view(torch.int16)), f"grouped launch, order {order}: linear N={lins[i].out_features} differs from its own launch"
    # eight row shards of every linear, each packed on its own
    for l, full in zip(lins, singles):
        parts = [_fwd(_row_shard(l, r, 8), x) for r in range(8)]
        assert torch.equal(torch.cat(parts, dim=1).view(torch.int16), full.view(torch.int16)), f"N={l.out_features} K={K}: the 8 row shards differ from the whole"
