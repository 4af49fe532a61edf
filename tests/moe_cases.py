"""Operands of test_gpu_moe.py, numpy only.  K = 128: one k-block, seven waves without work; 1408: eleven, an uneven split.  N = 48: whole tiles; 40: a ragged last
tile.  Experts with 0, 1, 16 and 17 pairs: the early exit, a single MFMA column, a full pass, the pass edge."""
import numpy as np

KS = (128, 1408)
EK = ((4, 1), (8, 2), (64, 8))
STAGES = [(K, N, E, k) for K, N in ((128, 48), (1408, 40)) for E, k in EK]  # every K, N and (E, k); the products K x N x (E, k) would add no path


def stacked(E, N, K, seed):
    """stacked q4_6 arrays: random codes, GENERAL zero points, scales sized for dot products with N(0, 1) rows of deviation ~1.5 (|gate| < 8 is asserted by the test)"""
    rng, ng, zw = np.random.default_rng(seed), K // 128, (K // 128 + 7) // 8
    pack = lambda nibbles: (nibbles.astype(np.uint32) << (np.arange(8, dtype=np.uint32) * 4)).sum(-1, dtype=np.uint32).view(np.int32)
    qweight, scales, z = pack(rng.integers(0, 16, (E, N, K // 8, 8))), np.zeros((E, N, zw * 8), np.float16), np.zeros((E, N, zw * 8), np.uint32)
    scales[..., :ng] = rng.uniform(0.5, 1.5, (E, N, ng)) * 1.5 / (6.5 * np.sqrt(K))
    z[..., :ng] = rng.integers(0, 16, (E, N, ng))
    return qweight, scales, pack(z.reshape(E, N, zw, 8))


def designed_ids(E, k, rows=20):
    """ids [rows][k]: expert 0 gets no pair, 1 one, 2 sixteen, 3 seventeen, the rest are dealt over the other experts; ONE word is then put out of range"""
    if k == 1:
        ids = np.array([1] + [2] * 16 + [3] * 17 + [3], np.int32).reshape(-1, 1)
    else:
        rest = rows * k - 34
        flat = np.sort(np.concatenate([[1], [2] * 16, [3] * 17, 4 + np.arange(rest) % (E - 4)]).astype(np.int32))
        ids = flat.reshape(k, rows).T.copy()  # column-major dealing: a row's k words are `rows` apart in the sorted order, so they differ
    bad = np.argwhere(ids == ids.max())[-1]
    ids[tuple(bad)] = E if k > 1 else -3
    return ids


def route_exact(K, E, k, rows=32, seed=3):
    """small integers: every fp32 partial sum is an integer below 2^24 in any order.  Experts 1 and E - 1 repeat expert 0's and E - 2's router rows: planted ties"""
    rng = np.random.default_rng(seed + K + E)
    x = rng.integers(-4, 5, (rows, K)).astype(np.float16)
    Wr = rng.integers(-4, 5, (E, K)).astype(np.float16)
    Wr[1], Wr[E - 1] = Wr[0], Wr[E - 2]
    assert (np.abs(x.astype(np.float64)) @ np.abs(Wr.astype(np.float64)).T).max() < 2 ** 24
    return x, Wr


def route_bounded(K, E, k, rows=24, seed=5):
    """Gaussian x whose first 16 columns are 1; Wr = small noise, with 16 columns of a_e = perm(e) / 32: logits 0.5 apart plus noise of deviation ~0.002 sqrt(K)"""
    rng = np.random.default_rng(seed + K + E)
    x = rng.normal(0, 1, (rows, K)).astype(np.float16)
    x[:, :16] = 1
    Wr = rng.normal(0, 0.002, (E, K)).astype(np.float16)
    Wr[:, :16] = (rng.permutation(E) / 32)[:, None]
    return x, Wr


def logit_error(x, Wr):
    """float64 [rows]: (K + 2) 2^-24 max_e sum_k |x_k Wr[e][k]| -- an fp32 sum of K exact products in ANY order, each partial sum rounded once"""
    return (x.shape[1] + 2) * 2.0 ** -24 * (np.abs(x.astype(np.float64)) @ np.abs(Wr.astype(np.float64)).T).max(axis=1)


def w4_tol(ref):
    """conftest.w4a16_close's per-element tolerance, per row of ref"""
    ref = np.asarray(ref, np.float64)
    return 1e-3 * np.maximum(np.abs(ref), np.sqrt(np.mean(ref * ref, axis=-1, keepdims=True)) / 64.0)


def act_bound(g, u):
    """|act - silu(g) u|: the chain's six fp16 roundings plus the input's, 8 * 2^-11 |ref|, and the projections' tolerances to first order (sup |silu'| < 1.1)"""
    silu = g / (1.0 + np.exp(-g))
    return 8 * 2.0 ** -11 * np.abs(silu * u) + 1.1 * np.abs(u) * w4_tol(g) + np.abs(silu) * w4_tol(u)


def weight_rel_bound(d, spread, E, k, renorm):
    """relative error of a routing weight through expm1: exp's argument is off by 2 d (both logits) plus its rounding 2^-24 spread, exp is within 1 ulp (2^-23), in
    the numerator and in every term of the denominator; the E-term sum adds (E - 1) 2^-24, the quotient 2^-24; renormalising divides two such numbers over a k-term sum"""
    one = 2 * (2 * d + 2.0 ** -24 * spread) + (E + 4) * 2.0 ** -24
    return np.expm1(2 * one + k * 2.0 ** -24 if renorm else one)
