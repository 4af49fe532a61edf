#!/usr/bin/env python3
"""The decode kernel's outputs on designed, seeded inputs, as bits -- the cases of tests/test_gpu_decode_tail.py (b) and (c) -- recorded from ONE build of the library:

    TCE_LIB_PATH=<the parent commit's libtce_hip.so> python scripts/decode_tail_record.py --out tests/golden/decode_tail_parent.npz

The decode-tail change (csrc/w4a16_gemv_i8.hip section 4; profiles/decode_tail/) reshapes how wave 0 adds the waves' partial rows and stores; the order of every
floating-point operation stays, so every output bit must stay.  The committed recording is the parent commit's library on an MI355X; the test runs the same cases on the
tree's build and compares int16 views.  Inputs come from numpy generators seeded per case (codes, scales, zero points and activations drawn directly: no quantiser in
between), so any machine forms the same bytes.  The test imports CASES / run_case from this file.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

# (b) dense inputs: N = one tile, a ragged tile, three tiles; K = 1024 x WK for WK waves, a ragged last wave (1152), sixteen units per wave (20480)
DENSE_N = (16, 24, 48)
DENSE_K = tuple(1024 * wk for wk in (1, 2, 3, 4, 5, 8, 14, 16)) + (1152, 20480)


def arrays(N, K, G, seed, general_zeros=False):
    """codes uint8 [N][K], scales fp16 [N][K / G], zero points uint8 [N][K / G] of one linear"""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 16, (N, K), dtype=np.uint8)
    scales = (rng.uniform(0.5, 1.5, (N, K // G)) * 0.01).astype(np.float16)
    zp = rng.integers(0, 16, (N, K // G), dtype=np.uint8) if general_zeros else np.full((N, K // G), 8, np.uint8)
    return codes, scales, zp


def linear(dev, codes, scales, zp, G):
    """the q4_6 arrays of (codes, scales, zero points) as a Linear_half_int4 with a packed copy of its own"""
    from tinychatengine_amd import quantize
    from tinychatengine_amd.linear import Linear_half_int4
    N, K = codes.shape
    zw = quantize.calculate_zeros_width(K, G)
    sh = np.arange(8, dtype=np.uint64) * 4
    qw = (codes.reshape(N, K // 8, 8).astype(np.uint64) << sh).sum(axis=2).astype(np.uint32)
    sc = np.zeros((N, zw * 8), np.float16)
    sc[:, : K // G] = scales
    zn = np.full((N, zw * 8), 8, np.uint8)
    zn[:, : K // G] = zp
    zz = (zn.reshape(N, zw, 8).astype(np.uint64) << sh).sum(axis=2).astype(np.uint32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return Linear_half_int4(t(qw.view(np.int32)), t(sc), t(zz.view(np.int32)), G)


def activations(M, K, seed):
    return np.random.default_rng(seed).standard_normal((M, K)).astype(np.float16)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().copy()


def forward(lin, x, flags=0, out=None, gamma=None, eps=0.0):
    """tce_w4a16_forward on the packed copy; the dispatch must be the int8 decode kernel"""
    from tinychatengine_amd import capi
    n_out = lin.out_features // 2 if flags & capi.TCE_W4_SILU_MUL_PAIRS else lin.out_features
    if out is None:
        out = torch.full((x.shape[0], n_out), float("nan"), dtype=torch.float16, device=x.device)
    d = lin.desc(x, out, flags=flags, gamma=gamma, eps=eps)
    assert capi.describe_dispatch(d).startswith("gemv-i8"), capi.describe_dispatch(d)
    capi.check(capi.w4a16_forward(d, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out


def forward_group(lins, x, outs, flags=0):
    from tinychatengine_amd import capi
    descs = [l.desc(x, o, flags=flags) for l, o in zip(lins, outs)]
    for d in descs:
        assert capi.describe_dispatch(d).startswith("gemv-i8"), capi.describe_dispatch(d)
    capi.check(capi.w4a16_forward_group(descs, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()


def _dense(N, K):
    def run(dev):
        lin = linear(dev, *arrays(N, K, 128, seed=1000 + N * 7 + K), 128).prepack()
        return bits(forward(lin, torch.from_numpy(activations(1, K, seed=2000 + N + K)).to(dev)))
    return run


def _form(M, N, K, G, general_zeros=False, flags=0, tiles=0, norm=False, nan_row=None):
    def run(dev):
        from tinychatengine_amd import capi
        lin = linear(dev, *arrays(N, K, G, seed=3000 + M + N + K + G, general_zeros=general_zeros), G).prepack()
        a = activations(M, K, seed=4000 + M + K)
        if nan_row is not None:
            a[nan_row, K // 3] = np.nan
        x = torch.from_numpy(a).to(dev)
        out = None
        if flags & capi.TCE_W4_ADD_TO_C:
            out = torch.from_numpy(activations(M, N, seed=5000 + N)).to(dev)
        gamma = torch.from_numpy(np.random.default_rng(6000 + K).uniform(0.8, 1.2, K).astype(np.float32)).to(dev) if norm else None
        try:
            capi.set_gemv_i8(0, tiles)
            return bits(forward(lin, x, flags=flags, out=out, gamma=gamma, eps=1e-6))
        finally:
            capi.set_gemv_i8()
    return run


def _rnorm(N, K, general_zeros=False):
    def run(dev):
        from tinychatengine_amd import capi
        lin = linear(dev, *arrays(N, K, 128, seed=7000 + N + K, general_zeros=general_zeros), 128).prepack()
        x = torch.from_numpy(activations(1, K, seed=7100 + K)).to(dev)
        c = torch.from_numpy(activations(1, N, seed=7200 + N)).to(dev)
        gamma = torch.from_numpy(np.random.default_rng(7300 + N).uniform(0.8, 1.2, N).astype(np.float32)).to(dev)
        xn = torch.full((1, N), float("nan"), dtype=torch.float16, device=dev)
        ws = torch.zeros(int(capi.lib().tce_w4a16_residual_rmsnorm_workspace_bytes()), dtype=torch.uint8, device=dev)
        capi.check(capi.w4a16_forward_residual_rmsnorm(lin.desc(x, c, flags=capi.TCE_W4_ADD_TO_C), gamma.data_ptr(), 1e-6, xn.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return np.concatenate([bits(c), bits(xn)])
    return run


def _group_copy(order, pairs=False):
    """three members of ONE group copy (16, 32 and 16 rows), launched together in `order` (0 1 2: the copy's order -- one linear of all rows; else through each member's own fields)"""
    def run(dev):
        from tinychatengine_amd import capi
        from tinychatengine_amd.linear import Linear_half_int4
        K = 1024
        lins = [linear(dev, *arrays(n, K, 128, seed=8000 + i), 128) for i, n in enumerate((16, 32, 16))]
        if not Linear_half_int4.prepack_group(lins):
            assert not capi.HAS_GROUP_COPIES  # (a library from before the group copies packs every member on its own: same bits)
        x = torch.from_numpy(activations(1, K, seed=8100)).to(dev)
        flags = capi.TCE_W4_SILU_MUL_PAIRS if pairs else 0
        outs = [torch.full((1, l.out_features // 2 if pairs else l.out_features), float("nan"), dtype=torch.float16, device=dev) for l in lins]
        forward_group([lins[i] for i in order], x, [outs[i] for i in order], flags=flags)
        return np.concatenate([bits(o) for o in outs], axis=1)
    return run


def _mixed(dev):
    """two linears that share nothing -- K = 1024 and K = 3072 -- as one launch (tce_w4a16_forward_independent)"""
    from tinychatengine_amd import capi
    shapes = ((24, 1024), (48, 3072))
    lins = [linear(dev, *arrays(n, k, 128, seed=9000 + k), 128).prepack() for n, k in shapes]
    xs = [torch.from_numpy(activations(1, k, seed=9100 + k)).to(dev) for _, k in shapes]
    outs = [torch.full((1, n), float("nan"), dtype=torch.float16, device=dev) for n, _ in shapes]
    descs = [l.desc(x, o) for l, x, o in zip(lins, xs, outs)]
    assert capi.describe_independent(descs).startswith("gemv-i8"), capi.describe_independent(descs)
    assert capi.w4a16_forward_independent(descs, torch.cuda.current_stream().cuda_stream) == 1
    torch.cuda.synchronize()
    return np.concatenate([bits(o) for o in outs], axis=1)


ADD, PAIRS = 16, 8  # TCE_W4_ADD_TO_C, TCE_W4_SILU_MUL_PAIRS (include/tce_matmul.h)
CASES = {f"dense N={N} K={K}": _dense(N, K) for N in DENSE_N for K in DENSE_K}
CASES.update({
    # (c) every form of the body at its smallest shape (N = 24: a ragged tile behind a whole one)
    "form M=1": _form(1, 24, 1024, 128),
    "form M=2": _form(2, 24, 1024, 128),
    "form M=3 (four rows per pass, one masked)": _form(3, 24, 1024, 128),
    "form M=4": _form(4, 24, 1024, 128),
    "form group 64": _form(1, 24, 1024, 64),
    "form M=2 group 64": _form(2, 24, 1024, 64),
    "form group 32": _form(1, 24, 1024, 32),
    "form general zero points": _form(1, 24, 1024, 128, general_zeros=True),
    "form M=4 general zero points": _form(4, 24, 1024, 128, general_zeros=True),
    "form M=2 group 64 general zero points": _form(2, 24, 1024, 64, general_zeros=True),
    "form group 32 general zero points": _form(1, 24, 1024, 32, general_zeros=True),
    "form residual add": _form(1, 24, 1024, 128, flags=ADD),
    "form M=2 residual add": _form(2, 24, 2048, 128, flags=ADD),
    "form SiLU pairs": _form(1, 24, 1024, 128, flags=PAIRS),
    "form M=4 SiLU pairs": _form(4, 40, 1024, 128, flags=PAIRS),
    "form two tiles per wave": _form(1, 48, 2048, 128, tiles=2),
    "form two tiles per wave, residual add": _form(1, 40, 1024, 128, tiles=2, flags=ADD),
    "form two tiles per wave, SiLU pairs": _form(1, 72, 1024, 128, tiles=2, flags=PAIRS),
    "form sixteen units per wave, general zero points": _form(1, 24, 18432, 128, general_zeros=True),
    "form NORM": _form(1, 24, 1024, 128, norm=True),
    "form NORM two tiles per wave": _form(1, 48, 2048, 128, norm=True, tiles=2),
    "form NORM SiLU pairs": _form(1, 24, 1024, 128, norm=True, flags=PAIRS),
    "form RNORM": _rnorm(24, 1024),
    "form RNORM general zero points": _rnorm(40, 5120, general_zeros=True),
    "form group copy in order": _group_copy((0, 1, 2)),
    "form group copy out of order": _group_copy((2, 0, 1)),
    "form group copy in order, SiLU pairs": _group_copy((0, 1, 2), pairs=True),
    "form mixed launch": _mixed,
    "form NaN row": _form(2, 24, 1024, 128, nan_row=1),
})


def run_case(dev, key):
    from tinychatengine_amd import capi
    capi.lib()
    capi.set_gemv_config()
    capi.set_gemm_config()
    capi.set_gemv_i8()
    return CASES[key](dev)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    from tinychatengine_amd import capi
    assert torch.cuda.is_available(), "the recording is made on the GPU"
    dev = torch.device("cuda:0")
    rec = {k: run_case(dev, k) for k in CASES}
    meta = {"library": os.path.basename(capi.LIB_PATH), "cases": len(rec), "what": "int16 views of the fp16 outputs of scripts/decode_tail_record.py's cases"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, __meta__=np.array(json.dumps(meta)), **rec)
    print(json.dumps({**meta, "out": a.out, "bytes": os.path.getsize(a.out)}))
