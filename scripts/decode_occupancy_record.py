#!/usr/bin/env python3
"""The decode kernel's outputs, as bits, on the shapes where the staging of the contraction's B operand can go wrong -- the cases of tests/test_gpu_decode_occupancy.py --
recorded from ONE build of the library:

    TCE_LIB_PATH=<the parent commit's libtce_hip.so> python scripts/decode_occupancy_record.py --out tests/golden/decode_occupancy_parent.npz

The occupancy change (csrc/w4a16_gemv_i8.hip section 3; profiles/decode_occupancy/) stages the digit planes of a 128-k unit two units ahead of the MFMAs that consume
them, in a ring of two register sets, where the parent held a whole pass of four.  No floating-point operation moves and the integer sums are exact, so every output bit
must stay.  The committed recording is the parent commit's library on an MI355X; the test runs the same cases on the tree's build and compares int16 views.  Inputs come
from numpy generators seeded per case (scripts/decode_tail_record.py's arrays / linear / activations: no quantiser in between), so any machine forms the same bytes.
The test imports CASES / run_case from this file.

What a wrong ring would show on: a register set of the ring must hold zeros in the lanes of the other units' columns.  A stale set adds (another unit's planes) x (this
unit's weights) to the column's integer sum -- so the activations here are also DESIGNED: per 1024-wide block one huge entry among tiny ones (the tiny ones live in the
lowest digit plane only, the huge one in the highest: a stale plane of either moves the sum by far more than a rounding), and a block of zeros (planes that must
contribute nothing).
"""
import argparse
import importlib.util
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch

_spec = importlib.util.spec_from_file_location("decode_tail_record", os.path.join(REPO, "scripts", "decode_tail_record.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)

ADD, PAIRS = T.ADD, T.PAIRS


def designed(M, K, seed, zero_block=None):
    """per 1024-wide block of every row: one entry of magnitude 256 .. 1024 at a seeded place, every other entry of magnitude 2^-10 .. 2^-8 (exactly representable below
    the block's exponent: within 2^19 of the maximum); block `zero_block` (None: none) is zeros in whole"""
    rng = np.random.default_rng(seed)
    a = (rng.uniform(1.0, 4.0, (M, K)) * 2.0 ** -10 * rng.choice([-1.0, 1.0], (M, K))).astype(np.float16)
    for m in range(M):
        for b in range((K + 1023) // 1024):
            lo, hi = 1024 * b, min(K, 1024 * (b + 1))
            a[m, lo + int(rng.integers(0, hi - lo))] = np.float16(rng.uniform(256.0, 1024.0) * rng.choice([-1.0, 1.0]))
            if zero_block is not None and b == zero_block:
                a[m, lo:hi] = 0
    return a


def _case(M, N, K, G=128, general_zeros=False, flags=0, norm=False, act="normal", zero_block=None):
    def run(dev):
        from tinychatengine_amd import capi
        lin = T.linear(dev, *T.arrays(N, K, G, seed=31000 + 13 * M + 7 * N + K + G, general_zeros=general_zeros), G).prepack()
        a = T.activations(M, K, seed=32000 + M + K) if act == "normal" else designed(M, K, seed=33000 + M + K, zero_block=zero_block)
        x = torch.from_numpy(a).to(dev)
        out = torch.from_numpy(T.activations(M, N, seed=34000 + N)).to(dev) if flags & capi.TCE_W4_ADD_TO_C else None
        gamma = torch.from_numpy(np.random.default_rng(35000 + K).uniform(0.8, 1.2, K).astype(np.float32)).to(dev) if norm else None
        return T.bits(T.forward(lin, x, flags=flags, out=out, gamma=gamma, eps=1e-6))
    return run


def _group_copy(K, pairs=False, act="normal"):
    """two members of ONE group copy (32 and 16 rows) launched together in the copy's order: one linear of all 48 rows"""
    def run(dev):
        from tinychatengine_amd import capi
        from tinychatengine_amd.linear import Linear_half_int4
        lins = [T.linear(dev, *T.arrays(n, K, 128, seed=36000 + K + i), 128) for i, n in enumerate((32, 16))]
        if not Linear_half_int4.prepack_group(lins):
            assert not capi.HAS_GROUP_COPIES
        a = T.activations(1, K, seed=36100 + K) if act == "normal" else designed(1, K, seed=36200 + K, zero_block=1)
        x = torch.from_numpy(a).to(dev)
        flags = PAIRS if pairs else 0
        outs = [torch.full((1, l.out_features // 2 if pairs else l.out_features), float("nan"), dtype=torch.float16, device=dev) for l in lins]
        T.forward_group(lins, x, outs, flags=flags)
        return np.concatenate([T.bits(o) for o in outs], axis=1)
    return run


CASES = {}
# one wave, two passes: the ring wraps exactly once (1024); a ragged last wave with 1 and 7 live units (1152, 1920: the missing units read the empty descriptor);
# four and fourteen K-waves, every wave's slot (4096, 14336)
for K in (1024, 1152, 1920, 4096, 14336):
    for N in (16, 48):
        for gz in (False, True):
            CASES[f"K={K} N={N}{' general zero points' if gz else ''}"] = _case(1, N, K, general_zeros=gz)
            CASES[f"designed K={K} N={N}{' general zero points' if gz else ''}"] = _case(1, N, K, general_zeros=gz, act="designed", zero_block=(K // 1024) // 2 if K > 1024 else None)  # (one block: nothing would be left)
CASES.update({
    # N not a multiple of 16: the surplus rows of the last tile are masked at the store
    "N=24 K=1152": _case(1, 24, 1152),
    "N=40 K=4096 general zero points": _case(1, 40, 4096, general_zeros=True),
    "N=17 K=1920 designed": _case(1, 17, 1920, act="designed", zero_block=0),
    # the other forms of the body (their staging is the parent's: two sets or one per pass)
    "group 64 K=1152": _case(1, 24, 1152, G=64),
    "group 64 K=4096 general zero points designed": _case(1, 16, 4096, G=64, general_zeros=True, act="designed", zero_block=1),
    "group 32 K=1920": _case(1, 24, 1920, G=32),
    "group 32 K=1024 general zero points designed": _case(1, 16, 1024, G=32, general_zeros=True, act="designed"),
    "M=2 K=1920": _case(2, 24, 1920),
    "M=2 K=4096 general zero points designed": _case(2, 16, 4096, general_zeros=True, act="designed", zero_block=2),
    "M=4 K=1152": _case(4, 24, 1152),
    "M=4 K=4096 designed": _case(4, 16, 4096, act="designed", zero_block=3),
    "M=2 group 64 K=1024": _case(2, 16, 1024, G=64),
    # the epilogues and the prologue on the plain form
    "SiLU pairs K=4096 N=48": _case(1, 48, 4096, flags=PAIRS),
    "SiLU pairs K=1152 N=24 designed": _case(1, 24, 1152, flags=PAIRS, act="designed", zero_block=0),
    "residual add K=14336 N=24": _case(1, 24, 14336, flags=ADD),
    "residual add K=1920 N=16 general zero points": _case(1, 16, 1920, flags=ADD, general_zeros=True),
    "NORM K=4096 N=24": _case(1, 24, 4096, norm=True),
    "NORM K=1152 N=16 general zero points": _case(1, 16, 1152, norm=True, general_zeros=True),
    "NORM K=1920 N=48 SiLU pairs designed": _case(1, 48, 1920, norm=True, flags=PAIRS, act="designed"),
    "group copy K=4096": _group_copy(4096),
    "group copy K=1152 SiLU pairs designed": _group_copy(1152, pairs=True, act="designed"),
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
    meta = {"library": os.path.basename(capi.LIB_PATH), "cases": len(rec), "what": "int16 views of the fp16 outputs of scripts/decode_occupancy_record.py's cases"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, __meta__=np.array(json.dumps(meta)), **rec)
    print(json.dumps({**meta, "out": a.out, "bytes": os.path.getsize(a.out)}))
