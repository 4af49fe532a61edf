"""Mixture of experts without a device: refusals of the entry points by kind and order (before any HIP call, through no pointer; alignment and size rules are
sampled), moe_reference's tie and NaN rules on hand-written rows, and the ValueErrors of the Python layer."""
import ctypes as C

import numpy as np
import pytest

from tinychatengine_amd import capi, moe

P = C.c_void_p(0x10000)  # never read: a refusal must not follow it; aligned to 256
BAD, GRP, SHP = capi.TCE_ERR_BAD_ARG, capi.TCE_ERR_UNSUPPORTED_GROUP, capi.TCE_ERR_UNSUPPORTED_SHAPE
OFF = C.c_void_p(0x10010)  # 16-byte, not 256-byte aligned

# entry point, its valid arguments (rows 4, k 2, E 8, N_max 256), then [(argument index or indices, value or values, code)]; with two faults the argument refusal comes first
ROUTE = ("tce_moe_route_f16", [P, 128, P, 4, 128, 8, 2, 1, 256, P, None],
         [(0, None, BAD), (2, None, BAD), (9, None, BAD), (3, 0, BAD), (5, 1, BAD), (6, 0, BAD), (1, 120, BAD), (4, 100, SHP), ((5, 6), (65, 9), SHP), (9, OFF, SHP), ((3, 4), (0, 100), BAD)])
UP = ("tce_moe_gate_up_f16", [P, 128, P, P, P, 4, 2, 8, 48, 128, 128, 0, 256, P, None],
      [(0, None, BAD), (2, None, BAD), (4, None, BAD), (13, None, BAD), (1, 64, BAD), (11, 16, BAD), (12, 16, BAD), (10, 64, GRP), ((1, 9), (256, 192), SHP), (8, 47, SHP), (6, 9, BAD), (7, 65, SHP),
       ((1, 9, 10), (256, 192, 64), GRP)])
DOWN = ("tce_moe_down_f16", [P, P, P, 4, 2, 8, 48, 128, 128, 0, 256, P, None],
        [(0, None, BAD), (11, None, BAD), (3, 0, BAD), (9, 3, BAD), (10, 100, BAD), (8, 32, GRP), (7, 64, SHP), ((7, 10), (32768 + 128, 1 << 16), SHP)])
COMBINE = ("tce_moe_combine_add_f16", [P, 56, 4, 2, 8, 48, 256, P, None],
           [(0, None, BAD), (7, None, BAD), (1, 40, BAD), (5, 300, BAD), (3, 0, BAD), ((1, 5), (52, 44), SHP), (2, 1 << 16, SHP), (7, OFF, SHP)])


@pytest.mark.parametrize("name,args,where,value,code", [(n, a, *c) for n, a, cases in (ROUTE, UP, DOWN, COMBINE) for c in cases])
def test_refusals(name, args, where, value, code):
    call = list(args)  # (the valid call itself is not made: it would launch)
    for i, v in zip(where, value) if isinstance(where, tuple) else [(where, value)]:
        call[i] = v
    assert getattr(capi.lib(), name)(*call) == code and capi.last_error()


def test_reference_rules():
    """ties to the lower index (-0 equals +0), NaN below every number -- below -inf too --, NaNs among themselves by index; weights of the selected, renormalised"""
    x = np.eye(1, 8).astype(np.float16)  # the row's logits are Wr's first column
    route = lambda logits, **kw: moe.route_reference(x, np.pad(np.array(logits, np.float16)[:, None], ((0, 0), (0, 7))), 3, **kw)
    rows = [[1, 3, 3, 2], [-0.0, 0.0, -1, -1], [np.nan, -np.inf, np.nan, -np.inf], [np.nan] * 4]
    assert [route(r)[0][0].tolist() for r in rows] == [[1, 2, 3], [0, 1, 2], [1, 3, 0], [0, 1, 2]]
    e = np.exp([0.0, 0.0, -1.0])
    assert np.allclose(route(rows[0])[1][0], e / e.sum(), rtol=1e-15) and np.allclose(route(rows[0], renormalize=False)[1][0], e / (e.sum() + np.exp(-2.0)), rtol=1e-15)
    count, lists = moe.group_reference(np.array([[1, 0], [7, 1], [1, -1]]), 4)
    assert count.tolist() == [1, 3, 0, 0] and lists[1].tolist() == [0, 3, 4]


def test_value_errors():
    from tinychatengine_amd.batch_decode import BatchedDecoder
    from tinychatengine_amd.decoder_block import DecoderBlock, layer_body
    blk = DecoderBlock.__new__(DecoderBlock)
    blk.moe = object()
    for match, call in [("moe", lambda: blk.step(None, 0)), ("moe", lambda: blk.step_chained(None, None, 0, None, None, None)), ("top_k", lambda: moe.MoeFFN(128, 128, 4, 5, "cpu")),
                        ("lora.*moe", lambda: layer_body(blk, *[None] * 7, lora=object())), ("lora.*moe", lambda: BatchedDecoder(blk, 2, lora=object()))]:
        with pytest.raises(ValueError, match=match):
            call()
