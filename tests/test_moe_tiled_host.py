"""The tiled MoE entry points without a device: the refusals of tce_moe_gate_up_f16 / tce_moe_down_f16 with the same codes, MoeFFN's tiled_from, and the grid bound."""
import numpy as np
import pytest

import moe_tiled_cases as tc
from test_moe_host import DOWN, UP
from tinychatengine_amd import capi, moe

TILED = [(n.replace("_f16", "_tiled_f16"), a, cases) for n, a, cases in (UP, DOWN)]


@pytest.mark.parametrize("name,args,where,value,code", [(n, a, *c) for n, a, cases in TILED for c in cases])
def test_refusals(name, args, where, value, code):
    call = list(args)  # (the valid call itself is not made: it would launch)
    for i, v in zip(where, value) if isinstance(where, tuple) else [(where, value)]:
        call[i] = v
    assert getattr(capi.lib(), name)(*call) == code and name in capi.last_error()


def test_tiled_from_is_a_pair_count():
    with pytest.raises(ValueError, match="tiled_from"):
        moe.MoeFFN(128, 128, 4, 2, "cpu", tiled_from=-1)
    assert moe.TILE_PAIRS % 16 == 0 and moe.MoeFFN.LAUNCHES == 5


@pytest.mark.parametrize("E,k", tc.EK)
def test_grid_bound(E, k):
    """P // TM + min(E, P) >= sum_e ceil(count[e] / TM): the tests' routing, every pair on one expert, one pair per expert"""
    TM, ids = moe.TILE_PAIRS, tc.tiled_ids(E, k, moe.TILE_PAIRS)
    for v in (ids, np.zeros_like(ids), np.arange(E, dtype=np.int32).reshape(-1, k)):
        count, P = moe.group_reference(v, E)[0], v.size
        assert int(((count + TM - 1) // TM).sum()) <= P // TM + min(E, P)
