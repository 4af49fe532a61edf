"""The parallel grouping's entry points without a device: tce_moe_route_f16's refusals with the same codes in the same order, the one refusal of their own (no room for
the per-chunk counts in the y section), and MoeFFN's parallel_group_from."""
import pytest

from test_moe_host import BAD, OFF, ROUTE, SHP, P
from tinychatengine_amd import capi, moe

# entry point, its valid arguments, [(argument index or indices, value or values, code)] as tests/test_moe_host.py writes them.  The last case of each: one row, k = 2,
# N_max = 1 -- a y section of 8 bytes against 8 experts' counts, 32 bytes; the one before it: that call and an argument fault, which comes first
ROUTE_PARALLEL = ("tce_moe_route_parallel_f16", ROUTE[1], ROUTE[2] + [((0, 3, 8), (None, 1, 1), BAD), ((3, 8), (1, 1), SHP)])
GROUP = ("tce_moe_group_parallel", [4, 2, 8, 256, P, None],
         [(4, None, BAD), (0, 0, BAD), (1, 0, BAD), (2, 1, BAD), (3, 0, BAD), ((1, 2), (9, 65), SHP), (0, 1 << 16, SHP), (4, OFF, SHP), ((0, 4), (0, OFF), BAD), ((0, 3, 4), (1, 1, None), BAD),
          ((0, 3), (1, 1), SHP)])


@pytest.mark.parametrize("name,args,where,value,code", [(n, a, *c) for n, a, cases in (ROUTE_PARALLEL, GROUP) for c in cases])
def test_refusals(name, args, where, value, code):
    call = list(args)  # (the valid call itself is not made: it would launch)
    for i, v in zip(where, value) if isinstance(where, tuple) else [(where, value)]:
        call[i] = v
    assert getattr(capi.lib(), name)(*call) == code and name in capi.last_error()


def test_parallel_group_from_is_a_pair_count():
    with pytest.raises(ValueError, match="parallel_group_from"):
        moe.MoeFFN(128, 128, 4, 2, "cpu", parallel_group_from=-1)
    assert moe.MoeFFN.LAUNCHES == 5
