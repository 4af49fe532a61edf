"""The tail of the int8 decode kernels -- what wave 0 runs between the K reduction's barrier and its store -- held on the compiled gfx950 object without a GPU
(csrc/w4a16_gemv_i8.hip section 4, profiles/decode_tail/; the head: tests/test_decode_head_isa.py).

Nothing overlaps between the 129 launches of a token, so what a launch does after its last weight byte has arrived is paid 129 times with the chip idle.  The parent
formed sixteen LDS addresses by scalar selects, read sixteen slots (twelve of them slot 0 again at four waves), added them through sixteen vector selects, and
computed the row, the bounds and the store address -- a 64-bit multiply -- behind the barrier: about 170 instructions on the plain path, run by one wave.

Held here on the plain kernel and the M = 2 / 4, group 64 / 32, two-tiles, NORM and mixed instantiations of the product object, from the final barrier to the first
global store on the way (branches followed, not the listing's order):
  * nothing selects (`s_cselect*`, `v_cndmask*`) in front of the first LDS read, and nothing multiplies into a high word (`s_mul_hi*`) anywhere on the way;
  * a launch reads exactly its WK partial rows: the scalar side of the tail is executed for every WK = 1 .. 16 (tinychatengine_amd/isa_paths.py, walk_scalar) and
    every way to the store holds WK dword LDS reads -- at most four for the launches of up to four waves, none of them a second read of slot 0;
  * the SiLU arithmetic (`v_exp_f32`, `v_rcp_f16`) sits behind ONE wave-uniform branch: with that branch's edge removed none of it can be reached.
"""
import os

import pytest

from tinychatengine_amd import build as tce_build
from tinychatengine_amd import isa_paths as P

K = "w4a16_gemv_i8_kernel"
# <MB, GPU, ROWS, UW, Z8, MAXT, NORM, RNORM, COMB>
FORMS = {
    "plain": K + "ILi1ELi1ELi1ELi8ELb1ELi1024ELb0ELb0ELi0E",
    "plain, general zero points": K + "ILi1ELi1ELi1ELi8ELb0ELi1024ELb0ELb0ELi0E",
    "M = 2": K + "ILi2ELi1ELi1ELi8ELb1ELi1024ELb0ELb0ELi0E",
    "M = 4": K + "ILi4ELi1ELi1ELi8ELb1ELi1024ELb0ELb0ELi0E",
    "group 64": K + "ILi1ELi2ELi1ELi8ELb1ELi1024ELb0ELb0ELi0E",
    "M = 2, group 64": K + "ILi2ELi2ELi1ELi8ELb1ELi1024ELb0ELb0ELi0E",
    "group 32": K + "ILi1ELi4ELi1ELi8ELb1ELi1024ELb0ELb0ELi0E",
    "two tiles": K + "ILi1ELi1ELi2ELi8ELb1ELi512ELb0ELb0ELi0E",
    "K > 16384": K + "ILi1ELi1ELi1ELi16ELb1ELi1024ELb0ELb0ELi0E",
    "NORM": K + "ILi1ELi1ELi1ELi8ELb1ELi1024ELb1ELb0ELi0E",
    "NORM, two tiles": K + "ILi1ELi1ELi2ELi8ELb1ELi512ELb1ELb0ELi0E",
    "mixed": "w4a16_gemv_i8_mixed_kernelILb1E",
    "mixed, general zero points": "w4a16_gemv_i8_mixed_kernelILb0E",
}


@pytest.fixture(scope="module")
def tails():
    """form -> (instructions, the final barrier's index) of the product build's w4a16_gemv_i8 object"""
    tce_build.build()
    code = P.listing(os.path.join(tce_build.LIB_DIR, "w4a16_gemv_i8.o"))
    out = {}
    for form, sym in FORMS.items():
        hits = [v for k, v in code.items() if sym in k]
        assert len(hits) == 1, (form, len(hits))
        bars = P.final_barriers(hits[0])
        assert len(bars) == 1, (form, bars)
        out[form] = (hits[0], bars[0])
    return out


def test_nothing_selects_in_front_of_the_first_lds_read(tails):
    for form, (ins, bar) in tails.items():
        front = P.walked(ins, bar, lambda t: P.lds_reads(t) > 0 or P.is_global_store(t))
        assert any(P.lds_reads(ins[i][1]) for i in front), form
        bad = [ins[i][1] for i in sorted(front) if P.op(ins[i][1]).startswith(("s_cselect", "v_cndmask"))]
        assert not bad, f"{form}: selects between the final barrier and the first LDS read: {bad[:4]}"


def test_no_wide_multiply_behind_the_barrier(tails):
    for form, (ins, bar) in tails.items():
        way = P.walked(ins, bar, P.is_global_store)
        bad = [ins[i][1] for i in sorted(way) if P.op(ins[i][1]).startswith(("s_mul_hi", "v_mul_hi", "v_mad_u64", "v_mad_i64"))]
        assert not bad, f"{form}: {bad[:4]}"


def _exact_reads(ins, bar, regs_of):
    """WK -> the instructions on the longest way to the store, when for every WK = 1 .. 16 each way holds exactly WK dword LDS reads; None otherwise"""
    longest = {}
    for wk in range(1, 17):
        paths = P.walk_scalar(ins, bar, regs_of(wk), P.is_global_store)
        if not paths or {sum(P.lds_reads(ins[k][1]) for k in p) for p in paths} != {wk}:
            return None
        longest[wk] = max(len(p) for p in paths)
    return longest


def test_a_launch_reads_exactly_its_waves_partial_rows(tails):
    for form, (ins, bar) in tails.items():
        cands = sorted(P.compared_sgprs(ins, P.walked(ins, bar, P.is_global_store)))
        # the register that holds WK is the compiler's choice: it is the one (exactly one) for which the reads come out as WK for all sixteen values.  The mixed
        # launch derives WK = ceil(U / 8) from its linear's K and compares either: there the pair (WK, U).
        schemes = [(c, None) for c in cands] if "mixed" not in form else [(a, b) for a in cands for b in cands if a != b]
        good = []
        for a, b in schemes:
            res = _exact_reads(ins, bar, (lambda wk: {a: wk}) if b is None else (lambda wk: {a: wk, b: 8 * wk}))
            if res:
                good.append(((a, b), res))
        assert len(good) == 1, f"{form}: no scalar register (of {cands}) makes every way from the barrier to the store hold exactly WK LDS reads for WK = 1 .. 16: {good}"


def test_the_silu_arithmetic_sits_behind_one_uniform_branch(tails):
    for form, (ins, bar) in tails.items():
        behind = P.reachable(ins, P.successors(ins, bar))
        silu = {i for i in behind if P.is_silu(ins[i][1])}
        assert silu, f"{form}: the pair epilogue is not in the kernel"
        gates = []
        for i in sorted(behind):
            o = P.op(ins[i][1])
            if o in ("s_cbranch_scc0", "s_cbranch_scc1", "s_cbranch_vccz", "s_cbranch_vccnz"):  # (a scalar condition; not a wave's exec mask running empty)
                gates += [(i, k) for k in P.successors(ins, i) if not silu & P.reachable_without(ins, bar, (i, k))]
        assert gates, f"{form}: no single scalar branch edge in front of the SiLU arithmetic"
        # and a way from the barrier to a store that passes none of it exists: the plain and the residual epilogue
        assert P.over_store_paths(ins, bar, lambda t: 1, min, P.is_silu) is not None, form
