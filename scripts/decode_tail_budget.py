#!/usr/bin/env python3
"""What wave 0 of a decode launch runs around the K reduction's barrier, counted on a compiled object without a GPU (profiles/decode_tail/instruction_budget.md):

    python scripts/decode_tail_budget.py <w4a16_gemv_i8.o> <label> [substring of a kernel symbol ...]

Per kernel (default: the plain form of every launch of the token and the NORM form), one markdown row:
  in front   instructions between the last MFMA (layout order) and the final barrier: every wave runs them with its contraction done;
  behind     instructions from the barrier to the store (the barrier not counted, the store counted) on the plain / residual-add way and on the SiLU-pair way, found by
             executing the tail's scalar side (tinychatengine_amd/isa_paths.py, walk_scalar) for launches of 4 and of 14 waves.  Where no scalar register decides the
             number of LDS reads (the sixteen-slot form) the way does not depend on the waves and one figure stands for both;
  LDS reads  dword reads on that way.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tinychatengine_amd import isa_paths as P

DEFAULT = ("w4a16_gemv_i8_kernelILi1ELi1ELi1ELi8ELb1ELi1024ELb0ELb0ELi0ELb0E", "w4a16_gemv_i8_kernelILi1ELi1ELi1ELi8ELb1ELi1024ELb1ELb0ELi0ELb0E",
           "w4a16_gemv_i8_kernelILi1ELi1ELi2ELi8ELb1ELi512ELb1ELb0ELi0ELb0E")


def ways(ins, bar, regs):
    paths = P.walk_scalar(ins, bar, regs, P.is_global_store)
    plain = [p for p in paths if not any(P.is_silu(ins[k][1]) for k in p)]
    silu = [p for p in paths if any(P.is_silu(ins[k][1]) for k in p)]
    reads = {sum(P.lds_reads(ins[k][1]) for k in p) for p in paths}
    f = lambda ps: "-" if not ps else (str(len(ps[0])) if len({len(p) for p in ps}) == 1 else f"{min(map(len, ps))} .. {max(map(len, ps))}")
    return f(plain), f(silu), "/".join(str(r) for r in sorted(reads))


def waves_register(ins, bar):
    """the scalar register for which every way holds exactly WK LDS reads, WK = 1 .. 16 (None: the reads do not depend on one)"""
    for c in sorted(P.compared_sgprs(ins, P.walked(ins, bar, P.is_global_store))):
        if all({sum(P.lds_reads(ins[k][1]) for k in p) for p in P.walk_scalar(ins, bar, {c: wk}, P.is_global_store)} == {wk} for wk in range(1, 17)):
            return c
    return None


if __name__ == "__main__":
    obj, label, wanted = sys.argv[1], sys.argv[2], sys.argv[3:] or DEFAULT
    print("| build | kernel | all | in front of the barrier | behind, 4 waves: plain or residual / SiLU pairs | LDS reads | behind, 14 waves: plain or residual / SiLU pairs | LDS reads |")
    print("|---|---|---|---|---|---|---|---|")
    for name, ins in P.listing(obj).items():
        if not any(w in name for w in wanted):
            continue
        bar = P.final_barriers(ins)[0]
        mfma = max(i for i, (_, t) in enumerate(ins) if t.startswith("v_mfma") and i < bar)
        reg = waves_register(ins, bar)
        cols = []
        for wk in (4, 14):
            plain, silu, reads = ways(ins, bar, {reg: wk} if reg else {})
            cols += [f"{plain} / {silu}", reads]
        short = P.isa_lint.demangle([name])[0].split("(")[0].replace("void ", "")
        print(f"| {label} | `{short}` | {len(ins)} | {bar - mfma - 1} | {cols[0]} | {cols[1]} | {cols[2]} | {cols[3]} |")
