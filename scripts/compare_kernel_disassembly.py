#!/usr/bin/env python3
"""Two builds of one translation unit, kernel by kernel, instruction for instruction (llvm-objdump -d of the gfx950 code object; addresses, encodings and padding
dropped; branch targets kept as the label text objdump prints).  Names are compared demangled, with template arguments that one side defaults spelled as given by
--rename OLD=NEW (a substring replacement on the old side's names).  A kernel that differs gets a second line: its new instruction count and the opcodes whose
counts moved.

    python scripts/compare_kernel_disassembly.py old.o new.o [--rename 'attn_prefill_prepare_kernel(=attn_prefill_prepare_kernel<false>('] [filter-substring]
"""
import os
import re
import sys
from collections import Counter

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tinychatengine_amd import isa_lint  # noqa: E402


def kernels(obj):
    ks = isa_lint.kernels(isa_lint.disassemble(obj))
    names = isa_lint.demangle(list(ks.keys()))
    out = {}
    for n, body in zip(names, ks.values()):
        n = re.sub(r"tce::\(anonymous namespace\)::", "", n)
        n = re.sub(r"^void ", "", n)
        lines = []
        for ln in body if isinstance(body, list) else str(body).splitlines():
            t = ln.split("//")[0].strip()
            if not t or t.startswith("s_nop") or t.startswith("s_code_end") or t == "...":
                continue
            lines.append(re.sub(r"\s+", " ", t))
        out[n] = lines
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    renames = []
    while "--rename" in args:
        i = args.index("--rename")
        renames.append(args[i + 1].split("=", 1))
        del args[i:i + 2]
    old, new = kernels(args[0]), kernels(args[1])
    flt = args[2] if len(args) > 2 else ""
    for a, b in renames:
        old = {k.replace(a, b): v for k, v in old.items()}
    for n in old:
        if flt and flt not in n:
            continue
        if n not in new:
            print(f"MISSING   {len(old[n]):5d} {n.split('(')[0]}")
        else:
            print(f"{'IDENTICAL' if old[n] == new[n] else 'DIFFERENT'} {len(old[n]):5d} {n.split('(')[0]}")
            if old[n] != new[n]:  # how different: the instruction count, and the opcodes whose counts moved (none: the same instructions in another order / registers)
                ho, hn = Counter(ln.split()[0] for ln in old[n]), Counter(ln.split()[0] for ln in new[n])
                delta = {op: hn[op] - ho[op] for op in sorted(set(ho) | set(hn)) if hn[op] != ho[op]}
                print(f"          {len(new[n]):5d} new; opcode histogram {'the same' if not delta else 'moved: ' + ' '.join(f'{op} {d:+d}' for op, d in delta.items())}")
    only = sorted(n.split("(")[0] for n in new if n not in old and (not flt or flt in n))
    print(f"new only: {only}")
