#!/usr/bin/env python3
"""The instruction budget of the plain decode kernel (w4a16_gemv_i8_kernel<1, 1, 1, 8, zero point 8, 1024>) by class, read off a built object -- no GPU:

    python scripts/instruction_budget.py tinychatengine_amd/lib/w4a16_gemv_i8.o [label]

Static counts over the whole kernel (both heads -- single linear and grouped -- and every epilogue are in it; a wave runs one head and one epilogue), classified by
mnemonic and operand form.  The classes: MFMA; unpack (nibbles -> signed bytes: v_bitop3, the shift by 4, the mask constants); conversion (x -> digit planes: the
exponent scan, the scaling v_fma_mix with a zero addend, truncation, the digit bias add / xor, the byte transposes, the LDS writes); loads (x, scales, weights, the
B operand reads); epilogue (scales, plane / group / wave sums, the stores and their arithmetic); addressing and everything else on the vector unit; scalar / control."""
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"
PLAIN = "w4a16_gemv_i8_kernelILi1ELi1ELi1ELi8ELb1ELi1024ELb0ELb0ELi0ELb0E"


def listing(obj):
    d = tempfile.mkdtemp(prefix="tce_budget_")
    try:
        shutil.copy(obj, os.path.join(d, "x.o"))
        subprocess.run([OBJDUMP, "--offloading", "x.o"], cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=False)
        co = [f for f in os.listdir(d) if "gfx950" in f][0]
        text = subprocess.run([OBJDUMP, "-d", os.path.join(d, co)], capture_output=True, text=True, check=True).stdout
    finally:
        shutil.rmtree(d, ignore_errors=True)
    m = re.search(r"<[^>]*" + PLAIN + r"[^>]*>:\n(.*?)\n\n", text, re.S)
    if m is None:
        sys.exit(f"{obj}: no symbol containing {PLAIN} in the gfx950 code object -- has the plain kernel's template signature changed?")
    return [ln.split("//")[0].strip() for ln in m.group(1).splitlines() if ln.startswith("\t")]


def classify(i):
    op = i.split()[0]
    if not op.startswith(("v_", "ds_", "buffer_", "global_", "flat_")):
        return "scalar / control"
    if op.startswith("v_mfma"):
        return "MFMA"
    if op == "v_bitop3_b32" or "0xf0f0f0f0" in i or re.match(r"v_lshlrev_b32_e32 v\d+, 4, v([2-9]|[1-3]\d)$", i):
        return "unpack"
    if ("0x7fff7fff" in i or "0x808080" in i or re.match(r"v_lshlrev_b32_e32 v\d+, 16, ", i) or (op == "v_fma_mix_f32" and "op_sel_hi:[1,0,0]" in i and ", 0 op_sel" in i) or
            op in ("v_max_u32_e32", "v_max3_u32", "v_max_u32_dpp", "v_readlane_b32", "v_perm_b32", "v_cvt_i32_f32_e32", "ds_write2_b32", "ds_write_b32")):
        return "conversion"
    if op.startswith("buffer_load") or op == "ds_read_b128":
        return "loads"
    if op in ("v_cvt_f32_i32_e32", "v_fma_mix_f32", "v_add_f32_e32", "v_add_f32_dpp", "v_mul_f32_e32", "ds_read_b32", "v_cvt_f16_f32_e32", "flat_store_short", "global_load_ushort",
              "v_add_f16_e32", "v_mul_f16_e32", "v_exp_f32_e32", "v_rcp_f16_e32", "v_rndne_f32_e32", "v_sub_f32_e32", "v_ldexp_f32", "v_cvt_f32_f16_e64", "v_mov_b32_dpp") or op.startswith("v_cmp_n"):
        return "epilogue"
    return "addressing / other vector"


def section3(ins):
    """the contraction: from the first read of a B operand (ds_read_b128) to the last MFMA, in the listing's order"""
    first = next(i for i, t in enumerate(ins) if t.startswith("ds_read_b128"))
    last = max(i for i, t in enumerate(ins) if t.startswith("v_mfma"))
    return ins[first:last + 1]


if __name__ == "__main__":
    argv = [a for a in sys.argv[1:] if a != "--section3"]
    ins = listing(argv[0])
    label = argv[1] if len(argv) > 1 else os.path.basename(argv[0])
    if "--section3" in sys.argv:  # profiles/decode_occupancy/: the contraction alone, by mnemonic
        sec = section3(ins)
        c = collections.Counter(i.split()[0] for i in sec)
        vec = sum(v for k, v in c.items() if k.startswith(("v_", "ds_")))
        print(f"| {label} | {len(sec)} | {vec} | " + ", ".join(f"{k} {v}" for k, v in sorted(c.items(), key=lambda kv: (-kv[1], kv[0]))) + " |")
        sys.exit(0)
    c = collections.Counter(classify(i) for i in ins)
    order = ["unpack", "conversion", "epilogue", "addressing / other vector", "loads", "MFMA", "scalar / control"]
    print(f"| {label} | " + " | ".join(str(c[k]) for k in order) + f" | {sum(v for k, v in c.items() if k != 'scalar / control')} | {len(ins)} |")
