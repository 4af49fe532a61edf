"""The head and the tail of the int8 decode kernels, held on the compiled gfx950 object without a GPU (csrc/w4a16_gemv_i8.hip, profiles/decode_head/).

What the flat argument list is for: a wave's first weight request must not sit behind scalar-memory round trips.  The parent's kernel took one struct by value (kernel
descriptor: kernarg_preload_length 0) and waited twice on scalar loads -- the second at an offset computed from the first -- before any request left; it fetched `M` again
between the final LDS sum and the store.  Held here, on every `w4a16_gemv_i8_kernel` instantiation of the product object (the mixed launch's kernel, P > 1 plans only,
keeps its struct and is not covered):
  * the kernel descriptor asks for preloaded arguments (length > 0);
  * from the PRELOADED entry (256 bytes behind the symbol: in front of it sits the compiler's prologue for machines that do not preload) to the first non-temporal weight
    load: the single-linear path of the plain Z8 form passes no `s_waitcnt` on lgkmcnt, and no path of any Z8 form passes more than one (a grouped launch: the one batch
    that holds the further linears' addressing fields).  The kernel decides between the two on the launch's count of linears (one scalar compare on a preloaded register),
    so the paths are followed through the branches, not read off the listing's order;
  * nothing reachable from the final barrier is a scalar load.
"""
import re
import subprocess
import os
import shutil
import tempfile

import pytest

from tinychatengine_amd import build as tce_build
from tinychatengine_amd import isa_lint

KERNEL = "w4a16_gemv_i8_kernel"
PLAIN_Z8 = "w4a16_gemv_i8_kernelILi1ELi1ELi1ELi8ELb1ELi1024ELb0ELb0ELi0E"  # <MB 1, GPU 1, ROWS 1, UW 8, Z8, 1024, no NORM, no RNORM, no COMB>: every plain launch of the token


def _code_object(obj, d):
    o = os.path.join(d, "x.o")
    shutil.copy(obj, o)
    subprocess.run([isa_lint.OBJDUMP, "--offloading", o], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=d, check=False)
    co = [f for f in os.listdir(d) if "gfx950" in f]
    assert co, "no gfx950 code object in " + obj
    return os.path.join(d, co[0])


@pytest.fixture(scope="module")
def listing():
    """(symbol -> [(address, instruction)], symbol -> preload length) of the product build's w4a16_gemv_i8 object"""
    tce_build.build()
    obj = os.path.join(tce_build.LIB_DIR, "w4a16_gemv_i8.o")
    d = tempfile.mkdtemp(prefix="tce_head_")
    try:
        co = _code_object(obj, d)
        text = subprocess.run([isa_lint.OBJDUMP, "-d", co], capture_output=True, text=True, check=True).stdout
        kds = subprocess.run([isa_lint.OBJDUMP, "-D", "-j", ".rodata", co], capture_output=True, text=True, check=True).stdout
    finally:
        shutil.rmtree(d, ignore_errors=True)
    code, cur = {}, None
    for ln in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:", ln)
        if m:
            cur = code.setdefault(m.group(1), [])
            continue
        m = re.match(r"^\t(.*?)\s*// ([0-9A-F]+):", ln)
        if m and cur is not None:
            cur.append((int(m.group(2), 16), m.group(1).strip()))
    preload, cur = {}, None
    for ln in kds.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)\.kd>:", ln)
        if m:
            cur = m.group(1)
        m = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", ln)
        if m and cur:
            preload[cur] = int(m.group(1))
    code = {k: v for k, v in code.items() if KERNEL in k}
    assert len(code) >= 20 and PLAIN_Z8 in "".join(code), sorted(code)
    return code, preload


def _successors(ins, i):
    """indices of the instructions that may run after instruction i"""
    addr, t = ins[i]
    op = t.split()[0]
    if op == "s_endpgm":
        return []
    assert op not in ("s_setpc_b64", "s_swappc_b64"), t
    nxt = [i + 1] if i + 1 < len(ins) else []
    if op == "s_branch" or op.startswith("s_cbranch_"):
        off = int(t.split()[1])
        off = off - 65536 if off >= 32768 else off
        target = addr + 4 + 4 * off
        idx = next((k for k, (a, _) in enumerate(ins) if a == target), None)
        assert idx is not None, (hex(addr), t)
        return [idx] if op == "s_branch" else nxt + [idx]
    return nxt


def _is_weight_load(t):
    return t.startswith("buffer_load_dwordx4") and t.split("//")[0].rstrip().endswith(" nt")


def _lgkm_wait(t):
    return t.startswith("s_waitcnt") and "lgkmcnt" in t


def _waits_to_first_weight_load(ins):
    """the set of lgkmcnt-wait counts over every path from the preloaded entry to the first non-temporal weight load"""
    entry = next(k for k, (a, _) in enumerate(ins) if a == ins[0][0] + 256)
    counts, seen, stack = set(), set(), [(entry, 0)]
    while stack:
        i, n = stack.pop()
        if (i, n) in seen:
            continue
        seen.add((i, n))
        t = ins[i][1]
        if _is_weight_load(t):
            counts.add(n)
            continue
        n += 1 if _lgkm_wait(t) else 0
        assert n <= 8, "a loop with a scalar wait in front of the weight requests"
        succ = _successors(ins, i)
        assert succ, "a path ends before any weight request"
        stack += [(k, n) for k in succ]
    return counts


def _reachable(ins, start):
    seen, stack = set(), list(start)
    while stack:
        i = stack.pop()
        if i in seen:
            continue
        seen.add(i)
        stack += _successors(ins, i)
    return seen


def test_the_decode_kernels_take_preloaded_arguments(listing):
    code, preload = listing
    for name in code:
        assert preload.get(name, 0) > 0, f"{name}: kernarg_preload_length {preload.get(name)}"
        # the compatible prologue: the preloaded arguments by scalar loads, ONE wait, a branch to the preloaded entry
        head = [t for _, t in code[name][:64]]
        assert head[0].startswith("s_load") and sum(_lgkm_wait(t) for t in head) == 1, head[:8]


def test_no_scalar_wait_in_front_of_the_weight_requests(listing):
    code, _ = listing
    for name, ins in code.items():
        z8 = re.search(KERNEL + r"I(?:Li\d+E){4}Lb([01])E", name).group(1) == "1"  # <MB, GPU, ROWS, UW, Z8, ...>
        counts = _waits_to_first_weight_load(ins)
        if PLAIN_Z8 in name:
            assert min(counts) == 0, f"{name}: the single-linear path waits on scalar memory in front of its first weight request ({sorted(counts)})"
        if z8 and "ELb0ELb0ELi0E" in name:  # plain forms (no NORM / RNORM / COMB prologue): single-linear none, grouped at most one
            assert min(counts) == 0 and max(counts) <= 1, f"{name}: waits on lgkmcnt per path to the first weight request {sorted(counts)}"


def test_grouped_launches_wait_at_most_once(listing):
    code, _ = listing
    ins = next(v for k, v in code.items() if PLAIN_Z8 in k)
    counts = _waits_to_first_weight_load(ins)
    assert counts == {0, 1}, counts  # 0: one linear; 1: a grouped launch's batch of the further linears' fields


def test_no_scalar_load_behind_the_final_barrier(listing):
    code, _ = listing
    for name, ins in code.items():
        bars = [i for i, (_, t) in enumerate(ins) if t.startswith("s_barrier")]
        assert bars, name
        # the final barrier(s): those from which no barrier is reached again
        for b in bars:
            after = _reachable(ins, _successors(ins, b))
            if any(k in after for k in bars):
                continue
            loads = [ins[k][1] for k in sorted(after) if ins[k][1].startswith(("s_load", "s_buffer_load"))]
            assert not loads, f"{name}: scalar loads behind the final barrier: {loads[:4]}"
