"""Paths through a compiled gfx950 kernel, without a GPU: what a wave can execute between two points of the listing (tests/test_decode_tail_isa.py,
scripts/decode_tail_budget.py; profiles/decode_tail/).

A kernel is a list of (address, instruction text) from `llvm-objdump -d` of the code object inside a host object file.  Branch targets are resolved from the encoded
offsets, so paths are followed through the branches and not read off the listing's order: as a graph (tail_dag, over_store_paths, reachable_without) or by executing
the scalar side for given register values (walk_scalar).
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import tempfile

from . import isa_lint

GLOBAL_STORES = ("global_store", "flat_store", "buffer_store", "global_atomic", "flat_atomic", "buffer_atomic")
LDS_READS = ("ds_read", "ds_load")


def listing(obj: str) -> dict[str, list[tuple[int, str]]]:
    """symbol -> [(address, instruction)] of the gfx950 code object embedded in `obj`"""
    d = tempfile.mkdtemp(prefix="tce_paths_")
    try:
        o = os.path.join(d, "x.o")
        shutil.copy(obj, o)
        subprocess.run([isa_lint.OBJDUMP, "--offloading", o], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=d, check=False)
        co = [f for f in os.listdir(d) if "gfx950" in f]
        assert co, "no gfx950 code object in " + obj
        text = subprocess.run([isa_lint.OBJDUMP, "-d", os.path.join(d, co[0])], capture_output=True, text=True, check=True).stdout
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
    return code


def op(t: str) -> str:
    return t.split()[0]


def successors(ins, i):
    """indices of the instructions that may run after instruction i"""
    addr, t = ins[i]
    o = op(t)
    if o == "s_endpgm":
        return []
    assert o not in ("s_setpc_b64", "s_swappc_b64"), t
    nxt = [i + 1] if i + 1 < len(ins) else []
    if o == "s_branch" or o.startswith("s_cbranch_"):
        off = int(t.split()[1])
        off = off - 65536 if off >= 32768 else off
        target = addr + 4 + 4 * off
        idx = next((k for k, (a, _) in enumerate(ins) if a == target), None)
        assert idx is not None, (hex(addr), t)
        return [idx] if o == "s_branch" else nxt + [idx]
    return nxt


def reachable(ins, start):
    seen, stack = set(), list(start)
    while stack:
        i = stack.pop()
        if i in seen:
            continue
        seen.add(i)
        stack += successors(ins, i)
    return seen


def final_barriers(ins):
    """the barriers from which no barrier is reached again"""
    bars = [i for i, (_, t) in enumerate(ins) if t.startswith("s_barrier")]
    return [b for b in bars if not any(k in reachable(ins, successors(ins, b)) for k in bars)]


def is_global_store(t: str) -> bool:
    return t.startswith(GLOBAL_STORES)


def lds_reads(t: str) -> int:
    """dwords-sized LDS reads of an instruction: ds_read_b32 one, ds_read2(st64)_b32 two"""
    if not t.startswith(LDS_READS):
        return 0
    return 2 if op(t).startswith(("ds_read2", "ds_load_2addr")) else 1


def tail_dag(ins, start):
    """What a wave can run from instruction `start` up to the first global store on its way, as a graph without its loops' back edges:
    (order, edges) -- edges[i]: the successors of i, a global store has none, an edge that closes a cycle (found by a depth-first walk from `start`: its target is
    still open) is left out; order: every node behind all of its successors.  A path of this graph is what a wave runs when every loop on its way runs once."""
    edges, order, state = {start: []}, [], {start: 1}
    stack = [(start, iter([] if is_global_store(ins[start][1]) else successors(ins, start)))]
    while stack:
        i, it = stack[-1]
        k = next(it, None)
        if k is None:
            state[i] = 2
            order.append(i)
            stack.pop()
            continue
        if state.get(k) == 1:
            continue  # a back edge
        edges[i].append(k)
        if k not in state:
            state[k] = 1
            edges[k] = []
            stack.append((k, iter([] if is_global_store(ins[k][1]) else successors(ins, k))))
    return order, edges


def over_store_paths(ins, start, weight, best=max, avoid=lambda t: False):
    """best (max / min) over the paths of tail_dag from `start` to a global store of the sum of weight(instruction text), `start` itself not counted, the store counted;
    paths through an instruction that `avoid` names do not count.  None: no such path."""
    order, edges = tail_dag(ins, start)
    val = {}
    for i in order:
        t = ins[i][1]
        if avoid(t):
            val[i] = None
        elif is_global_store(t):
            val[i] = weight(t)
        else:
            sub = [val[k] for k in edges[i] if val.get(k) is not None]
            val[i] = (0 if i == start else weight(t)) + best(sub) if sub else None
    return val[start]


def reachable_without(ins, start, edge):
    """the instructions a wave can run from `start` on when the branch edge (from, to) is never taken"""
    seen, stack = set(), [start]
    while stack:
        i = stack.pop()
        if i in seen:
            continue
        seen.add(i)
        stack += [k for k in successors(ins, i) if (i, k) != edge]
    return seen


# ---- the scalar side of a tail, executed: which way a wave goes for a given value of one scalar register ----
_M32 = 0xFFFFFFFF
_CMP = {"eq": lambda a, b: a == b, "lg": lambda a, b: a != b, "lt": lambda a, b: a < b, "le": lambda a, b: a <= b, "gt": lambda a, b: a > b, "ge": lambda a, b: a >= b}


def _operands(t):
    rest = t.split(None, 1)[1] if " " in t else ""
    return [x.strip() for x in rest.split(",")] if rest else []


def _val(regs, x):
    """a 32-bit operand's value (None: unknown)"""
    if re.fullmatch(r"-?\d+", x):
        return int(x) & _M32
    if re.fullmatch(r"0x[0-9a-fA-F]+", x):
        return int(x, 16) & _M32
    return regs.get(x)


def _mask(regs, x):
    """a 64-bit operand as a lane mask: True all ones / not zero, False zero, None unknown or per lane"""
    if x in ("-1", "exec"):
        return True if x == "-1" else regs.get("exec", True)
    if x == "0":
        return False
    return regs.get(x)


def _signed(v):
    return v - (1 << 32) if v & 0x80000000 else v


def walk_scalar(ins, start, regs, stop, max_steps=4000):
    """Run the instructions behind `start` with the scalar registers `regs` (name -> value; everything else unknown), the wave's exec mask not zero (a way on which it is zero ends there).  A conditional
    branch whose condition is known goes one way; otherwise both ways are followed (once per branch and path).  Scalar arithmetic the walk does not model makes its result unknown.
    Returns the paths (lists of instruction indices) that end at the first instruction `stop` names; a path that reaches the kernel's end without one is dropped."""
    out = []
    todo = [(successors(ins, start)[0], dict(regs, exec=True), [], frozenset())]
    while todo:
        i, r, path, forks = todo.pop()
        r = dict(r)
        path = list(path)
        while True:
            assert len(path) < max_steps, "the walk does not end"
            t = ins[i][1]
            o, a = op(t), _operands(t)
            path.append(i)
            if stop(t):
                out.append(path)
                break
            if o == "s_endpgm":
                break
            nxt = None
            if o == "s_branch":
                nxt = successors(ins, i)[0]
            elif o.startswith("s_cbranch_"):
                kind = o[len("s_cbranch_"):]
                cond = {"scc0": ("scc", False), "scc1": ("scc", True), "vccz": ("vcc", False), "vccnz": ("vcc", True), "execz": ("exec", False), "execnz": ("exec", True)}[kind]
                have = r.get(cond[0])
                fall, taken = successors(ins, i) if len(successors(ins, i)) == 2 else (None, successors(ins, i)[0])
                if have is None:
                    if i in forks:  # a loop whose end the known registers do not decide: not followed round and round
                        break
                    forks = forks | {i}
                    # both ways; each knows the condition from here on
                    if not (cond[0] == "exec" and cond[1] is False):  # (the way on which no lane is left is not followed)
                        todo.append((taken, dict(r, **{cond[0]: cond[1]}), list(path), forks))
                    r[cond[0]] = not cond[1]
                    nxt = fall
                else:
                    nxt = taken if have == cond[1] else fall
                if nxt is None or r.get("exec") is False:  # (no lane left: nothing the wave does from here on counts)
                    break
            elif o.startswith("s_cmp_") and o[6:8] in _CMP:
                x, y = _val(r, a[0]), _val(r, a[1])
                if x is None or y is None:
                    r["scc"] = None
                else:
                    r["scc"] = _CMP[o[6:8]](_signed(x), _signed(y)) if o.endswith("i32") else _CMP[o[6:8]](x, y)
            elif o in ("s_bitcmp0_b32", "s_bitcmp1_b32"):
                x, y = _val(r, a[0]), _val(r, a[1])
                r["scc"] = None if x is None or y is None else (((x >> (y & 31)) & 1) == (1 if o == "s_bitcmp1_b32" else 0))
            elif o == "s_mov_b32":
                r[a[0]] = _val(r, a[1])
            elif o == "s_mov_b64":
                r[a[0]] = _mask(r, a[1])
            elif o in ("s_add_i32", "s_add_u32", "s_sub_i32", "s_sub_u32"):
                x, y = _val(r, a[1]), _val(r, a[2])
                r[a[0]] = None if x is None or y is None else ((x + y) if "add" in o else (x - y)) & _M32
                r["scc"] = None
            elif o == "s_and_b32":
                x, y = _val(r, a[1]), _val(r, a[2])
                r[a[0]] = None if x is None or y is None else x & y
                r["scc"] = None if r[a[0]] is None else r[a[0]] != 0
            elif o == "s_cselect_b32":
                r[a[0]] = None if r.get("scc") is None else _val(r, a[1] if r["scc"] else a[2])
            elif o == "s_cselect_b64":
                r[a[0]] = None if r.get("scc") is None else _mask(r, a[1] if r["scc"] else a[2])
            elif o in ("s_and_b64", "s_or_b64", "s_andn2_b64", "s_orn2_b64", "s_and_saveexec_b64"):
                if o == "s_and_saveexec_b64":
                    x, y, dst = _mask(r, "exec"), _mask(r, a[1]), "exec"
                    r[a[0]] = x
                else:
                    x, y, dst = _mask(r, a[1]), _mask(r, a[2]), a[0]
                if "n2" in o:
                    y = None if y is None else not y
                # (True: all ones or, for exec, not zero -- either way `and` with an all-ones / zero mask is decided, with a per-lane mask it is not)
                if "and" in o:
                    v = False if x is False or y is False else (True if x and y else None)
                else:
                    v = True if x or y else (False if x is False and y is False else None)
                r[dst] = v
                r["scc"] = v
            elif o.startswith(("s_nop", "s_waitcnt", "s_barrier", "s_sleep", "s_setprio")):
                pass
            elif o.startswith("s_"):
                if a:
                    r[a[0]] = None
                r["scc"] = None
            elif o.startswith("v_cmp"):
                r[a[0] if a and a[0].startswith(("s[", "vcc")) else "vcc"] = None
            elif o.startswith(("v_readfirstlane", "v_readlane")):
                r[a[0]] = None
            elif o.startswith("v_") and "vcc" in a[:2]:  # (a carry out)
                r["vcc"] = None
            i = nxt if nxt is not None else (successors(ins, i) or [None])[0]
            if i is None:
                break
    return out


def walked(ins, start, stop, regs=None):
    """every instruction on a way walk_scalar finds from `start` to the first instruction `stop` names"""
    return {i for p in walk_scalar(ins, start, regs or {}, stop) for i in p}


def compared_sgprs(ins, region):
    """the scalar registers that a compare, an add or an `and` inside `region` reads"""
    regs = set()
    for i in region:
        t = ins[i][1]
        if op(t).startswith(("s_cmp_", "s_add_i32", "s_sub_i32", "s_and_b32")):
            regs |= {x for x in _operands(t) if re.fullmatch(r"s\d+", x)}
    return regs


def is_silu(t):
    """the transcendental steps of the SiLU-pair epilogue"""
    return op(t).startswith(("v_exp_f32", "v_rcp_f16"))
