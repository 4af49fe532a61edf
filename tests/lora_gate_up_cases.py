"""Designed operands for the gate/up LoRA launch (tce_lora_expand_silu_mul_f16, tinychatengine_amd/csrc/lora.hip), built from the generators of tests/lora_cases.py
and shared by tests/test_lora_gate_up_host.py (CPU) and tests/test_gpu_lora_gate_up.py.

A case is a dict: x fp16 [rows][K], A fp16 [n][2R][K] (rows 0 .. R-1 gate's, R .. 2R-1 up's), Bg / Bu fp16 [n][R][N], scale fp32 [n], y fp16 [rows][2N] (what the
base gate_up linear left behind: column 2n = gate n, column 2n + 1 = up n).  lora_cases' generator is asked for rank 2R, so its claims (exact: no fp32 partial result
rounds; bounded: finite, with cancellation rows and an outlier row) hold for the stacked shrink and for sums over ALL 2R rows -- a fortiori for each segment's R.

    block_structured(case)   the same adapter as ONE ordinary expand: B' fp16 [n][2R][2N], gate's rows in the even columns, up's rows in the odd columns, zeros
                             elsewhere -- a lora_cases case {x, A, B, scale, C = y} whose result, de-interleaved, is (g, u)
    segment(case, which)     gate's or up's half as a lora_cases case of its own: A's R rows, Bg or Bu, C = y's even or odd columns -- what the kernel sums
"""
import numpy as np

import lora_cases as lc


def gate_up_case(kind: str, seed: int, rows: int, K: int, N: int, R: int, n: int) -> dict:
    make = {"exact": lc.exact_case, "bounded": lc.bounded_case}[kind]
    a, b = make(seed, rows, K, N, 2 * R, n), make(seed + 1000, rows, K, N, 2 * R, n)  # (b: only its C is used -- up's half of y)
    y = np.empty((rows, 2 * N), np.float16)
    y[:, 0::2], y[:, 1::2] = a["C"], b["C"]
    return {"kind": kind, "x": a["x"], "A": a["A"], "Bg": np.ascontiguousarray(a["B"][:, :R]), "Bu": np.ascontiguousarray(a["B"][:, R:]), "scale": a["scale"], "y": y}


def block_structured(case: dict) -> dict:
    n, R, N = case["Bg"].shape
    B = np.zeros((n, 2 * R, 2 * N), np.float16)
    B[:, :R, 0::2], B[:, R:, 1::2] = case["Bg"], case["Bu"]
    return {"kind": case["kind"], "x": case["x"], "A": case["A"], "B": B, "scale": case["scale"], "C": case["y"]}


def segment(case: dict, which: str) -> dict:
    R = case["Bg"].shape[1]
    rows, B, cols = (slice(0, R), case["Bg"], slice(0, None, 2)) if which == "gate" else (slice(R, 2 * R), case["Bu"], slice(1, None, 2))
    return {"kind": case["kind"], "x": case["x"], "A": np.ascontiguousarray(case["A"][:, rows]), "B": B, "scale": case["scale"], "C": np.ascontiguousarray(case["y"][:, cols])}


def words_patterns(rows: int, n: int) -> dict:
    """lora_cases.patterns plus one that carries -7 and n (one past the pool) in every block of four beside two adapters"""
    pats = dict(lc.patterns(rows, n))
    pats["outside"] = np.array([[-7, 0, n, n - 1][i % 4] for i in range(rows)], np.int64)
    return pats


# the host test's shapes (rows, K, N, R, n): numpy's emulation stays quick
HOST_SHAPES = [(1, 8, 8, 8, 1), (5, 520, 40, 24, 4), (3, 2056, 8, 96, 1), (17, 72, 520, 8, 4)]
