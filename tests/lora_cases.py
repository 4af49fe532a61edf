"""Designed operands for the LoRA kernels (tinychatengine_amd/csrc/lora.hip), shared by tests/test_lora_host.py (CPU) and tests/test_gpu_lora.py.

A case is a dict: x fp16 [rows][K], A fp16 [n][R][K], B fp16 [n][R][N], scale fp32 [n], C fp16 [rows][N] (what the base linear left behind).  The adapter words are
not part of a case: patterns(rows, n) gives the index patterns every case is run under.

    exact     x, A in {-2 .. 2}, B in {-1, 0, 1}, scale = 2^-10, C a multiple of 2^-10 with |C| < 2^13.  With K <= 14336 and R <= 192: |t| <= 4 K < 2^16, every partial
              sum of the expand is an integer below 192 * 2^16 < 2^24, and float(C) + 2^-10 * sum is a multiple of 2^-10 below 2^14 (the generator asserts both on the data it
              made): 24 bits hold it.  Every fp32
              partial result is exact in ANY summation order, fused or not, so the kernels must equal lora_reference BIT FOR BIT (test_lora_host.py checks the claim with two
              fp32 emulations).
    bounded   Gaussian operands, rows whose delta cancels against C (C = -delta rounded: the result is what the roundings leave), and one row of x scaled to the 2^15
              range.  Held per element to bound(): |got - ref64| <= 1/2 ulp16(ref64) + (K + R + 2) 2^-24 (|C| + |s| sum_j (sum_k |x A|) |B_jn|) -- the first-order bound
              of fp32 accumulation in any order (K - 1 adds in the shrink; one product and R - 1 adds per term in the expand; the scale and the last add) plus the one
              rounding to fp16.  No floor, no element left out.
"""
import numpy as np

from tinychatengine_amd.lora import lora_reference

INT32_MAX = 2 ** 31 - 1


def exact_case(seed: int, rows: int, K: int, N: int, R: int, n: int) -> dict:
    assert K <= 14336 and R <= 192
    rng = np.random.default_rng(seed)
    x = rng.integers(-2, 3, (rows, K)).astype(np.float16)
    A = rng.integers(-2, 3, (n, R, K)).astype(np.float16)
    B = rng.integers(-1, 2, (n, R, N)).astype(np.float16)
    x[0, :] = 2  # the largest sums the design allows: |t| = 4 K against an all-2 adapter, and as many B rows of 1 as keep 2^-10 * sum at 2^13 or below
    A[0, :, :] = 2
    B[0, :, :] = 0
    B[0, :min(R, 2 ** 21 // K), :] = 1
    # multiples of 2^-10 that binary16 holds: |C| < 1 on the 2^-10 grid, integers up to 2048, multiples of 4 up to 8188
    kind = rng.integers(0, 3, (rows, N))
    C = np.where(kind == 0, rng.integers(-1023, 1024, (rows, N)) * 2.0 ** -10, np.where(kind == 1, rng.integers(-2048, 2049, (rows, N)), rng.integers(-2047, 2048, (rows, N)) * 4.0))
    C16 = C.astype(np.float16)
    assert np.array_equal(C16.astype(np.float64), C) and np.abs(C).max() < 2 ** 13
    case = {"kind": "exact", "x": x, "A": A, "B": B, "scale": np.full(n, 2.0 ** -10, np.float32), "C": C16}
    # the claim, held on THIS data for every (row, adapter): sums of absolute values bound every partial sum of any order -- integers below 2^24 -- and the result is
    # a multiple of 2^-10 below 2^14: 24 bits
    for a in range(n):
        mag = (np.abs(x.astype(np.float64)) @ np.abs(A[a].astype(np.float64)).T) @ np.abs(B[a].astype(np.float64))
        assert mag.max() < 2 ** 24 and (np.abs(C) + mag * 2.0 ** -10).max() < 2 ** 14
    return case


def bounded_case(seed: int, rows: int, K: int, N: int, R: int, n: int) -> dict:
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (rows, K))
    big = rows - 1  # the outlier row: the 2^15 range (|x| <= 1.9 * 2^15 < 65504)
    x[big] = np.clip(x[big], -1.9, 1.9) * 2.0 ** 15
    x = x.astype(np.float16)
    A = (rng.normal(0, 1, (n, R, K)) / np.sqrt(K)).astype(np.float16)
    B = (rng.normal(0, 1, (n, R, N)) / np.sqrt(R)).astype(np.float16)
    scale = rng.uniform(0.05, 0.125, n).astype(np.float32)  # (the outlier row's delta then stays below ~2^14)
    C = rng.normal(0, 1, (rows, N)).astype(np.float16)
    case = {"kind": "bounded", "x": x, "A": A, "B": B, "scale": scale, "C": C}
    # cancellation rows (every third, never the outlier): C = -delta under the adapter `different` gives the row, so that pattern leaves only what the roundings leave
    words = patterns(rows, n)["different"]
    d = delta64(case, words)
    for i in range(0, rows - 1, 3):
        C[i] = (-d[i]).astype(np.float16)
    assert np.isfinite(C.astype(np.float64)).all()
    return case


def patterns(rows: int, n: int) -> dict:
    """The index patterns: every word -1; every row on the last adapter; row i on adapter i % n; and a mix that includes n (one past the pool), -7 and 2^31 - 1."""
    mixed = np.array([[0, n, -7, n - 1, INT32_MAX, -1][i % 6] for i in range(rows)], np.int64)
    return {"none": np.full(rows, -1, np.int64), "one": np.full(rows, n - 1, np.int64), "different": np.arange(rows, dtype=np.int64) % n, "mixed": mixed}


def _by_adapter(case: dict, words):
    n = case["A"].shape[0]
    words = np.asarray(words).astype(np.int64)
    for a in range(n):
        rows = np.nonzero(words == a)[0]
        if rows.size:
            yield a, rows


def delta64(case: dict, words) -> np.ndarray:
    """float64 [rows][N]: scale[a] * sum_j (sum_k x A) B of every row's adapter, 0 for a row without one"""
    out = np.zeros(case["C"].shape, np.float64)
    for a, rows in _by_adapter(case, words):
        t = case["x"][rows].astype(np.float64) @ case["A"][a].astype(np.float64).T
        out[rows] = np.float64(case["scale"][a]) * (t @ case["B"][a].astype(np.float64))
    return out


def reference64(case: dict, words) -> np.ndarray:
    """float64 [rows][N], NOT rounded to fp16 (what bound() is centred on); an untouched row is float(C)"""
    return case["C"].astype(np.float64) + delta64(case, words)


def reference(case: dict, words) -> np.ndarray:
    """lora_reference on the case: fp16 [rows][N]"""
    return lora_reference(case["x"], case["A"], case["B"], case["scale"], words, case["C"])


def ulp16(v: np.ndarray) -> np.ndarray:
    """The spacing of binary16 at |v| (float64 in, float64 out): 2^(floor(log2 |v|) - 10), 2^-24 in the subnormal range"""
    a = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return np.exp2(e - 10)


def bound(case: dict, words) -> np.ndarray:
    """float64 [rows][N]: the per-element bound of the module docstring (rows without an adapter: 0 -- they keep their bits)"""
    K, R = case["A"].shape[2], case["A"].shape[1]
    ref = reference64(case, words)
    mag = np.zeros(case["C"].shape, np.float64)
    touched = np.zeros(case["C"].shape[0], bool)
    for a, rows in _by_adapter(case, words):
        tabs = np.abs(case["x"][rows].astype(np.float64)) @ np.abs(case["A"][a].astype(np.float64)).T
        mag[rows] = np.abs(case["C"][rows].astype(np.float64)) + abs(float(case["scale"][a])) * (tabs @ np.abs(case["B"][a].astype(np.float64)))
        touched[rows] = True
    b = 0.5 * ulp16(ref) + (K + R + 2) * 2.0 ** -24 * mag
    b[~touched] = 0.0
    return b


def emulate_fp32(case: dict, words, order: str) -> np.ndarray:
    """The two kernels in numpy fp32, every product and sum rounded to fp32 (unfused), in one of two summation orders -> fp16 [rows][N]:
         "sequential"  k ascending in ONE accumulator; j ascending
         "lanes"       64 interleaved accumulators over the 8-element pieces (piece c in accumulator c % 64), met in a binary tree; j ascending in the expand"""
    f32 = np.float32
    out = case["C"].copy()
    K = case["A"].shape[2]
    for a, rows in _by_adapter(case, words):
        A = case["A"][a].astype(f32)
        for i in rows:
            prod = A * case["x"][i].astype(f32)[None, :]  # [R][K], exact
            if order == "sequential":
                t = np.cumsum(prod, axis=1, dtype=f32)[:, -1]
            else:
                pieces = K // 8
                pad = (-pieces) % 64
                p = np.concatenate([prod, np.zeros((prod.shape[0], pad * 8), f32)], axis=1).reshape(prod.shape[0], -1, 64, 8)  # [R][step][lane][8]
                lanes = np.zeros((prod.shape[0], 64), f32)
                for s in range(p.shape[1]):
                    for e in range(8):
                        lanes = (lanes + p[:, s, :, e]).astype(f32)
                w = 32
                while w >= 1:
                    lanes = (lanes[:, :w] + lanes[:, w:2 * w]).astype(f32)
                    w //= 2
                t = lanes[:, 0]
            acc = np.zeros(case["B"].shape[2], f32)
            Bf = case["B"][a].astype(f32)
            for j in range(Bf.shape[0]):
                acc = (acc + (t[j] * Bf[j]).astype(f32)).astype(f32)
            with np.errstate(over="ignore"):
                out[i] = (case["C"][i].astype(f32) + (case["scale"][a] * acc).astype(f32)).astype(f32).astype(np.float16)
    return out


# the shapes the GPU test launches: (rows, K, N, R, n_adapters, patterns).  K 8 / 2056 / 14336 (one piece; 257 pieces: four full steps of 64 lanes and one lane more;
# the largest), N 8 / 1032 / 6144 (one lane; two full workgroups and one lane of a third; twelve workgroups), R 8 / 48 / 192, rows 1 / 3 / 17 / 130 (17: a second block of one
# row; 130: nine blocks, the last of two rows; more than one pass of four in a block wherever rows share an adapter), 1 and 4 adapters.
GPU_SHAPES = [
    (1, 8, 8, 8, 1, ("none", "one", "mixed")),
    (3, 2056, 1032, 48, 4, ("none", "one", "different", "mixed")),
    (17, 14336, 1032, 192, 1, ("one", "mixed")),
    (130, 2056, 8, 8, 4, ("one", "different", "mixed")),
    (130, 8, 6144, 48, 1, ("one", "mixed")),
    (17, 2056, 1032, 192, 4, ("none", "one", "different", "mixed")),
]
# the host test's shapes: the same generators where numpy's emulation stays quick
HOST_SHAPES = [(1, 8, 8, 8, 1), (3, 2056, 1032, 48, 4), (3, 14336, 8, 192, 1), (17, 520, 40, 8, 4)]
