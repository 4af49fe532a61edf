"""Designed accumulators for the tests of the W8A8 (SmoothQuant) kernels (a helper: no tests here, nothing pytest collects).

The int8 contraction is exact in int32, so uniformly random operands test it well.  What they cannot reach is the handful of fp32 operations behind it:
  * |acc| stays near 10^6 < 2^24 (the -128 corner's 16384 * K is a multiple of 2^14): the int -> fp32 conversion never rounds;
  * with ALPHA = 33 * 2^-16 the product f * alpha is exact for |acc| < 2^24 / 33, so a fused multiply-add and two separately rounded operations are the same number;
  * exact ties of the final rounding (n + 0.5) occur about once in 2^16 elements and never at a chosen place, and no clamp edge is placed anywhere.
The generators here build operands whose ACCUMULATORS are chosen: given one int8 row `a` of A and a target integer T, design_row() returns an int8 row b with a.b == T.
Every case asserts its property on the values actually stored before it is handed out.

The reference (reference()) is written one operation at a time, every step ONE np.float32 operation, independent of oracle/tce_oracle.c:
  acc (int64 contraction) -> f = float32(acc) -> v = f * alpha -> u = float32(bias) * beta (int8 bias) or u = bias (fp32 bias) -> v = v + u ->
  r = copysign(floor(|v| + 0.5), v) -> clamp on the rounded value -> narrow;  fp32 output with `accumulate`: C0 + v, one rounding.
(|v| + 0.5 is formed in float64, where it is exact for every fp32 v: in fp32 the sum itself would round, 0.49999997 + 0.5 -> 1.0.)

A case holds both A-row kinds: `+a` / `-a` copies of the designed row at the first and last row of a tile and in the partial edge tile (whole rows of the output judged, both
signs), and random rows (checked bit for bit like everything else, not judged).  judged(kind) is the set of elements that carry the family's property for that output
kind, decided by a predicate on the reference's own intermediates (a tie is a tie because |v| - floor|v| == 0.5 on the stored numbers, not because it was meant to be one).
"""
import functools

import numpy as np

KINDS = ("i8_bias", "i8_nobias", "relu", "f32_bias", "f32_nobias", "f32_acc")
INT8_KINDS = ("i8_bias", "i8_nobias", "relu")
FAMILIES = ("round_ties", "clamp_edges", "clamp_narrow", "clamp_far", "cvt_inexact", "separate_roundings", "minus128", "accumulate")
LONG_K_FAMILIES = ("cvt_inexact", "minus128")  # run at K = 1536 (|acc| up to 2^24 + 4 * 10^6 needs it)
SHORT_K_FAMILIES = ("round_ties", "clamp_edges", "clamp_narrow", "clamp_far", "separate_roundings")  # what K = 33 can express
NONDYADIC = (0.0071, 0.13)


# ---- the exact reference ----
def contraction(A, B, per_row=False):
    """int64 [M][N]; per_row: B is [M][N][K], row m of A meets its own B_m."""
    A, B = A.astype(np.int64), B.astype(np.int64)
    return np.einsum("mk,mnk->mn", A, B) if per_row else A @ B.T


def round_half_away(v):
    v64 = v.astype(np.float64)
    return np.copysign(np.floor(np.abs(v64) + 0.5), v64)  # exact: |v| + 0.5 needs at most 25 + 24 bits


def reference(acc, kind, alpha, beta=0.0, bias8=None, biasf=None, qmin=-128, qmax=127, C0=None):
    """-> (out, v): the output of `kind` and the fp32 value in front of the rounding / the store."""
    f = acc.astype(np.float32)  # round to nearest even (checked in the host test on 2^24 + 1, + 3)
    v = f * np.float32(alpha)
    if kind in ("i8_bias", "relu"):
        u = bias8.astype(np.float32) * np.float32(beta)
        v = v + u[None, :]
    elif kind in ("f32_bias", "f32_acc"):
        v = v + biasf.astype(np.float32)[None, :]
    assert v.dtype == np.float32 and np.all(np.abs(v.astype(np.float64)) < 2.0 ** 31), "beyond 2^31 the reference's cast is undefined"
    if kind in INT8_KINDS:
        lo = 0 if kind == "relu" and qmin < 0 else qmin
        r = np.clip(round_half_away(v), lo, qmax)
        return r.astype(np.int32).astype(np.int8), v
    if kind == "f32_acc":
        return C0.astype(np.float32) + v, v
    return v, v


# ---- designing a row of B ----
def base_row(K, rng):
    """One int8 row of A with |a_k| in [96, 127] and two reserved columns, drawn per case, that hold 1 and 127."""
    a = rng.integers(96, 128, K) * rng.choice([-1, 1], K)
    p1, p127 = rng.choice(K, 2, replace=False)
    a[p1], a[p127] = 1, 127
    return a.astype(np.int64), int(p1), int(p127)


def capacity(a, p1, p127):
    """The largest |T| design_row takes for this row."""
    free = np.ones(a.size, bool)
    free[[p1, p127]] = False
    return 126 * int(np.abs(a[free]).sum())


def design_row(a, p1, p127, T, rng):
    """An int8 row b (|b_k| <= 127) with a . b == T: b_k = +-m sign(a_k) to approach T, the remainder spread over random columns, the rest on the two reserved columns
    (x * 1 + y * 127 reaches any residual up to 127 * 128)."""
    K, T = a.size, int(T)
    assert abs(a[p1]) == 1 and abs(a[p127]) == 127
    free = np.ones(K, bool)
    free[[p1, p127]] = False
    idx = np.flatnonzero(free)
    af, sg = np.abs(a[idx]), np.sign(a[idx])
    S = int(af.sum())
    assert abs(T) <= 126 * S, f"|T| = {abs(T)} is beyond what K = {K} reaches"
    m = abs(T) // S
    b = np.zeros(K, np.int64)
    b[idx] = (1 if T >= 0 else -1) * m * sg
    amp = min(16, 127 - m - 8)
    if amp >= 1:
        b[idx] += rng.integers(-amp, amp + 1, idx.size)
    R = T - int(a @ b)
    for _ in range(64):
        if abs(R) <= 16000:
            break
        s = 1 if R > 0 else -1
        perm = rng.permutation(idx.size)
        step = s * sg[perm]
        room = 127 - step * b[idx[perm]]
        d = np.minimum(rng.integers(0, 9, idx.size), room)
        c = np.cumsum(d * af[perm])
        keep = c <= abs(R)
        if keep.any():
            b[idx[perm[keep]]] += (step * d)[keep]
            R -= s * int(c[keep][-1])
    assert abs(R) <= 16000, "design_row: the remainder does not fit the reserved columns"
    y = int(np.rint(R / 127.0))
    b[p127], b[p1] = y * np.sign(a[p127]), (R - 127 * y) * np.sign(a[p1])
    assert int(a @ b) == T and np.abs(b).max() <= 127
    return b.astype(np.int8)


def designed_rows(M, want_plus=1):
    """{row: sign}: the first and last row of the 32-, 64- and 128-row tiles and of the partial edge tile, +a and -a in turn (at least `want_plus` rows of +a)."""
    rows = sorted({r for r in (0, 15, 16, 31, 32, 63, 64, 127, 128, M - 1) if 0 <= r < M})
    out = {r: (1 if i % 2 == 0 else -1) for i, r in enumerate(rows)}
    r = 0
    while sum(1 for s in out.values() if s > 0) < min(want_plus, M) and r < M:
        out[r] = 1
        r += 1
    return out


def grid_exponent(cap, vmax):
    """The largest e with vmax * 2^e <= cap: the case's alpha is 2^-e, its accumulators are v * 2^e."""
    e = int(np.floor(np.log2(cap / vmax)))
    assert e >= 1
    return min(e, 22)


# ---- the case ----
class Case:
    def __init__(self, family, A, B, alpha, beta, bias8, biasf, qmin, qmax, C0, rows, per_row=False, kinds=KINDS):
        self.family, self.A, self.B, self.alpha, self.beta, self.bias8, self.biasf = family, A, B, float(alpha), float(beta), bias8, biasf
        self.qmin, self.qmax, self.C0, self.rows, self.per_row, self.kinds = qmin, qmax, C0, rows, per_row, tuple(kinds)
        self.M, self.K = A.shape
        self.N = B.shape[-2]
        self.acc = contraction(A, B, per_row)
        self.acc.setflags(write=False)
        self.designed = np.zeros((self.M, self.N), bool)
        self.designed[sorted(rows)] = True
        self._out, self._judged = {}, {}

    def bounds(self, kind):
        return (0 if kind == "relu" and self.qmin < 0 else self.qmin), self.qmax

    def expected(self, kind):
        """(out, v) of the exact reference."""
        if kind not in self._out:
            self._out[kind] = reference(self.acc, kind, self.alpha, self.beta, self.bias8, self.biasf, self.qmin, self.qmax, self.C0)
        return self._out[kind]

    def judged(self, kind):
        """bool [M][N]: the elements that carry the family's property for this output kind."""
        if kind not in self._judged:
            self._judged[kind] = _judged(self, kind)
        return self._judged[kind]


def is_tie(v):
    w = np.abs(v.astype(np.float64))
    return w - np.floor(w) == 0.5


def fused_value(case, kind):
    """fl(f * alpha + u) with ONE rounding.  float64 is exact here: f * alpha has at most 25 + 24 bits, and the sum with u stays within 53 bits because the families
    that use this keep |acc| < 2^25, alpha's last bit at 2^-31 or above and u a multiple of 2^-31 below 2^6 (asserted)."""
    f = case.acc.astype(np.float32).astype(np.float64)
    al = float(np.float32(case.alpha))
    assert np.abs(case.acc).max() < 2 ** 25 and (al * 2.0 ** 31) % 1.0 == 0.0
    if kind in ("i8_bias", "relu"):
        u = (case.bias8.astype(np.float32) * np.float32(case.beta)).astype(np.float64)
    elif kind in ("f32_bias", "f32_acc"):
        u = case.biasf.astype(np.float64)
    else:
        u = np.zeros(case.N)
    assert np.all((u * 2.0 ** 31) % 1.0 == 0.0) and np.abs(u).max(initial=0.0) < 64.0
    return (f * al + u[None, :]).astype(np.float32)


def _judged(case, kind):
    out, v = case.expected(kind)
    fam, d = case.family, case.designed
    if kind not in case.kinds:
        return np.zeros_like(d)
    if fam == "round_ties":
        return d & is_tie(v) if kind in INT8_KINDS else d
    if fam in ("clamp_edges", "clamp_narrow", "clamp_far"):
        return d
    if fam == "cvt_inexact":
        a = np.abs(case.acc)
        return d & (a >= 2 ** 24) & (a % 2 == 1)
    if fam == "separate_roundings":
        if kind in ("i8_nobias", "f32_nobias"):
            return np.zeros_like(d)  # (one rounding either way)
        fv = fused_value(case, kind)
        if kind in INT8_KINDS:
            lo, hi = case.bounds(kind)
            return d & (np.clip(round_half_away(fv), lo, hi) != out)
        if kind == "f32_acc":
            return d & ((case.C0 + fv).view(np.uint32) != out.view(np.uint32))
        return d & (fv.view(np.uint32) != out.view(np.uint32))
    if fam == "minus128":
        return d & case.marked_cols[None, :]  # the all -128 rows of A against the all -128, all +127 and alternating rows of B
    if fam == "accumulate":
        return case.acc_marks > 0 if kind == "f32_acc" else np.zeros_like(d)
    raise AssertionError(fam)


def _rng(family, M, N, K, seed, per_row):
    return np.random.default_rng([seed, FAMILIES.index(family), M, N, K, int(per_row)])


def _assemble(family, M, N, K, rng, a, b_rows, rows, per_row, A=None, **kw):
    """A: the designed rows as +-a, the others random (or the given activations); B: b_rows (per_row: designed rows of A meet b_rows, the others a random B_m)."""
    if A is None:
        A = rng.integers(-127, 128, (M, K)).astype(np.int8)
        for r, s in rows.items():
            A[r] = (s * a).astype(np.int8)
    if per_row:
        B = rng.integers(-127, 128, (M, N, K)).astype(np.int8)
        for r in rows:
            B[r] = b_rows
    else:
        B = b_rows
    return Case(family, A, B, rows=rows, per_row=per_row, **kw)


def _fill(fixed, N, rng, draw, offset=0):
    """N targets: the fixed list from `offset` on, then draws."""
    t = list(fixed[offset:offset + N])
    while len(t) < N:
        t.append(draw())
    return t


ROUND_J = (0, 1, 2, 3, 7, 8, 15, 16, 31, 32, 62, 63, 64, 100, 125, 126, 127, 128)
EDGES = {  # v targets as (value, steps of the grid 2^-e to add): 127.49.. is 127.5 minus one step of the case's grid (one fp32 ulp when e = 17)
    "clamp_edges": ((126.5, 0), (127.5, -1), (127.5, 0), (128.5, 0), (-128.5, 1), (-128.5, 0), (-129.5, 0), (-126.5, 0), (-127.5, 0), (-127.5, 1), (-0.5, 0), (-0.5, 1), (-1.5, 0),
                    (0.5, 0), (0.5, -1), (1.5, 0), (0.0, 0)),
    "clamp_narrow": ((-5.5, 0), (-5.5, 1), (-4.5, 0), (-6.5, 0), (9.5, 0), (9.5, -1), (8.5, 0), (10.5, 0), (-100.0, 0), (100.0, 0), (-128.5, 0), (127.5, 0), (0.5, 0), (-0.5, 0)),
    "clamp_far": ((200.0, 0), (-200.0, 0), (300.0, 0), (-300.0, 0), (200.5, 0), (-200.5, 0), (255.5, 0), (-255.5, 0), (256.0, 0), (-256.0, 0), (383.5, 0), (-384.5, 0), (127.5, 0),
                  (-128.5, 0), (511.5, 0), (-512.5, 0)),
}


@functools.lru_cache(maxsize=None)
def make_case(family, M, N, K, seed=0, per_row=False, offset=0):
    """One seeded case (deterministic: the generator is seeded by every argument).  offset: where in the family's fixed list of targets column 0 starts (launches
    with fewer columns than targets run the list in several cases).  The scalars and the biases depend on (family, N, K, offset) alone: the entries of a batch,
    which differ in `seed`, share them as one launch must."""
    return build_case(family, M, N, K, seed, per_row, offset)


def build_case(family, M, N, K, seed=0, per_row=False, offset=0, given=None):
    """given = (A int8 [M][K], {row: sign}, p1, p127): the activations are somebody else's output (LayerNormQ's); the rows named are +-(one row) with 1 and 127 in
    magnitude at p1 and p127 and 96 .. 127 elsewhere, and B is designed against them."""
    rng = _rng(family, M, N, K, seed + 1000 * offset, per_row)
    rng_b = np.random.default_rng([77, FAMILIES.index(family), N, K, offset])  # biases
    if given is None:
        a, p1, p127 = base_row(K, rng)
    else:
        A_given, rows_given, p1, p127 = given
        r0 = min(r for r, sg in rows_given.items() if sg > 0)
        a = A_given[r0].astype(np.int64)
        for r, sg in rows_given.items():
            assert np.array_equal(A_given[r].astype(np.int64), sg * a)
        free = np.ones(K, bool)
        free[[p1, p127]] = False
        assert np.all((np.abs(a[free]) >= 96) & (np.abs(a[free]) <= 127))
    # the grid of a dyadic family comes from what EVERY base row of this K reaches, not from this row's own capacity: one alpha per (family, K)
    cap = 126 * 96 * (K - 2)
    assert cap <= capacity(a, p1, p127)
    kw = dict(qmin=-128, qmax=127, C0=rng.standard_normal((M, N)).astype(np.float32))
    want_plus = 1
    if family == "round_ties":
        e = grid_exponent(cap, 170.0)
        alpha, beta = 2.0 ** -e, 0.25
        bias8 = (2 * rng_b.integers(-64, 64, N)).astype(np.int8)  # u = bias * 0.25: a multiple of 0.5, |u| <= 32
        bias8[0::3] = 0
        fixed = [s * (j + 0.5) for j in ROUND_J for s in (1.0, -1.0)]
        t = np.array(_fill(fixed, N, rng, lambda: float(rng.choice([-1.0, 1.0]) * (rng.integers(0, 130) + 0.5)), offset))
        T = np.rint((t - bias8 * 0.25) * 2.0 ** e).astype(np.int64)  # v = t on the +a rows, -t + 2u (a tie again) on the -a rows
        biasf = (rng_b.integers(-64, 65, N) * 0.5).astype(np.float32)
    elif family in EDGES:
        far = family == "clamp_far"
        e = grid_exponent(cap, 520.0 if far else 135.0)
        alpha, beta = 2.0 ** -e, 2.0 ** -3
        fixed = [val + st * 2.0 ** -e for val, st in EDGES[family]] * 2  # the list twice: without a bias (the same v with and without one), then with
        bias8 = rng_b.integers(-32, 33, N).astype(np.int8)  # |u| <= 4, on the grid
        bias8[np.arange(N) + offset < len(fixed) // 2] = 0
        t = np.array(_fill(fixed, N, rng, lambda: fixed[int(rng.integers(0, len(fixed)))], offset))
        T = np.rint((t - bias8 * 2.0 ** -3) * 2.0 ** e).astype(np.int64)
        assert np.array_equal(T * 2.0 ** -e + bias8 * 2.0 ** -3, t), "clamp: a target is off the case's grid"
        biasf = (rng_b.integers(-8, 9, N) * 0.25).astype(np.float32)
        if family == "clamp_narrow":
            kw.update(qmin=-5, qmax=9)
    elif family == "cvt_inexact":
        assert capacity(a, p1, p127) >= 2 ** 24 + 4_000_000, "cvt_inexact needs K >= 1536"
        alpha, beta = 2.0 ** -18, 1.0
        bias8 = rng_b.integers(-8, 9, N).astype(np.int8)
        n = np.arange(N) + offset
        jj = 64 + (n // 6) % 15  # (2j + 1) * 2^17 <= 2^24 + 4 * 10^6: j = 64 .. 78
        q = rng.integers(0, 1_000_000, N)
        T = np.where(n % 3 == 0, (2 * jj + 1) * 2 ** 17 - 1, 2 ** 24 + 4 * q + np.where(n % 3 == 1, 1, 3)) * np.where((n // 3) % 2 == 0, 1, -1)
        biasf = rng_b.integers(-8, 9, N).astype(np.float32)
    elif family == "separate_roundings":
        alpha, beta = NONDYADIC
        hits8 = _fused_hits()
        want_plus = -(-32 // N)
        sel = (np.arange(N) + offset)
        T, bias8 = hits8[sel % len(hits8), 0], hits8[sel % len(hits8), 1].astype(np.int8)
        # fp32 output: the columns keep their accumulators, the fp32 bias of each is searched (multiples of 2^-20 below 8, so that the fused value is exact in float64)
        biasf = _fused_bias_f32(T, alpha, rng_b)
    elif family == "minus128":
        return _minus128(M, N, K, rng, rng_b, per_row, kw)
    elif family == "accumulate":
        return _accumulate(M, N, K, rng, rng_b, a, p1, p127, per_row, kw)
    else:
        raise AssertionError(family)
    rows = designed_rows(M, want_plus) if given is None else dict(rows_given)
    b_rows = np.stack([design_row(a, p1, p127, int(Tn), rng) for Tn in T])
    case = _assemble(family, M, N, K, rng, a, b_rows, rows, per_row, A=None if given is None else A_given, alpha=alpha, beta=beta, bias8=bias8, biasf=biasf, **kw)
    for r, s in rows.items():
        assert np.array_equal(case.acc[r], s * T), "the designed accumulators are not the stored operands'"
    assert np.abs(case.A.astype(np.int64)).max() <= 127 and np.abs(case.B.astype(np.int64)).max() <= 127
    case.targets = T
    return case


@functools.lru_cache(maxsize=None)
def _fused_hits():
    """Every (acc, int8 bias) with |v| inside the clamp where fl(fl(f * alpha) + u) and fl(f * alpha + u) round to DIFFERENT int8 values under NONDYADIC (an exhaustive
    search of |acc| <= 18000 x 256 biases: about one pair in a million)."""
    alpha, beta = np.float32(NONDYADIC[0]), np.float32(NONDYADIC[1])
    acc = np.arange(-18000, 18001, dtype=np.int64)
    f = acc.astype(np.float32)
    p = f * alpha
    p64 = f.astype(np.float64) * float(alpha)
    found = []
    for b in range(-128, 128):
        u = np.float32(b) * beta
        sep = round_half_away(p + u)
        fus = round_half_away((p64 + float(u)).astype(np.float32))
        for i in np.flatnonzero((sep != fus) & (np.abs(sep) <= 127)):
            found.append((int(acc[i]), b))
    hits = np.array(found, np.int64)
    assert len(hits) >= 8, f"separate_roundings: only {len(hits)} accumulators tell a fused multiply-add apart"
    hits = hits[np.argsort(-hits[:, 0], kind="stable")]  # positive v first (the ReLU form clamps the others away)
    return hits


def _fused_bias_f32(T, alpha, rng):
    """Per column an fp32 bias (a multiple of 2^-20, |b| < 8) with fl(fl(f * alpha) + b) != fl(f * alpha + b) in bits."""
    al = np.float32(alpha)
    out = np.zeros(len(T), np.float32)
    for n, t in enumerate(T):
        f = np.float32(int(t))
        cand = (rng.integers(-(2 ** 23) + 1, 2 ** 23, 256) * 2.0 ** -20).astype(np.float32)
        sep = f * al + cand
        fus = (float(f) * float(al) + cand.astype(np.float64)).astype(np.float32)
        ok = np.flatnonzero(sep.view(np.uint32) != fus.view(np.uint32))
        assert ok.size, "separate_roundings: no fp32 bias found for a column"
        out[n] = cand[ok[0]]
    return out


def _minus128(M, N, K, rng, rng_b, per_row, kw):
    """Rows that are all -128 meet rows that are all -128, all +127 and alternating: the largest accumulators of either sign (K = 1536: 2^14 * 1536 > 2^24, exact)."""
    rows = designed_rows(M)
    A = rng.integers(-127, 128, (M, K)).astype(np.int8)
    for r in rows:
        A[r] = -128
    Bm = rng.integers(-127, 128, (N, K)).astype(np.int8)
    for n in range(N):
        if n % 4 == 0:
            Bm[n] = -128
        elif n % 4 == 1:
            Bm[n] = 127
        elif n % 4 == 2:
            Bm[n] = np.where(np.arange(K) % 2 == (n // 4) % 2, -128, 127)
    B = np.broadcast_to(Bm, (M, N, K)).copy() if per_row else Bm
    alpha = 120.0 / (16384.0 * K)  # the all -128 pair lands at 120, the -128 x +127 pair at -119.06: inside the clamp, so the sign and the size both show
    case = Case("minus128", A, B, alpha, 0.13, rng_b.integers(-32, 33, N).astype(np.int8), rng_b.standard_normal(N).astype(np.float32), rows=rows, per_row=per_row, **kw)
    assert case.acc.max() == 16384 * K and case.acc.min() == -128 * 127 * K
    case.marked_cols = np.arange(N) % 4 != 3
    return case


def _accumulate(M, N, K, rng, rng_b, a, p1, p127, per_row, kw):
    """fp32 output accumulating into C0 under a non-dyadic alpha, C0 chosen per element (marks 1 .. 4 by column):
    1: C0 = -v plus one ulp (cancellation), 2: C0 = 2^30 (v absorbed), 3: C0 = -0.0 with acc = 0 and a -0.0 bias, 4: C0 + v is an exact tie of the fp32 addition."""
    rows = designed_rows(M)
    lim = min(2_000_000, 126 * 96 * (K - 2))
    T = np.where(np.arange(N) % 4 == 2, 0, rng_b.integers(-lim, lim + 1, N))  # (with the biases: one rule for what a column is)
    T = np.where(np.arange(N) % 4 == 1, rng_b.integers(-3500, 3501, N), T)  # |v| < 32: half the spacing just below 2^30
    b_rows = np.stack([design_row(a, p1, p127, int(t), rng) for t in T])
    biasf = rng_b.standard_normal(N).astype(np.float32)
    biasf[2::4] = -0.0
    case = _assemble("accumulate", M, N, K, rng, a, b_rows, rows, per_row, alpha=NONDYADIC[0], beta=0.0, bias8=np.zeros(N, np.int8), biasf=biasf, kinds=("f32_acc",), **kw)
    v = reference(case.acc, "f32_bias", case.alpha, biasf=biasf)[0]
    C0, marks = case.C0.copy(), np.zeros((M, N), np.int8)
    col = np.arange(N)[None, :] % 4 + np.zeros((M, 1), np.int64)
    d = case.designed
    m1 = d & (col == 0) & (v != 0)
    C0[m1] = np.nextafter(-v[m1], np.float32(np.inf))
    m2 = d & (col == 1)
    C0[m2] = np.float32(2.0 ** 30)
    m3 = d & (col == 2)
    assert np.all(case.acc[m3] == 0) and np.all(v[m3] == 0)
    C0[m3] = np.float32(-0.0)
    # 4: v = odd * 2^q with 2^p <= |v| < 2^(p+1); C0 = sign(v) * 2^(p+1) is a multiple of 2^(q+1), the exact sum an odd multiple of 2^q in [1.5, 2) * 2^(p+1): a tie
    m4 = d & (col == 3) & (v != 0) & ((v.view(np.uint32) & 1) == 1) & (np.abs(v) >= 2.0 ** -100)
    p = np.floor(np.log2(np.abs(v[m4].astype(np.float64))))
    C0[m4] = (np.sign(v[m4]) * 2.0 ** (p + 1)).astype(np.float32)
    s = C0[m4].astype(np.float64) + v[m4].astype(np.float64)  # exact
    s32 = s.astype(np.float32)
    other = np.where(s32.astype(np.float64) > s, np.nextafter(s32, np.float32(-np.inf)), np.nextafter(s32, np.float32(np.inf))).astype(np.float64)
    assert np.all(s32.astype(np.float64) != s) and np.all(np.abs(s32.astype(np.float64) - s) == np.abs(other - s)), "accumulate: not a tie of the fp32 addition"
    for mk, i in ((m1, 1), (m2, 2), (m3, 3), (m4, 4)):
        marks[mk] = i
    case.C0, case.acc_marks = C0, marks
    out = case.expected("f32_acc")[0]
    assert np.all(np.abs(out[m1]) <= 2 * np.spacing(np.abs(v[m1]))) and np.all(out[m2] == np.float32(2.0 ** 30)) and np.all(out[m3].view(np.uint32) == 0)
    return case


# ---- numpy emulations of subtly wrong epilogues (the host test shows that the families catch each; `operands`: any object with the Case fields) ----
def _cvt(acc, mode):
    """int -> fp32 that truncates, or rounds ties up in magnitude, instead of to even."""
    a = np.abs(acc)
    e = np.maximum(0, np.floor(np.log2(np.maximum(a, 1).astype(np.float64))).astype(np.int64) - 23)
    q, rem = a >> e, a & ((np.int64(1) << e) - 1)
    if mode == "half_up":
        q = q + (2 * rem >= (np.int64(1) << e)) * (e > 0)
    return (np.sign(acc) * (q << e)).astype(np.float64).astype(np.float32)  # (exact: 24 or 25 significant bits with trailing zeros)


def mutant(case, kind, which):
    """The output of `kind` from an epilogue with one defect."""
    acc = case.acc
    if which == "minus128_as_plus128":
        acc = contraction(np.where(case.A == -128, 128, case.A.astype(np.int64)), case.B, case.per_row)
    f = acc.astype(np.float32)
    if which == "cvt_truncates":
        f = _cvt(acc, "trunc")
    elif which == "cvt_half_up":
        f = _cvt(acc, "half_up")
    al = np.float32(case.alpha)
    u = None
    if kind in ("i8_bias", "relu"):
        u = (case.bias8.astype(np.float32) * np.float32(case.beta))[None, :]
    elif kind in ("f32_bias", "f32_acc"):
        u = case.biasf.astype(np.float32)[None, :]
    if which == "fused":
        v = (f.astype(np.float64) * float(al) + (0.0 if u is None else u.astype(np.float64))).astype(np.float32)
    elif which == "bias_before_scaling" and u is not None:
        v = (f + u) * al
    else:
        v = f * al
        if u is not None:
            v = v + u
    if kind in INT8_KINDS:
        lo, hi = case.bounds(kind)
        if which == "clamp_before_rounding":
            return round_half_away(np.clip(v, np.float32(lo), np.float32(hi))).astype(np.int32).astype(np.int8)
        r = np.rint(v.astype(np.float64)) if which == "half_even" else round_half_away(v)
        if which == "narrow_before_clamp":
            return np.clip(r.astype(np.int64).astype(np.int8), lo, hi).astype(np.int8)
        if which == "saturating_narrow":
            lo, hi = -128, 127
        return np.clip(r, lo, hi).astype(np.int32).astype(np.int8)
    if kind == "f32_acc":
        if which == "accumulate_in_double":
            return (case.C0.astype(np.float64) + acc.astype(np.float64) * float(al) + (0.0 if u is None else u.astype(np.float64))).astype(np.float32)
        return case.C0.astype(np.float32) + v
    return v


# mutant -> the (family, output kind) pairs built to catch it
MUTANTS = {
    "fused": (("separate_roundings", "i8_bias"), ("separate_roundings", "relu"), ("separate_roundings", "f32_bias"), ("separate_roundings", "f32_acc")),
    "half_even": (("round_ties", "i8_bias"), ("round_ties", "i8_nobias"), ("round_ties", "relu")),
    "cvt_truncates": (("cvt_inexact", "i8_bias"), ("cvt_inexact", "i8_nobias"), ("cvt_inexact", "f32_nobias"), ("cvt_inexact", "f32_bias")),
    "cvt_half_up": (("cvt_inexact", "f32_nobias"), ("cvt_inexact", "f32_bias")),
    "narrow_before_clamp": (("clamp_far", "i8_bias"), ("clamp_far", "i8_nobias"), ("clamp_far", "relu")),
    "saturating_narrow": (("clamp_narrow", "i8_bias"), ("clamp_narrow", "i8_nobias"), ("clamp_edges", "relu")),
    "bias_before_scaling": (("separate_roundings", "i8_bias"), ("round_ties", "i8_bias"), ("separate_roundings", "f32_bias")),
    "minus128_as_plus128": (("minus128", "i8_bias"), ("minus128", "i8_nobias"), ("minus128", "f32_nobias")),
    "accumulate_in_double": (("accumulate", "f32_acc"),),
}
# clamp(round(v)) == round(clamp(v)) for integer bounds: rounding is monotone and leaves the bounds where they are.  Not a defect, so no family can (or should) tell it apart.
EQUIVALENT = ("clamp_before_rounding",)


def families_for(K):
    """The families a launch with this K can express (the generic kernel's K = 33 runs the short list)."""
    return [f for f in FAMILIES if f in SHORT_K_FAMILIES or (K >= 1536 and f in LONG_K_FAMILIES) or (f == "accumulate" and K >= 64)]


# ---- the table of launches: the GPU test runs these, the host test proves every case of them sound ----
class Form:
    """One kernel form of launch_w8a8: the smallest shape that reaches it with partial edge tiles, the switches that force it, and what the dispatcher must call it."""

    def __init__(self, name, M, N, Ks, describe, tuning=(0, 0, 0), modes=(), scratch=False, per_row=False, batch=1, ld=(0, 0, 0)):
        self.name, self.M, self.N, self.Ks, self.describe, self.tuning, self.modes = name, M, N, tuple(Ks), describe, tuple(tuning), tuple(modes)
        self.scratch, self.per_row, self.batch, self.ld = scratch, per_row, batch, tuple(ld)

    def kinds(self):
        return ("i8_nobias", "f32_nobias") if self.per_row else KINDS  # (the *_batch members have no bias and no `accumulate` counterpart in the reference)

    def families(self, K):
        return [f for f in families_for(K) if not (self.per_row and f in ("accumulate", "separate_roundings"))]

    def cases(self):
        """[(family, K, offset)]: a launch with fewer columns than a family has fixed targets runs the list in several cases."""
        out = []
        for K in self.Ks:
            for fam in self.families(K):
                if len(self.Ks) > 1 and K == max(self.Ks) and fam not in LONG_K_FAMILIES:
                    continue  # (the long K of a tiled form runs what the short one cannot express)
                n_fixed = {"round_ties": 2 * len(ROUND_J), "cvt_inexact": 90}.get(fam, 2 * len(EDGES.get(fam, ())))
                for off in range(0, max(n_fixed, 1), self.N) if self.N < n_fixed else (0,):
                    out.append((fam, K, off))
        return out


TILE_KS = (1088, 1536)  # 17 k-steps (odd, prime: no even split over quartets) and 24 (the cut across workgroups, cvt_inexact, minus128)
# debug modes (tce_w4a16_set_debug_mode): 191 / 192 the 32 x 64 tiles forced / off, 19001 the k-slice forms off, 19304 / 19404 / 19904 forced, 182 / 188 the cut forced
FORMS = (
    Form("generic", 5, 7, (33,), "w8a8 generic (one output per thread)"),
    Form("wave-per-column rows=1", 1, 70, (1536,), "w8a8 wave-per-column rows=1"),
    Form("wave-per-column rows=2", 2, 70, (1536,), "w8a8 wave-per-column rows=2"),
    Form("wave-per-column rows=4", 4, 70, (1536,), "w8a8 wave-per-column rows=4"),
    Form("wave-per-column rows=8", 8, 70, (2048,), "w8a8 wave-per-column rows=8"),
    Form("wave-per-output", 5, 9, (1536,), "w8a8 wave-per-output (a B per row of A)", per_row=True),
    Form("64x64 quartets=1", 70, 100, TILE_KS, "w8a8 tile=64x64 quartets=1", tuning=(1, 0, 0), modes=(192,)),
    Form("64x64 quartets=2", 70, 100, TILE_KS, "w8a8 tile=64x64 quartets=2", tuning=(2, 0, 0), modes=(192,)),
    Form("64x64 quartets=4", 70, 100, TILE_KS, "w8a8 tile=64x64 quartets=4", tuning=(4, 0, 0), modes=(192,)),
    Form("32x64 quartets=1", 70, 100, TILE_KS, "w8a8 tile=32x64 quartets=1", tuning=(1, 0, 0), modes=(191,)),
    Form("32x64 quartets=2", 70, 100, TILE_KS, "w8a8 tile=32x64 quartets=2", tuning=(2, 0, 0), modes=(191,)),
    Form("deep-pipeline quartets=1", 70, 100, TILE_KS, "w8a8 tile=64x64 deep-pipeline quartets=1", tuning=(0, 0, 1)),
    Form("deep-pipeline quartets=2", 70, 100, TILE_KS, "w8a8 tile=64x64 deep-pipeline quartets=2", tuning=(0, 0, 2)),
    Form("deep-pipeline quartets=4", 70, 100, TILE_KS, "w8a8 tile=64x64 deep-pipeline quartets=4", tuning=(0, 0, 4)),
    Form("kcut by the rule", 70, 100, (1536,), "w8a8 tile=64x64 quartets=2 kcut=4", modes=(19001,), scratch=True),
    Form("kcut=2", 70, 100, (1536,), "w8a8 tile=64x64 quartets=2 kcut=2", modes=(19001, 182), scratch=True),
    Form("kcut=8", 70, 100, (1536,), "w8a8 tile=64x64 quartets=1 kcut=8", modes=(19001, 188), scratch=True),
    Form("k-slice 32x48", 70, 100, TILE_KS, "w8a8 k-slice tile=32x48 waves=4 workgroups=9", modes=(19304,)),
    Form("k-slice 32x64", 70, 100, TILE_KS, "w8a8 k-slice tile=32x64 waves=4 workgroups=6", modes=(19404,)),
    Form("k-slice 64x64", 70, 100, TILE_KS, "w8a8 k-slice tile=64x64 waves=4 workgroups=4", modes=(19904,)),
    Form("128x128 quartets=1", 130, 130, TILE_KS, "w8a8 tile=128x128 quartets=1", tuning=(0, 1, 0)),
    Form("128x64 quartets=1", 130, 130, TILE_KS, "w8a8 tile=128x64 quartets=1", tuning=(0, 2, 0)),
    Form("128x128 quartets=2", 130, 130, TILE_KS, "w8a8 tile=128x128 quartets=2", tuning=(0, 3, 0)),
    Form("128x64 quartets=2", 130, 130, TILE_KS, "w8a8 tile=128x64 quartets=2", tuning=(0, 4, 0)),
    Form("64x64 quartets=2, batch of 2, leading dimensions", 70, 100, (1088,), "w8a8 tile=64x64 quartets=2", tuning=(2, 0, 0), modes=(192,), batch=2, ld=(1104, 1120, 112)),
    Form("k-slice 32x48, batch of 2, leading dimensions", 70, 100, (1536,), "w8a8 k-slice tile=32x48 waves=4 workgroups=18", modes=(19304,), batch=2, ld=(1552, 1568, 116)),
    Form("wave-per-column rows=2, batch of 2, leading dimensions", 2, 70, (1536,), "w8a8 wave-per-column rows=2", batch=2, ld=(1552, 1568, 80)),
)
RESTORE_MODES = (70, 75, 170, 180, 190, 19000)  # every switch back to its rule


def launched_cases():
    """Every make_case argument set the GPU test's form sweep launches, once."""
    seen = []
    for form in FORMS:
        for fam, K, off in form.cases():
            for b in range(form.batch):
                key = (fam, form.M, form.N, K, b, form.per_row, off)
                if key not in seen:
                    seen.append(key)
    return seen


# ---- LayerNormQ: a numpy restatement with sequential fp32 sums ----
def layernorm_q_exact(x, w, b):
    """LayerNormQ::forward one np.float32 operation at a time, the two sums sequential (all rows at once, element after element)."""
    x = x.astype(np.float32)
    m, n = x.shape
    mean = np.zeros(m, np.float32)
    for k in range(n):
        mean = mean + x[:, k]
    mean = mean / np.float32(n)
    d = x - mean[:, None]
    p = d * d
    sq = np.zeros(m, np.float32)
    for k in range(n):
        sq = sq + p[:, k]
    std = np.sqrt(sq / np.float32(n) + np.float32(0.00001))
    f = (d / std[:, None]) * w.astype(np.float32)[None, :] + b.astype(np.float32)[None, :]
    assert np.all(np.abs(f) < 2.0 ** 31)
    return round_half_away(f).astype(np.int64).astype(np.int32).astype(np.int8), f  # (no clamp in the reference: the narrowing wraps)


def designed_activations(m, k, seed):
    """x fp32 [m][k] whose LayerNormQ output is a designable row: x = +-1 in equal numbers (mean 0, variance 1, both sums exact), the affine weight an integer + 0.3 in
    96.3 .. 127.3 (1.3 and 127.3 at the two reserved columns), no affine bias: q_k = +-floor(w_k).  Row 1 is -row 0, the others are other sign patterns."""
    rng = np.random.default_rng([seed, m, k])
    s = rng.permutation(np.repeat([1.0, -1.0], k // 2))
    x = np.stack([s, -s] + [rng.permutation(s) for _ in range(m - 2)])[:m].astype(np.float32)
    w = (rng.integers(96, 128, k) + 0.3).astype(np.float32)
    p1, p127 = (int(p) for p in rng.choice(k, 2, replace=False))
    w[p1], w[p127] = 1.3, 127.3
    return x, w, np.zeros(k, np.float32), p1, p127


def layernorm_rows(m, n):
    """x [m][n], w, b for tce_layernorm_q alone -> (x, w, b, the exact int8 output, the fp32 values in front of the rounding, the tie columns): a constant row, rows with
    one outlier, Gaussian rows; columns with w = 0 and b = j + 0.5 in both signs (exact ties whatever the row), columns with |w| = 400 (outputs far beyond +-127)."""
    rng = np.random.default_rng(m + n)
    x = (rng.standard_normal((m, n)) * 2 + 0.25).astype(np.float32)
    x[0] = 0.7                                   # a constant row: every deviation the same tiny number or zero
    x[1] = 3.0
    x[1, n // 3] = 1.0e4                         # one outlier
    if m > 2:
        x[2] = rng.standard_normal(n).astype(np.float32) * np.float32(1e-3)
        x[2, n - 1] = -5.0e5
    w = (rng.standard_normal(n) * 20).astype(np.float32)
    b = (rng.standard_normal(n) * 5).astype(np.float32)
    ties = np.array([s * (j + 0.5) for j in (0, 1, 2, 62, 63, 126, 127, 128, 200) for s in (1.0, -1.0)], np.float32)
    cols = np.arange(ties.size) * (n // ties.size)
    w[cols], b[cols] = 0.0, ties
    far = cols[:-1] + 1
    w[far] = 400.0 * np.where(np.arange(far.size) % 2 == 0, 1.0, -1.0)  # |t| is about 1 on the Gaussian rows: outputs far beyond +-127
    want, f = layernorm_q_exact(x, w, b)
    assert np.all(np.abs(f[:, cols]) == np.abs(ties)[None, :]) and (np.abs(f[:, far]) > 128.5).any()
    return x, w, b, want, f, cols


ATTENTION_SCALES = (1.0e-3, 2.0 ** -7)  # a_qk, a_pv


def attention_tie_case(heads, hd, m, pos, max_keys):
    """Inputs of one OPT attention decode step whose pv product is made of exact ties -> (q, k, v, k cache, v^T cache, mask, the (cached, new) key pair of every row, the
    exact int8 attention rows, the number of ties)."""
    E, tgz = heads * hd, pos + m
    rng = np.random.default_rng(heads + hd + pos)
    a_qk, a_pv = ATTENTION_SCALES
    kc0 = rng.integers(-128, 128, (heads, max_keys, hd)).astype(np.int8)
    vt0 = rng.integers(-128, 128, (heads, hd, max_keys)).astype(np.int8)
    q = rng.integers(-128, 128, (m, E)).astype(np.int8)
    k = rng.integers(-128, 128, (m, E)).astype(np.int8)
    v = rng.integers(-128, 128, (m, E)).astype(np.int8)
    mask = np.full((m, tgz), np.finfo(np.float32).min, np.float32)
    pairs = []
    for r in range(m):
        cached, new = 1 + 2 * r, pos + r
        assert cached < pos  # (key 0 stays masked: row (0, 0)'s first probability, the start of every later row's maximum, is then 0)
        pairs.append((cached, new))
        mask[r, [cached, new]] = 0.0
        for h in range(heads):
            qh = q[r, h * hd:(h + 1) * hd].astype(np.int64)
            key = (np.where(qh >= 0, 1, -1) * rng.integers(1, 4, hd)).astype(np.int8)  # q . key > 0: the row's maximum is its own tie score, not the 0 it starts from
            kc0[h, cached], k[r, h * hd:(h + 1) * hd] = key, key
            sums = np.concatenate([[251, -255, 253, -253, -256, 254, 1, -1, 3, -3, 127, -127], rng.integers(-127, 127, hd - 12) * 2 + 1])[rng.permutation(hd)]  # (two int8 reach -256 .. 254)
            v1 = np.clip(sums // 2 + rng.integers(-20, 21, hd), np.maximum(-128, sums - 127), np.minimum(127, sums + 128))
            vt0[h, :, cached], v[r, h * hd:(h + 1) * hd] = v1.astype(np.int8), (sums - v1).astype(np.int8)
            assert np.array_equal(vt0[h, :, cached].astype(np.int64) + v[r, h * hd:(h + 1) * hd], sums)
    # the exact reference: int8 probabilities 64 / 64, the pv product through w8a8_cases.reference
    want = np.zeros((m, E), np.int8)
    ties = 0
    for r, (c1, c2) in enumerate(pairs):
        for h in range(heads):
            vnew = v[r, h * hd:(h + 1) * hd].astype(np.int64)
            acc = (64 * (vt0[h, :, c1].astype(np.int64) + vnew))[None, :]
            out, vv = reference(acc, "i8_nobias", a_pv)
            want[r, h * hd:(h + 1) * hd] = out[0]
            ties += int(is_tie(vv).sum())
    assert ties >= m * heads * hd // 4
    return q, k, v, kc0, vt0, mask, pairs, want, ties
