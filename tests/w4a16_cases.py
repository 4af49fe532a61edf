"""Designed weights and activations for the tests of the W4A16 kernels (a helper: no tests here, nothing pytest collects).

Gaussian weights through the quantizer against Gaussian activations give group scales that all sit near 0.005, a zero-mean q - z, a row sum of about sqrt(K), partial
sums that never grow and no element more than 2^4 below its block's maximum: the regime in which the kernels' own numerical arguments were made (the bias-and-subtract
unpack of w4a16_gemv.hip, the block exponent of w4a16_gemv_i8.hip, the rescale chain of w4a16_gemm_pk.hip).  The generators here build operands outside it and ASSERT
the property each was designed for on the values actually stored, after every rounding, before they hand a case out.

A case is (a f16 [M][K], qweight u32 [N][K/8], scales f16 [N][zw*8], zeros u32 [N][zw]) in the q4_6 layout of oracle.pack_q4_6, plus the judged column sets.
Reference: float64, a @ ((q - z) * s)^T on the stored values -- NOT the oracle's sequential fp32 sum.  Judging: conftest.w4a16_close unchanged (1e-3 * max(|ref|,
rms/64), ratio <= 1.0), per activation row and per judged column set, so that rms is the set's own; in every judged set at most 5 % of the elements may sit under the
floor (|ref| < rms/64), or the floor would be what passes the case (floor_share).  That cap holds BY CONSTRUCTION, it is not evidence about a generator: a Gaussian
row that would break it is drawn again (make_activations), and a set that breaks it by design is split until every part keeps it (sets_for) -- which makes the judging
stricter, never looser: a split-off part is held to 1e-3 of ITS OWN rms.  What shows a badly designed family is the host test's oracle <= 0.6 on every part.

Where a family's parameters leave what ANY correct kernel can store in binary16 they are scaled, never the bound (each place says so):
  * `ladder` uses 1024-wide k blocks where K > 1024; on a shorter K the four scales take a quarter of K each (whole 32s): one block alone would be the 2^-12 one and
    every output a binary16 subnormal, whose spacing (2^-24) is coarser than the bound.  Likewise `scale_ladder` on fewer than three
    groups ends its rotation on the middle rung (two groups: 2^6, 1; one group: 1), not on 2^-10 alone.
  * the `outlier` row of a `mixed_rows x scale_ladder` launch has its 2^15 in a group of the ladder's middle rung (k0 moves by whole groups): against a 2^6 scale
    2^15 * 15 * 0.4 overflows binary16 in every column.
  * a `mixed_rows` launch cannot give its `subnormal` row the sigma-200 weights the family needs (the weights are the launch's): that row is 2^-7 * g there
    (`small`) -- 2^22 below the `outlier` row's maximum in the same launch, its outputs still normal halves.  Subnormal activations themselves: the pair of their own.
"""
import numpy as np

from conftest import w4a16_close

HALF_MAX = 65504.0
FLOOR_CAP = 0.05
ACT_FAMILIES = ("gauss", "positive", "dc", "outlier", "ladder", "subnormal", "sparse")
WEIGHT_FAMILIES = ("random", "coherent", "balanced", "extreme", "scale_ladder", "subnormal_scale", "null_at_outlier", "sigma200")
LADDER_ACT = (2.0 ** -12, 1.0, 2.0 ** 8, 2.0 ** -6)
LADDER_SCALE = (2.0 ** -10, 2.0 ** 6, 1.0)
OUTLIER = 2.0 ** 15
OUTLIER_FLOOR = 2.0 ** -4  # 2^(15 - 19): the i8 kernel documents every element within 2^19 of its block's maximum as exact

# name, activation family, weight family, activation multiplier
PAIRS = (
    ("gauss x random", "gauss", "random", 1.0),
    ("positive x coherent", "positive", "coherent", 1.0),
    ("positive x random", "positive", "random", 1.0),
    ("dc x balanced", "dc", "balanced", 1.0),
    ("dc x random", "dc", "random", 1.0),
    ("outlier x null_at_outlier", "outlier", "null_at_outlier", 1.0),
    ("ladder x random", "ladder", "random", 1.0),
    ("ladder x scale_ladder", "ladder", "scale_ladder", 1.0),
    ("gauss x scale_ladder", "gauss", "scale_ladder", 1.0),
    ("gauss x extreme", "gauss", "extreme", 1.0),
    ("subnormal x sigma200", "subnormal", "sigma200", 1.0),
    ("gauss*64 x subnormal_scale", "gauss", "subnormal_scale", 64.0),
    ("sparse x random", "sparse", "random", 1.0),
)
PAIR_NAMES = tuple(p[0] for p in PAIRS)
Z8_PAIRS = ("dc x balanced", "subnormal x sigma200")  # the pairs whose zero points are all 8 (the all-8 fast paths, the AWQ layout)
MIXED = ("mixed_rows x random", "mixed_rows x scale_ladder")
MIXED_ROWS = tuple("small" if f == "subnormal" else f for f in ACT_FAMILIES)  # row r of a launch takes entry r mod 7
# decode launches are too short for the rotation to put rows of different ranges side by side (M = 2: gauss, positive): they also run these
DECODE_ROWS = {2: (MIXED_ROWS[:2], ("outlier", "small")), 4: (MIXED_ROWS[:4], MIXED_ROWS[3:7])}


# ---- layout ----
def zeros_width(K, G):
    mult = {128: 1, 64: 2, 32: 4}[G]
    w = (K // G + 7) // 8
    return (w + mult - 1) // mult * mult


def pack_q4_6(codes, z, s, G):
    """codes u8 [N][K], z u8 [N][K/G], s f16 [N][K/G] -> qweight u32 [N][K/8] (nibble i of word j = code 8j + i), scales f16 [N][zw*8] (zero padded),
    zeros u32 [N][zw] (nibble g % 8 of word g / 8; the padding nibbles are 8, as the quantizer leaves them)."""
    N, K = codes.shape
    ng, zw = K // G, zeros_width(K, G)
    sh = (np.arange(8, dtype=np.uint32) * 4)
    qw = (codes.astype(np.uint32).reshape(N, K // 8, 8) << sh).sum(axis=2).astype(np.uint32)
    sc = np.zeros((N, zw * 8), np.float16)
    sc[:, :ng] = s
    zn = np.full((N, zw * 8), 8, np.uint32)
    zn[:, :ng] = z
    zp = (zn.reshape(N, zw, 8) << sh).sum(axis=2).astype(np.uint32)
    return qw, sc, zp


def k0_for(K, where="last"):
    """Where the outlier sits: word 1, element 5 of the second 32-weight chunk (mid-chunk) of the first or of the last 1024-wide k block -- the last is a block that a
    non-first wave owns wherever K is split over waves (and the 2048-wide last block of the i8 kernel's 16-unit waves, K > 16384)."""
    base = 0 if where == "first" else (K - 1) // 1024 * 1024
    return base + 32 + 13 if base + 45 < K else K // 2 + 13


# ---- activations ----
def ladder_width(K):
    return 1024 if K > 1024 else max(32, K // 4 // 32 * 32)


def make_row(family, K, rng, k0, dc=8.0):
    g = rng.standard_normal(K)
    if family == "gauss":
        x = g
    elif family == "positive":
        x = np.abs(g) + 0.25
    elif family == "dc":
        x = dc + 0.5 * g
    elif family == "outlier":
        x = np.where(g < 0, -1.0, 1.0) * np.maximum(np.abs(g), OUTLIER_FLOOR)
        x[k0] = OUTLIER
    elif family == "ladder":
        x = g * np.asarray(LADDER_ACT)[(np.arange(K) // ladder_width(K)) % 4]
    elif family == "subnormal":
        x = 3e-6 * g
    elif family == "small":
        x = 2.0 ** -7 * g
    elif family == "sparse":
        x = np.zeros(K)
        x[0], x[K - 1] = 1.0, -3.0
    else:
        raise AssertionError(family)
    x = x.astype(np.float16)
    check_row(family, x, k0, dc)
    return x


def check_row(family, x, k0, dc=8.0):
    """The row's design property on the stored halves."""
    K = x.size
    v = x.astype(np.float64)
    assert np.isfinite(v).all()
    if family == "positive":
        assert np.all(v >= 0.25)
    elif family == "dc":
        assert np.all(v > 0) and v.sum() > 0.9 * dc * K, "dc: the row sum is not large against the signal"
    elif family == "outlier":
        assert v[k0] == OUTLIER and k0 % 32 not in (0, 31), "outlier: not mid-chunk"
        assert np.all(np.abs(v) >= OUTLIER_FLOOR), "outlier: an element lies more than 2^19 below the maximum"
        assert np.abs(np.delete(v, k0)).max() < 8.0
    elif family == "ladder":
        w = ladder_width(K)
        tops = [np.abs(v[b:b + w]).max() for b in range(0, K, w)]
        for i in range(1, len(tops)):
            want = LADDER_ACT[i % 4] / LADDER_ACT[(i - 1) % 4]
            assert want / 4 < tops[i] / tops[i - 1] < want * 4, "ladder: neighbouring blocks do not differ by the designed factor"
    elif family == "subnormal":
        assert np.abs(v).max() < 2.0 ** -14 and np.count_nonzero(v) > K // 2, "subnormal: a normal half, or mostly zeros"
    elif family == "small":
        assert np.abs(v).max() < 2.0 ** -4
    elif family == "sparse":
        assert np.count_nonzero(v) == 2 and v[0] == 1.0 and v[K - 1] == -3.0


def _row_floor_share(ref_row, sets):
    worst = 0.0
    for _, cols in sets:
        v = np.abs(ref_row[cols])
        if v.any():
            worst = max(worst, float((v < np.sqrt(np.mean(v * v)) / 64.0).mean()))
    return worst


def make_activations(families, K, rng, k0, mult=1.0, deq=None, sets=None, dc=8.0):
    """One row per entry of `families`.  With deq (the dequantized weights [N][K]) and the judged sets: a row that would leave more than FLOOR_CAP of a judged set
    under the rms/64 floor is drawn again (a set of 17 columns may hold none, and one Gaussian output in 80 is that small) -- the cap is a condition on the data, so
    the data is chosen to meet it; make_case asserts it on what comes out."""
    rows = []
    for f in families:
        for _ in range(64):
            x = make_row(f, K, rng, k0, dc)
            if mult != 1.0:
                x = (x.astype(np.float64) * mult).astype(np.float16)
            if deq is None or f == "sparse" or _row_floor_share(x.astype(np.float64) @ deq.T, sets) <= FLOOR_CAP:
                break
        rows.append(x)
    return np.stack(rows)


# ---- weights ----
def make_weights(family, N, K, G, rng, k0, z8=False):
    """-> codes u8 [N][K], z u8 [N][K/G], s f16 [N][K/G]; the family's property asserted on them."""
    ng = K // G
    codes = rng.integers(0, 16, (N, K)).astype(np.uint8)
    z = rng.integers(0, 16, (N, ng)).astype(np.uint8)
    s = 0.005 * rng.uniform(1.0, 1.3, (N, ng))
    if z8:  # the family on zero points that are all 8 (the token kernel takes no others)
        assert family in ("random", "null_at_outlier", "scale_ladder")
        z[:] = 8
    if family in ("random", "null_at_outlier"):
        if family == "null_at_outlier":
            g0 = k0 // G
            z[:, g0] = np.clip(z[:, g0], 1, 14)  # room for z +- 1
            n = np.arange(N)
            codes[:, k0] = np.where(n % 2 == 0, z[:, g0], z[:, g0] + np.where(rng.integers(0, 2, N) == 0, -1, 1)).astype(np.uint8)
            d = codes[:, k0].astype(np.int64) - z[:, g0]
            assert np.all(d[0::2] == 0) and np.all(np.abs(d[1::2]) == 1), "null_at_outlier: q - z at k0"
    elif family == "coherent":
        z[:] = 0
    elif family == "balanced":
        z[:] = 8
        h = rng.integers(1, 8, (N, ng, G // 2))
        codes = rng.permuted(np.concatenate([8 + h, 8 - h], axis=2), axis=2).reshape(N, K).astype(np.uint8)
        assert np.all((codes.astype(np.int64).reshape(N, ng, G) - 8).sum(axis=2) == 0), "balanced: sum(q - z) != 0 in a group"
    elif family == "extreme":
        codes = (15 * rng.integers(0, 2, (N, K))).astype(np.uint8)
        z = (15 * rng.integers(0, 2, (N, ng))).astype(np.uint8)
        d = codes.astype(np.int64).reshape(N, ng, G) - z[:, :, None]
        assert np.all(np.isin(d, (-15, 0, 15))) and (d == 15).any() and (d == -15).any()
    elif family == "scale_ladder":
        s = s * np.asarray(LADDER_SCALE)[(np.arange(ng) + max(0, 3 - ng)) % 3][None, :] * rng.choice([-1.0, 1.0], (N, ng))
        s[0::5, 0] = 0.0   # a leading zero scale,
        s[2::7, -1] = 0.0  # a trailing one,
        s[1, :] = 0.0      # and a whole row
    elif family == "subnormal_scale":
        s = 2.0 ** -20 * rng.uniform(1.0, 1.3, (N, ng))
    elif family == "sigma200":  # sigma-200 Gaussian weights through a symmetric 4-bit group quantizer: zero point 8, scale = the group's largest magnitude / 8
        w = 200.0 * rng.standard_normal((N, ng, G))
        z[:] = 8
        s = np.abs(w).max(axis=2) / 8.0
        codes = np.clip(np.rint(w / s[:, :, None]) + 8, 0, 15).reshape(N, K).astype(np.uint8)
    else:
        raise AssertionError(family)
    s = s.astype(np.float16)
    if family == "scale_ladder":
        m = np.abs(s.astype(np.float64))
        assert np.all(s[1] == 0) and s[0, 0] == 0 and s[2, -1] == 0
        if ng >= 4:
            r = m[3, 1] / m[3, 0], m[3, 2] / m[3, 1]  # (row 3 has no zero scale)
            assert 2.0 ** 15 < r[0] < 2.0 ** 17 and 2.0 ** -7 < r[1] < 2.0 ** -5, "scale_ladder: neighbouring groups do not differ by 2^16 / 2^-6"
        assert (s < 0).any() and (s > 0).any()
    elif family == "subnormal_scale":
        assert np.all(np.abs(s.astype(np.float64)) < 2.0 ** -14) and np.all(s != 0), "subnormal_scale: a scale is a normal half, or zero"
    else:
        assert np.all(s > 0)
    return codes, z, s


# ---- the case ----
class Case:
    def __init__(self, name, a, codes, z, s, G, sets, k0=None, rows=None, inf_set=None):
        self.name, self.a, self.codes, self.z, self.s, self.G, self.sets, self.k0, self.rows, self.inf_set = name, a, codes, z, s, G, sets, k0, rows, inf_set
        self.M, self.K = a.shape
        self.N = codes.shape[0]
        self.qw, self.sc, self.zp = pack_q4_6(codes, z, s, G)
        self.zeros_are_8 = bool(np.all(z == 8))
        self._ref, self._row_sets = None, {}

    def dequantized(self):
        """(q - z) * s in float64, [N][K]."""
        d = self.codes.astype(np.float64).reshape(self.N, -1, self.G) - self.z.astype(np.float64)[:, :, None]
        return (d * self.s.astype(np.float64)[:, :, None]).reshape(self.N, self.K)  # (= _deq)

    def reference(self):
        if self._ref is None:
            self._ref = self.a.astype(np.float64) @ self.dequantized().T
            self._ref.setflags(write=False)
        return self._ref

    def sets_for(self, r):
        """The judged sets of activation row r: the case's, any that breaks the floor cap on this row split -- what is under the floor becomes a set of its own,
        with its own rms -- until every part keeps the cap."""
        if r not in self._row_sets:
            out = []
            for label, cols in self.sets:
                out += [(label, c) for c in _split(self.reference()[r], cols)]
            self._row_sets[r] = out
        return self._row_sets[r]

    def with_rows(self, M):
        """The same weights against the first M activation rows (a decode kernel's M = 1 launch of a case built for more)."""
        c = Case(self.name, self.a[:M].copy(), self.codes, self.z, self.s, self.G, self.sets, self.k0, self.rows, self.inf_set)
        return c


def _split(ref_row, cols):
    v = np.abs(ref_row[cols])
    if not v.any():
        return [cols]
    small = v < np.sqrt(np.mean(v * v)) / 64.0
    if small.mean() <= FLOOR_CAP:
        return [cols]
    return _split(ref_row, cols[~small]) + _split(ref_row, cols[small])  # (the larger part again: its rms rose when the small ones left)


def floor_share(case):
    """The largest share, over rows and judged sets, of elements with |ref| < rms/64 (where the floor, not the 1e-3, is the bound)."""
    ref, worst = case.reference(), 0.0
    for r in range(case.M):
        for _, cols in case.sets_for(r):
            v = np.abs(ref[r, cols])
            if v.any():  # (a set that is zero by design has no floor: judge asks for exact zeros there)
                worst = max(worst, float((v < np.sqrt(np.mean(v * v)) / 64.0).mean()))
    return worst


def judge(case, got):
    """The worst w4a16_close ratio over the rows and the judged sets (inf where an output that should be finite is not); the overflow set, where the case has one, must
    hold +-inf with the reference's sign (that is what binary16's round-to-nearest gives past 65520)."""
    ref = case.reference()
    got = np.asarray(got)
    assert got.shape == ref.shape and got.dtype == np.float16
    worst = 0.0
    for r in range(case.M):
        for _, cols in case.sets_for(r):
            g = got[r, cols]
            if not np.isfinite(g.astype(np.float32)).all():
                return float("inf")
            if not ref[r, cols].any():  # a set that is exactly zero by design (every scale of the row is zero): rms = 0 leaves w4a16_close no bound but equality
                if g.any():
                    return float("inf")
                continue
            worst = max(worst, w4a16_close(g, ref[r, cols])[1])
        if case.inf_set is not None:
            g = got[r, case.inf_set].astype(np.float64)
            if not np.all(np.isinf(g) & (np.sign(g) == np.sign(ref[r, case.inf_set]))):
                return float("inf")
    return worst


def _rng(name, M, N, K, G, seed, where):
    names = PAIR_NAMES + MIXED + ("overflow", "nonfinite")
    return np.random.default_rng([seed, names.index(name), M, N, K, G, 0 if where == "last" else 1])


def _deq(codes, z, s, G):
    N, K = codes.shape
    d = codes.astype(np.float64).reshape(N, -1, G) - z.astype(np.float64)[:, :, None]
    return (d * s.astype(np.float64)[:, :, None]).reshape(N, K)


def make_case(name, M, N, K, G, seed=0, where="last", rows=None, z8=False):
    """One seeded case: a pair of PAIRS, a MIXED launch (rows: the row families, default MIXED_ROWS in rotation) or `overflow`.  Deterministic: the generator is
    seeded by every argument."""
    rng = _rng(name, M, N, K, G, seed, where)
    k0 = k0_for(K, where)
    if name == "overflow":
        return _overflow(M, N, K, G, rng, k0)
    if name in MIXED:
        rows = tuple(rows) if rows is not None else tuple(MIXED_ROWS[r % 7] for r in range(M))
        wf, mult = name.split(" x ")[1], 1.0
        if wf == "scale_ladder":  # the outlier meets a group on the ladder's middle rung: against the 2^6 one, 2^15 * 15 * 0.4 leaves binary16 (scaled, see the docstring)
            ng = K // G
            mid = [g for g in range(ng) if LADDER_SCALE[(g + max(0, 3 - ng)) % 3] == 1.0]
            k0 = min(mid, key=lambda g: abs(g - k0 // G)) * G + k0 % G
    else:
        assert rows is None
        _, af, wf, mult = PAIRS[PAIR_NAMES.index(name)]
        rows = (af,) * M
    assert len(rows) == M
    codes, z, s = make_weights(wf, N, K, G, rng, k0, z8)
    sets = _sets(wf, s)
    # `dc` as a pair on a prefill launch (M > 16) has the offset 4, not 8: over the 27 000 - 78 000 outputs of those launches the ORACLE's own sequential fp32 sum reaches
    # 0.61 - 0.66 of the bound on dc x balanced at 8 and at 6 (the worst of that many draws), 0.55 at 4 -- the family is scaled, not the oracle's 0.6
    dc = 4.0 if M > 16 and name not in MIXED else 8.0
    case = Case(name, make_activations(rows, K, rng, k0, mult, _deq(codes, z, s, G), sets, dc), codes, z, s, G, sets, k0, rows if name in MIXED else None)
    share = floor_share(case)
    assert share <= FLOOR_CAP, f"{name} {M}x{N}x{K} g{G}: {share:.3f} of a judged set sits under the rms/64 floor"
    # (rows whose sets had to be split, sets_for: `sparse` -- nothing to draw again, its outputs are one or two exact products --, `outlier` against weights that were not
    # built around k0 -- one column in 16 has q = z there and is 2^-15 of the others: what the floor hid --, and `ladder` against `scale_ladder` where a dead last group
    # takes a column's only large product away.  The parts are small by DESIGN, not by cancellation; the host test holds the oracle to 0.6 on every one of them.)
    if "small" in rows:  # (the reason the row is `small` and not `subnormal`: see the module's docstring)
        r = rows.index("small")
        assert np.sqrt(np.mean(case.reference()[r] ** 2)) >= 2.0 ** -9, "mixed_rows: the small row's outputs are not normal halves"
    return case


def _sets(wf, s):
    N = s.shape[0]
    if wf == "null_at_outlier":
        return [("even", np.arange(0, N, 2)), ("odd", np.arange(1, N, 2))]
    if wf == "scale_ladder":  # the rows whose scales are all zero are judged by themselves (exactly zero): in the other set they would be floor elements by design
        # and the others by the largest rung they have alive: a row whose only 2^6 group is dead is 2^-6 of its neighbours (few groups: K = 256 has two)
        dead = np.all(s == 0, axis=1)
        top = np.abs(s.astype(np.float64)).max(axis=1)
        rung = np.array([int(np.argmin([abs(np.log2(max(v, 1e-30) / (0.005 * r))) for r in LADDER_SCALE])) for v in top])
        sets = [(f"rows whose largest scale is on rung {LADDER_SCALE[i]:g}", np.flatnonzero(~dead & (rung == i))) for i in range(3)]
        return [x for x in sets if x[1].size] + [("all-zero rows", np.flatnonzero(dead))]
    return [("all", np.arange(N))]


def _overflow(M, N, K, G, rng, k0):
    """positive x coherent, each column's scales chosen so that even columns land at -+1.3 * 65504 and odd ones at +-0.7 * 65504 (the sign alternates in pairs)."""
    codes, z, s = make_weights("coherent", N, K, G, rng, k0)
    a = make_activations(("positive",) * M, K, rng, k0)
    unit = Case("overflow", a, codes, z, s, G, []).reference()  # with the 0.005 scales
    n = np.arange(N)
    target = np.where(n % 2 == 0, 1.3, 0.7) * HALF_MAX * np.where((n // 2) % 2 == 0, 1.0, -1.0)
    s = (s.astype(np.float64) * (target / np.median(unit, axis=0))[:, None]).astype(np.float16)
    case = Case("overflow", a, codes, z, s, G, [("in range", n[1::2])], k0, inf_set=n[0::2])
    mag = np.abs(case.reference())
    assert np.all(mag[:, 0::2] > 1.05 * HALF_MAX) and np.all(mag[:, 1::2] < 0.95 * HALF_MAX), "overflow: a column sits near the edge of binary16's range"
    return case


def nonfinite_case(M, N, K, G, seed=0, z8=False):
    """gauss x random, and the (row, k) where the test plants an inf, then a NaN: the last row, mid-chunk."""
    rng = _rng("nonfinite", M, N, K, G, seed, "last")
    codes, z, s = make_weights("random", N, K, G, rng, 0, z8)
    return Case("nonfinite", make_activations(("gauss",) * M, K, rng, 0), codes, z, s, G, [("all", np.arange(N))]), M - 1, k0_for(K)


# ---- the table of launches: the GPU test runs these, the host test proves every one of them sound ----
GEMV_SHAPES = ((1, 72, 4096, 128), (4, 40, 1408, 64), (2, 40, 512, 32))
STREAM_SHAPES = ((1, 72, 4096, 128), (1, 520, 4096, 128))
# (the i8 kernel takes rows x groups-per-128 <= 4: M = 1 at every group size, M = 2 down to groups of 64, M = 4 on groups of 128)
I8_SHAPES = ((1, 72, 4096, 128), (1, 72, 4096, 64), (1, 72, 4096, 32), (2, 72, 4096, 128), (2, 72, 4096, 64), (4, 72, 4096, 128), (1, 100, 1408, 128), (2, 100, 1408, 128), (4, 100, 1408, 128), (1, 40, 16512, 128))
SKINNY_SHAPES = ((16, 17, 128, 128), (5, 40, 256, 128))
GEMM_SHAPES = ((33, 200, 1024, 128), (70, 136, 512, 32), (130, 200, 1024, 64))
PK_SHAPES = ((200, 136, 384, 128), (260, 300, 1408, 128), (260, 300, 1408, 64))
AWQ_SHAPES = ((4, 136, 1024, 128), (64, 136, 1024, 128))
TOKEN_SHAPE = (1, 264, 4096, 128)


# the cases that also exist with every zero point 8 (`scale_ladder` through the Gaussian row, `mixed_rows` against `random`: with the `ladder` row on the prefill
# shapes' K = 1408 -- one 384-wide block at full scale, over three groups on three rungs -- the z = 8 draws leave outputs that are sums of a few comparable group
# terms, and the ORACLE's own ratio reaches 0.71 - 7.9 on the parts sets_for splits off; those two are not launched with z = 8)
Z8_EXTRA = ("gauss x random", "outlier x null_at_outlier", "gauss x scale_ladder", "mixed_rows x random")


def cases_for(shape, z8_only=False, outlier_where=("last",), z8_extra=False):
    """Every case a kernel family launches at `shape`: (label, make_case arguments) in a fixed order.
    z8_only:  the cases whose zero points are all 8 -- the two pairs that have them by design and the Z8_EXTRA families built with z = 8 (the AWQ layout has no other).
    z8_extra: all cases, and the Z8_EXTRA ones a second time with z = 8 (the packed GEMM's wide forms run only on linears whose zero points are all 8)."""
    M, N, K, G = shape
    out = []
    for name in PAIR_NAMES:
        if z8_only and name not in Z8_PAIRS:
            continue
        for where in (outlier_where if name.startswith("outlier") else ("last",)):
            out.append((name if where == "last" else name + " (first block)", dict(name=name, M=M, N=N, K=K, G=G, where=where)))
    mixed = []
    if M > 1:
        for name in MIXED:
            for i, rows in enumerate(DECODE_ROWS.get(M, (None,))):
                mixed.append((name if i == 0 else f"{name} ({', '.join(rows)})", dict(name=name, M=M, N=N, K=K, G=G, rows=rows)))
    if not z8_only:
        out += mixed + [("overflow", dict(name="overflow", M=M, N=N, K=K, G=G))]
    if z8_only or z8_extra:
        for name in Z8_EXTRA[:3]:
            out.append((name + " (z = 8)", dict(name=name, M=M, N=N, K=K, G=G, z8=True)))
        out += [(label + " (z = 8)", dict(kw, z8=True)) for label, kw in mixed if kw["name"] in Z8_EXTRA]
    return out


TOKEN_CASES = tuple(dict(name=n, M=TOKEN_SHAPE[0], N=TOKEN_SHAPE[1], K=TOKEN_SHAPE[2], G=TOKEN_SHAPE[3], z8=True) for n in ("outlier x null_at_outlier", "ladder x scale_ladder"))
# kernel family -> (its shapes, how cases_for is called for it): the one table the GPU test launches from and the host test proves sound
LAUNCHES = {
    "gemv": (GEMV_SHAPES, {}),
    "stream": (STREAM_SHAPES, {}),
    "i8": (I8_SHAPES, dict(outlier_where=("first", "last"))),
    "skinny": (SKINNY_SHAPES, {}),
    "gemm": (GEMM_SHAPES, {}),
    "pk": (PK_SHAPES, dict(z8_extra=True)),
    "awq": (AWQ_SHAPES, dict(z8_only=True)),
}


def family_cases(family, shape):
    return cases_for(shape, **LAUNCHES[family][1])


def launched_cases():
    """{shape: [(label, make_case arguments)]} of everything the GPU test launches, each argument set once."""
    out, seen = {}, set()
    todo = [(shape, c) for family, (shapes, _) in LAUNCHES.items() for shape in shapes for c in family_cases(family, shape)]
    todo += [(TOKEN_SHAPE, (kw["name"] + " (z = 8, token plan)", kw)) for kw in TOKEN_CASES]
    for shape, (label, kw) in todo:
        key = tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in kw.items() if v is not None))
        if key not in seen:
            seen.add(key)
            out.setdefault(shape, []).append((label, kw))
    return out
