"""Designed rows for the glue between the W4A16 linears of a llama decoder layer -- RMSNorm, SiLU*mul, the binary16 residual add -- with their references and with
kernels that are wrong on purpose (a helper: numpy only, no tests here, nothing pytest collects).

Gaussian rows of sigma 2.5 - 3 leave this code unobserved where it can go wrong: mean(x^2) ~ 6 hides eps, nothing reaches the clamp at +-64504, no output is a
subnormal half, no gate is below -11.09 (where hexp(-g) is +inf in binary16) and no product overflows.  The generators here build rows that sit there and ASSERT the
property each is named for on the stored halves (check_row), before they hand a row out.

RMSNorm -- the reference and the bound.
  Reference (rmsnorm_ref), float64 from the binary16 inputs: rs = 1 / sqrt(mean(x^2) + float32(eps)), f = (x * rs) * gamma, then rmsnorm_out's clamp as it is written in
  C -- f > 0 ? fminf(f, 64504) : fmaxf(f, -64504) -- with np.fmin / np.fmax, so that a NaN product goes to -64504 exactly as the source sends it.
  Judged: |got - ref| <= (0.5 + M_MARGIN) * ulp16(ref), ulp16 floored at 2^-24 (binary16 denormals are not flushed in this library); a zero reference must come out as a
  zero of the same sign; the reference is never non-finite (the clamp), so neither may the output be.
  M_MARGIN, derived for the documented order (tce_common.hpp), u = 2^-24 the unit roundoff of fp32:
    * the square of a half is exact in fp32 (11 x 11 bits), so fmaf(v, v, s) is ONE rounding of an exact sum; all terms are >= 0, so a sum that went through R
      roundings has a relative error <= (1 + u)^R - 1 =: g(R) (no cancellation);
    * a square reaches `tot` through at most 8 (the piece's chain; the first, 0 + v^2, is exact) + 3 (up to four pieces per slot at n = 24584, the first add to 0 exact)
      + 15 (sixteen slots per lane, the first add exact) + 6 (the DPP tree) = 32 roundings: R = 32;
    * tot / n: + u.  (+ eps): the sum of two non-negative terms, + u; eps itself is the float32 the reference uses.  So mean + eps carries <= g(34);
    * sqrt halves a relative error and rounds: g(34) / 2 + u up to second order; 1 / s: + u; x * rs: + u (x is exact); * gamma: + u (gamma is the fp32 given).
    f carries a relative error <= (34 / 2 + 4) u (1 + O(34 u)) = 21 u (1 + 2e-6) < 21.001 * 2^-24.  No operand is an fp32 subnormal on the rows used here (|x| >= 2^-24,
    rs >= 2^-16, |gamma| >= 2^-3 where it is not a designed 0).  ulp16(ref) >= |ref| * 2^-11, so the error before the last rounding is <= 21.001 * 2^-13 = 2.564e-3
    binary16 ulps < 2^-8 = 3.906e-3: M_MARGIN = 2^-8 holds with a third to spare.  The clamp is monotone and 1-Lipschitz, so it does not widen this; the final
    conversion adds the 0.5 (to the ulp of the REFERENCE: where the fp32 value and the reference straddle a power of two, the half nearest the fp32 value is that power,
    within M_MARGIN of the reference).
  The reference kernel's own order (oracle.rmsnorm_half: n / 512 sequential terms per thread, then two butterflies) goes through more roundings at the widest rows
  (48 + 10 at n = 24584: 33 u by the same count, 4.0e-3 ulps) -- it is HELD to the bound by the host test on every case, where it stays at a fraction of it, but it is
  not what the margin is derived from.

SiLU*mul -- the reference and the ambiguous gates.
  The definition in tce_common.hpp (SiLuMul_half): e = half(exp(-g)), d = half(1 + e), r = half(1 / d), sv = half(g * r), out = half(sv * u), evaluated in float64 with
  every operation rounded once to binary16.  1 + e and the two products are exact in float64 (a product of two 11-bit significands has 22 bits; 1 + e spans at most
  2^-24 .. 2^16); the quotient of two halves rounded to 53 bits and then to 11 is the correctly rounded quotient (53 >= 2 * 11 + 2).  What is left is half(exp(-g)): the
  device forms it from its fp32 expf.  ROCm documents the device expf at a maximum error of 1 ulp (HIP math API reference, single-precision functions), so when the true
  exponential lies more than 1 fp32 ulp from every binary16 rounding boundary, the device's float is on the same side as the true value and the half is the same.
  T_ULPS = 2 (one ulp of margin over the documented one) defines the AMBIGUOUS gates, computed here from float64 over all 65536 gate patterns: exp(-g) within T_ULPS fp32
  ulps of a boundary (a midpoint of two neighbouring halves, 2^-25, 65520).  There the result from EITHER neighbouring e is accepted; every other gate must match bit for
  bit, NaN must match NaN.  The set has 13 members at T = 2 (7 / 13 / 26 / 53 at T = 1 / 2 / 4 / 8); more than AMBIGUOUS_CAP = 64 and the reference fails by itself.

Residual add -- exact: one rounding of an exact float64 sum.

Mutants (RMS_MUTANTS, SILU_MUTANTS, ADD_MUTANTS): numpy implementations with one fault each, used by tests/test_glue_adversarial_host.py to show that the cases catch
them -- or, for `skip_first_rounding`, that NO case can: both evaluations are inside the bound (it changes f by at most one fp32 ulp in front of the same final
rounding), which is the bound saying that it does not prescribe the order of the roundings in fp32.
"""
import numpy as np

CLAMP = 65504.0 - 1000.0
M_MARGIN = 2.0 ** -8
T_ULPS = 2
AMBIGUOUS_CAP = 64
EPS_VALUES = (1e-6, 1e-5)
WIDTHS = (8, 64, 520, 4096, 8192, 8200, 11008, 16384, 24584)
HALF_MAX = 65504.0
SUB = 2.0 ** -14  # the smallest normal half


def h16(v):
    """float64 -> binary16, one rounding to nearest even, overflow to inf, denormals kept."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(v, np.float64).astype(np.float16)


def ulp16(ref):
    """The spacing of binary16 at |ref| (float64), floored at 2^-24.  The exponent is frexp's, exact: a log2 may round a value just below a power of two up to it."""
    a = np.abs(np.asarray(ref, np.float64))
    _, e = np.frexp(a)  # a = m * 2^e, 0.5 <= m < 1: a lies in [2^(e - 1), 2^e)
    e = np.where(a == 0, -100, e)  # (frexp gives a zero the exponent 0)
    return 2.0 ** (np.clip(e - 1, -14, 15) - 10)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# RMSNorm
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _clamp(f):
    with np.errstate(invalid="ignore"):
        return np.where(f > 0, np.fmin(f, CLAMP), np.fmax(f, -CLAMP))


def rmsnorm_ref(x16, gamma32, eps):
    """float64 reference of half(clamp((x * rs) * gamma)) BEFORE the final rounding: [m][n] float64, always finite."""
    x = np.atleast_2d(np.asarray(x16, np.float16)).astype(np.float64)
    with np.errstate(all="ignore"):
        rs = 1.0 / np.sqrt(np.mean(x * x, axis=1) + np.float64(np.float32(eps)))
        f = (x * rs[:, None]) * np.asarray(gamma32, np.float32).astype(np.float64)[None, :]
    f = _clamp(f)
    assert np.isfinite(f).all()
    return f


def rmsnorm_ratio(got16, ref):
    """worst |got - ref| / ((0.5 + M_MARGIN) ulp16(ref)) over an array; inf where the output is not finite or a zero reference is not met by a zero of its sign."""
    got16 = np.asarray(got16)
    assert got16.dtype == np.float16 and got16.shape == ref.shape, (got16.dtype, got16.shape, ref.shape)
    g = got16.astype(np.float64)
    if not np.isfinite(g).all():
        return float("inf")
    z = ref == 0
    if np.any(z & ((g != 0) | (np.signbit(g) != np.signbit(ref)))):
        return float("inf")
    return float(np.max(np.abs(g - ref) / ((0.5 + M_MARGIN) * ulp16(ref)))) if g.size else 0.0


def margin_used(ratio):
    """The share of M_MARGIN a worst ratio stands for: (|err| / ulp - 0.5) / M_MARGIN (negative: the final rounding's half ulp was not even reached)."""
    return (ratio * (0.5 + M_MARGIN) - 0.5) / M_MARGIN


RMS_FAMILIES = ("gauss", "one_hot", "eps_rules", "zeros", "all_max", "wide", "saturate", "negative_gamma", "nonfinite")
ONE_HOT_MAGS = (60000.0, SUB)
NONFINITE_KINDS = ("+inf", "-inf", "nan")


def one_hot_positions(n):
    """Elements 0, 7, 8 (the second piece), 511 (the last element of the first 64-piece term), 512, 8191, 8192 (the first piece that shares a slot), n - 8, n - 1."""
    return tuple(sorted({p for p in (0, 7, 8, 511, 512, 8191, 8192, n - 8, n - 1) if 0 <= p < n}))


def plain_gamma(n, rng):
    return np.clip(1.0 + 0.2 * rng.standard_normal(n), 0.5, 1.5).astype(np.float32)


def make_rms_row(family, n, rng, variant=None):
    """One fp16 row of the family.  variant: (position, magnitude) for one_hot, one of NONFINITE_KINDS for nonfinite."""
    g = rng.standard_normal(n)
    if family in ("gauss", "negative_gamma"):
        x = 2.5 * g
    elif family == "saturate":  # Gaussian with |g| >= 0.75: x * rs >= 0.66 in magnitude, so that every column whose gamma is +-1e5 lands beyond the clamp
        x = 2.5 * np.where(g < 0, -1.0, 1.0) * np.maximum(np.abs(g), 0.75)
    elif family == "one_hot":
        pos, mag = variant
        x = np.zeros(n)
        x[pos] = mag if pos % 2 == 0 else -mag
    elif family == "eps_rules":  # magnitudes 2^-24 .. 2^-13: a quarter of the row one or two subnormal steps, the rest log-uniform around 2^-14
        mag = 2.0 ** rng.uniform(-18, -13, n)
        mag[0::4] = np.where(np.arange(n)[0::4] % 8 == 0, 2.0 ** -24, 2.0 ** -23)
        x = np.where(g < 0, -1.0, 1.0) * mag
    elif family == "zeros":
        x = np.where(np.arange(n) % 3 == 1, -0.0, 0.0)
    elif family == "all_max":
        x = np.where(g < 0, -HALF_MAX, HALF_MAX)
    elif family == "wide":
        x = np.where(g < 0, -1.0, 1.0) * rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-20, 15, n)
    elif family == "nonfinite":
        x = 2.5 * g
        x[n // 2 + 3 if n > 8 else 3] = {"+inf": np.inf, "-inf": -np.inf, "nan": np.nan}[variant]
    else:
        raise AssertionError(family)
    x = h16(x)
    check_row(family, x, variant)
    return x


def check_row(family, x16, variant=None):
    """The row's design property on the stored halves (the properties of `saturate` and `negative_gamma` are gamma's: check_gamma)."""
    n = x16.size
    v = x16.astype(np.float64)
    ms = np.mean(v * v) if np.isfinite(v).all() else np.nan
    if family in ("gauss", "saturate", "negative_gamma"):
        assert np.isfinite(v).all() and np.abs(v).max() < 16.0 and ms > 0.2, f"{family}: not the control it is meant to be"
    elif family == "one_hot":
        pos, mag = variant
        assert np.count_nonzero(v) == 1 and abs(v[pos]) == mag and not np.signbit(v[v == 0]).any(), "one_hot: more than the one element, or a -0"
        assert np.float64(np.float32(mag * mag)) == mag * mag, "one_hot: v^2 is not exact in fp32"
    elif family == "eps_rules":
        assert np.abs(v).max() < 2.0 ** -12 and np.count_nonzero(v) == n, "eps_rules: a large or a zero element"
        assert (np.abs(v) < SUB).sum() >= n // 4 and ms < min(EPS_VALUES) / 16, "eps_rules: too few subnormals, or mean(x^2) is not far below eps"
    elif family == "zeros":
        assert not v.any() and np.signbit(v).any() and not np.signbit(v).all(), "zeros: not a mix of +0 and -0"
    elif family == "all_max":
        assert np.all(np.abs(v) == HALF_MAX) and np.float64(np.float32(n * HALF_MAX ** 2)) < 3.0e38
    elif family == "wide":
        assert np.isfinite(v).all()
        if n >= 64:
            e = np.floor(np.log2(np.abs(v)))
            assert e.min() <= -17 and e.max() >= 11, "wide: the exponents do not span the designed range"
    elif family == "nonfinite":
        bad = ~np.isfinite(v)
        assert bad.sum() == 1
        b = v[bad][0]
        assert {"+inf": b == np.inf, "-inf": b == -np.inf, "nan": np.isnan(b)}[variant]
    else:
        raise AssertionError(family)


SAT_NEAR = (-31.0, -8.0, -1.0, 1.0, 8.0, 31.0)  # distances from the clamp, all inside one binary16 step (32) of it


def saturate_gamma(x16, eps, rng):
    """gamma for a `saturate` launch, built against its row 0 (a Gaussian row): a third of the columns carry +-1e5, columns 5 and 6 of every 16 carry 0 and -0, and
    12 columns (6 per sign, where n >= 64) are solved so that the product lands SAT_NEAR away from +-64504, on both sides of it."""
    n = x16.size
    gamma = plain_gamma(n, rng).astype(np.float64)
    idx = np.arange(n)
    gamma[idx % 3 == 0] = 1e5
    gamma[idx % 6 == 3] = -1e5
    gamma[idx % 16 == 5] = 0.0
    gamma[idx % 16 == 6] = -0.0
    if n >= 64:
        v = x16.astype(np.float64)
        xr = v / np.sqrt(np.mean(v * v) + np.float64(np.float32(eps)))
        free = [int(i) for i in idx if i % 3 == 1 and i % 16 not in (5, 6) and abs(xr[i]) > 0.25][:12]
        assert len(free) == 12
        for j, i in enumerate(free):
            sign = 1.0 if j < 6 else -1.0
            gamma[i] = sign * (CLAMP + SAT_NEAR[j % 6]) / xr[i]
    return gamma.astype(np.float32)


def negative_gamma(n, rng):
    return (-plain_gamma(n, rng)).astype(np.float32)


def check_gamma(family, x16, gamma32, eps):
    """The launch's design property where it is gamma's."""
    n = x16.size
    if family == "negative_gamma":
        assert np.all(gamma32 < 0)
    elif family == "saturate":
        v = x16.astype(np.float64)
        f = v / np.sqrt(np.mean(v * v) + np.float64(np.float32(eps))) * gamma32.astype(np.float64)
        assert (gamma32 == 0).any() and np.signbit(gamma32[gamma32 == 0]).any() and not np.signbit(gamma32[gamma32 == 0]).all(), "saturate: no 0 and -0 in gamma"
        if n >= 64:
            d = np.abs(f) - CLAMP
            need = 32 if n >= 512 else n // 8  # (a row of 64 has 32 columns that carry +-1e5 and 12 that sit within a step of the clamp: there are not 32 on each side)
            assert (d > 32).sum() >= need and (d < -32).sum() >= need, "saturate: fewer than 32 outputs clamped, or fewer than 32 not"
            for s in (1.0, -1.0):
                near = d[(np.sign(f) == s) & (np.abs(d) < 32)]
                assert (near > 0.5).any() and (near < -0.5).any(), "saturate: nothing within a step of the clamp on one of its sides"
            assert (f > CLAMP).any() and (f < -CLAMP).any()


class RmsLaunch:
    """One tce_rmsnorm_half launch: x fp16 [m][n], gamma fp32 [n], eps, the family of every row (with its variant), the float64 reference (computed once)."""

    def __init__(self, label, x, gamma, eps, rows):
        self.label, self.x, self.gamma, self.eps, self.rows = label, np.ascontiguousarray(x), gamma, eps, tuple(rows)
        self.m, self.n = self.x.shape
        self._ref = None

    def reference(self):
        if self._ref is None:
            self._ref = rmsnorm_ref(self.x, self.gamma, self.eps)
            self._ref.setflags(write=False)
        return self._ref

    def judge(self, got16):
        """{family: worst ratio} over the launch's rows."""
        ref, out = self.reference(), {}
        for r, (fam, _) in enumerate(self.rows):
            out[fam] = max(out.get(fam, 0.0), rmsnorm_ratio(np.asarray(got16)[r], ref[r]))
        return out


def _fam_id(name):
    return RMS_FAMILIES.index(name)


def rms_launches(n, eps):
    """Every stand-alone launch at width n: each family as a launch of one row, then launches of three rows with different families side by side (the same rows; a
    row's result must not depend on its neighbours).  Deterministic."""
    e6 = int(round(eps * 1e7))
    rng = np.random.default_rng([7, n, e6])
    gamma = plain_gamma(n, rng)
    rows = [("gauss", None), ("eps_rules", None), ("zeros", None), ("all_max", None), ("wide", None)]
    rows += [("nonfinite", k) for k in NONFINITE_KINDS]
    rows += [("one_hot", (p, mag)) for p in one_hot_positions(n) for mag in ONE_HOT_MAGS]
    xs = [make_rms_row(f, n, rng, v) for f, v in rows]
    out = [RmsLaunch(f"{f}{'' if v is None else ' ' + str(v)}", x[None, :], gamma, eps, [(f, v)]) for (f, v), x in zip(rows, xs)]
    for i in range(0, len(rows) - 2, 3):
        out.append(RmsLaunch("rows " + ", ".join(f for f, _ in rows[i:i + 3]), np.stack(xs[i:i + 3]), gamma, eps, rows[i:i + 3]))
    # the launches whose property is gamma's
    xs_g = make_rms_row("saturate", n, rng)
    gs = saturate_gamma(xs_g, eps, rng)
    check_gamma("saturate", xs_g, gs, eps)
    out.append(RmsLaunch("saturate", xs_g[None, :], gs, eps, [("saturate", None)]))
    out.append(RmsLaunch("rows saturate, zeros, all_max", np.stack([xs_g, xs[2], xs[3]]), gs, eps, [("saturate", None), ("zeros", None), ("all_max", None)]))
    xn = make_rms_row("negative_gamma", n, rng)
    gn = negative_gamma(n, rng)
    check_gamma("negative_gamma", xn, gn, eps)
    out.append(RmsLaunch("negative_gamma", xn[None, :], gn, eps, [("negative_gamma", None)]))
    out.append(RmsLaunch("rows negative_gamma, wide, eps_rules", np.stack([xn, xs[4], xs[1]]), gn, eps, [("negative_gamma", None), ("wide", None), ("eps_rules", None)]))
    if n >= 64:  # eps_rules: outputs partly subnormal (a property of the launch: it needs gamma and eps)
        o = np.abs(out[1].reference()[0])
        assert ((o > 0) & (o < SUB)).any() and (o >= SUB).any(), "eps_rules: the outputs are not partly subnormal"
    return out


def rms_row_launch(family, n, eps, variant=None, seed=0):
    """One designed row with its gamma, for the fused forms (M = 1): an RmsLaunch of one row."""
    rng = np.random.default_rng([11, n, int(round(eps * 1e7)), _fam_id(family), seed])
    x = make_rms_row(family, n, rng, variant)
    gamma = saturate_gamma(x, eps, rng) if family == "saturate" else negative_gamma(n, rng) if family == "negative_gamma" else plain_gamma(n, rng)
    if family in ("saturate", "negative_gamma"):
        check_gamma(family, x, gamma, eps)
    return RmsLaunch(f"{family}{'' if variant is None else ' ' + str(variant)}", x[None, :], gamma, eps, [(family, variant)])


# ---- the project's order in numpy fp32, and its mutants ----
def _dpp_tree(t):
    """wave_sum_dpp_lane63 on 64 fp32 values: the value lane 63 ends with."""
    v = t.astype(np.float32).copy()
    lane = np.arange(64)
    v = v + v[lane ^ 1]                               # quad_perm [1,0,3,2]
    v = v + v[lane ^ 2]                               # quad_perm [2,3,0,1]
    v = v + v[(lane & ~7) | (7 - (lane & 7))]         # row_half_mirror
    v = v + v[(lane & ~15) | (15 - (lane & 15))]      # row_mirror
    add = np.zeros(64, np.float32)
    add[16:32], add[48:64] = v[15], v[47]             # row_bcast15 into rows 1 and 3
    v = v + add
    add = np.zeros(64, np.float32)
    add[32:64] = v[31]                                # row_bcast31 into rows 2 and 3
    v = v + add
    return v[63]


RMS_MUTANTS = ("no_eps", "eps_times_n", "padded_n", "drop_second_round", "drop_partial_term", "fp16_accumulate", "clamp_65504", "clamp_before_gamma",
               "flush_denormals", "skip_first_rounding")


def rmsnorm_project(x16, gamma32, eps, fault=None):
    """tce_common.hpp's order restated in numpy fp32 (the piece's fmaf chain -- the square of a half is exact in fp32, so fmaf(v, v, s) = fl(v * v + s) --, 1024 slots,
    sixteen terms per lane, the DPP tree), then rmsnorm_out; `fault`: one of RMS_MUTANTS.  -> fp16 [m][n]."""
    assert fault is None or fault in RMS_MUTANTS
    x16 = np.atleast_2d(np.asarray(x16, np.float16))
    m, n = x16.shape
    f32 = np.float32
    gam = np.asarray(gamma32, f32)
    out = np.empty((m, n), np.float16)
    with np.errstate(all="ignore"):
        for r in range(m):
            x = x16[r].astype(f32)
            pieces = n // 8
            acc_t = np.float16 if fault == "fp16_accumulate" else f32
            s = np.zeros(pieces, acc_t)
            sq = (x * x).reshape(pieces, 8)
            for e in range(8):
                s = (s + sq[:, e].astype(acc_t)).astype(acc_t)
            s = s.astype(f32)
            if fault == "drop_partial_term":
                s[pieces // 64 * 64:] = 0
            slot = np.zeros(1024, f32)
            for base in range(0, pieces if fault != "drop_second_round" else min(pieces, 1024), 1024):
                part = np.zeros(1024, f32)
                part[:min(1024, pieces - base)] = s[base:base + 1024]
                slot = slot + part
            t = np.zeros(64, f32)
            for c in range(16):
                t = t + slot[c * 64:(c + 1) * 64]
            tot = _dpp_tree(t)
            nn = f32((n + 63) // 64 * 64) if fault == "padded_n" else f32(n)
            e32 = f32(0) if fault == "no_eps" else f32(eps) * f32(n) if fault == "eps_times_n" else f32(eps)
            rs = f32(1) / np.sqrt(f32(tot / nn) + e32, dtype=f32)
            lim = f32(HALF_MAX if fault == "clamp_65504" else CLAMP)
            clamp = lambda f: np.where(f > 0, np.fmin(f, lim), np.fmax(f, -lim)).astype(f32)
            if fault == "skip_first_rounding":
                f = ((x.astype(np.float64) * np.float64(rs)) * gam.astype(np.float64)).astype(f32)
                f = clamp(f)
            elif fault == "clamp_before_gamma":
                f = (clamp((x * rs).astype(f32)) * gam).astype(f32)
            else:
                f = clamp(((x * rs).astype(f32) * gam).astype(f32))
            o = f.astype(np.float16)
            if fault == "flush_denormals":
                o = np.where(np.abs(o.astype(np.float64)) < SUB, np.copysign(0.0, o.astype(np.float64)), o.astype(np.float64)).astype(np.float16)
            out[r] = o
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# SiLU * mul
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
ALL_GATES = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
SILU_UPS = h16([1.0, -1.0, 1.0 / 3.0, HALF_MAX, 2.0 ** -24, 0.0, -0.0, np.inf, np.nan])


def _half_boundaries():
    """The binary16 rounding boundaries of a positive value: the midpoints of neighbouring halves from 0 up, and 65520."""
    pos = np.arange(0, 0x7C00, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float64)  # 0 .. 65504 ascending
    return np.concatenate([(pos[:-1] + pos[1:]) / 2.0, [65520.0]])


_BOUNDS = _half_boundaries()


def _exp_neg(g16):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp(-g16.astype(np.float64))


def ambiguous_gates(g16, t_ulps=T_ULPS):
    """bool mask: exp(-g) (float64) lies within t_ulps fp32 ulps of a binary16 rounding boundary."""
    e = _exp_neg(np.asarray(g16, np.float16))
    ok = np.isfinite(e)
    ev = np.where(ok, e, 1.0)
    i = np.clip(np.searchsorted(_BOUNDS, ev), 1, _BOUNDS.size - 1)
    lo, hi = _BOUNDS[i - 1], _BOUNDS[i]
    b = np.where(np.abs(ev - lo) <= np.abs(hi - ev), lo, hi)
    ulp32 = 2.0 ** (np.maximum(np.floor(np.log2(b)), -126) - 23)
    return ok & (np.abs(ev - b) <= t_ulps * ulp32)


def ambiguous_set(t_ulps=T_ULPS):
    """The gate bit patterns (u16) of the ambiguous set over all 65536 gates; fails by itself past AMBIGUOUS_CAP."""
    s = np.flatnonzero(ambiguous_gates(ALL_GATES, t_ulps)).astype(np.uint16)
    assert s.size <= AMBIGUOUS_CAP, f"the ambiguous set holds {s.size} of the 65536 gates at T = {t_ulps}: the reference would excuse too much"
    return s


def _silu_from_e(g, e16, u):
    with np.errstate(all="ignore"):
        d = h16(1.0 + e16.astype(np.float64))
        r = h16(1.0 / d.astype(np.float64))
        sv = h16(g.astype(np.float64) * r.astype(np.float64))
        return h16(sv.astype(np.float64) * u.astype(np.float64))


def silu_mul_ref(g16, u16):
    """-> (ref, alt) fp16: the definition with e = half(exp(-g)) from float64; alt = the result from the half on the OTHER side of the boundary for the ambiguous gates
    (equal to ref everywhere else)."""
    g, u = np.asarray(g16, np.float16), np.asarray(u16, np.float16)
    ex = _exp_neg(g)
    e = h16(ex)
    ref = _silu_from_e(g, e, u)
    amb = ambiguous_gates(g)
    with np.errstate(all="ignore"):
        up = np.nextafter(e, np.float16(np.inf))
        dn = np.nextafter(e, np.float16(-np.inf))
        other = np.where(ex > e.astype(np.float64), up, dn).astype(np.float16)  # the neighbour on the side of the true value: the boundary lies between e and it
    alt = np.where(amb, _silu_from_e(g, np.where(amb, other, e).astype(np.float16), u), ref).astype(np.float16)
    return ref, alt


def same_half(a, b):
    """Bit for bit, any NaN matching any NaN."""
    a, b = np.asarray(a, np.float16), np.asarray(b, np.float16)
    return (a.view(np.uint16) == b.view(np.uint16)) | (np.isnan(a) & np.isnan(b))


def silu_mismatches(got16, ref, alt):
    """Indices where got is neither ref nor alt."""
    return np.flatnonzero(~(same_half(got16, ref) | same_half(got16, alt)))


def silu_operands(tail=0):
    """Every gate pattern against every entry of SILU_UPS: 9 * 65536 elements (less `tail` at the end, so that the kernel's scalar tail runs)."""
    g = np.tile(ALL_GATES, SILU_UPS.size)
    u = np.repeat(SILU_UPS, 65536)
    n = g.size - tail
    return np.ascontiguousarray(g[:n]), np.ascontiguousarray(u[:n])


SILU_MUTANTS = ("r_in_fp32", "exp_saturates", "one_rounding_product")


def silu_mul_mutant(g16, u16, fault):
    g, u = np.asarray(g16, np.float16), np.asarray(u16, np.float16)
    g64, u64 = g.astype(np.float64), u.astype(np.float64)
    with np.errstate(all="ignore"):
        ex = _exp_neg(g)
        if fault == "exp_saturates":
            e = h16(np.minimum(ex, HALF_MAX))
            return _silu_from_e(g, np.where(np.isnan(ex), np.float16(np.nan), e).astype(np.float16), u)
        e = h16(ex).astype(np.float64)
        if fault == "r_in_fp32":  # 1 / (1 + e) in fp32, rounded to half once
            r = h16((np.float32(1) / (np.float32(1) + e.astype(np.float32))).astype(np.float64))
            return h16(h16(g64 * r.astype(np.float64)).astype(np.float64) * u64)
        if fault == "one_rounding_product":
            r = h16(1.0 / h16(1.0 + e).astype(np.float64)).astype(np.float64)
            return h16(g64 * r * u64)
    raise AssertionError(fault)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the residual add
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def add_ref(a16, b16):
    with np.errstate(invalid="ignore"):
        return h16(np.asarray(a16, np.float16).astype(np.float64) + np.asarray(b16, np.float16).astype(np.float64))


def add_operands(n=65536):
    """(a, b, {property: index array}): designed pairs first, random bit patterns behind them, n elements."""
    rng = np.random.default_rng(65536)
    A, B, where = [], [], {}

    def put(name, a, b):
        a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
        start = sum(len(x) for x in A)
        A.append(a); B.append(b)
        where[name] = np.arange(start, start + a.size)

    put("overflow", [HALF_MAX, HALF_MAX, 60000, -HALF_MAX, -HALF_MAX, 40000, HALF_MAX, -HALF_MAX], [HALF_MAX, 16, 60000, -16, -HALF_MAX, 30000, 32, -2048])
    put("just_below_overflow", [HALF_MAX, -HALF_MAX, 65472, HALF_MAX], [15.9921875, -8, 40, 2.0 ** -24])
    mags = rng.integers(1, 0x7C00, 512).astype(np.uint16).view(np.float16).astype(np.float64)
    put("cancel_to_plus_zero", np.concatenate([mags, -mags]), np.concatenate([-mags, mags]))
    put("signed_zeros", [-0.0, 0.0, -0.0, 0.0], [-0.0, -0.0, 0.0, 0.0])
    sub = rng.integers(1, 0x200, 256).astype(np.uint16).view(np.float16).astype(np.float64)
    put("subnormal_sums", np.concatenate([sub[:128], SUB * (1 + rng.integers(0, 1024, 128) / 1024.0)]), np.concatenate([sub[128:] * rng.choice([-1, 1], 128), -SUB * (1 + rng.integers(0, 1024, 128) / 1024.0)]))
    ta, tb = [], []
    for e in range(-13, 16):  # a tie at every exponent where half an ulp is itself a half: a = 2^e (1 + k 2^-10), b = +-2^(e - 11), k even and odd
        for k in (0, 1, 2, 511, 1022, 1023):
            for s in (1.0, -1.0):
                for sb in (1.0, -1.0) if k else (1.0,):  # (2^e less half an ulp is a half of the binade below: no tie)
                    ta.append(s * 2.0 ** e * (1 + k / 1024.0)); tb.append(sb * s * 2.0 ** (e - 11))
    put("ties", ta, tb)
    put("inf_and_nan", [np.inf, -np.inf, np.inf, np.inf, np.nan, 1.0, -np.inf], [-np.inf, np.inf, np.inf, -1.0, 1.0, np.nan, -np.inf])
    a, b = h16(np.concatenate(A)), h16(np.concatenate(B))
    assert np.array_equal(a.astype(np.float64), np.concatenate(A), equal_nan=True) and np.array_equal(b.astype(np.float64), np.concatenate(B), equal_nan=True), "a designed operand is no half"
    fill = n - a.size
    assert fill > 0
    a = np.concatenate([a, rng.integers(0, 65536, fill).astype(np.uint16).view(np.float16)])
    b = np.concatenate([b, rng.integers(0, 65536, fill).astype(np.uint16).view(np.float16)])
    check_add_operands(a, b, where)
    return a, b, where


def check_add_operands(a, b, where):
    """The properties the designed pairs are named for, on the stored halves."""
    with np.errstate(invalid="ignore"):
        s = a.astype(np.float64) + b.astype(np.float64)
    ref = add_ref(a, b)
    i = where["overflow"]
    assert np.isinf(ref[i]).all() and np.isfinite(a[i]).all() and np.isfinite(b[i]).all()
    i = where["just_below_overflow"]
    assert np.all(np.abs(ref[i].astype(np.float64)) == HALF_MAX) and np.all(np.abs(s[i]) > HALF_MAX)
    i = where["cancel_to_plus_zero"]
    assert np.all(ref[i].view(np.uint16) == 0)
    i = where["signed_zeros"]
    assert list(ref[i].view(np.uint16)) == [0x8000, 0, 0, 0]
    i = where["subnormal_sums"]
    assert np.all(np.abs(ref[i].astype(np.float64)) < SUB) and np.count_nonzero(ref[i]) > i.size // 2
    i = where["ties"]
    q = s[i] / ulp16(s[i])
    assert np.all(q - np.floor(q) == 0.5), "ties: a sum is no midpoint of two halves"
    i = where["inf_and_nan"]
    assert np.isnan(ref[i][0]) and np.isnan(ref[i][1]) and ref[i][2] == np.inf and ref[i][6] == -np.inf


ADD_MUTANTS = ("round_toward_zero",)


def add_mutant(a16, b16, fault):
    assert fault == "round_toward_zero"
    with np.errstate(all="ignore"):
        s = np.asarray(a16, np.float16).astype(np.float64) + np.asarray(b16, np.float16).astype(np.float64)
        r = h16(s)
        back = r.astype(np.float64)
        away = np.isfinite(s) & (np.abs(back) > np.abs(s))  # rounded away from zero: step back towards it
        r2 = np.where(away, np.nextafter(r, np.float16(0)), r).astype(np.float16)
        return r2


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# designed values for the fused epilogues: one-hot activations against per-row scales, so that every unfused output is ONE exact product
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _gate_values():
    """Gates in (-inf, -11.09], every half within 12 steps of -ln(65520) = -11.0901 (where hexp(-g) turns inf) -- nearest first --, +0, subnormals, and large positive
    ones.  The first nine meet, through UP_VALUES, every kind of edge (a launch of 18 columns holds no more): -0 from r = 0, a zero gate, two overflowing products,
    subnormals, the edge itself."""
    edge = int(np.float16(-11.09).view(np.uint16))
    order = [edge] + [edge + s * d for d in range(1, 13) for s in (1, -1)]
    around = np.asarray(order, np.uint16).view(np.float16).astype(np.float64)
    head = [-HALF_MAX, 0.0, 30000.0, 1000.0, -12.0, 2.0 ** -24, -SUB, around[0], around[1]]
    rest = [-30000.0, -1000.0, -100.0, -20.0, -8.0, -1.0, -2.0 ** -24, -2.0 ** -20, 2.0 ** -17, SUB, 0.5, 1.0, 3.0, 8.0, 11.0, 17.5, 40.0, 40000.0, HALF_MAX]
    return h16(np.concatenate([head, around[2:], rest]))


GATE_VALUES = _gate_values()
UP_VALUES = h16([1.0, -1.0, 3.0, HALF_MAX, -HALF_MAX, 2.0 ** -24, 1.0 / 3.0, 0.0, -7.5, 2.0, 1000.0])  # (11 values against 51 gates: coprime)


def epilogue_values(N, shift=0):
    """N designed unfused outputs of an interleaved gate/up linear (even N): column 2h the gate of pair h, column 2h + 1 its up value.  `shift` rotates the pairing (a
    different set per activation row).  All finite and no -0: each is ONE product 1 * scale of the kernel."""
    assert N % 2 == 0
    hh = np.arange(N // 2) + shift
    v = np.empty(N, np.float16)
    v[0::2] = GATE_VALUES[hh % GATE_VALUES.size]
    v[1::2] = UP_VALUES[(hh + hh // GATE_VALUES.size) % UP_VALUES.size]
    return v


def residual_for(y16, shift=0):
    """Residuals against the exact outputs y, from the add cases: -y (+0), y (doubling: overflow at the top), half an ulp of y (a tie), +-65504 (overflow against a large y),
    a subnormal, 0, in rotation."""
    y = np.asarray(y16, np.float16).astype(np.float64)
    k = (np.arange(y.size) + shift) % 6
    half_ulp = ulp16(y) / 2
    r = np.select([k == 0, k == 1, k == 2, k == 3, k == 4], [-y, y, np.where(half_ulp >= 2.0 ** -24, half_ulp, 2.0 ** -24), np.where(y >= 0, HALF_MAX, -HALF_MAX), 2.0 ** -24 * 3], 0.0)
    return h16(r)


class OneHotLinear:
    """A q4_6 linear (zero points all 8) and one-hot activations whose every output is one exact product: row r of the launch has x[r][k_r] = 1; code k_r of every
    weight row is 9 (q - z = 1), every other code 8 (q - z = 0, so no other product exists, whatever the scale); scale[n][group of k_r] = values(r)[n].  Rows that share
    a group (M > K / G) share their outputs."""

    def __init__(self, M, N, K, G, values_of_group):
        ng = K // G
        self.M, self.N, self.K, self.G = M, N, K, G
        self.k = [(r % ng) * G + 5 + (r // ng) % (G - 8) for r in range(M)]
        self.codes = np.full((N, K), 8, np.uint8)
        self.codes[:, sorted(set(self.k))] = 9
        self.z = np.full((N, ng), 8, np.uint8)
        self.s = np.stack([np.asarray(values_of_group(g), np.float16) for g in range(ng)], axis=1)  # [N][ng]
        assert self.s.shape == (N, ng) and np.isfinite(self.s.astype(np.float64)).all()
        self.a = np.zeros((M, K), np.float16)
        for r, k in enumerate(self.k):
            self.a[r, k] = 1.0
        self.y = np.stack([self.s[:, k // G] for k in self.k])  # [M][N]: the exact unfused outputs
        assert not np.signbit(self.y[self.y == 0]).any(), "a -0 output cannot be designed: the kernels' sums start from +0"


def rnorm_operands(family, N, eps, variant=None, seed=0):
    """A designed row that a one-hot linear and a residual ADD UP to (tce_w4a16_forward_residual_rmsnorm): the target t is a row of the family; the linear's exact
    output y is t / 2 where that is a non-zero half (+0 where it underflows, 1 where t is zero or non-finite: no -0, nothing non-finite in a scale), the residual is
    half(t - y).  -> (y, res, c = the exact half sum, gamma).  The family's property is asserted on c -- except that a sum is never -0 here (x + (-x) is +0), so `zeros`
    is all +0."""
    rng = np.random.default_rng([13, N, int(round(eps * 1e7)), _fam_id(family), seed])
    t = make_rms_row(family, N, rng, variant).astype(np.float64)
    fin = np.isfinite(t)
    half = h16(np.where(fin, t / 2, 0.0)).astype(np.float64)
    y = np.where(fin & (t != 0), np.where(half == 0, 0.0, half), 1.0)
    with np.errstate(invalid="ignore"):
        res = h16(t - y)
    y = h16(y)
    c = add_ref(res, y)
    if family == "zeros":
        assert not c.view(np.uint16).any()
    elif family in ("saturate", "negative_gamma"):
        check_row(family, c)
    else:
        check_row(family, c, variant)
    gamma = saturate_gamma(c, eps, rng) if family == "saturate" else negative_gamma(N, rng) if family == "negative_gamma" else plain_gamma(N, rng)
    if family in ("saturate", "negative_gamma"):
        check_gamma(family, c, gamma, eps)
    assert np.isfinite(y.astype(np.float64)).all() and not np.signbit(y[y == 0]).any()
    return y, res, c, gamma
