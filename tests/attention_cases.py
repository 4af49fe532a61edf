"""Designed attention rows for the tests of the attention kernels (a helper: no tests here, nothing pytest collects).

Gaussian q, K and V give score rows that span 2 - 5 nats: the running maximum of an online softmax never has to move, every merge weight is near 1 and no score
leaves binary16's range, so the rescale, the merges and the check_inf_half rule of the kernels do nothing that a test could see.  The generators here build rows on
which they do, and ASSERT that -- on the float64 scores of the values actually stored, after every rounding -- before they hand a case out.

Construction (make_case): per key / value head a pilot direction d (a binary16 Gaussian vector, truncated at 2.5 sigma -- 2 for the out-of-range families -- so that no designed key overflows binary16),
    q[row][head] = a * d + 0.05 * noise            a in {1, -1, 1/2, 2} in rotation over (row + head)
    K[j]         = t_j * d / (alpha |d|^2) + 0.3 * noise
so that alpha q . K[j] is about a * t_j: one K gives an ascending row (a = 1), a descending one (a = -1), a gentler and a steeper one.  V is Gaussian, sigma 0.8.
A property of a family is therefore asserted on scores / a (the family's own direction), for every head.

Also here: the float64 reference (tests/test_gpu_attention.py::_attention_reference_f64 with the same clamp rule, plus an optional per-row visibility for prefill),
the bound, and the error ratio.
"""
import numpy as np

HD = 128
ALPHA = float(np.float16(1.0 / np.sqrt(HD)))  # what alpha_half.bin holds
HALF_MAX = 65504.0
A_ROTATION = (1.0, -1.0, 0.5, 2.0)

FAMILIES = ("sink_first", "sink_last", "sink_own", "two_peaks", "stairs_up", "stairs_down", "ramp_up", "flat", "out_of_range", "all_out_of_range", "subnormal_v")
OUT_OF_RANGE = ("out_of_range", "all_out_of_range")
# the sizes of the decode tests, chosen for the chunk rule of the step (one chunk up to 320 keys, four up to 640 or 1024, eight beyond) and for runs of a wave that
# are no multiple of its 16-key block
SIZES = (1, 5, 17, 128, 320, 321, 641, 1025)


# ---- reference, bound, ratio ----
def reference_f64(q, K, V, alpha=ALPHA, mask=None, visible=None):
    """softmax(alpha q K^T + mask) V per head in float64 on binary16 inputs; a score outside binary16's range (inf and NaN included) becomes -65504 and still takes
    part (check_inf_half).  q [heads][hd], K / V [heads][keys][hd] (already repeated per query head), mask [keys] additive or None.  visible: bool [keys] or None -- a
    key that is not visible (behind a prefill row's causal bound) weighs nothing at all, which is not the clamp."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = alpha * np.einsum("hd,hkd->hk", q.astype(np.float64), K.astype(np.float64))
        if mask is not None:
            s = s + mask.astype(np.float64)[None, :]
        s = np.where(np.abs(s) <= HALF_MAX, s, -HALF_MAX)
    if visible is not None:
        s = np.where(np.asarray(visible, bool)[None, :], s, -np.inf)
    s = s - s.max(axis=1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=1, keepdims=True)
    return np.einsum("hk,hkd->hd", p, V.astype(np.float64))


def bound(ref):
    """The project's bound for the fp32 attention kernels, |out - ref| <= 2e-3 max|ref| per head + 2^-11 |ref| (tests/test_gpu_attention.py), plus 2^-25: half the
    spacing of binary16 subnormals, the rounding of the final conversion when the output itself is subnormal (a correctly rounded result of the `subnormal_v` family
    is up to that far from float64, which the two relative terms do not cover there; everywhere else the term is below 1e-4 of the bound)."""
    ref = np.asarray(ref, np.float64)
    return 2e-3 * np.abs(ref).max(axis=-1, keepdims=True) + 2.0 ** -11 * np.abs(ref) + 2.0 ** -25


def error_ratio(got, ref):
    """The worst |got - ref| / bound(ref); inf where got is not finite."""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / bound(ref)).max())


# ---- the e4m3 grid ----
def e4m3_exponent_for(x):
    """The smallest scale exponent e in [-8, 7] with max|x| <= 448 * 2^e."""
    top = float(np.abs(np.asarray(x, np.float64)).max())
    for e in range(-8, 8):
        if top <= 448.0 * 2.0 ** e:
            return e
    raise AssertionError(f"max |x| = {top} does not fit e4m3 with an exponent up to 7")


def on_e4m3_grid(x_f16, e):
    from tinychatengine_amd.paged_kv import fp8_dequantize_reference, fp8_quantize_reference
    return fp8_dequantize_reference(fp8_quantize_reference(np.ascontiguousarray(x_f16), e), e)


# ---- the cases ----
class Case:
    """q fp16 [rows][heads][hd] (a decode step has one row), K / V fp16 [kv_heads][n][hd], a [rows][heads] (0 where a row has no pilot), ke / ve: the e4m3 exponents
    K and V were rounded for, or None."""

    def __init__(self, family, n, q, K, V, a, ke=None, ve=None, own=None):
        self.family, self.n, self.q, self.K, self.V, self.a, self.ke, self.ve = family, n, q, K, V, a, ke, ve
        self.own = n - 1 if own is None else own  # the key index of the token's own row (what `sink_own` peaks at)
        self.rows, self.heads = q.shape[0], q.shape[1]
        self.kv_heads = K.shape[0]
        self.rep = self.heads // self.kv_heads

    def repeated(self, upto=None):
        """K and V per QUERY head, the first `upto` keys."""
        upto = self.n if upto is None else upto
        return np.repeat(self.K[:, :upto], self.rep, axis=0), np.repeat(self.V[:, :upto], self.rep, axis=0)

    def scores(self, row=0):
        """The raw float64 scores alpha q . K of the stored values, [heads][n]: no mask, no clamp."""
        Kr, _ = self.repeated()
        return ALPHA * np.einsum("hd,hkd->hk", self.q[row].astype(np.float64), Kr.astype(np.float64))

    def reference(self, row=0, mask=None, upto=None, visible=None):
        Kr, Vr = self.repeated(upto)
        return reference_f64(self.q[row], Kr, Vr, ALPHA, mask, visible)

    def check(self):
        """Assert the family's defining property on what the case holds NOW (a test that replaces q or a key by its rotated form calls this again)."""
        for r in range(self.rows):
            _assert_property(self, r, self.own)

    def qkv_row(self, row=0, key=None):
        """The fused projection's row [(heads + 2 kv_heads) * hd] for a launch that appends key index `key` (default: the last one) with query row `row`."""
        key = self.n - 1 if key is None else key
        return np.concatenate([self.q[row].reshape(-1), self.K[:, key].reshape(-1), self.V[:, key].reshape(-1)])


def _targets(family, n, step, own):
    t = np.zeros(n)
    j = np.arange(n)
    if family == "sink_first":
        t[0] = 40.0
    elif family == "sink_last":
        t[max(n - 2, 0)] = 40.0
    elif family == "sink_own":
        t[own] = 40.0
    elif family == "two_peaks":
        t[min(3, n - 1)] = 50.0
        t[max(n - 2, 0)] = 50.0
    elif family == "stairs_up":
        t = step * (j // 16).astype(np.float64)
    elif family == "stairs_down":
        t = -step * (j // 16).astype(np.float64)
    elif family == "ramp_up":
        t = 0.5 * j
    return t


def make_case(family, n, heads, kv_heads, seed, rows=1, own=None, e4m3=False, ke=None, ve=0, step=100.0):
    """One seeded case of `family` with n keys.
    own:  the key index of the token's own row for `sink_own` (default n - 1, the decode step's).
    e4m3: K and V are rounded to the e4m3 grid -- K for `ke` (default: the smallest exponent that holds it; Case.ke says which), V for `ve`.
    step: the height of a stair.  The table's 100 on binary16; the e4m3 grid's rounding of K moves a score of t by about 0.004 t, so a
          staircase on that grid needs taller stairs to keep every one above 90: 200 keeps them."""
    assert family in FAMILIES and n >= 1 and heads % kv_heads == 0
    rep = heads // kv_heads
    rng = np.random.default_rng([seed, FAMILIES.index(family), n, heads, kv_heads, rows])
    g = lambda *shape: rng.standard_normal(shape)
    own = n - 1 if own is None else own
    a = np.array([[A_ROTATION[(r + h) % 4] for h in range(heads)] for r in range(rows)])
    V = (g(kv_heads, n, HD) * 0.8).astype(np.float16)
    if family == "subnormal_v":  # no pilot: Gaussian q and K, the values are what is designed
        a = np.zeros_like(a)
        q = (g(rows, heads, HD) * 0.9).astype(np.float16)
        K = (g(kv_heads, n, HD) * 0.8).astype(np.float16)
        # clipped: a 5 sigma draw would reach 2^-14, the smallest normal, and 3.5 * 2^-16 would round up to it on the e4m3 grid of
        # exponent -8, whose step is 2^-17
        V = (np.clip(g(kv_heads, n, HD) * 0.8, -3.4, 3.4) * 2.0 ** -16).astype(np.float16)
    else:
        # out of range: a larger |d|^2 keeps the designed keys, 4 * 65504 d / (alpha |d|^2), below 40000
        sigma = 2.0 if family in OUT_OF_RANGE else 1.0
        clip = 2.0 if family in OUT_OF_RANGE else 2.5
        d = (np.clip(g(kv_heads, HD), -clip, clip) * sigma).astype(np.float16).astype(np.float64)
        unit = d / (ALPHA * (d * d).sum(axis=1, keepdims=True))  # alpha unit . d == 1
        if family == "flat":
            a = np.zeros_like(a)
            q = np.zeros((rows, heads, HD), np.float16)
        else:
            q = (a[:, :, None] * np.repeat(d, rep, axis=0)[None] + 0.05 * g(rows, heads, HD)).astype(np.float16)
        if family in OUT_OF_RANGE:
            t = np.zeros(n)
            if family == "out_of_range":
                hit = rng.choice(n, size=min(n, max(2, n // 9)), replace=False)
                t[hit] = 4.0 * HALF_MAX * rng.choice([-1.0, 1.0], size=hit.size)
            else:
                t = 4.0 * HALF_MAX * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        else:
            t = _targets(family, n, step, own)
        noise = 0.3 * g(kv_heads, n, HD)
        if family == "two_peaks":  # the two peaks are the SAME row: equal scores to the bit, whatever q's noise; merge weights of exactly 1/2
            noise[:, [min(3, n - 1), max(n - 2, 0)]] = 0.0
        K = t[None, :, None] * unit[:, None, :] + noise
        assert np.abs(K).max() < 40000.0, f"{family}: a designed key reaches {np.abs(K).max():.0f}"
        K = K.astype(np.float16)
    if e4m3:
        fits = e4m3_exponent_for(K)
        assert ke is None or ke >= fits, f"{family}: K needs the exponent {fits}, not {ke}"
        ke = fits if ke is None else ke
        K, V = on_e4m3_grid(K, ke), on_e4m3_grid(V, ve)
    case = Case(family, n, q, K, V, a, ke if e4m3 else None, ve if e4m3 else None, own)
    case.check()
    return case


def _assert_property(case, row, own):
    """The family's defining property on the achieved float64 scores of the stored values -- in the row's own direction (scores / a) wherever the row has one."""
    f, n = case.family, case.n
    s = case.scores(row)
    what = f"{f}, n = {n}, row {row}"
    if f in OUT_OF_RANGE:
        mag = np.abs(s)
        assert np.all((mag > 1.5 * HALF_MAX) | (mag < 0.5 * HALF_MAX)), f"{what}: a score sits near the edge of binary16's range"
        if f == "all_out_of_range":
            assert np.all(mag > 1.5 * HALF_MAX), f"{what}: a score is in range"
        else:
            assert np.all((mag > 1.5 * HALF_MAX).sum(axis=1) >= min(n, 2)), f"{what}: fewer than two scores out of range"
        return
    if f == "flat":
        assert np.all(s == 0.0), f"{what}: the scores are not all exactly 0"
        return
    if f == "subnormal_v":
        assert float(np.abs(case.V.astype(np.float64)).max()) < 2.0 ** -14, f"{what}: a value is a normal binary16 number"
        assert np.any(case.reference(row) != 0.0), f"{what}: the float64 reference is all zero"
        return
    u = s / case.a[row][:, None]  # every head in its own direction
    if f in ("sink_first", "sink_last", "sink_own"):
        win = {"sink_first": 0, "sink_last": max(n - 2, 0), "sink_own": own}[f]
        if n > 1:
            assert np.all(u[:, win:win + 1] - np.delete(u, win, axis=1) >= 30.0), f"{what}: the sink is not 30 nats above every other key"
    elif f == "two_peaks":
        p0, p1 = min(3, n - 1), max(n - 2, 0)
        assert np.all(np.abs(u[:, p0] - u[:, p1]) <= 1.0), f"{what}: the peaks differ by more than a nat"
        rest = np.delete(u, [p0, p1], axis=1)
        if rest.shape[1]:
            assert np.all(np.minimum(u[:, p0], u[:, p1])[:, None] - rest >= 30.0), f"{what}: a peak is not 30 nats above the rest"
    elif f in ("stairs_up", "stairs_down"):
        sign = 1.0 if f == "stairs_up" else -1.0
        if n > 16:
            assert np.all(sign * (u[:, 16:] - u[:, :-16]) >= 90.0), f"{what}: a stair is lower than 90 nats (lowest {(sign * (u[:, 16:] - u[:, :-16])).min():.1f})"
    elif f == "ramp_up":
        # the maxima of the full 16-key blocks rise strictly; a trailing partial block (as little as one key) is above the block before the last full one
        bm = np.array([u[:, b:b + 16].max(axis=1) for b in range(0, n - n % 16, 16)]).reshape(-1, u.shape[0])
        assert np.all(np.diff(bm, axis=0) > 0.0), f"{what}: the block maxima are not monotone"
        if n % 16 and len(bm) >= 2:
            assert np.all(u[:, n - n % 16:].max(axis=1) > bm[-2]), f"{what}: the trailing block falls behind"


def masked_sink(case):
    """An additive mask [n] that switches the family's sink key off (-65504), and the key's index."""
    win = {"sink_first": 0, "sink_last": max(case.n - 2, 0)}[case.family]
    mask = np.zeros(case.n, np.float16)
    mask[win] = np.float16(-HALF_MAX)
    return mask, win


# ---- rotation ----
def rope_tables(positions, seed):
    """cos / sin fp16 [positions][hd] of random angles, both halves alike: a true rotation of the pairs (j, j + hd / 2), as RotaryPosEmb's tables are."""
    ang = np.random.default_rng(seed).uniform(0, 2 * np.pi, (positions, HD // 2))
    return np.concatenate([np.cos(ang), np.cos(ang)], axis=1).astype(np.float16), np.concatenate([np.sin(ang), np.sin(ang)], axis=1).astype(np.float16)


def unrotate(y, cos_row, sin_row):
    """The binary16 x [..][hd] whose rotation x cos + (-x[hd/2:], x[:hd/2]) sin is y up to binary16 rounding: the inverse rotation in float64, rounded."""
    y, c, s = y.astype(np.float64), cos_row.astype(np.float64)[: HD // 2], sin_row.astype(np.float64)[: HD // 2]
    lo, hi = y[..., : HD // 2], y[..., HD // 2:]
    return np.concatenate([lo * c + hi * s, hi * c - lo * s], axis=-1).astype(np.float16)
