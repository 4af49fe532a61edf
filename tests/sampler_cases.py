"""Designed logits for the tests of the device sampler (a helper: no tests here, nothing pytest collects; numpy only, nothing of the package is imported).

Gaussian rows spread the top-k evenly over the 4096-logit chunks, almost never tie on purpose, never sit on a threshold and never reach ids >= 2^17.  The cases
here place every winner, every tie and every threshold: at the first and last id, on both sides of a thread (16), wave (1024) and chunk (4096) boundary, in one
chunk or in all, on a cumulative sum or midway between two.

THE REFERENCE (reference()) is written one rule at a time and shares no code with generate.sample_reference:
  1. the penalties id by id, every step ONE np.float32 operation (llm/src/Generate.cc:14-60 of the reference); window ids outside [0, vocab) name no candidate;
  2. the order: a plain Python sort of ALL in-vocabulary ids by descending value -- stable, so equal values (+0 and -0 among them) keep ascending ids;
  3. both softmaxes in float64 on the fp32 candidate values (temperature: the float64 quotient by the fp32 temp);
  4. the top-p cut (the first i >= 1 whose running sum EXCEEDS top_p; that candidate is dropped) and the inverse-CDF draw (the first i with u < cdf_i, else n - 1)
     on the float64 sums.
It also returns d_top_p / d_u: the distance of top_p / u from the nearest float64 cumulative sum that could change n / the choice.

TWO KINDS OF CASE.
  exact       every operation of the fp32 chain is exact (or one correctly rounded division of small integers), so any correct implementation returns the same
              bits: equal logits with a power-of-two number kept (p = 1/k), or one candidate >= 120 above the rest (expf gives 0: p = {1, 0, ...}).  ids, logit
              bits, p and final_p bits, n, choice and token are asserted exactly; top_p and u may sit ON a cumulative sum.
  toleranced  generic values.  ids, logit bits, n, choice and token are still asserted exactly -- the table is built so that sampling_rules.n_band is one value
              and the draw rule (accepted()) leaves one position, which tests/test_sampler_adversarial_host.py asserts for EVERY toleranced case.  p and final_p:
              relative error against float64 <= sampling_rules.tol(k) = (k + 8) 2^-23.
  greedy      temp <= 0: the first maximum of the penalised row.
  undefined   a +inf or NaN logit in a sampled row: the reference's softmax gives NaN and std::discrete_distribution on NaN is undefined.  Only "a token inside
              the vocabulary, the row advances once, the neighbours do not notice" is asserted (a greedy row with +inf IS defined: the +inf id).

THE TEMPERATURE BOUND.  tol(k) has no term for the two roundings the kernel performs in front of the second expf, `lg[i] / temp` and `... - t0` (sampling.hip:
sample_temperature, then sample_token's softmax): each is at most half an ulp of a value of magnitude <= M = max |l_i| / temp, i.e. <= 2^-24 M each, so the
argument of expf is off by at most delta = 2^-23 M, and expf carries an absolute error of its argument into the same RELATIVE error of its value (first order).
Numerator and sum both move by at most delta, so final_p moves by at most 2 delta:
      tol_final(k, M) = tol(k) + 2 * 2^-23 * M.
At ordinary settings (|l| <= 8, temp >= 0.5) the cases keep the two operations exact or the term far below tol(k), and tol(k) alone is asserted; the cases with
temp = 2^-6 and temp = 64 (`temp_extreme`) use tol_final.  M is computed from the case's inputs (the candidates' penalised values), never from a device result.

Gaps between candidate values avoid (87, 104): there expf's true value is an fp32 subnormal, which a device may flush.  Beyond 104 it rounds to 0 in any mode.
"""
from __future__ import annotations

import dataclasses
import functools
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_rules as R  # noqa: E402  (tol, n_band: the project's rules; numpy only)

F16 = np.float16
F32 = np.float32
RING = 64
INT_MIN = -2 ** 31
ONE_BELOW = float(F32(1.0) - F32(2.0 ** -24))  # the largest fp32 below 1: what the generator's 24-bit uniform can reach, and a top_p that is not "off"


@dataclasses.dataclass(frozen=True)
class P:
    """The sampling fields of a row (generate.SamplingParams' names, so that SamplingParams(**dataclasses.asdict(p)) is the same setting)."""
    temp: float = 0.8
    top_k: int = 40
    top_p: float = 0.95
    repeat_penalty: float = 1.0
    alpha_frequency: float = 0.0
    alpha_presence: float = 0.0
    repeat_last_n: int = 64


@dataclasses.dataclass
class Case:
    name: str
    family: str          # geometry | ties | penalties | parameters | nonfinite
    kind: str            # exact | toleranced | greedy | undefined
    vocab: int
    bound: int           # the call's top_k_bound
    logits: np.ndarray   # fp16 [vocab]
    prm: P
    u: float
    ring: np.ndarray = None   # int32 [64]
    pushed: int = 0
    expect: dict = dataclasses.field(default_factory=dict)  # values the design itself fixes (ids, n, choice, token): asserted on the reference by the host test
    temp_extreme: bool = False

    def __post_init__(self):
        if self.ring is None:
            self.ring = np.zeros(RING, np.int32)
        self.ring = np.asarray(self.ring, np.int32)
        assert self.logits.dtype == F16 and self.logits.shape == (self.vocab,) and self.ring.shape == (RING,)

    @property
    def window(self) -> np.ndarray:
        return window_of(self.ring, self.pushed, self.prm.repeat_last_n)

    @property
    def k(self) -> int:
        return 1 if self.prm.temp <= 0 else min(max(self.prm.top_k, 1), self.bound, self.vocab)


def window_of(ring, pushed: int, last_n: int) -> np.ndarray:
    """The last min(last_n, 64) entries of a 64-entry ring after `pushed` pushes, newest first (slots never pushed hold what the ring was made with)."""
    n = min(max(int(last_n), 0), RING)
    return np.array([int(ring[(int(pushed) - 1 - t) % RING]) for t in range(n)], np.int64)


# ---- the reference ----
def penalise(logits_f16: np.ndarray, window_ids, prm) -> np.ndarray:
    x = logits_f16.astype(F32)  # exact
    V = x.size
    rp, af, ap = F32(prm.repeat_penalty), F32(prm.alpha_frequency), F32(prm.alpha_presence)
    counts: dict = {}
    for t in np.asarray(window_ids, np.int64).tolist():
        if 0 <= t < V:
            counts[t] = counts.get(t, 0) + 1
    for t, c in counts.items():
        v = F32(x[t])
        if rp != F32(1.0):
            v = F32(v * rp) if v <= F32(0.0) else F32(v / rp)
        if not (af == F32(0.0) and ap == F32(0.0)):
            pen = F32(F32(F32(c) * af) + F32(F32(1.0) * ap))
            v = F32(v - pen)
        x[t] = v
    return x


def reference(logits_f16: np.ndarray, window_ids, params, u, top_k_bound: int = 256) -> dict:
    """ids int32 [k], logits fp32 [k] (-0 returned as +0), p float64 [k], n, final_p float64 [n], choice, token, d_top_p, d_u.  Greedy (temp <= 0): one candidate,
    p = final_p = {0} (what the device's debug block holds for a greedy row)."""
    assert logits_f16.dtype == F16 and logits_f16.ndim == 1
    x = penalise(logits_f16, window_ids, params)
    assert not np.isnan(x).any() and not np.isposinf(x).any(), "a NaN or +inf logit is outside what the reference's code defines"
    V = x.size
    vals = x.astype(np.float64).tolist()
    order = sorted(range(V), key=vals.__getitem__, reverse=True)  # stable, also under reverse: equal values keep ascending ids; -0.0 == 0.0
    inf = float("inf")
    if params.temp <= 0:
        tok = order[0]
        return {"ids": np.array([tok], np.int32), "logits": np.array([x[tok]], F32) + F32(0.0), "p": np.zeros(1), "n": 1, "final_p": np.zeros(1), "choice": 0,
                "token": tok, "d_top_p": inf, "d_u": inf}
    k = min(max(int(params.top_k), 1), int(top_k_bound), V)
    ids = order[:k]
    l32 = np.array([x[i] for i in ids], F32) + F32(0.0)
    l = l32.astype(np.float64)
    assert l[0] != -inf, "a row of -inf only has no distribution"
    e = np.exp(l - l[0])
    p = e / e.sum()
    cum = np.cumsum(p)
    tp = float(F32(params.top_p))
    n, d_top_p = k, inf
    if tp < 1.0:
        for i in range(1, k):
            if cum[i] > tp:
                n = i
                break
        if k > 1:
            d_top_p = float(np.abs(cum[1:] - tp).min())
    lt = l[:n] / float(F32(params.temp))
    e2 = np.exp(lt - lt[0])
    fp = e2 / e2.sum()
    cdf = np.cumsum(fp)
    uu = float(F32(u))
    choice = n - 1
    for i in range(n):
        if uu < cdf[i]:
            choice = i
            break
    d_u = float(np.abs(cdf[:n - 1] - uu).min()) if n > 1 else inf
    return {"ids": np.array(ids, np.int32), "logits": l32, "p": p, "n": n, "final_p": fp, "choice": choice, "token": int(ids[choice]), "d_top_p": d_top_p, "d_u": d_u}


@functools.lru_cache(maxsize=None)
def _ref_of(name: str) -> dict:
    c = by_name(name)
    return reference(c.logits, c.window, c.prm, c.u, c.bound)


def ref_of(c: Case) -> dict:
    """The reference's result of a case of the table: computed once, shared, not to be modified."""
    return _ref_of(c.name)


# ---- tolerances and the two decisiveness rules ----
def tol_p(c: Case) -> float:
    return R.tol(c.k)


def tol_final(c: Case, ref: dict) -> float:
    if not c.temp_extreme:
        return R.tol(c.k)
    l = np.abs(ref["logits"][:ref["n"]].astype(np.float64))
    M = float(l[np.isfinite(l)].max()) / float(F32(c.prm.temp))
    return R.tol(c.k) + 2.0 * 2.0 ** -23 * M


def accepted(final_p, t: float, u) -> set:
    """sampling_rules.draw_points' acceptance rule for one u: position i is accepted if cdf_{i-1} - t <= u < cdf_i + t (the last position for any u at or above its
    lower edge), cdf the sequential fp32 running sum of the fp32 final p."""
    fp = np.asarray(final_p, F32)
    n = fp.size
    cdf = np.cumsum(fp, dtype=F32).astype(np.float64)
    lo = np.concatenate([[0.0], cdf[:-1]])
    uf = float(F32(u))
    return {i for i in range(n) if lo[i] - t <= uf and (uf < cdf[i] + t or i == n - 1)}


def rel_err(got, ref) -> float:
    """The worst relative error of got against ref; where ref is 0 as an fp32 number (a -inf candidate, or a gap beyond expf's fp32 range) got must be exactly 0."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, f"{got.size} values, the reference has {ref.size}"
    zero = ref.astype(F32) == 0.0
    assert np.all(got[zero] == 0.0), "a candidate of probability exactly 0 has weight"
    return float((np.abs(got[~zero] - ref[~zero]) / ref[~zero]).max()) if (~zero).any() else 0.0


# ---- building rows ----
def boundary_ids(V: int) -> list:
    """The first and last id and both sides of a thread (16), wave (1024) and every chunk (4096) boundary below V, and of the last thread boundary."""
    s = {0, V - 1, 15, 16, 1023, 1024}
    for b in range(4096, V + 1, 4096):
        s |= {b - 1, b}
    m = (V - 1) // 16 * 16
    s |= {m - 1, m}
    return sorted(i for i in s if 0 <= i < V)


def _row(V: int, fill: float) -> np.ndarray:
    r = np.full(V, fill, F16)
    assert float(r[0]) == fill or np.isinf(fill)
    return r


def _put(row: np.ndarray, ids, vals) -> None:
    ids = list(ids)
    assert len(set(ids)) == len(ids) == len(list(vals))
    for i, v in zip(ids, vals):
        row[i] = F16(v)
        assert float(row[i]) == float(v), f"{v!r} is no fp16 value"


def _scrambled(n: int, top: float, step: float, seed: int) -> list:
    """n distinct fp16-exact values top, top - step, ... in a seeded order (so that id order and value order differ)."""
    perm = np.random.default_rng(seed).permutation(n)
    return [top - step * int(j) for j in perm]


def _ring32(ids, filler: int) -> np.ndarray:
    ids = list(ids)
    assert len(ids) <= RING
    return np.array(ids + [filler] * (RING - len(ids)), np.int32)


def _decide(c: Case, want_n: int | None, want_choice: int) -> Case:
    """Places top_p midway between the float64 cumulative sums cum[want_n - 1] and cum[want_n] (None: top_p stays), then u at the midpoint of the CDF interval of
    position want_choice of the final distribution.  The host test asserts that both are then farther than the tolerance from every sum."""
    if want_n is not None:
        r = reference(c.logits, c.window, dataclasses.replace(c.prm, top_p=1.0), 0.0, c.bound)
        cum = np.cumsum(r["p"])
        assert 1 <= want_n < cum.size
        c.prm = dataclasses.replace(c.prm, top_p=float(F32((cum[want_n - 1] + cum[want_n]) / 2)))
    r = reference(c.logits, c.window, c.prm, 0.0, c.bound)
    assert want_n is None or r["n"] == want_n
    cdf = np.concatenate([[0.0], np.cumsum(r["final_p"])])
    assert 0 <= want_choice < r["n"]
    c.u = float(F32((cdf[want_choice] + cdf[want_choice + 1]) / 2))
    c.expect = {**c.expect, "choice": want_choice, **({"n": want_n} if want_n is not None else {})}
    return c


# ---- the table ----
def _geometry() -> list:
    out = []
    one = np.array([2.5], F16)
    for tag, u in (("u0", 0.0), ("ulast", ONE_BELOW), ("u1", 1.0)):
        out.append(Case(f"vocab1_{tag}", "geometry", "exact", 1, 40, one.copy(), P(temp=0.7, top_k=40, top_p=0.95), u, expect={"ids": [0], "n": 1, "choice": 0, "token": 0}))
    five = np.array([1.0, -0.5, 2.0, 0.25, 1.5], F16)
    out.append(_decide(Case("vocab5", "geometry", "toleranced", 5, 40, five, P(temp=0.5, top_k=40), 0.0, expect={"ids": [2, 4, 0, 3, 1]}), 3, 2))
    for V in (40, 4095, 4096, 4097, 8191, 4099):
        W = boundary_ids(V)
        row = _row(V, -30.0)
        _put(row, W, _scrambled(len(W), 4.0, 0.25, V))
        n = len(W) // 2 + 1
        out.append(_decide(Case(f"vocab{V}", "geometry", "toleranced", V, 40, row, P(temp=0.5, top_k=40), 0.0), n, n - 1))
    # 2^20 entries, 256 chunks: ids with bits 17, 18 and 19 set, the last id tied with a low one, k = 32 = the bound at which 256 chunks x k survivors still fit
    V = 1 << 20
    row = _row(V, -30.0)
    big = {(1 << 17) + 5: 3.0, (1 << 18) + 4095: 2.5, (1 << 19) + 4096: 3.5, V - 1: 2.0, 7: 2.0, V - 4096: 1.0, (1 << 19) + (1 << 18) + (1 << 17) + 16: 0.5}
    _put(row, big.keys(), big.values())
    want = [(1 << 19) + 4096, (1 << 17) + 5, (1 << 18) + 4095, 7, V - 1, V - 4096, (1 << 19) + (1 << 18) + (1 << 17) + 16]
    out.append(_decide(Case("vocab_2p20", "geometry", "toleranced", V, 32, row, P(temp=1.0, top_k=32), 0.0, expect={"ids_head": want}), 6, 4))
    # 128256 at k = 256 (256 x 32 chunks = 8192 survivors): the winners in one chunk, eight per chunk, all in the last, partial chunk
    V = 128256
    vals = _scrambled(256, 6.0, 1.0 / 32, 256)
    last = 31 * 4096
    layouts = {"one_chunk": [5 * 4096 + 16 * i + (i % 16) for i in range(256)],
               "eight_per_chunk": [c * 4096 + o for c in range(32) for o in (0, 15, 16, 1023, 1024, 1100, 1278, 1279)],
               "last_chunk": [last + 5 * i for i in range(255)] + [V - 1]}
    for tag, ids in layouts.items():
        row = _row(V, -30.0)
        _put(row, ids, vals)
        out.append(_decide(Case(f"vocab128256_{tag}", "geometry", "toleranced", V, 256, row, P(temp=1.0, top_k=256), 0.0), 100, 57))
    return out


def _ties() -> list:
    out = []
    V = 8197  # three chunks: 4096, 4096 and 5 entries (fewer than any k > 5: the chunk pads with "no element"); vocab % 8 != 0
    flat = _row(V, 1.5)
    out.append(Case("one_value_k1", "ties", "exact", V, 40, flat.copy(), P(temp=0.7, top_k=1, top_p=0.5), 0.5, expect={"ids": [0], "n": 1, "choice": 0, "token": 0}))
    out.append(_decide(Case("one_value_k40", "ties", "toleranced", V, 40, flat.copy(), P(temp=1.0, top_k=40), 0.0, expect={"ids": list(range(40))}), 20, 13))
    out.append(Case("one_value_k256", "ties", "exact", V, 256, flat.copy(), P(temp=0.7, top_k=256, top_p=0.5), 0.5,
                    expect={"ids": list(range(256)), "n": 128, "choice": 64, "token": 64}))
    upper = [5, 100, 1023, 1024, 2000, 3000, 4000, 4094, 4095, 4096, 4097, 5000, 5119, 5120, 6000, 7000, 8000, 8190, 8191, 8192, 8193, 8194, 8195, 8196]
    row = _row(V, -1.0)
    _put(row, upper, [2.0] * 24)
    out.append(Case("two_valued_3k", "ties", "exact", V, 40, row, P(temp=0.7, top_k=8, top_p=0.5), 0.5, expect={"ids": upper[:8], "n": 4, "choice": 2, "token": 1023}))
    row = _row(V, -30.0)
    _put(row, range(4093, 4101), [2.0] * 8)
    out.append(Case("tie_cut_straddles_chunk_exact", "ties", "exact", V, 40, row.copy(), P(temp=0.7, top_k=4, top_p=0.5), 0.5,
                    expect={"ids": [4093, 4094, 4095, 4096], "n": 2, "choice": 1, "token": 4094}))
    _put(row, [8196, 17, 6000], [3.0, 2.5, 2.75])
    out.append(_decide(Case("tie_cut_straddles_chunk", "ties", "toleranced", V, 40, row, P(temp=1.0, top_k=8), 0.0,
                            expect={"ids": [8196, 6000, 17, 4093, 4094, 4095, 4096, 4097]}), 6, 5))
    # the issue's two worked examples: eight equal logits of a 4101-entry row
    V2 = 4101
    eight = [0, 15, 16, 1023, 1024, 4095, 4096, 4100]
    row = _row(V2, -30.0)
    _put(row, eight, [1.25] * 8)
    out.append(Case("eight_equal_half", "ties", "exact", V2, 40, row.copy(), P(temp=0.7, top_k=8, top_p=0.5), 0.5, expect={"ids": eight, "n": 4, "choice": 2, "token": 16}))
    out.append(Case("eight_equal_all", "ties", "exact", V2, 40, row.copy(), P(temp=0.7, top_k=8, top_p=1.0), 1.0, expect={"ids": eight, "n": 8, "choice": 7, "token": 4100}))
    # +0 and -0 are one value: ascending ids whatever the sign, and the candidates come back as +0
    row = _row(V, -4.0)
    _put(row, [3, 5, 4095, 4096, 8190, 8196], [-0.0, 0.0, -0.0, 0.0, 0.0, -0.0])
    assert np.signbit(row[3]) and np.signbit(row[4095]) and not np.signbit(row[5])
    out.append(Case("zeros_mixed", "ties", "exact", V, 40, row, P(temp=0.7, top_k=4, top_p=0.5), 0.5, expect={"ids": [3, 5, 4095, 4096], "n": 2, "choice": 1, "token": 5}))
    row = np.zeros(V, F16)
    row[::2] = F16(-0.0)
    out.append(Case("zeros_interleaved", "ties", "exact", V, 40, row, P(temp=0.7, top_k=8, top_p=1.0), 1.0, expect={"ids": list(range(8)), "n": 8, "choice": 7, "token": 7}))
    # every value negative: the other branch of the order-preserving key
    W = boundary_ids(V)
    row = _row(V, -30.0)
    _put(row, W, _scrambled(len(W), -1.0, 0.25, 77))
    out.append(_decide(Case("all_negative", "ties", "toleranced", V, 40, row, P(temp=0.5, top_k=8), 0.0), 5, 3))
    # fewer finite entries than k, the rest -inf: probability exactly 0, never drawn
    row = _row(V2, -np.inf)
    _put(row, [4100, 16, 1023], [1.0, 0.5, -0.25])
    out.append(_decide(Case("few_finite", "ties", "toleranced", V2, 40, row, P(temp=0.5, top_k=8), 0.0, expect={"ids": [4100, 16, 1023, 0, 1, 2, 3, 4]}), 2, 1))
    row = _row(V2, -np.inf)
    _put(row, [4096, 4095], [0.75, 0.75])
    out.append(Case("two_finite_among_ninf", "ties", "exact", V2, 40, row, P(temp=0.7, top_k=8, top_p=0.9), 0.75,
                    expect={"ids": [4095, 4096, 0, 1, 2, 3, 4, 5], "n": 1, "choice": 0, "token": 4095}))
    row = _row(V2, -np.inf)
    _put(row, [4096, 4095, 7], [0.75, 0.75, 0.75])
    out.append(Case("three_finite_u_last", "ties", "exact", V2, 40, row, P(temp=1.0, top_k=8, top_p=1.0), ONE_BELOW,
                    expect={"ids": [7, 4095, 4096, 0, 1, 2, 3, 4], "n": 8, "choice": 2, "token": 4096}))  # n = 8 kept, five of them of weight 0: u just below 1 still draws a finite one
    # the largest and smallest finite halves
    row = _row(V, 1.0)
    _put(row, [V - 1, 0], [65504.0, -65504.0])
    out.append(Case("max_half", "ties", "exact", V, 40, row, P(temp=0.7, top_k=8, top_p=0.95), 0.5, expect={"ids": [V - 1, 1, 2, 3, 4, 5, 6, 7], "n": 1, "choice": 0, "token": V - 1}))
    row = _row(V, -65504.0)
    _put(row, [4096], [65504.0])
    out.append(Case("min_half_row", "ties", "exact", V, 40, row, P(temp=0.7, top_k=8, top_p=1.0), 1.0, expect={"ids": [4096, 0, 1, 2, 3, 4, 5, 6], "n": 8, "choice": 7, "token": 6}))
    # fp16 subnormals: distinct values that differ by 2^-24
    sub = {4095: 1, 4096: 3, 0: 1023, 8196: -1, 15: -2, 16: 2, 1024: -1023, 1023: 512}
    row = _row(V, -4.0)
    _put(row, sub.keys(), [j * 2.0 ** -24 for j in sub.values()])
    out.append(_decide(Case("subnormals", "ties", "toleranced", V, 40, row, P(temp=1.0, top_k=8), 0.0, expect={"ids": [0, 1023, 4096, 16, 4095, 8196, 15, 1024]}), 5, 2))
    # a peak 120 above the rest: expf gives exactly 0
    row = _row(4099, -20.0)
    _put(row, [4098], [100.0])
    out.append(Case("peak_120", "ties", "exact", 4099, 40, row, P(temp=0.7, top_k=8, top_p=0.95), ONE_BELOW, expect={"ids": [4098, 0, 1, 2, 3, 4, 5, 6], "n": 1, "choice": 0, "token": 4098}))
    # greedy: the maximum in three chunks, the lowest id wins
    row = _row(V, -2.0)
    _put(row, [8196, 4096, 77], [3.0, 3.0, 3.0])
    out.append(Case("greedy_tie_three_chunks", "ties", "greedy", V, 40, row, P(temp=0.0), 0.0, expect={"token": 77}))
    return out


def _penalties() -> list:
    out = []
    V = 8197
    W = boundary_ids(V)  # 0 15 16 1023 1024 4095 4096 8191 8192 8196
    free = [7, 2000, 5000]
    # every boundary id in the ring, some twice and thrice; the unpenalised competitors beside them
    row = _row(V, -30.0)
    _put(row, W + free, _scrambled(len(W), 5.0, 0.125, 5) + [3.0, 2.75, 3.25])
    ring = _ring32(W + W[::2] + W[::3], 2)
    out.append(_decide(Case("pen_boundaries", "penalties", "toleranced", V, 40, row.copy(), P(temp=1.0, top_k=8, repeat_penalty=1.3, alpha_frequency=0.3, alpha_presence=0.2), 0.0,
                            ring=ring, pushed=64), 5, 3))
    out.append(_decide(Case("pen_rp_off_alphas_on", "penalties", "toleranced", V, 40, row.copy(), P(temp=1.0, top_k=8, repeat_penalty=1.0, alpha_frequency=0.3, alpha_presence=0.2), 0.0,
                            ring=ring, pushed=64), 5, 1))
    out.append(_decide(Case("pen_rp_on_alphas_off", "penalties", "toleranced", V, 40, row.copy(), P(temp=1.0, top_k=8, repeat_penalty=1.3), 0.0, ring=ring, pushed=64), 5, 4))
    # ids outside the vocabulary (behind it, where the padding holds 60000; far behind; negative) name nothing
    ring = _ring32([V, V + 3, V + 15, 1 << 20, 2 ** 31 - 1, -1, INT_MIN, 16, -V, -16], 2)
    out.append(_decide(Case("pen_out_of_range", "penalties", "toleranced", V, 40, row.copy(), P(temp=1.0, top_k=8, repeat_penalty=1.3, alpha_frequency=0.3, alpha_presence=0.2), 0.0,
                            ring=ring, pushed=64), 4, 2))
    # one id 64 times: count 64
    row = _row(V, -30.0)
    _put(row, [1024, 15, 4096, 8196, 300], [6.0, 2.5, 2.0, 1.5, 2.25])
    out.append(_decide(Case("pen_count64", "penalties", "toleranced", V, 40, row, P(temp=1.0, top_k=4, repeat_penalty=1.1, alpha_frequency=0.05), 0.0,
                            ring=_ring32([1024] * 64, 2), pushed=64, expect={"ids": [15, 1024, 300, 4096]}), 3, 2))  # 6 / 1.1 - 64 * 0.05 = 2.2545 > 2.25
    # 0, -0 and the smallest negative half under repeat_penalty: the `<= 0` side multiplies
    tiny = 2.0 ** -24
    row = _row(V, -4.0)
    _put(row, [16, 1023, 4096, 8191, 100, 5000], [0.0, -0.0, -tiny, tiny, 0.5, 0.25])
    out.append(_decide(Case("pen_zero_branch", "penalties", "toleranced", V, 40, row, P(temp=1.0, top_k=8, repeat_penalty=1.3), 0.0, ring=_ring32([16, 1023, 4096, 8191], 2), pushed=64,
                            expect={"ids": [100, 5000, 8191, 16, 1023, 4096, 0, 1]}), 5, 4))
    # a window of 17 on a ring pushed 150 times: pushes 133 .. 149 = slots 5 .. 21
    row = _row(V, -30.0)
    strong = [15, 16, 1024, 4095, 4096, 8192, 8196, 600]
    _put(row, strong, [5.0, 4.75, 4.5, 4.25, 4.0, 3.75, 3.5, 3.25])
    ring = np.full(RING, 2, np.int32)
    ring[[5, 13, 21]] = [15, 4096, 8196]   # inside the window
    ring[[4, 22, 63, 0]] = [16, 1024, 4095, 8192]  # just outside it
    out.append(_decide(Case("pen_wrapped_17", "penalties", "toleranced", V, 40, row, P(temp=1.0, top_k=8, repeat_penalty=1.3, alpha_presence=0.5, repeat_last_n=17), 0.0, ring=ring, pushed=150,
                            expect={"ids": [16, 1024, 4095, 8192, 15, 600, 4096, 8196]}), 6, 3))
    # the penalty takes the row's maximum out of its chunk's k and out of the row's k
    row = _row(V, -30.0)
    _put(row, [10, 20, 30, 5000], [5.0, 4.0, 3.5, 3.0])
    out.append(_decide(Case("pen_max_out_of_k", "penalties", "toleranced", V, 40, row, P(temp=1.0, top_k=2, top_p=1.0, repeat_penalty=2.0), 0.0, ring=_ring32([10], 2), pushed=64,
                            expect={"ids": [20, 30]}), None, 1))
    # a negative alpha_frequency lifts an id from outside the k to its head
    row = _row(V, -30.0)
    _put(row, [6000, 15, 16, 4095, 4096], [1.0, 4.0, 3.0, 2.0, 1.5])
    out.append(_decide(Case("pen_negative_alpha", "penalties", "toleranced", V, 40, row, P(temp=1.0, top_k=4, alpha_frequency=-0.5), 0.0, ring=_ring32([6000] * 8, 2), pushed=64,
                            expect={"ids": [6000, 15, 16, 4095]}), 3, 0))
    # greedy on a penalised maximum: 12 / 1.5 = 8 < 10
    row = _row(V, -2.0)
    _put(row, [4096, 15], [12.0, 10.0])
    out.append(Case("greedy_penalised_max", "penalties", "greedy", V, 40, row, P(temp=0.0, repeat_penalty=1.5), 0.0, ring=_ring32([4096], 2), pushed=64, expect={"token": 15}))
    return out


def _parameters() -> list:
    out = []
    V = 4099
    ids = [0, 15, 16, 1023, 1024, 4095, 4096, 4098]
    # temp = 2^-6: gaps of 2^-6 become gaps of 1; two penalised (generic fp32) values among them; the background is 2000 below after the division
    row = _row(V, -30.0)
    _put(row, ids, [1.0, 1.0 - 2.0 ** -6, 1.28125, 1.0 - 3 * 2.0 ** -6, 1.0 - 2.0 ** -5, 1.265625, 1.0 - 5 * 2.0 ** -6, 1.0 - 2.0 ** -4])
    out.append(_decide(Case("temp_small", "parameters", "toleranced", V, 40, row, P(temp=2.0 ** -6, top_k=8, repeat_penalty=1.3), 0.0, ring=_ring32([16, 4095], 2), pushed=64,
                            temp_extreme=True), 6, 2))
    row = _row(V, -30.0)
    _put(row, ids, _scrambled(8, 4.0, 0.5, 64))
    out.append(_decide(Case("temp_large", "parameters", "toleranced", V, 40, row.copy(), P(temp=64.0, top_k=8, repeat_penalty=1.3), 0.0, ring=_ring32([16, 4095], 2), pushed=64,
                            temp_extreme=True), 6, 4))
    base = P(temp=1.0, top_k=8, top_p=1.0)
    out.append(Case("top_p_tiny", "parameters", "toleranced", V, 40, row.copy(), dataclasses.replace(base, top_p=1e-9), 0.5, expect={"n": 1, "choice": 0}))
    out.append(Case("u_zero", "parameters", "toleranced", V, 40, row.copy(), base, 0.0, expect={"n": 8, "choice": 0}))
    out.append(Case("u_last", "parameters", "toleranced", V, 40, row.copy(), base, ONE_BELOW, expect={"n": 8, "choice": 7}))
    out.append(Case("u_one", "parameters", "toleranced", V, 40, row.copy(), base, 1.0, expect={"n": 8, "choice": 7}))
    # top_p = the largest fp32 below 1 is NOT "off": eight equal candidates reach exactly 1.0 at the last one, which is dropped
    eq = _row(V, -30.0)
    _put(eq, ids, [0.5] * 8)
    out.append(Case("top_p_below_one", "parameters", "exact", V, 40, eq, P(temp=0.7, top_k=8, top_p=ONE_BELOW), 0.5, expect={"ids": ids, "n": 7, "choice": 3, "token": 1023}))
    # a row's top_k above the call's bound is clamped to the bound
    row = _row(V, -30.0)
    fifty = [(83 * i) % V for i in range(48)] + [4095, 4096]
    _put(row, fifty, _scrambled(50, 5.0, 1.0 / 16, 50))
    out.append(_decide(Case("top_k_clamped", "parameters", "toleranced", V, 40, row, P(temp=1.0, top_k=100), 0.0), 25, 11))
    return out


def _nonfinite() -> list:
    V = 4099
    out = []
    for tag, bad in (("pinf", np.inf), ("nan", np.nan)):
        row = _row(V, -30.0)
        _put(row, [0, 15, 16, 1023, 1024, 4095], [2.0, 1.5, 1.0, 0.5, 0.25, 0.0])
        row[4096] = F16(bad)
        out.append(Case(f"sampled_{tag}", "nonfinite", "undefined", V, 40, row, P(temp=1.0, top_k=8, top_p=0.9), 0.5))
    row = _row(V, -30.0)
    _put(row, [15, 4096, 4098], [5.0, np.inf, np.inf])
    out.append(Case("greedy_pinf", "nonfinite", "greedy", V, 40, row, P(temp=0.0), 0.0, expect={"token": 4096}))
    return out


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    out = _geometry() + _ties() + _penalties() + _parameters() + _nonfinite()
    assert len({c.name for c in out}) == len(out)
    for c in out:
        c.logits.setflags(write=False)
        c.ring.setflags(write=False)
    return tuple(out)


def by_name(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


def defined(c: Case) -> bool:
    """The cases the reference's code defines (reference() runs on them)."""
    return c.kind != "undefined" and c.name != "greedy_pinf"


def recordable(c: Case) -> bool:
    """The cases tests/golden/make_sampler_designed_golden.py records from the reference's own code: finite logits (its softmax and its `-inf - -inf` are not asked
    for NaN), vocab <= 8200, and k <= vocab (the recording harness insists on k candidates)."""
    return defined(c) and c.vocab <= 8200 and bool(np.isfinite(c.logits.astype(F32)).all()) and (c.prm.temp <= 0 or min(max(c.prm.top_k, 1), c.bound) <= c.vocab)


def digest(cs) -> str:
    h = hashlib.sha256()
    for c in cs:
        h.update(c.name.encode())
        h.update(c.logits.tobytes())
        h.update(c.window.astype(np.int32).tobytes())
        h.update(np.array([c.prm.temp, c.prm.top_p, c.prm.repeat_penalty, c.prm.alpha_frequency, c.prm.alpha_presence], F32).tobytes())
        h.update(np.array([c.k], np.int32).tobytes())
    return h.hexdigest()


def padded(c: Case) -> np.ndarray:
    """The case's row as a call sees it: ld = ceil8(vocab) + 8 entries, 60000.0 behind the vocabulary (the largest values of the row: never candidates)."""
    ld = (c.vocab + 7) // 8 * 8 + 8
    r = np.full(ld, 60000.0, F16)
    r[:c.vocab] = c.logits
    return r
