"""Designed rows for the tests of the mirostat rule (a helper: no tests here, nothing pytest collects; numpy only, nothing of the package is imported).  The model is
tests/stage_cases.py; sampler_cases.penalise / window_of are reused.

THE REFERENCE (reference()) restates the rule of include/tce_matmul.h one statement at a time in float64 and shares no code with generate.mirostat_reference:
  1. the penalties (sampler_cases.penalise), then a stable Python sort of the in-vocabulary ids by descending value: equal values keep ascending ids; kk = min(top_k,
     top_k_bound, vocab) candidates;
  2. l_i = fp32(logit_i / temp) -- ONE IEEE fp32 division, bit-equal in every implementation --, everything behind it in float64: p = exp(l_i - l_0) / sum;
  3. mode 1: nt = min(m - 1, kk - 1) terms (m - 1 < 0: kk - 1), t_i = ln((i + 2) / (i + 1)), b_i = ln(p_i / p_{i+1}), s_hat = sum t b / sum t^2, eps = s_hat - 1,
     k_f = (eps 2^mu / (1 - N^-eps))^(1 / s_hat), with fp32's range restated: 2^mu beyond 2^128 is +inf (and below 2^-150 is 0), which C's powf then carries through;
     k' = 1 for a NaN or k_f < 1, kk for k_f >= kk, else trunc(k_f);
  4. mode 2: k' = the first i with -log2(p_i) > mu, or kk; 0 becomes 1;
  5. final p = the first k' of p renormalised; the inverse-CDF draw on u; mu_out = mu - eta (-log2(final p of the drawn) - tau);
  6. temp <= 0: greedy, the first maximum; mu stays.
It also returns what makes a case DECIDED (tests/mirostat_rules.py: v1_decided / v2_decided on the float64 p) and d_u, the distance of u from the nearest edge of the
final CDF.  tests/test_mirostat_host.py asserts for every case that the cut and the draw are decided, so the device test may assert kept, choice and token exactly.
"""
from __future__ import annotations

import dataclasses
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mirostat_rules as MR  # noqa: E402
import sampling_rules as R  # noqa: E402
from sampler_cases import F16, F32, RING, penalise, window_of  # noqa: E402


@dataclasses.dataclass(frozen=True)
class P:
    """The sampling fields of a row (generate.SamplingParams' names) and the row's m."""
    temp: float = 0.8
    top_k: int = 40
    top_p: float = 0.95
    repeat_penalty: float = 1.0
    alpha_frequency: float = 0.0
    alpha_presence: float = 0.0
    repeat_last_n: int = 64
    tfs_z: float = 1.0
    typical_p: float = 1.0
    mirostat: int = 2
    mirostat_tau: float = 5.0
    mirostat_eta: float = 0.1
    m: int = 100


@dataclasses.dataclass
class Case:
    name: str
    logits: np.ndarray   # fp16 [vocab]
    prm: P
    mu: float            # the row's mu going in
    u: float = 0.5
    bound: int = 40      # the call's top_k_bound
    ring: np.ndarray = None
    pushed: int = 0
    expect: dict = dataclasses.field(default_factory=dict)  # what the design itself fixes: asserted on the reference by the host test

    def __post_init__(self):
        if self.ring is None:
            self.ring = np.zeros(RING, np.int32)
        self.ring = np.asarray(self.ring, np.int32)
        assert self.logits.dtype == F16 and self.logits.ndim == 1 and self.ring.shape == (RING,)

    @property
    def vocab(self) -> int:
        return int(self.logits.size)

    @property
    def window(self) -> np.ndarray:
        return window_of(self.ring, self.pushed, self.prm.repeat_last_n)


def _pow2_f32(mu: float) -> float:
    """2^mu with fp32's range: +inf from 2^128 on, 0 below 2^-150"""
    if mu >= 128.0:
        return float("inf")
    if mu < -150.0:
        return 0.0
    return 2.0 ** mu


def _c_pow(x: float, y: float) -> float:
    """C's pow on doubles, with its special cases (math.pow raises where C returns a value)"""
    try:
        return math.pow(x, y)
    except OverflowError:
        return float("inf")
    except ValueError:
        if x == 0.0 and y < 0:
            return float("inf")
        return float("nan")
    except ZeroDivisionError:
        return float("inf")


def reference(c: Case) -> dict:
    prm = c.prm
    x = penalise(c.logits, c.window, prm)
    V = x.size
    vals = x.astype(np.float64).tolist()
    srt = sorted(range(V), key=vals.__getitem__, reverse=True)  # stable: equal values keep ascending ids
    mu = float(F32(c.mu))
    if prm.temp <= 0:
        tok = srt[0]
        return {"ids": np.array([tok], np.int32), "logits": np.array([x[tok]], F32) + F32(0.0), "mode": 0, "kept": 1, "choice": 0, "token": tok, "mu_out": mu, "decided": True,
                "d_u": 1.0, "p": np.zeros(1), "final_p": np.zeros(1), "s_hat": 0.0, "k_f": 0.0, "surprise": 0.0}
    kk = min(max(int(prm.top_k), 1), c.bound, V)
    ids = np.array(srt[:kk], np.int64)
    l32 = np.array([x[i] for i in ids], F32) + F32(0.0)
    lt = (l32 / F32(prm.temp)).astype(F32).astype(np.float64)
    e = np.exp(lt - lt[0])
    p = e / e.sum()
    s_hat = k_f = 0.0
    tau, eta = float(F32(prm.mirostat_tau)), float(F32(prm.mirostat_eta))
    if prm.mirostat == 1:
        nt = kk - 1 if (prm.m - 1 < 0 or prm.m - 1 > kk - 1) else prm.m - 1
        A = B = 0.0
        for i in range(nt):
            t = math.log((i + 2.0) / (i + 1.0))
            A += t * math.log(p[i] / p[i + 1])
            B += t * t
        s_hat = A / B if B != 0.0 else float("nan")
        eps = s_hat - 1.0
        if math.isnan(s_hat):
            k_f = float("nan")
        else:
            num = eps * _pow2_f32(mu)
            den = 1.0 - _c_pow(float(V), -eps)
            q = num / den if den != 0.0 else (float("nan") if num == 0.0 or math.isnan(num) else math.copysign(float("inf"), num))
            k_f = _c_pow(q, 1.0 / s_hat) if s_hat != 0.0 else float("nan")
        kept = MR.keep_rule(k_f, kk)
        decided = MR.v1_decided(p, mu, V, prm.m, c.bound)[0] if (math.isfinite(k_f) and -120.0 < mu < 120.0) else True  # (a NaN, an infinity: the rule's own branch)
    else:
        kept = kk
        for i in range(kk):
            if -math.log2(p[i]) > mu:
                kept = i
                break
        kept = max(kept, 1)
        decided = MR.v2_decided(p, mu, c.bound)[0]
    fp = p[:kept] / p[:kept].sum()
    cdf = np.cumsum(fp)
    u = float(F32(c.u))
    hit = np.nonzero(u < cdf)[0]
    choice = int(hit[0]) if hit.size else kept - 1
    edges = np.concatenate([[0.0], cdf[:-1]])  # (the last edge, 1.0, is no edge: the last candidate takes whatever rounding leaves)
    surprise = -math.log2(fp[choice])
    return {"ids": ids.astype(np.int32), "logits": l32, "p": p, "mode": prm.mirostat, "s_hat": s_hat, "k_f": k_f, "kept": kept, "final_p": fp, "choice": choice,
            "token": int(ids[choice]), "surprise": surprise, "mu_out": mu - eta * (surprise - tau), "decided": bool(decided), "d_u": float(np.abs(edges[1:] - u).min()) if kept > 1 else 1.0}


def mu_bound(c: Case, ref: dict) -> float:
    """mirostat_rules' dmu on the case's float64 values"""
    return MR.dmu(c.bound, ref["surprise"], c.prm.mirostat_tau, c.prm.mirostat_eta, ref["mu_out"])


def _generic(V: int, seed: int, sigma: float = 2.5) -> np.ndarray:
    return (np.random.default_rng(seed).standard_normal(V, dtype=np.float32) * F32(sigma)).astype(F16)


def _ladder(V: int, vals, at=None, fill: float = -40.0) -> np.ndarray:
    """A row of `fill` with the given fp16-exact values at ids `at` (default: spread over the row, not in value order)."""
    row = np.full(V, fill, F16)
    vals = list(vals)
    at = list(at) if at is not None else [(7 + 37 * j) % V for j in range(len(vals))]
    assert len(set(at)) == len(at) == len(vals)
    for i, v in zip(at, vals):
        row[i] = v
        assert float(row[i]) == v, f"{v} is not an fp16 value"
    return row


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    out = []
    # geometry: one chunk; a second chunk that holds ONE id (the row's best); top_k_bound 256 with kk = 256, 2 and 1
    out.append(Case("v300_one_chunk_v2", _generic(300, 11), P(mirostat=2, mirostat_tau=3.0), mu=4.0))
    out.append(Case("v300_one_chunk_v1", _generic(300, 12), P(mirostat=1, mirostat_tau=3.0), mu=6.0))
    x = _generic(4097, 13)
    x[4096] = 12.0
    out.append(Case("v4097_last_id_best_v1", x.copy(), P(mirostat=1, mirostat_tau=3.0), mu=6.0, u=0.01, expect={"token": 4096}))
    out.append(Case("v4097_last_id_best_v2", x.copy(), P(mirostat=2, mirostat_tau=3.0), mu=5.0, u=0.01, expect={"token": 4096}))
    out.append(Case("kk256_v2_all_pass", _generic(300, 14, 1.0), P(mirostat=2, top_k=256), mu=50.0, u=0.7, bound=256, expect={"kept": 256}))
    out.append(Case("kk256_v1", _generic(300, 15), P(mirostat=1, top_k=256, mirostat_tau=2.0), mu=4.0, u=0.3, bound=256))
    out.append(Case("kk2_v1", _generic(300, 16), P(mirostat=1, top_k=2), mu=3.0, bound=256))
    out.append(Case("kk2_v2", _generic(300, 17), P(mirostat=2, top_k=2), mu=0.9, bound=256))
    out.append(Case("kk1_v1", _generic(300, 18), P(mirostat=1, top_k=1), mu=10.0, bound=256, expect={"kept": 1, "nan": True}))
    out.append(Case("kk1_v2", _generic(300, 19), P(mirostat=2, top_k=1), mu=10.0, bound=256, expect={"kept": 1}))
    # m: two candidates' worth of terms; more terms asked for than there are candidates; m = 1 (no term: NaN)
    out.append(Case("m2_v1", _generic(4097, 20), P(mirostat=1, m=2, mirostat_tau=3.0), mu=5.0))
    out.append(Case("m_above_kk_v1", _generic(4097, 21), P(mirostat=1, m=1000, mirostat_tau=3.0), mu=6.0))
    out.append(Case("m0_v1", _generic(4097, 21), P(mirostat=1, m=0, mirostat_tau=3.0), mu=6.0))  # (size_t(m - 1): every term, the same row as above)
    out.append(Case("kf_nan_m1_v1", _generic(4097, 22), P(mirostat=1, m=1), mu=10.0, expect={"kept": 1, "nan": True}))
    # k_f < 1, >= kk, +inf
    out.append(Case("kf_below_1_v1", _generic(4097, 23), P(mirostat=1), mu=-20.0, expect={"kept": 1}))
    out.append(Case("kf_above_kk_v1", _generic(4097, 24), P(mirostat=1), mu=30.0, u=0.9, expect={"kept": 40}))
    out.append(Case("kf_inf_v1", _generic(4097, 25), P(mirostat=1), mu=200.0, u=0.9, expect={"kept": 40, "inf": True}))
    # mode 2: nothing passes (the rule keeps one); everything passes
    out.append(Case("mu_small_v2", _generic(4097, 26), P(mirostat=2), mu=0.001, expect={"kept": 1}))
    out.append(Case("mu_large_v2", _generic(4097, 27), P(mirostat=2), mu=60.0, u=0.95, expect={"kept": 40}))
    # equal logits around the cut: four distinct candidates, six equal ones, the rest far below.  Equal logits have bit-equal p and surprise in any implementation, so mu a
    # little above their surprise keeps all six, a little below drops all six
    lad = [8.0, 7.0, 6.5, 6.0] + [5.0] * 6 + [1.0 - 0.25 * j for j in range(30)]
    row = _ladder(300, lad)
    pe = reference(Case("probe", row, P(mirostat=2), mu=60.0))["p"]
    s_eq = -math.log2(pe[4])
    assert all(pe[4] == pe[j] for j in range(4, 10))
    out.append(Case("equal_logits_inside_v2", row, P(mirostat=2), mu=float(F32(s_eq + 0.01)), u=0.99, expect={"kept": 10}))
    out.append(Case("equal_logits_outside_v2", row, P(mirostat=2), mu=float(F32(s_eq - 0.01)), u=0.99, expect={"kept": 4}))
    # penalties in front of the rule: the window holds the row's best ids
    g = _generic(4097, 28)
    best = np.argsort(-g.astype(F32), kind="stable")[:3]
    ring = np.zeros(RING, np.int32)
    ring[:3] = best
    out.append(Case("penalised_v2", g, P(mirostat=2, repeat_penalty=1.3, alpha_frequency=0.2, mirostat_tau=3.0), mu=4.5, ring=ring, pushed=3))
    out.append(Case("penalised_v1", g, P(mirostat=1, repeat_penalty=1.3, alpha_presence=0.5, mirostat_tau=3.0), mu=6.0, ring=ring, pushed=3))
    # greedy rows: the mode is set, nothing of it runs
    out.append(Case("greedy_mode2", _generic(4097, 29), P(mirostat=2, temp=0.0), mu=7.25, expect={"kept": 1}))
    out.append(Case("greedy_mode1", _generic(4097, 30), P(mirostat=1, temp=-1.0), mu=-3.5, expect={"kept": 1}))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def by_name(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def _ref_of(name: str) -> dict:
    return reference(by_name(name))


def ref_of(c: Case) -> dict:
    """The reference's result of a case of the table: computed once, shared, not to be modified."""
    return _ref_of(c.name)


def padded(c: Case) -> np.ndarray:
    """The case's row as a call sees it: ld = ceil8(vocab) + 8 entries, 60000.0 behind the vocabulary (the largest values of the row: never candidates)."""
    ld = (c.vocab + 7) // 8 * 8 + 8
    r = np.full(ld, 60000.0, F16)
    r[:c.vocab] = c.logits
    return r
