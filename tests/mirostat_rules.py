"""How a sampler's mirostat rule is compared with the reference's own (tests/golden/mirostat_golden.npz, recorded from llm/src/Generate.cc's sample_token_mirostat and
sample_token_mirostat_v2): the rules shared by tests/test_mirostat_host.py (generate.mirostat_reference) and tests/test_gpu_mirostat.py (tce_sample_mirostat_f16).
Not a test module.  tests/sampling_rules.py stays what it is: tol(k), the candidate and p rules are its own.

Two expf / logf / log2f / powf implementations differ in their last bits, so the count a row keeps is asserted only where it is DECIDED, and whether it is decided
is computed in float64 from the reference's recorded values and the row's inputs -- never from the result under test.  With eps = 2^-23 (one fp32 ulp, relative: the
bound taken for every transcendental) and T = tol(k) = (k + 8) eps (sampling_rules: what two correct softmaxes over k candidates differ by, relative):

* mode 2 (v2_decided).  The cut compares s_i = -log2f(p_i) with mu.  logit / temp is one IEEE division in every implementation: bit-equal.  p_i moves by T p_i, so s_i
  by T / ln 2 (d(-log2 p) = -dp / (p ln 2)); log2f adds eps |s_i|.  Doubled for slack: delta_i = 2 (T / ln 2 + eps |s_i|).  Decided iff |s_i - mu_in| > delta_i for
  EVERY candidate (the first one past mu decides, but one that may or may not be past mu in front of it moves the cut).
* mode 1 (v1_decided).  First-order propagation through the reference's statements, nt = min(m - 1, kk - 1) terms:
    b_i = logf(p_i / p_{i+1}):  the quotient moves by 2 T + eps relative, logf adds eps |b_i|:        db_i = 2 T + eps + eps |b_i|
    t_i = logf(float(i + 2) / float(i + 1)): the argument is bit-equal, logf adds eps |t_i|
    A = sum t_i b_i:  dA = sum |t_i| db_i + (2 + nt) eps sum |t_i b_i|   (t's ulp, the product's rounding, nt sequential additions)
    B = sum t_i^2:    dB = (3 + nt) eps B
    s = A / B:        ds = (dA + |s| dB) / B + eps |s|,  and eps' = s - 1 adds eps |s|:                 ds' = ds + eps |s|
    L(s) = ln k_f = (ln |s - 1| + mu ln 2 - ln |1 - N^-(s-1)|) / s   (the quotient inside the outer powf is positive on both sides of s = 1)
    dL/ds = -L / s + (1 / (s - 1) - N^-(s-1) ln N / (1 - N^-(s-1))) / s
    roundings behind s: powf(2, mu) eps; powf(N, -eps') eps on N^-eps', which moves 1 - N^-eps' by eps N^-eps' / |1 - N^-eps'| + eps; the product and the quotient
    eps each: e_Q = 4 eps + eps N^-eps' / |1 - N^-eps'|; the exponent 1 / s rounds by eps: eps |ln Q| / |s| on L; the outer powf eps.
    delta_k = 2 (|dL/ds| ds' + (e_Q + eps |ln Q|) / |s| + eps)          -- relative, doubled for slack
  Decided iff every float64 value is finite and |k_f - j| > delta_k k_f for every integer j in [1, kk] (j = 1 guards "k_f < 1 -> 1", j = kk guards "k_f >= kk -> kk").
  kk == 1: no term, s_hat NaN in every implementation, one candidate: decided.
* a decided row: kept equals the reference's; the final p within T, relative; with uniform_override at the midpoint of X's interval in the reference's final p the
  position drawn is X's position and the token's penalised logit is bit-equal to X's -- the token IS X wherever that logit value is unique in the row
  (inside a tie class the reference's order is unspecified and the project's is ascending id); an interval narrower than 4 T has no such point and is not drawn on.
  mu_out: s_X = -log2f(final p of X) moves by T / ln 2 + eps |s_X|; the subtraction of tau, the product with eta and the last subtraction round by half an ulp each,
  taken as eps: dmu = 2 (eta (T / ln 2 + eps |s_X| + eps |s_X - tau|) + eps |eta (s_X - tau)| + eps |mu_out|).
* an undecided row: a token among the candidates, one advance, a finite mu_out.
* at most 10 % of a configuration's rows may be undecided (MAX_UNDECIDED; asserted by the host test from the fixture alone).
"""
from __future__ import annotations

import hashlib
import importlib.util
import math
import os

import numpy as np

import sampling_rules as R

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_mirostat_golden", os.path.join(HERE, "golden", "make_mirostat_golden.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)

CONFIGS = maker.CONFIGS
M = maker.M
REPEAT_PENALTY = maker.REPEAT_PENALTY
tol = R.tol
EPS = 2.0 ** -23
MAX_UNDECIDED = 0.10


def load_fixture() -> dict:
    return dict(np.load(maker.OUT))


def config_inputs(name: str, fixture: dict) -> list:
    """[(logits fp16, recent int32)] of a configuration, regenerated from its seed and checked against the digest recorded with the reference's results."""
    rows = maker.config_rows(name)
    h = hashlib.sha256()
    for logits, recent in rows:
        h.update(logits.tobytes())
        h.update(recent.tobytes())
    assert h.hexdigest() == str(fixture[name + "/digest"]), f"{name}: the regenerated inputs are not the ones the fixture was recorded for (re-record it)"
    return rows


def params_of(name: str):
    from tinychatengine_amd.generate import SamplingParams
    mode, vocab, k, sigma, temp, tau, eta, rows, seed = CONFIGS[name]
    return SamplingParams(temp=temp, top_k=k, top_p=0.95, repeat_penalty=REPEAT_PENALTY, repeat_last_n=64, mirostat=mode, mirostat_tau=tau, mirostat_eta=eta)


def v2_decided(p, mu, k: int) -> tuple[bool, int]:
    """(decided, kept in float64) for the softmax p over the kk sorted candidates (the reference's, or a case's in float64) and the row's mu."""
    p = np.asarray(p, np.float64)
    mu = float(np.float32(mu))
    if np.any(p <= 0.0) or not math.isfinite(mu):
        return False, 1
    s = -np.log2(p)
    delta = 2 * (tol(k) / math.log(2.0) + EPS * np.abs(s))
    hit = np.nonzero(s > mu)[0]
    kept = max(int(hit[0]) if hit.size else int(p.size), 1)
    return bool(np.all(np.abs(s - mu) > delta)), kept


def v1_values(p, mu, vocab: int, m: int) -> dict:
    """s_hat, k_f and the derivation's quantities in float64, from the softmax p over the kk sorted candidates."""
    p = np.asarray(p, np.float64)
    kk = int(p.size)
    nt = kk - 1 if (m - 1 < 0 or m - 1 > kk - 1) else m - 1
    if nt == 0:
        return {"nt": 0, "s_hat": float("nan"), "k_f": float("nan")}
    i = np.arange(nt)
    t = np.log((i + 2.0) / (i + 1.0))
    with np.errstate(all="ignore"):
        b = np.log(p[:nt] / p[1:nt + 1])
        A, B = float((t * b).sum()), float((t * t).sum())
        s = A / B
        e = s - 1.0
        Nn = float(vocab) ** (-e)
        lnQ = math.log(abs(e)) + float(mu) * math.log(2.0) - math.log(abs(1.0 - Nn)) if e != 0.0 and Nn != 1.0 and math.isfinite(Nn) else float("nan")
        L = lnQ / s if s != 0.0 else float("nan")
        k_f = math.exp(L) if math.isfinite(L) and L < 700 else (float("inf") if L >= 700 else float("nan"))
    return {"nt": nt, "t": t, "b": b, "A": A, "B": B, "s_hat": s, "eps": e, "Nn": Nn, "lnQ": lnQ, "L": L, "k_f": k_f}


def keep_rule(k_f: float, kk: int) -> int:
    """the project's rule for k' (include/tce_matmul.h), on a float64 value"""
    if not k_f >= 1.0:
        return 1
    return kk if k_f >= kk else int(k_f)


def v1_decided(p, mu, vocab: int, m: int, k: int) -> tuple[bool, int, dict]:
    """(decided, kept in float64, the float64 values) -- the derivation is the module's docstring."""
    p = np.asarray(p, np.float64)
    kk = int(p.size)
    if kk == 1:
        return True, 1, {"s_hat": float("nan"), "k_f": float("nan")}
    if np.any(p <= 0.0):
        return False, 1, {}
    v = v1_values(p, mu, vocab, m)
    s, k_f = v["s_hat"], v["k_f"]
    if not all(math.isfinite(z) for z in (s, v["lnQ"], v["L"])) or not k_f > 0.0:
        return False, 1, v
    T, nt, t, b, B = tol(k), v["nt"], v["t"], v["b"], v["B"]
    db = 2 * T + EPS + EPS * np.abs(b)
    dA = float((np.abs(t) * db).sum()) + (2 + nt) * EPS * float(np.abs(t * b).sum())
    dB = (3 + nt) * EPS * B
    ds = (dA + abs(s) * dB) / B + EPS * abs(s) + EPS * abs(s)
    Nn, e, lnN = v["Nn"], v["eps"], math.log(float(vocab))
    dL = abs(-v["L"] / s + (1.0 / e - Nn * lnN / (1.0 - Nn)) / s)
    eQ = 4 * EPS + EPS * Nn / abs(1.0 - Nn)
    delta_k = 2 * (dL * ds + (eQ + EPS * abs(v["lnQ"])) / abs(s) + EPS)
    v["delta_k"] = delta_k
    if not math.isfinite(k_f):  # (L >= 700: far past any kk)
        return True, kk, v
    j = np.arange(1, kk + 1, dtype=np.float64)
    return bool(np.all(np.abs(k_f - j) > delta_k * k_f)), keep_rule(k_f, kk), v


def row_decided(name: str, r: int, fixture: dict) -> bool:
    mode, vocab, k, *_ = CONFIGS[name]
    p, mu = fixture[name + "/p"][r], fixture[name + "/mu_in"][r]
    return v2_decided(p, mu, k)[0] if mode == 2 else v1_decided(p, mu, vocab, M, k)[0]


def undecided_count(name: str, fixture: dict) -> tuple[int, int]:
    rows = CONFIGS[name][7]
    return rows, sum(1 for r in range(rows) if not row_decided(name, r, fixture))


def x_position(name: str, r: int, fixture: dict) -> int:
    kept = int(fixture[name + "/kept"][r])
    where = np.nonzero(fixture[name + "/ids"][r][:kept] == fixture[name + "/X"][r])[0]
    assert where.size == 1, f"{name} row {r}: the reference's X is not among the candidates it kept"
    return int(where[0])


def row_u(name: str, r: int, fixture: dict) -> tuple[np.float32, bool]:
    """(u, exact): the midpoint of X's interval in the reference's final p, and whether the interval is wide enough (>= 4 tol) for the draw to be an exact check."""
    k = CONFIGS[name][2]
    kept, i = int(fixture[name + "/kept"][r]), x_position(name, r, fixture)
    cdf = np.cumsum(fixture[name + "/final_p"][r][:kept], dtype=np.float32).astype(np.float64)
    lo = float(cdf[i - 1]) if i else 0.0
    return np.float32((lo + float(cdf[i])) / 2), bool(float(cdf[i]) - lo >= 4 * tol(k))


def dmu(k: int, s: float, tau: float, eta: float, mu_out: float) -> float:
    """the docstring's bound on |mu_out - the other implementation's| for the surprise s of the candidate drawn"""
    return 2 * (eta * (tol(k) / math.log(2.0) + EPS * abs(s) + EPS * abs(s - tau)) + EPS * abs(eta * (s - tau)) + EPS * abs(mu_out))


def mu_bound(name: str, r: int, fixture: dict) -> float:
    mode, vocab, k, sigma, temp, tau, eta, rows, seed = CONFIGS[name]
    pX = float(fixture[name + "/final_p"][r][x_position(name, r, fixture)])
    return dmu(k, -math.log2(pX), tau, eta, float(fixture[name + "/mu_out"][r]))


def check_row(what: str, name: str, r: int, fixture: dict, x: np.ndarray, got: dict) -> dict:
    """One row's result `got` (keys: ids, logits, p, kept, final_p, choice, token, mu_out -- run with mu = the fixture's mu_in and u = row_u's) against the fixture.
    x: the penalised fp32 row (sampling_rules.penalised).  Returns {"decided", "worst": the largest relative error of a p seen}."""
    mode, vocab, k, sigma, temp, tau, eta, rows, seed = CONFIGS[name]
    f = lambda key: fixture[f"{name}/{key}"][r]
    ids = np.asarray(got["ids"], np.int64)
    assert ids.size == k, f"{what}: {ids.size} candidates behind top-k"
    R.check_candidates(what, x, got["ids"], got["logits"], f("ids"), f("logit"))
    worst = R.check_p(what + " p", got["p"], f("p"), k)
    token, kept = int(got["token"]), int(got["kept"])
    assert token in set(ids.tolist()), f"{what}: the token is not among the top-k candidates"
    assert 1 <= kept <= k and math.isfinite(float(got["mu_out"])), f"{what}: kept {kept}, mu_out {got['mu_out']}"
    if not row_decided(name, r, fixture):
        return {"decided": False, "worst": worst}
    kept_ref = int(f("kept"))
    assert kept == kept_ref, f"{what}: keeps {kept}, the reference {kept_ref}"
    worst = max(worst, R.check_p(what + " final p", np.asarray(got["final_p"])[:kept], f("final_p")[:kept_ref], k))
    u, exact = row_u(name, r, fixture)
    if exact:
        i = x_position(name, r, fixture)
        assert int(got["choice"]) == i, f"{what}: u = {u} draws position {got['choice']}, the reference's X stands at {i}"
        assert token == int(ids[i])
        X = int(f("X"))
        assert np.float32(x[token]).view(np.uint32) == np.float32(x[X]).view(np.uint32), f"{what}: token {token}, the reference drew {X} (another logit value)"
        if int(np.count_nonzero(x == np.float32(x[X]))) == 1:  # (over the whole row: a tie class may reach across the top-k boundary)
            assert token == X, f"{what}: token {token}, the reference drew {X}"
        bound = mu_bound(name, r, fixture)
        err = abs(float(got["mu_out"]) - float(f("mu_out")))
        assert err <= bound, f"{what}: mu_out {got['mu_out']} vs the reference's {f('mu_out')}: {err:.3e} > {bound:.3e}"
    return {"decided": True, "worst": worst}
