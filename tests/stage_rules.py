"""How a sampler's tail-free and typical stages are compared with the reference's own (tests/golden/sampler_stages_golden.npz, recorded from llm/src/Generate.cc): the
rules shared by tests/test_sampler_stages_host.py (generate._chain) and tests/test_gpu_sampler_stages.py (tce_sample_stages_f16).  Not a test module.
tests/sampling_rules.py stays what it is: tol(k), the candidate, p and draw rules are its own.

Two expf / logf implementations differ in their last bits, so a cut or an order is asserted only where it is DECIDED, and whether it is decided is computed from the
reference's values and the row's inputs in float64 -- never from the result under test:

* tail-free (tfs_decided): tfs_z lies farther than delta_tfs = 16 * 2^-23 / S + tol(k) from every cumulative weight with index >= 1 (index 0 cannot cut), S = the float64
  sum of the |second differences|.
* typical (typical_decided): typical_p lies farther than tol(k) from every cumulative sum of p in score order, and among the first n2 + 1 positions of that order any two
  candidates of DIFFERENT logit value differ in score by more than eps_s = 2 tol(k) (1 + max_i |ln p_i|).  Candidates of equal logit have bit-equal p and score in any
  implementation; the project's rule orders them by id (the earlier candidate first).
* a decided row: n_tfs and n_typ equal the reference's; the final order equals the reference's value for value (bit-equal logits position by position), its ids being
  the sorted candidates' own ids class by class in ascending order; n lies in sampling_rules.n_band of the reference's p_top and EQUALS the reference's wherever top_p
  itself is decided (the band is then one value); p and p_top within tol(k) relative; where n equals the reference's, the final p within tol(k) and every draw point of the reference's final p.
* an undecided row: a token among the top-k candidates, and (on the device) the row advances once.
* at most 10 % of a configuration's rows may be undecided (asserted by the host test from the fixture alone).
"""
from __future__ import annotations

import hashlib
import importlib.util
import os

import numpy as np

import sampling_rules as R

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_sampler_stages_golden", os.path.join(HERE, "golden", "make_sampler_stages_golden.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)

CONFIGS = maker.CONFIGS
VOCAB = maker.VOCAB
TOP_P, TEMP, REPEAT_PENALTY = maker.TOP_P, maker.TEMP, maker.REPEAT_PENALTY
tol = R.tol
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
    k, sigma, z, typ, rows, seed = CONFIGS[name]
    return SamplingParams(temp=TEMP, top_k=k, top_p=TOP_P, repeat_penalty=REPEAT_PENALTY, repeat_last_n=64, tfs_z=z, typical_p=typ)


def tfs_decided(p, z, k: int) -> tuple[bool, int]:
    """(decided, n1 in float64) for the softmax p (the reference's, or a case's in float64) over the kk sorted candidates and tail-free's z.

    delta_tfs, derived.  p_i = e_i / s: the divisor s is common to every p and cancels in w_i = d2_i / S, so what two correct implementations disagree on is one expf ulp
    per e_i, a relative 2^-23 =: eps of p_i (the roundings of the two subtractions are half ulps of smaller magnitudes).  d2_i = |p_i - 2 p_{i+1} + p_{i+2}| moves by at
    most eps (p_i + 2 p_{i+1} + p_{i+2}), and since sum p = 1 all d2 together move by at most 4 eps.  cum_i = (sum_{j <= i} d2_j) / S with cum_i <= 1: the numerator moves
    by <= 4 eps and S by <= 4 eps, so cum_i moves by <= (4 eps + cum_i 4 eps) / S <= 8 eps / S; doubled for slack: 16 * 2^-23 / S.  Then up to k sequential fp32
    additions of the weights and their divisions, a relative tol(k) of a value <= 1.  Nothing in this derivation exceeds the bound the rules state, so it is the one used.
    S == 0: every weight is NaN in every implementation, nothing is cut: decided.  The stage does not run for z >= 1 or kk <= 2: decided."""
    p = np.asarray(p, np.float64)
    kk = int(p.size)
    zf = float(np.float32(z))
    if not zf < 1.0 or kk <= 2:
        return True, kk
    d1 = p[:-1] - p[1:]
    d2 = np.abs(d1[:-1] - d1[1:])
    S = float(d2.sum())
    if S == 0.0:
        return True, kk
    cum = np.cumsum(d2 / S)
    delta = 16 * 2.0 ** -23 / S + tol(k)
    hit = np.nonzero(cum[1:] > zf)[0]
    n1 = int(hit[0]) + 1 if hit.size else kk
    return bool(np.all(np.abs(cum[1:] - zf) > delta)), n1


def typical_decided(logit, n1: int, typical_p, k: int) -> tuple[bool, np.ndarray, int]:
    """(decided, order, n2) in float64 for the sorted candidates' logits (bit-equal in every implementation), the first n1 of which reach the typical stage."""
    l = np.asarray(logit, np.float64)[:n1]
    tf = float(np.float32(typical_p))
    if not tf < 1.0:
        return True, np.arange(n1), n1
    e = np.exp(l - l[0])
    p = e / e.sum()
    if np.any(p == 0.0):  # (-inf scores: the NaN path keeps the order in every implementation only where fp32 underflows too: not decided here)
        return False, np.arange(n1), n1
    lp = np.log(p)
    H = float(-(p * lp).sum())
    s = np.abs(-lp - H)
    order = np.lexsort((np.arange(n1), s))
    cum = np.cumsum(p[order])
    hit = np.nonzero(cum > tf)[0]
    n2 = int(hit[0]) + 1 if hit.size else n1
    ok = bool(np.all(np.abs(cum - tf) > tol(k)))
    eps_s = 2 * tol(k) * (1 + float(np.abs(lp).max()))
    head = order[:min(n2 + 1, n1)]
    for a in range(head.size):
        for b in range(a + 1, head.size):
            if l[head[a]] != l[head[b]] and abs(s[head[a]] - s[head[b]]) <= eps_s:
                ok = False
    return ok, order, n2


def row_decided(name: str, r: int, fixture: dict) -> tuple[bool, bool]:
    """(tail-free decided, typical decided) for row r of a configuration, from the fixture alone.  Typical is judged on the reference's n_tfs; a row whose tail-free cut
    is undecided is undecided as a whole."""
    k, sigma, z, typ, rows, seed = CONFIGS[name]
    t_ok, n1 = tfs_decided(fixture[name + "/p"][r], z, k)
    y_ok, _, _ = typical_decided(fixture[name + "/logit"][r], int(fixture[name + "/n_tfs"][r]), typ, k)
    return t_ok, y_ok


def undecided_counts(name: str, fixture: dict) -> tuple[int, int, int]:
    """(rows, undecided by tail-free, undecided by typical)"""
    rows = CONFIGS[name][4]
    d = [row_decided(name, r, fixture) for r in range(rows)]
    return rows, sum(1 for t, y in d if not t), sum(1 for t, y in d if not y)


def expected_final_ids(sorted_ids, sorted_logit, final_logit) -> np.ndarray:
    """The ids of a final order given value for value: every value's ids are the sorted candidates' ids of that value, in ascending order (the earlier candidate first)."""
    sorted_ids, sorted_logit = np.asarray(sorted_ids, np.int64), np.asarray(sorted_logit, np.float32)
    taken, out = {}, []
    for v in np.asarray(final_logit, np.float32):
        cls = sorted_ids[sorted_logit == v]
        i = taken.get(float(v), 0)
        assert i < cls.size, f"value {v} stands in the final order more often than among the sorted candidates"
        out.append(int(cls[i]))
        taken[float(v)] = i + 1
    return np.array(out, np.int64)


def check_row(what: str, name: str, r: int, fixture: dict, x: np.ndarray, got: dict) -> dict:
    """One row's result `got` (generate._chain's keys: ids, logits, p, n_tfs, n_typ, order, p_top, final_ids, n, final_p, token) against the fixture.  x: the penalised
    fp32 row (sampling_rules.penalised).  Returns {"decided", "draws": [(u, accepted positions)] or [], "worst": the largest relative error seen}."""
    k, sigma, z, typ, rows, seed = CONFIGS[name]
    f = lambda key: fixture[f"{name}/{key}"][r]
    kk = int(np.asarray(got["ids"]).size)
    assert kk == k, f"{what}: {kk} candidates behind top-k"
    R.check_candidates(what, x, got["ids"], got["logits"], f("ids"), f("logit"))
    worst = R.check_p(what + " p", got["p"], f("p"), k)
    assert int(got["token"]) in set(np.asarray(got["ids"]).tolist()), f"{what}: the token is not among the top-k candidates"
    t_ok, y_ok = row_decided(name, r, fixture)
    if not (t_ok and y_ok):
        return {"decided": False, "draws": [], "worst": worst}
    n1, n2, n_ref = int(f("n_tfs")), int(f("n_typ")), int(f("n"))
    assert int(got["n_tfs"]) == n1, f"{what}: tail-free keeps {got['n_tfs']}, the reference {n1}"
    assert int(got["n_typ"]) == n2, f"{what}: typical keeps {got['n_typ']}, the reference {n2}"
    order = np.asarray(got["order"], np.int64)[:n2]
    final_ids = np.asarray(got["final_ids"], np.int64)[:n2]
    assert np.array_equal(final_ids, np.asarray(got["ids"], np.int64)[order]), f"{what}: final_ids is not ids[order]"
    final_logit = np.asarray(got["logits"], np.float32)[order]
    ref_final_logit = x[f("ids_typ")[:n2]]
    assert np.array_equal(final_logit.view(np.uint32), (ref_final_logit + np.float32(0.0)).view(np.uint32)), f"{what}: the order behind typical differs from the reference's"
    assert np.array_equal(final_ids, expected_final_ids(got["ids"], got["logits"], final_logit)), f"{what}: equal logits are not in ascending id order behind typical"
    worst = max(worst, R.check_p(what + " p_top", np.asarray(got["p_top"])[:n2], f("p_top")[:n2], k))
    lo, hi = R.n_band(f("p_top")[:n2], TOP_P, k)
    n = int(got["n"])
    assert lo <= n <= hi, f"{what}: n = {n} outside [{lo}, {hi}]"
    if lo == hi:  # top_p itself is decided: the band is one value, the reference's
        assert n == n_ref, f"{what}: n = {n}, the reference keeps {n_ref}"
    draws = []
    if n == n_ref:
        worst = max(worst, R.check_p(what + " final p", np.asarray(got["final_p"])[:n], f("final_p")[:n_ref], k))
        draws = R.draw_points(f("final_p")[:n_ref], k, seed * 1000 + r)
    return {"decided": True, "draws": draws, "worst": worst}
