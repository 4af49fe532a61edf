"""The designed sampler cases (tests/sampler_cases.py) on the host: every case is what it claims, the numpy restatement generate.sample_reference and the reference's
own code (tests/golden/sampler_designed_golden.npz, recorded by tests/golden/make_sampler_designed_golden.py) agree with the new reference, and five mutants of a
copy of the new reference are each caught by a named case.  Nothing here needs a GPU or the reference tree."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_cases as S  # noqa: E402
import sampling_rules as R  # noqa: E402

F32 = np.float32
CASES = S.cases()
DEFINED = [c for c in CASES if S.defined(c)]
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_designed_golden.npz")


def _bits(a) -> np.ndarray:
    return np.asarray(a, F32).view(np.uint32)


def chain32(l32: np.ndarray, prm, u) -> dict:
    """The chain behind the ordering with every operation ONE fp32 operation in the order sampling.hip and Generate.cc perform them (sequential sums)."""
    def softmax(v):
        e = np.exp((v - v[0]).astype(F32)).astype(F32)
        s = F32(0.0)
        for t in e:
            s = F32(s + t)
        return (e / s).astype(F32)
    with np.errstate(all="ignore"):
        p = softmax(l32)
        n = l32.size
        if F32(prm.top_p) < F32(1.0):
            cum = F32(0.0)
            for i in range(l32.size):
                cum = F32(cum + p[i])
                if cum > F32(prm.top_p) and i >= 1:
                    n = i
                    break
        fp = softmax((l32[:n] / F32(prm.temp)).astype(F32))
    choice, cdf = n - 1, F32(0.0)
    for i in range(n):
        cdf = F32(cdf + fp[i])
        if F32(u) < cdf:
            choice = i
            break
    return {"p": p, "n": n, "final_p": fp, "choice": choice}


@pytest.mark.parametrize("c", DEFINED, ids=lambda c: c.name)
def test_every_case_is_what_it_claims(c):
    ref = S.ref_of(c)
    k = c.k
    assert ref["ids"].size == k and (ref["ids"] < c.vocab).all() and len(set(ref["ids"].tolist())) == k
    for key, want in c.expect.items():
        got = ref["ids"][:len(want)].tolist() if key in ("ids", "ids_head") else ref[key]
        assert got == want, f"{c.name}: the design says {key} = {want}, the reference gives {got}"
    pad = S.padded(c)
    assert pad.size % 8 == 0 and pad.size >= c.vocab + 8 and (pad[c.vocab:] == np.float16(60000.0)).all() and np.array_equal(pad[:c.vocab].view(np.uint16), c.logits.view(np.uint16))
    if c.kind == "greedy":
        return
    if c.kind == "exact":
        # the fp32 chain and the float64 chain give the same bits and the same decisions: no rounding anywhere an implementation could take differently
        got = chain32(ref["logits"], c.prm, c.u)
        assert np.array_equal(_bits(got["p"]), _bits(ref["p"])) and np.array_equal(_bits(got["final_p"]), _bits(ref["final_p"])), f"{c.name}: fp32 and float64 differ"
        assert (got["n"], got["choice"]) == (ref["n"], ref["choice"]), f"{c.name}: fp32 decides (n, choice) = {(got['n'], got['choice'])}, float64 {(ref['n'], ref['choice'])}"
        e1 = np.unique(ref["logits"][np.isfinite(ref["logits"])].astype(np.float64) - float(ref["logits"][0]))
        assert all(d == 0.0 or d <= -120.0 for d in e1), f"{c.name}: a gap that expf has to round"
        return
    # toleranced: the band of n is one value and the draw rule leaves one position
    t, tf = S.tol_p(c), S.tol_final(c, ref)
    lo, hi = R.n_band(ref["p"].astype(F32), c.prm.top_p, k)
    assert lo == hi == ref["n"], f"{c.name}: n may be {lo} .. {hi}: top_p is not decisive"
    ok = S.accepted(ref["final_p"].astype(F32), tf, c.u)
    assert ok == {ref["choice"]}, f"{c.name}: u = {c.u!r} may draw {sorted(ok)}: not decisive"
    assert ref["d_top_p"] > t, f"{c.name}: top_p lies {ref['d_top_p']:.2e} from a cumulative sum (tolerance {t:.2e})"
    if ref["choice"] < ref["n"] - 1 or ref["n"] == 1 or F32(c.u) < F32(1.0) - F32(1e-3):
        assert ref["d_u"] > tf, f"{c.name}: u lies {ref['d_u']:.2e} from a cumulative sum (tolerance {tf:.2e})"
    if c.temp_extreme:
        assert tf > 2 * t or c.prm.temp > 1, f"{c.name}: the derived bound is not what sets the tolerance"
    else:
        l = ref["logits"][:ref["n"]].astype(np.float64)
        assert np.abs(l[np.isfinite(l)]).max() <= 8.0 and c.prm.temp >= 0.5, f"{c.name}: an ordinary case outside the magnitudes tol(k) is stated for"


def test_winners_and_window_ids_land_where_stated():
    by = S.by_name
    for V in (40, 4095, 4096, 4097, 8191, 4099):
        c, W = by(f"vocab{V}"), S.boundary_ids(V)
        assert {0, V - 1} <= set(W) and sorted(S.ref_of(c)["ids"][:len(W)].tolist()) == W, f"vocab{V}: the winners are not the boundary ids"
        for b in (16, 1024, 4096):
            if b < V:
                assert {b - 1, b} <= set(W)
    ids = S.ref_of(by("vocab_2p20"))["ids"].tolist()
    assert any(i >> 17 & 1 for i in ids) and any(i >> 18 & 1 for i in ids) and any(i >> 19 & 1 for i in ids) and ids[3:5] == [7, (1 << 20) - 1]
    for tag, chunks in (("one_chunk", {5}), ("eight_per_chunk", set(range(32))), ("last_chunk", {31})):
        got = S.ref_of(by("vocab128256_" + tag))["ids"]
        assert got.size == 256 and set((got // 4096).tolist()) == chunks and (tag != "eight_per_chunk" or (np.bincount(got // 4096) == 8).all())
    w = by("pen_boundaries").window.tolist()
    assert set(S.boundary_ids(8197)) <= set(w) and w.count(0) == 3 and w.count(15) == 1
    w = by("pen_out_of_range").window.tolist()
    assert {8197, 8200, 8212, 1 << 20, 2 ** 31 - 1, -1, S.INT_MIN, -8197, -16} <= set(w) and sum(0 <= t < 8197 for t in set(w)) == 2  # id 16 and the filler
    assert by("pen_count64").window.tolist() == [1024] * 64
    c = by("pen_wrapped_17")
    assert c.pushed == 150 and c.window.size == 17 and set(c.window.tolist()) == {15, 4096, 8196, 2} and {16, 1024, 4095, 8192} <= set(c.ring.tolist())
    x = S.penalise(by("pen_zero_branch").logits, by("pen_zero_branch").window, by("pen_zero_branch").prm)
    assert x[16] == 0 and not np.signbit(x[16]) and np.signbit(x[1023]) and x[1023] == 0 and x[4096] == F32(F32(-2.0 ** -24) * F32(1.3)) and x[8191] == F32(F32(2.0 ** -24) / F32(1.3))
    c = by("pen_max_out_of_k")
    assert int(np.argmax(c.logits.astype(F32))) == 10 and 10 not in S.ref_of(c)["ids"]
    c = by("pen_negative_alpha")
    assert 6000 not in np.argsort(-c.logits.astype(F32), kind="stable")[:4] and S.ref_of(c)["ids"][0] == 6000
    assert by("top_k_clamped").prm.top_k == 100 and by("top_k_clamped").k == 40
    families = {c.family for c in CASES}
    assert families == {"geometry", "ties", "penalties", "parameters", "nonfinite"}


def _params(c, k=None):
    from tinychatengine_amd.generate import SamplingParams
    d = dataclasses.asdict(c.prm)
    d["top_k"] = c.k if k is None else k  # (the call's bound clamps a row's top_k; sample_reference knows no bound)
    return SamplingParams(**d)


def _same_decisions(what, got, ref, c):
    assert got["ids"].tolist() == ref["ids"].tolist(), f"{what}: candidate ids {got['ids'].tolist()[:12]}, the reference {ref['ids'].tolist()[:12]}"
    assert np.array_equal(_bits(got["logits"]), _bits(ref["logits"])), f"{what}: candidate logits"
    assert (got["n"], got["choice"], got["token"]) == (ref["n"], ref["choice"], ref["token"]), \
        f"{what}: (n, choice, token) = {(got['n'], got['choice'], got['token'])}, the reference {(ref['n'], ref['choice'], ref['token'])}"


@pytest.mark.parametrize("c", DEFINED, ids=lambda c: c.name)
def test_sample_reference_agrees(c):
    from tinychatengine_amd.generate import sample_reference
    ref = S.ref_of(c)
    got = sample_reference(c.logits, c.window, _params(c), c.u)
    _same_decisions(c.name, got, ref, c)
    if c.kind == "exact":
        assert np.array_equal(_bits(got["p"]), _bits(ref["p"])) and np.array_equal(_bits(got["final_p"]), _bits(ref["final_p"])), f"{c.name}: p / final p bits"
    elif c.kind == "toleranced":
        assert S.rel_err(got["p"], ref["p"]) <= S.tol_p(c) and S.rel_err(got["final_p"], ref["final_p"]) <= S.tol_final(c, ref), f"{c.name}: p / final p"


def test_the_references_own_code_agrees():
    """The recorded results of llm/src/Generate.cc on the finite cases of vocab <= 8200, under sampling_rules: tie classes by the ordering rule, p and final p by
    tolerance, n exactly (every case is decisive or exact).  The reference keeps -0 where the device returns +0: both sides are compared as +0."""
    fx = dict(np.load(FIXTURE))
    cs = [c for c in CASES if S.recordable(c)]
    assert [c.name for c in cs] == fx["names"].tolist() and S.digest(cs) == str(fx["digest"]), "the case table is not the one the fixture was recorded for (re-record it)"
    assert os.path.getsize(FIXTURE) < os.path.getsize(R.maker.OUT)
    assert len(cs) >= 35
    for c in cs:
        g = S.reference(c.logits, c.window, dataclasses.replace(c.prm, temp=0.0), 0.0, c.bound)
        assert int(fx[c.name + "/greedy"]) == g["token"], f"{c.name}: the reference's greedy id {fx[c.name + '/greedy']}, the new reference {g['token']}"
        if c.prm.temp <= 0:
            continue
        ref = S.ref_of(c)
        x = S.penalise(c.logits, c.window, c.prm)
        R.check_candidates(c.name, x, ref["ids"], ref["logits"], fx[c.name + "/ids"], fx[c.name + "/logit"] + F32(0.0))
        assert S.rel_err(fx[c.name + "/p"], ref["p"]) <= S.tol_p(c), f"{c.name}: p"
        lo, hi = R.n_band(fx[c.name + "/p"], c.prm.top_p, c.k)
        assert lo <= ref["n"] <= hi and int(fx[c.name + "/n"]) == ref["n"], f"{c.name}: the reference keeps {fx[c.name + '/n']}, the new reference {ref['n']} (band {lo} .. {hi})"
        assert S.rel_err(fx[c.name + "/final_p"][:ref["n"]], ref["final_p"]) <= S.tol_final(c, ref), f"{c.name}: final p"
        assert (fx[c.name + "/final_p"][ref["n"]:] == 0).all()
        if c.kind == "exact":
            assert np.array_equal(_bits(fx[c.name + "/p"]), _bits(ref["p"])) and np.array_equal(_bits(fx[c.name + "/final_p"][:ref["n"]]), _bits(ref["final_p"])), f"{c.name}: bits"


# ---- mutants of a copy of the new reference ----
def mutant_reference(logits_f16, window_ids, params, u, top_k_bound, mutant):
    """sampler_cases.reference, copied, with one rule broken:
       cut_ge        `>=` in the top-p cut                       draw_le     `<=` in the draw
       ties_high     ties to the highest id                      per_occurrence  the penalties applied once per occurrence in the window
       no_le_branch  the `v <= 0` branch of the repetition penalty missing: every value is divided.  (`v < 0` in place of `v <= 0` alone is an EQUIVALENT mutant:
                     it differs only at v = +-0, where 0 * penalty and 0 / penalty are the same zero.)"""
    x = logits_f16.astype(F32)
    V = x.size
    rp, af, ap = F32(params.repeat_penalty), F32(params.alpha_frequency), F32(params.alpha_presence)
    counts: dict = {}
    for t in np.asarray(window_ids, np.int64).tolist():
        if 0 <= t < V:
            counts[t] = counts.get(t, 0) + 1
    for t, c in counts.items():
        v = F32(x[t])
        for _ in range(c if mutant == "per_occurrence" else 1):
            cc = 1 if mutant == "per_occurrence" else c
            if rp != F32(1.0):
                v = F32(v * rp) if (v <= F32(0.0) and mutant != "no_le_branch") else F32(v / rp)
            if not (af == F32(0.0) and ap == F32(0.0)):
                v = F32(v - F32(F32(F32(cc) * af) + F32(F32(1.0) * ap)))
        x[t] = v
    vals = x.astype(np.float64).tolist()
    if mutant == "ties_high":
        order = sorted(range(V - 1, -1, -1), key=vals.__getitem__, reverse=True)
    else:
        order = sorted(range(V), key=vals.__getitem__, reverse=True)
    if params.temp <= 0:
        tok = order[0]
        return {"ids": np.array([tok], np.int32), "logits": np.array([x[tok]], F32) + F32(0.0), "n": 1, "choice": 0, "token": tok}
    k = min(max(int(params.top_k), 1), int(top_k_bound), V)
    ids = order[:k]
    l32 = np.array([x[i] for i in ids], F32) + F32(0.0)
    l = l32.astype(np.float64)
    e = np.exp(l - l[0])
    p = e / e.sum()
    cum = np.cumsum(p)
    tp = float(F32(params.top_p))
    n = k
    if tp < 1.0:
        for i in range(1, k):
            if (cum[i] >= tp) if mutant == "cut_ge" else (cum[i] > tp):
                n = i
                break
    lt = l[:n] / float(F32(params.temp))
    e2 = np.exp(lt - lt[0])
    fp = e2 / e2.sum()
    cdf = np.cumsum(fp)
    uu = float(F32(u))
    choice = n - 1
    for i in range(n):
        if (uu <= cdf[i]) if mutant == "draw_le" else (uu < cdf[i]):
            choice = i
            break
    return {"ids": np.array(ids, np.int32), "logits": l32, "n": n, "choice": choice, "token": int(ids[choice])}


def _caught_by(mutant) -> list:
    out = []
    for c in DEFINED:
        if c.vocab > 8200:
            continue
        got, ref = mutant_reference(c.logits, c.window, c.prm, c.u, c.bound, mutant), S.ref_of(c)
        if got["ids"].tolist() != ref["ids"].tolist() or not np.array_equal(_bits(got["logits"]), _bits(ref["logits"])) or \
                (got["n"], got["choice"], got["token"]) != (ref["n"], ref["choice"], ref["token"]):
            out.append(c.name)
    return out


def test_the_copy_without_a_mutation_is_the_reference():
    assert _caught_by(None) == []


@pytest.mark.parametrize("mutant,named", [("cut_ge", "eight_equal_half"), ("draw_le", "eight_equal_half"), ("ties_high", "two_valued_3k"), ("per_occurrence", "pen_count64"),
                                          ("no_le_branch", "pen_zero_branch")])
def test_each_mutant_fails_a_named_case(mutant, named):
    caught = _caught_by(mutant)
    assert named in caught, f"the mutant `{mutant}` passes the case `{named}` that was designed against it (it fails {caught or 'no case at all'})"
    print(f"{mutant}: caught by {caught}")
