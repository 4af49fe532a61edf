"""Designed logits for the tests of the tail-free and typical stages (a helper: no tests here, nothing pytest collects; numpy only, nothing of the package is imported).
The model is tests/sampler_cases.py, whose penalise / window_of are reused (they share nothing with the package either).

THE REFERENCE (reference()) is written one rule at a time, in float64 on the fp32 candidate values, and shares no code with generate._chain:
  1. the penalties (sampler_cases.penalise), then a stable Python sort of the allowed in-vocabulary ids by descending value: equal values keep ascending ids;
  2. softmax(m candidates in their CURRENT order): exp(l_i - l_first) / sum.  An argument below -104 gives exactly 0, as fp32 expf does in any mode (sampler_cases: gaps
     between candidate values avoid (87, 104));
  3. tail-free: the |second differences| of p, their sum S, the running sum of d2 / S, the first i >= 1 that exceeds tfs_z; S == 0 cuts nothing;
  4. typical: H = -sum p ln p, scores |-ln p - H|, the rank rule #{ j : s_j < s_i || (!(s_i < s_j) && j < i) } in two plain loops; a p of 0 makes every score NaN and
     the rule leaves the order as it is; the walk cuts behind the first running sum that exceeds typical_p;
  5. top-p, temperature, the inverse-CDF draw, as sampler_cases.reference.
It also returns the distances that make a case DECIDED: d_tfs (of tfs_z from the nearest cumulative weight of index >= 1) with S, d_typ (of typical_p from the nearest
cumulative sum), gap_s (the smallest score difference between candidates of different value among the first n2 + 1 positions) with eps_s' factor max |ln p|, d_top_p, d_u.

TWO KINDS OF CASE, as in sampler_cases.py.  exact: every fp32 operation of the chain is exact or one correctly rounded operation on equal inputs (equal logits with a
power-of-two count; one candidate >= 120 above the rest, p = {1, 0, ...}); thresholds may sit ON a cumulative sum; everything is asserted exactly.  toleranced:
generic values, built so that every cut and the order are decided (tests/test_sampler_stages_host.py asserts that for every such case); n_tfs, n_typ, the order, n,
choice and token are asserted exactly, p / p_top / final_p within sampling_rules.tol(k) of the float64 values.
"""
from __future__ import annotations

import dataclasses
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_rules as R  # noqa: E402
from sampler_cases import F16, F32, ONE_BELOW, RING, penalise, window_of  # noqa: E402

VOCAB = 8200  # three chunks of 4096, the last partial


@dataclasses.dataclass(frozen=True)
class P:
    """The sampling fields of a row (generate.SamplingParams' names)."""
    temp: float = 0.8
    top_k: int = 40
    top_p: float = 0.95
    repeat_penalty: float = 1.0
    alpha_frequency: float = 0.0
    alpha_presence: float = 0.0
    repeat_last_n: int = 64
    tfs_z: float = 1.0
    typical_p: float = 1.0


@dataclasses.dataclass
class Case:
    name: str
    kind: str            # exact | toleranced
    logits: np.ndarray   # fp16 [vocab]
    prm: P
    u: float = 0.5
    bound: int = 64      # the call's top_k_bound
    ring: np.ndarray = None
    pushed: int = 0
    allowed: tuple = None  # ids a mask leaves (ascending), None: every id
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


def _softmax(l: np.ndarray) -> np.ndarray:
    d = l - l[0]
    assert not np.any((d < -87.0) & (d > -104.0)), "a gap inside (87, 104): fp32 expf is subnormal there"
    e = np.where(d < -104.0, 0.0, np.exp(np.minimum(d, 700.0)))
    return e / e.sum()


def reference(c: Case) -> dict:
    inf = float("inf")
    prm = c.prm
    x = penalise(c.logits, c.window, prm)
    V = x.size
    pool = range(V) if c.allowed is None else [i for i in c.allowed if 0 <= i < V]
    vals = x.astype(np.float64).tolist()
    srt = sorted(pool, key=vals.__getitem__, reverse=True)  # stable: equal values keep ascending ids
    kk = min(max(int(prm.top_k), 1), c.bound, len(srt))
    ids = np.array(srt[:kk], np.int64)
    l32 = np.array([x[i] for i in ids], F32) + F32(0.0)
    l = l32.astype(np.float64)
    p = _softmax(l)
    out = {"ids": ids.astype(np.int32), "logits": l32, "p": p, "S": inf, "d_tfs": inf, "d_typ": inf, "gap_s": inf, "max_ln": 0.0}
    # tail-free
    z, n1 = float(F32(prm.tfs_z)), kk
    if z < 1.0 and kk > 2:
        d1 = [p[i] - p[i + 1] for i in range(kk - 1)]
        d2 = [abs(d1[i] - d1[i + 1]) for i in range(kk - 2)]
        S = sum(d2)
        out["S"] = S
        if S > 0.0:
            cum, cums = 0.0, []
            for i in range(kk - 2):
                cum += d2[i] / S
                cums.append(cum)
            for i in range(1, kk - 2):
                if cums[i] > z:
                    n1 = i
                    break
            if kk > 3:
                out["d_tfs"] = min(abs(v - z) for v in cums[1:])
    # typical
    typ, order, n2 = float(F32(prm.typical_p)), list(range(n1)), n1
    if typ < 1.0:
        p1 = _softmax(l[:n1])
        if np.any(p1 == 0.0):  # logf(0) = -inf, H = NaN, every score NaN: no comparison of the rank rule holds but j < i
            s = [float("nan")] * n1
        else:
            lp = np.log(p1)
            H = -float((p1 * lp).sum())
            s = [abs(-lp[i] - H) for i in range(n1)]
            out["max_ln"] = float(np.abs(lp).max())
        rank = [sum(1 for j in range(n1) if s[j] < s[i] or (not (s[i] < s[j]) and j < i)) for i in range(n1)]
        order = [0] * n1
        for i, rk in enumerate(rank):
            order[rk] = i
        cum, cums = 0.0, []
        for i in range(n1):
            cum += p1[order[i]]
            cums.append(cum)
        for i in range(n1):
            if cums[i] > typ:
                n2 = i + 1
                break
        out["d_typ"] = min(abs(v - typ) for v in cums)
        head = order[:min(n2 + 1, n1)]
        gaps = [abs(s[a] - s[b]) for ai, a in enumerate(head) for b in head[ai + 1:] if l[a] != l[b] and s[a] == s[a]]
        out["gap_s"] = min(gaps) if gaps else inf
    order = np.array(order[:n2], np.int64)
    lf, final_ids = l[order], ids[order]
    on = z < 1.0 or typ < 1.0
    p_top = _softmax(lf) if on else p
    # top-p
    tp, n, d_top_p = float(F32(prm.top_p)), n2, inf
    if tp < 1.0:
        cum = np.cumsum(p_top)
        for i in range(1, n2):
            if cum[i] > tp:
                n = i
                break
        if n2 > 1:
            d_top_p = float(np.abs(cum[1:] - tp).min())
    lt = lf[:n] / float(F32(prm.temp))
    fp = _softmax(lt)
    cdf = np.cumsum(fp)
    uu = float(F32(c.u))
    choice = n - 1
    for i in range(n):
        if uu < cdf[i]:
            choice = i
            break
    out.update({"n_tfs": n1, "n_typ": n2, "order": order.astype(np.int32), "final_ids": final_ids.astype(np.int32), "p_top": p_top, "n": n, "final_p": fp, "choice": choice,
                "token": int(final_ids[choice]), "d_top_p": d_top_p, "d_u": float(np.abs(cdf[:n - 1] - uu).min()) if n > 1 else inf})
    return out


def decided(c: Case, ref: dict) -> dict:
    """The margins of a toleranced case against the rules of tests/stage_rules.py, from the case's own float64 reference: every value must be True."""
    k = int(ref["ids"].size)
    t = R.tol(k)
    return {"tfs": ref["d_tfs"] > 16 * 2.0 ** -23 / ref["S"] + t if ref["S"] not in (0.0, float("inf")) else True,
            "typ": ref["d_typ"] > t, "score": ref["gap_s"] > 2 * t * (1 + ref["max_ln"]), "top_p": ref["d_top_p"] > t, "u": ref["d_u"] > t}


# ---- the cases ----
def _row(values: dict, floor: float = -20.0, vocab: int = VOCAB) -> np.ndarray:
    """fp16 [vocab]: `floor` descending slowly with the id (no ties below the placed values, every value far below them), then the placed {id: value}."""
    x = np.full(vocab, floor, np.float32) - (np.arange(vocab, dtype=np.float32) % 1024) * np.float32(2.0 ** -5) - (np.arange(vocab) // 1024).astype(np.float32) * 40
    x = np.maximum(x, -60000.0)
    for i, v in values.items():
        x[i] = v
    return x.astype(F16)


EDGE_IDS = [0, 15, 16, 1023, 1024, 4095, 4096, 8191, 8192, VOCAB - 1]  # thread (16), wave (1024) and chunk (4096) edges, the first and the last id
GENERIC = [3.0, 2.5, 1.75, 0.5, 0.0, -1.0, -1.5, -2.25, -3.0, -4.0]    # p ~ .48 .29 .14 .04 .02 ...: every cut far from a threshold


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    out = []
    add = lambda *a, **kw: out.append(Case(*a, **kw))
    eq8 = {i: 2.0 for i in [5, 16, 1024, 4095, 4096, 6000, 8191, VOCAB - 1]}
    # exact: equal logits, k a power of two -- tail-free has S = 0 and cuts nothing; typical has equal scores and cuts at the first (i + 1) / k > typical_p, ON a sum
    add("equal8_both", "exact", _row(eq8), P(top_k=8, tfs_z=0.5, typical_p=0.5), expect={"n_tfs": 8, "n_typ": 5, "order": [0, 1, 2, 3, 4], "n": 4})
    add("equal16_typical_on_a_sum", "exact", _row({i * 500 + 3: 1.0 for i in range(16)}), P(top_k=16, typical_p=0.25), expect={"n_tfs": 16, "n_typ": 5})
    add("equal8_one_below", "exact", _row(eq8), P(top_k=8, tfs_z=ONE_BELOW, typical_p=ONE_BELOW), expect={"n_tfs": 8, "n_typ": 8})
    add("equal8_exactly_one", "exact", _row(eq8), P(top_k=8, tfs_z=1.0, typical_p=1.0), expect={"n_tfs": 8, "n_typ": 8, "n": 7})
    # exact: one candidate >= 120 above the rest, p = {1, 0, ...}
    peak = {7: 60.0, **{i: -60.0 for i in [8, 1030, 4100, 5000, 6000, 7000, 8000]}}
    add("peak_tail_free", "exact", _row(peak, floor=-200.0), P(top_k=8, tfs_z=0.5), expect={"n_tfs": 1, "n_typ": 1, "token": 7})
    add("peak_typical_nan_path", "exact", _row(peak, floor=-200.0), P(top_k=8, typical_p=0.5), expect={"n_tfs": 8, "n_typ": 1, "order": [0], "token": 7})
    add("peak_both_one_below", "exact", _row(peak, floor=-200.0), P(top_k=8, tfs_z=ONE_BELOW, typical_p=ONE_BELOW), expect={"n_tfs": 1, "n_typ": 1, "token": 7})
    # exact: the kk > 2 guard
    add("kk1", "exact", _row(peak, floor=-200.0), P(top_k=1, tfs_z=0.0, typical_p=0.0), expect={"n_tfs": 1, "n_typ": 1, "token": 7})
    add("kk2_tail_free_does_not_run", "exact", _row({9: 1.0, 4097: 1.0}), P(top_k=2, tfs_z=0.0, top_p=1.0), u=0.75, expect={"n_tfs": 2, "n_typ": 2, "n": 2, "token": 4097})
    add("kk3_one_weight_cannot_cut", "exact", _row(peak, floor=-200.0), P(top_k=3, tfs_z=0.3), expect={"n_tfs": 3, "n_typ": 3, "token": 7})
    # exact: fewer allowed tokens than k under a mask
    add("mask_leaves_four", "exact", _row({i: 2.0 for i in [40, 41, 5000, 8199]}), P(top_k=40, tfs_z=0.5, typical_p=0.5), allowed=(40, 41, 5000, 8199),
        expect={"n_tfs": 4, "n_typ": 3, "order": [0, 1, 2]})
    # exact: tail-free cuts at the LAST possible index -- equal candidates, then one drop: the only nonzero second difference is the last, its weight exactly 1
    add("tail_free_last_index", "toleranced", _row({**{i: 2.0 for i in [3, 17, 1025, 4097, 8193]}, 6000: 1.0}), P(top_k=6, tfs_z=0.5, top_p=1.0), expect={"n_tfs": 3, "n_typ": 3, "n": 3})
    # toleranced
    gen = dict(zip(EDGE_IDS, GENERIC))
    add("tail_free_first_index", "toleranced", _row({0: 8.0, 15: 2.0, 16: 1.5, 1023: 1.0, 1024: 0.5, 4095: 0.0}), P(top_k=6, tfs_z=0.5), expect={"n_tfs": 1})
    add("z_zero_keeps_one", "toleranced", _row(gen), P(top_k=10, tfs_z=0.0), expect={"n_tfs": 1})
    add("z_negative_keeps_one", "toleranced", _row(gen), P(top_k=10, tfs_z=-1.0), expect={"n_tfs": 1})
    add("typical_zero_keeps_the_nearest_to_H", "toleranced", _row(gen), P(top_k=10, typical_p=0.0), expect={"n_typ": 1})
    add("typical_negative_keeps_one", "toleranced", _row(gen), P(top_k=10, typical_p=-0.5), expect={"n_typ": 1})
    # a typical order that puts a non-maximal candidate first: top-p's softmax sees a positive argument, the draw follows the permuted order
    nm = {4095: 3.0, 4096: 2.5, 8192: 0.0, 1024: -1.0, 16: -2.0, 0: -3.0}
    add("typical_non_maximal_first", "toleranced", _row(nm), P(top_k=6, typical_p=0.5, top_p=1.0), u=0.9, expect={"n_typ": 2, "order": [1, 0], "final_ids": [4096, 4095], "token": 4095})
    # two candidates on opposite sides of H, scores apart by a designed margin (|.545 - H| vs |1.05 - H| at H ~ .87: .32 against .18)
    add("typical_opposite_sides_of_H", "toleranced", _row(nm), P(top_k=6, typical_p=0.3, top_p=1.0), u=0.1, expect={"n_typ": 1, "order": [1], "token": 4096})
    # winners at chunk, wave and thread edges: the permuted ids are looked up across chunks
    add("edges_both_stages", "toleranced", _row(gen), P(top_k=10, tfs_z=0.9, typical_p=0.8), u=0.6)
    add("edges_typical_only_all_kept", "toleranced", _row(gen), P(top_k=10, typical_p=0.97, top_p=1.0), u=0.97)
    # ids near 2^20 - 1
    big = 1 << 20
    add("ids_near_2_20", "toleranced", _row(dict(zip([big - 1, big - 2, big - 4097, 0, big - 4096, 12345], GENERIC)), vocab=big), P(top_k=6, tfs_z=0.95, typical_p=0.7), u=0.8,
        bound=8)
    # both stages, then a top-p that cuts again
    add("top_p_cuts_again", "toleranced", _row(gen), P(top_k=10, tfs_z=0.97, typical_p=0.9, top_p=0.6), u=0.3)
    # penalties move a candidate across a stage's cut: id 15 (2.5) is in the window; penalised it falls to 1.25 and another candidate stands in the typical set
    ring = np.zeros(RING, np.int32)
    ring[:3] = [15, 15, 77]
    add("penalty_moves_across_the_cut", "toleranced", _row(gen), P(top_k=10, typical_p=0.5, repeat_penalty=2.0), ring=ring, pushed=3, u=0.4)
    add("penalty_off_twin", "toleranced", _row(gen), P(top_k=10, typical_p=0.5, repeat_penalty=1.0), ring=ring, pushed=3, u=0.4)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def by_name(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def _ref_of(name: str) -> dict:
    return reference(by_name(name))


def ref_of(c: Case) -> dict:
    """The case's reference, computed once and shared (treat it as read-only)."""
    return _ref_of(c.name)
