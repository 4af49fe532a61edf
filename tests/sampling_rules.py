"""How a sampler's results are compared with the reference's own (tests/golden/sampling_golden.npz, recorded from llm/src/Generate.cc): the rules shared by
tests/test_sampling_host.py (the numpy restatement) and tests/test_gpu_sampling.py (tce_sample_f16).  Not a test module.

The reference's tie order is unspecified (std::partial_sort is not stable; fp16 logits tie constantly) and two expf implementations differ in their last bits:

* greedy id: equal.  Sorted penalised logit VALUES: bit-equal.  Ids: equal wherever the value is unique in the row; inside a tie class the ids are that class's
  lowest ids in ascending order (the ordering rule: descending logit, ascending id among equals).
* p and final p: relative error <= tol(k) = (k + 8) * 2^-23 -- one ulp per expf (the bound HIP's math documentation gives for expf; no copy of that documentation is
  installed beside the compiler, so the published bound is used), k sequential additions, one division.
* n: with cum the fp32 running sum of the REFERENCE's p, cut(top_p - tol) <= n <= cut(top_p + tol), cut(t) = the first i >= 1 with cum_i > t (k if none).  The
  band is a single value in at least 95 % of the rows of every configuration (asserted by tests/test_sampling_host.py from the fixture alone).
* the draw: u at the midpoint of every CDF interval of the reference's final p and 64 seeded random u; position i is accepted if cdf_{i-1} - tol <= u < cdf_i + tol
  (the last position also for any u at or above its lower edge).  For a u farther than tol from both edges of its interval the rule leaves exactly one position:
  the midpoints are then exact checks (an interval narrower than 2 tol has no such point; nearer than tol to an edge two correct samplers may differ).
"""
from __future__ import annotations

import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_sampling_golden", os.path.join(HERE, "golden", "make_sampling_golden.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)

CONFIGS = maker.CONFIGS
VOCAB = maker.VOCAB


def load_fixture() -> dict:
    return dict(np.load(maker.OUT))


def config_inputs(name: str, fixture: dict) -> list:
    """[(logits fp16, recent int32)] of a configuration, regenerated from its seed and checked against the digest recorded with the reference's results."""
    rows = list(maker.config_rows(name))
    import hashlib
    h = hashlib.sha256()
    for logits, recent in rows:
        h.update(logits.tobytes())
        h.update(recent.tobytes())
    assert h.hexdigest() == str(fixture[name + "/digest"]), f"{name}: the regenerated inputs are not the ones the fixture was recorded for (re-record it)"
    return rows


def tol(k: int) -> float:
    return (k + 8) * 2.0 ** -23


def penalised(logits: np.ndarray, recent: np.ndarray, rp: float, af: float, ap: float) -> np.ndarray:
    """The penalised fp32 row, written out id by id (Generate.cc:14-60) -- independent of the package's vectorised restatement."""
    x = logits.astype(np.float32)
    counts = {}
    for t in recent.tolist():
        counts[t] = counts.get(t, 0) + 1
    for t, c in counts.items():
        v = x[t]
        if np.float32(rp) != np.float32(1.0):
            v = np.float32(v * np.float32(rp)) if v <= 0 else np.float32(v / np.float32(rp))
        if not (af == 0.0 and ap == 0.0):
            v = np.float32(v - np.float32(np.float32(c) * np.float32(af) + np.float32(1.0) * np.float32(ap)))
        x[t] = v
    return x


def check_candidates(what: str, x: np.ndarray, got_ids, got_logit, ref_ids, ref_logit) -> None:
    got_ids, ref_ids = np.asarray(got_ids, np.int64), np.asarray(ref_ids, np.int64)
    got_logit, ref_logit = np.asarray(got_logit, np.float32), np.asarray(ref_logit, np.float32)
    assert got_logit.shape == ref_logit.shape, f"{what}: {got_logit.size} candidates, the reference has {ref_logit.size}"
    assert np.array_equal(got_logit.view(np.uint32), ref_logit.view(np.uint32)), f"{what}: sorted penalised logits differ from the reference's"
    near = np.nonzero(x >= ref_logit.min())[0]  # (ascending ids) every member of every tie class of the list
    xn = x[near]
    for v in np.unique(got_logit):
        where = np.nonzero(got_logit == v)[0]
        cls = near[xn == v]
        assert np.array_equal(got_ids[where], cls[:where.size]), f"{what}: value {v}: ids {got_ids[where].tolist()}, the tie class's lowest are {cls[:where.size].tolist()}"
        if cls.size == 1:
            assert ref_ids[where[0]] == got_ids[where[0]], f"{what}: id of the unique value {v} differs from the reference's"


def check_p(what: str, got, ref, k: int) -> float:
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, f"{what}: {got.size} values, the reference has {ref.size}"
    rel = np.abs(got - ref) / ref
    worst = float(rel.max()) if rel.size else 0.0
    assert worst <= tol(k), f"{what}: relative error {worst:.3e} > {tol(k):.3e}"
    return worst


def cut(cum: np.ndarray, t: float) -> int:
    hit = np.nonzero(cum[1:].astype(np.float64) > t)[0]
    return int(hit[0]) + 1 if hit.size else int(cum.size)


def n_band(ref_p: np.ndarray, top_p: float, k: int) -> tuple[int, int]:
    if np.float32(top_p) >= np.float32(1.0):
        return int(ref_p.size), int(ref_p.size)
    cum = np.cumsum(np.asarray(ref_p, np.float32), dtype=np.float32)
    t = float(np.float32(top_p))
    return cut(cum, t - tol(k)), cut(cum, t + tol(k))


def draw_points(ref_final_p: np.ndarray, k: int, seed: int) -> list:
    """[(u, positions accepted)]: the midpoint of every CDF interval of the reference's final p, then 64 seeded random u."""
    fp = np.asarray(ref_final_p, np.float32)
    n, t = fp.size, tol(k)
    cdf = np.cumsum(fp, dtype=np.float32).astype(np.float64)
    lo = np.concatenate([[0.0], cdf[:-1]])
    rng = np.random.default_rng(seed)
    us = [np.float32((lo[i] + cdf[i]) / 2) for i in range(n)] + [np.float32(v) for v in rng.random(64, dtype=np.float32)]
    out = []
    for j, u in enumerate(us):
        uf = float(u)
        ok = {i for i in range(n) if lo[i] - t <= uf and (uf < cdf[i] + t or i == n - 1)}
        if j < n and lo[j] + t <= uf < cdf[j] - t:
            assert ok == {j}  # a midpoint farther than tol from its interval's edges: the rule leaves exactly its own position
        out.append((u, ok))
    return out
