"""Generation: the piece between lm_head's output and the next step's input, on the device, and a front that admits prompts and returns token ids.

The batched / paged decoders (batch_decode.py, paged_kv.py) run a "step" = the layers, fed a hidden row per sequence.  Here a TOKEN step is

    1        tce_embed_rows_f16      row next_token[b] of the fp16 embedding table -> hidden[b]            (active rows)
    7 x L    the layers              BatchedDecoder.step / PagedBatchedDecoder.step, unchanged
    1        tce_rmsnorm_half        the final norm, B rows
    1        tce_w4a16_forward       lm_head at M = B -> logits fp16 [B][vocab]
    2        tce_sample_f16          penalties, top-k, softmax, top-p, temperature, draw; token -> next_token, log, ring; pos += 1 or -1 (retired)
                                     (stages=True: tce_sample_stages_f16, the same two launches with tail-free and typical sampling per slot between top-k and top-p)
                                     (mirostat_rows=True: tce_sample_mirostat_f16, the same two launches with mirostat v1 / v2 per slot, mu kept on the device)
                                     (logprobs=True: tce_sample_logprobs_f16, the same two launches, which also write the token's log-probability)
                                     (constraints=True: tce_sample_constrained_f16, the same two launches under a token automaton and a logit bias per slot:
                                     constrain.py)

7 L + 5 launches, captured once in one torch.cuda.graph: ONE REPLAY IS ONE TOKEN for all B sequences, with no host round trip.  Everything a replay needs lives
on the device (positions, sampling parameters, recent-token rings, generator counters, output logs), so a slot changes hands without recapture.

    sample_reference      the sampling chain restated in numpy (fp32 throughout, sequential sums, the ordering rule): the CPU-side yardstick of tce_sample_f16
    philox4x32_10, uniform   the counter-based generator restated in numpy; the device matches it bit for bit
    logprob_reference     logprob = x_t - LSE(x) on the raw fp16 logits, in float64: the yardstick of the device's log-probabilities
    Sampler               the per-row device state + workspace; step(logits, pos_device, pos_bound)
    score_plan            score()'s host bookkeeping: slots, reservations, packed tokens and targets, row chunks.  No device, no launch.
    SlotBook              host bookkeeping of live slots (positions, budgets): which pages run(n) must reserve.  No device, no launch.
    BatchedGenerator      admit / run / tokens / logprobs / release over a list of PagedBatchedDecoder (one PageAllocator) or BatchedDecoder; score(prompts): the
                          log-probability of every prompt token given the tokens before it (perplexity), with no logits leaving the device
    HostDrivenLoop        the same decoders driven from the host -- logits copied back, numpy argmax, the row looked up and copied over: what a caller had to do
                          before this module, kept as the yardstick for tests and scripts/generate_time.py

Reference: llm/src/Generate.cc (sample_*), llm/src/nn_modules/non_cuda/LLaMA3Generate.cc:127-198 (the order of the chain, min_keep 1, last_n_tokens).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import capi

RING = capi.TCE_SAMPLE_RING
MAX_K = capi.TCE_SAMPLE_MAX_K


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the generator: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), counter (index, 0, 0, 0), key (seed_lo, seed_hi)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10(counter, key) -> tuple[int, int, int, int]:
    """counter: four 32-bit words, key: two -> four 32-bit words (ten rounds, the key bumped by the Weyl constants between rounds)."""
    c0, c1, c2, c3 = (int(v) & _MASK for v in counter)
    k0, k1 = (int(v) & _MASK for v in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _MASK, p1 & _MASK, ((p0 >> 32) ^ c3 ^ k1) & _MASK, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def uniform(seed: int, index: int) -> np.float32:
    """The uniform in [0, 1) that draws token `index` of the sequence seeded `seed` (64 bits): the top 24 bits of the first output word.  It depends on nothing
    else -- not the slot, the batch or the number of launches."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10((index, 0, 0, 0), (seed & _MASK, seed >> 32))[0]
    return np.float32(w >> 8) * np.float32(2.0 ** -24)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the sampling chain in numpy
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class SamplingParams:
    """opt_params' sampling fields with the reference's defaults (llm/include/Generate.h:60-69).  temp <= 0: greedy."""
    temp: float = 0.8
    top_k: int = 40
    top_p: float = 0.95
    repeat_penalty: float = 1.1
    alpha_frequency: float = 0.0
    alpha_presence: float = 0.0
    repeat_last_n: int = 64
    tfs_z: float = 1.0
    typical_p: float = 1.0
    mirostat: int = 0
    mirostat_tau: float = 5.0
    mirostat_eta: float = 0.1

    def check(self, top_k_bound: int = MAX_K, stages: bool = False, mirostat_rows: bool = False) -> None:
        """stages=False: what tce_sample_f16 can run (tfs_z 1.0, typical_p 1.0).  stages=True: what tce_sample_stages_f16 can run -- any tfs_z / typical_p but NaN.
        mirostat_rows=True (implies stages=True, as in Sampler): what tce_sample_mirostat_f16 can run -- also mirostat 1 or 2 with finite tau and eta, eta >= 0."""
        stages = stages or mirostat_rows
        if mirostat_rows:
            if self.mirostat not in (0, 1, 2):
                raise ValueError(f"mirostat {self.mirostat}: 0, 1 or 2")
            if not (np.isfinite(self.mirostat_tau) and np.isfinite(self.mirostat_eta)) or self.mirostat_eta < 0:
                raise ValueError(f"mirostat_tau {self.mirostat_tau} / mirostat_eta {self.mirostat_eta}: finite, eta >= 0")
        if stages:
            if self.mirostat != 0 and not mirostat_rows:
                raise ValueError("mirostat sampling is not built (mirostat 0 only)")
            if self.tfs_z != self.tfs_z or self.typical_p != self.typical_p:
                raise ValueError("tfs_z / typical_p: NaN")
        elif self.tfs_z != 1.0 or self.typical_p != 1.0 or self.mirostat != 0:
            raise ValueError("tail-free, typical and mirostat sampling are not built (tfs_z 1.0, typical_p 1.0, mirostat 0 only)")
        if self.temp > 0 and not 1 <= self.top_k <= top_k_bound:
            raise ValueError(f"top_k {self.top_k}: 1 .. {top_k_bound} (top_k <= 0 = the whole vocabulary is not built)")
        if not 0 <= self.repeat_last_n <= RING:
            raise ValueError(f"repeat_last_n {self.repeat_last_n}: 0 .. {RING}")


def penalised_logits(logits_f16_row: np.ndarray, recent, params: SamplingParams) -> np.ndarray:
    """fp32 logits after sample_repetition_penalty and sample_frequency_and_presence_penalties over the window `recent` (Generate.cc:14-60)."""
    assert logits_f16_row.dtype == np.float16 and logits_f16_row.ndim == 1
    return _penalise(logits_f16_row.astype(np.float32), recent, params)  # half2float: exact


def _penalise(x: np.ndarray, recent, params: SamplingParams) -> np.ndarray:
    """The two penalties on fp32 values, in place (penalised_logits on the widened row; constrain.constrained_reference on the biased one)."""
    recent = np.asarray(recent, dtype=np.int64).reshape(-1)
    recent = recent[(recent >= 0) & (recent < x.size)]
    if recent.size == 0:
        return x
    ids, counts = np.unique(recent, return_counts=True)
    rp, af, ap = np.float32(params.repeat_penalty), np.float32(params.alpha_frequency), np.float32(params.alpha_presence)
    v = x[ids]
    if rp != np.float32(1.0):
        v = np.where(v <= 0, v * rp, v / rp).astype(np.float32)
    if not (af == 0 and ap == 0):
        v = (v - (counts.astype(np.float32) * af + np.float32(1.0) * ap)).astype(np.float32)
    x[ids] = v
    return x


def _softmax_sorted(l: np.ndarray) -> np.ndarray:
    """sample_softmax on sorted candidates (Generate.cc:91-100): subtract the maximum, expf, a SEQUENTIAL fp32 sum, divide."""
    e = np.exp((l - l[0]).astype(np.float32)).astype(np.float32)
    s = np.cumsum(e, dtype=np.float32)[-1]  # cumsum accumulates in order
    return (e / s).astype(np.float32)


def top_p_cut(p: np.ndarray, top_p) -> int:
    """sample_top_p with min_keep 1 (Generate.cc:304-327): the first i >= 1 whose running sum exceeds top_p; candidates [0, i) stay (the one that crosses is dropped)."""
    if np.float32(top_p) >= np.float32(1.0):
        return int(p.size)
    cum = np.cumsum(p, dtype=np.float32)
    hit = np.nonzero(cum[1:] > np.float32(top_p))[0]
    return int(hit[0]) + 1 if hit.size else int(p.size)


def _softmax_first(l: np.ndarray) -> np.ndarray:
    """sample_softmax on candidates whose `sorted` flag is set (Generate.cc:91-100): subtract the value of the candidate that stands FIRST -- behind sample_typical not
    the maximum --, expf, a SEQUENTIAL fp32 sum, divide.  On sorted candidates this is _softmax_sorted, operation for operation."""
    with np.errstate(over="ignore", invalid="ignore"):
        return _softmax_sorted(l)


def tail_free_cut(p: np.ndarray, z) -> int:
    """sample_tail_free with min_keep 1 (Generate.cc:203-246) on the softmax p of the sorted candidates: |second differences| of p, normalised by their SEQUENTIAL fp32
    sum; the first i >= 1 whose running sum of weights exceeds z; candidates [0, i) stay.  z >= 1 or fewer than 3 candidates: nothing runs.  A zero sum gives NaN weights
    and cuts nothing; so does a NaN z."""
    z, k = np.float32(z), int(p.size)
    if z >= np.float32(1.0) or k <= 2:
        return k
    d1 = (p[:-1] - p[1:]).astype(np.float32)
    d2 = np.abs((d1[:-1] - d1[1:]).astype(np.float32))
    S = np.cumsum(d2, dtype=np.float32)[-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        cum = np.cumsum((d2 / S).astype(np.float32), dtype=np.float32)
        hit = np.nonzero(cum[1:] > z)[0]
    return int(hit[0]) + 1 if hit.size else k


def typical_order(p: np.ndarray, typical_p) -> tuple[np.ndarray, int]:
    """sample_typical with min_keep 1 (Generate.cc:248-302) on the softmax p of the candidates: H = sum (-p_i) * logf(p_i) (sequential, one multiply and one add per
    term), scores |-logf(p_i) - H|, the candidates in ASCENDING score with the earlier one first among equals (the rank rule of include/tce_matmul.h: NaN scores leave
    the order as it is), cut behind the first candidate whose running sum of p exceeds typical_p.  Returns (order, n2): order[i] = the index of the candidate that
    stands at position i."""
    k = int(p.size)
    with np.errstate(divide="ignore", invalid="ignore"):
        lp = np.log(p).astype(np.float32)
        H = np.cumsum(((-p).astype(np.float32) * lp).astype(np.float32), dtype=np.float32)[-1]
        s = np.abs(((-lp).astype(np.float32) - H).astype(np.float32))
        less = s[None, :] < s[:, None]                        # [i][j]: s_j < s_i
        tie = ~(s[:, None] < s[None, :]) & (np.arange(k)[None, :] < np.arange(k)[:, None])  # !(s_i < s_j) && j < i
    rank = (less | tie).sum(axis=1)
    order = np.arange(k)
    order[rank] = np.arange(k)
    cum = np.cumsum(p[order], dtype=np.float32)
    hit = np.nonzero(cum > np.float32(typical_p))[0]
    return order.astype(np.int32), (int(hit[0]) + 1 if hit.size else k)


MIROSTAT_M = 100  # the reference's mirostat_m (LLaMA3Generate.cc:164)


def mirostat_keep(k_f, kk: int) -> int:
    """The project's rule where C leaves int(k) open (include/tce_matmul.h, rule 2): NaN or k_f < 1 -> 1; k_f >= kk (+inf included) -> kk; otherwise int(k_f)."""
    k_f = np.float32(k_f)
    if not k_f >= np.float32(1.0):
        return 1
    return int(kk) if k_f >= np.float32(kk) else int(k_f)


def mirostat_reference(sorted_logits: np.ndarray, params: "SamplingParams", mu, u, vocab: int, m: int = MIROSTAT_M) -> dict:
    """tce_sample_mirostat_f16's rule for a row whose mode is 1 or 2 and whose temp > 0, restated in numpy fp32: sample_temperature, sample_softmax and
    sample_token_mirostat[_v2] (Generate.cc:72-100, 138-201) on the row's kk sorted penalised candidates.  sorted_logits: fp32, descending.  Returns p (the softmax over
    logit / temp), s_hat and k_f (mode 1; else 0), kept, final_p (kept entries), choice, surprise and mu_out."""
    f32 = np.float32
    l = np.asarray(sorted_logits, f32)
    kk, mu = int(l.size), f32(mu)
    with np.errstate(all="ignore"):
        lt = (l / f32(params.temp)).astype(f32)
        p = _softmax_sorted(lt)
        s_hat = k_f = f32(0.0)
        if int(params.mirostat) == 1:
            nt = kk - 1 if (m - 1 < 0 or m - 1 > kk - 1) else m - 1
            i = np.arange(nt)
            t = np.log(((i + 2).astype(f32) / (i + 1).astype(f32)).astype(f32)).astype(f32)
            bi = np.log((p[:nt] / p[1:nt + 1]).astype(f32)).astype(f32)
            A = np.cumsum((t * bi).astype(f32), dtype=f32)[-1] if nt else f32(0.0)
            B = np.cumsum((t * t).astype(f32), dtype=f32)[-1] if nt else f32(0.0)
            s_hat = f32(A / B)
            eps = f32(s_hat - f32(1.0))
            num = f32(eps * _powf(2.0, mu))
            den = f32(f32(1.0) - _powf(f32(vocab), f32(-eps)))
            k_f = _powf(f32(num / den), f32(f32(1.0) / s_hat))
            kept = mirostat_keep(k_f, kk)
        else:
            hit = np.nonzero((-np.log2(p).astype(f32)).astype(f32) > mu)[0]
            kept = max(int(hit[0]) if hit.size else kk, 1)
        fp = _softmax_sorted(lt[:kept])
        choice = draw_reference(fp, u)
        surprise = f32(-np.log2(fp[choice]).astype(f32))
        mu_out = f32(mu - f32(f32(params.mirostat_eta) * f32(surprise - f32(params.mirostat_tau))))
    return {"p": p, "s_hat": s_hat, "k_f": k_f, "kept": kept, "final_p": fp, "choice": choice, "surprise": surprise, "mu_out": mu_out}


def _powf(x, y) -> np.float32:
    """powf as one rounding of the float64 power (what the device computes); pow's special cases (a negative base with a fractional exponent: NaN)."""
    with np.errstate(all="ignore"):
        return np.float32(np.power(np.float64(np.float32(x)), np.float64(np.float32(y))))


def draw_reference(final_p: np.ndarray, u) -> int:
    """Inverse CDF on the sequential fp32 running sum of final_p: the first i with u < cdf_i, the last candidate if rounding leaves none."""
    cdf = np.cumsum(final_p, dtype=np.float32)
    hit = np.nonzero(np.float32(u) < cdf)[0]
    return int(hit[0]) if hit.size else int(final_p.size) - 1


def sample_reference(logits_f16_row: np.ndarray, recent, params: SamplingParams, u, mu=None) -> dict:
    """One row through the chain tce_sample_f16 implements.  recent: the penalty window (the last repeat_last_n ids of the ring, initial zeros included).
    Ordering rule: descending penalised logit, ascending id among equals.  Returns ids / logits (the k sorted candidates), p (first softmax), n (kept by top-p),
    final_p (after temperature, n entries), choice and token.  params.mirostat 1 or 2 with temp > 0 (tce_sample_mirostat_f16): mu is the row's running value (None:
    2 * tau, a fresh slot's); the result also carries mirostat_reference's keys, mu_out among them."""
    x = penalised_logits(logits_f16_row, recent, params)
    return _chain(x, np.arange(x.size), params, u, mu)


def _chain(x: np.ndarray, among: np.ndarray, params: SamplingParams, u, mu=None) -> dict:
    """sample_reference behind the penalties, over the ids `among` (ascending) of the penalised fp32 row x: every id (sample_reference) or the allowed ones
    (constrain.constrained_reference).  The ids keep their values: ties go to the lowest id, and fewer than k ids make k their number."""
    xa = x[among]
    V = xa.size
    if params.temp <= 0:
        tok = int(among[int(np.argmax(xa))])  # the first maximum: std::max_element
        return {"ids": np.array([tok], np.int32), "logits": x[tok:tok + 1].copy(), "p": np.zeros(1, np.float32), "n": 1, "final_p": np.zeros(1, np.float32),
                "choice": 0, "token": tok, "n_tfs": 1, "n_typ": 1, "order": np.zeros(1, np.int32), "p_top": np.zeros(1, np.float32), "final_ids": np.array([tok], np.int32)}
    k = min(max(int(params.top_k), 1), V)
    if k < V:
        kth = np.partition(xa, V - k)[V - k]
        gt = np.nonzero(xa > kth)[0]
        eq = np.nonzero(xa == kth)[0][:k - gt.size]  # the lowest ids of the boundary's tie class
        cand = among[np.concatenate([gt, eq])]
    else:
        cand = among
    order = np.lexsort((cand, -x[cand].astype(np.float64)))
    ids = cand[order].astype(np.int32)
    l = (x[ids] + np.float32(0.0)).astype(np.float32)  # (-0 -> +0, as the device returns it)
    if int(params.mirostat) in (1, 2):  # tce_sample_mirostat_f16: instead of the stages, top-p and temperature
        mu = np.float32(2.0) * np.float32(params.mirostat_tau) if mu is None else mu
        r = mirostat_reference(l, params, mu, u, x.size)
        kept = r["kept"]
        r.update({"ids": ids, "logits": l, "n": kept, "token": int(ids[r["choice"]]), "n_tfs": int(l.size), "n_typ": int(l.size), "order": np.arange(l.size, dtype=np.int32),
                  "p_top": r["p"], "final_ids": ids, "mu_in": np.float32(mu)})
        return r
    p = _softmax_sorted(l)
    # the two stages of tce_sample_stages_f16 (rules 2 and 3 of include/tce_matmul.h); with tfs_z and typical_p both >= 1 nothing below differs from the chain without them
    tfs_on, typ_on = not np.float32(params.tfs_z) >= np.float32(1.0), not np.float32(params.typical_p) >= np.float32(1.0)
    n1 = tail_free_cut(p, params.tfs_z) if tfs_on else int(p.size)
    order, n2 = np.arange(n1, dtype=np.int32), n1
    if typ_on:
        order, n2 = typical_order(_softmax_first(l[:n1]), params.typical_p)
    order = order[:n2]
    lf, final_ids = l[order], ids[order]
    p_top = _softmax_first(lf) if (tfs_on or typ_on) else p
    n = top_p_cut(p_top, params.top_p)
    lt = (lf[:n] / np.float32(params.temp)).astype(np.float32)
    fp = _softmax_first(lt)
    choice = draw_reference(fp, u)
    return {"ids": ids, "logits": l, "p": p, "n": n, "final_p": fp, "choice": choice, "token": int(final_ids[choice]), "n_tfs": n1, "n_typ": n2, "order": order,
            "p_top": p_top, "final_ids": final_ids}


def logprob_reference(logits_f16_row: np.ndarray, target: int) -> float:
    """logprob = x_t - LSE(x) over the row's RAW fp16 logits (no penalties, no truncation, no temperature: the model's distribution), LSE(x) = M + log sum exp(x_i - M),
    in float64.  The device's degenerate rows: a NaN or +inf logit, or a row of -inf only, gives NaN.  target -1 ("no target"): 0.0; any other id outside the row: NaN."""
    assert logits_f16_row.dtype == np.float16 and logits_f16_row.ndim == 1 and logits_f16_row.size >= 1
    target = int(target)
    if target == -1:
        return 0.0
    if not 0 <= target < logits_f16_row.size:
        return float("nan")
    x = logits_f16_row.astype(np.float64)
    m = x.max() if not np.isnan(x).any() else np.nan
    if not np.isfinite(m):  # NaN, +inf, or every entry -inf
        return float("nan")
    return float(x[target] - (m + np.log(np.exp(x - m).sum())))


def perplexity(values) -> float:
    """exp(-mean logprob) over the values of one or several score() results."""
    v = np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in values]) if isinstance(values, (list, tuple)) else np.asarray(values, np.float64).reshape(-1)
    return float(np.exp(-v.mean()))


def ring_window(ring: np.ndarray, pushed: int, repeat_last_n: int) -> np.ndarray:
    """The penalty window of a ring [64] after `pushed` pushes: its last repeat_last_n entries (zeros where fewer tokens have been pushed)."""
    n = min(max(int(repeat_last_n), 0), RING)
    return np.array([ring[(pushed - 1 - t) % RING] for t in range(n)], np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# device state
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
_ROW_WORDS = C.sizeof(capi.SampleRow) // 4
_DEBUG_WORDS = C.sizeof(capi.SampleDebug) // 4
_MIRO_WORDS = C.sizeof(capi.MirostatRow) // 4


def make_row(params: SamplingParams, seed: int, max_new: int, prompt_ids=()) -> capi.SampleRow:
    """A fresh tce_sample_row: the ring starts as 64 zeros (the reference's last_n_tokens) and takes the prompt's tokens in order."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = capi.SampleRow(temp=params.temp, top_k=params.top_k, top_p=params.top_p, repeat_penalty=params.repeat_penalty, alpha_frequency=params.alpha_frequency,
                       alpha_presence=params.alpha_presence, repeat_last_n=params.repeat_last_n, max_new=int(max_new), seed_lo=seed & _MASK, seed_hi=seed >> 32,
                       generated=0, ring_pushed=0)
    for t in prompt_ids:
        r.ring[r.ring_pushed % RING] = int(t)
        r.ring_pushed += 1
    return r


def make_mirostat_row(params: SamplingParams, m: int = MIROSTAT_M) -> capi.MirostatRow:
    """A fresh tce_mirostat_row: the request's mode, tau and eta, the reference's m, and mu = 2 * tau in fp32 (LLaMA3Generate.cc:163) -- per slot, at every admission."""
    tau = np.float32(params.mirostat_tau)
    return capi.MirostatRow(mode=int(params.mirostat), m=int(m), tau=float(tau), eta=float(np.float32(params.mirostat_eta)), mu=float(np.float32(2.0) * tau))


class Sampler:
    """The per-row device state of tce_sample_f16 for `batch` rows: rows (parameters, ring, counters), next_token, the output log [batch][log_stride], the workspace
    (zeroed once).  debug=True keeps the sorted candidates of the last call (tests).  logprobs=True: step() calls tce_sample_logprobs_f16 -- the same two launches --
    and out_logprob fp32 [batch][log_stride] holds, beside every token of out_log, its log-probability under the raw logits (NaN where nothing was written yet); last_lse
    [batch] the log-sum-exp of the row each slot's last token was drawn from.  logprobs=False: the call, the launches and a captured graph are what they were.
    constraints=True: the sampler owns the constraint rows [batch] (struct tce_constraint_row: automaton, state, logit bias), the automaton table (constrain.
    AutomatonTable) and the violations word, and step() calls tce_sample_constrained_f16 -- still two launches; set_row(..., automaton=, logit_bias=) gives a slot its
    automaton (an index from table.register) and bias.  constraints=False: the existing entry points, untouched.
    stages=True: the sampler owns the stage rows [batch] (struct tce_stage_row: tfs_z, typical_p; (1.0, 1.0) until set_row writes a slot's pair from its SamplingParams)
    and step() calls tce_sample_stages_f16 -- still two launches --, with the constraint and logprob blocks when those options are on; debug=True also keeps the
    stage records (stage_debug_row).  stages=False: the call, the launches and a captured graph are what they were, and set_row refuses a SamplingParams whose
    tfs_z / typical_p are not 1.0.
    mirostat_rows=True (implies stages=True): the sampler also owns the mirostat rows [batch] (struct tce_mirostat_row: mode, m, tau, eta, mu; every slot mode 0 until
    set_row writes a slot's row from its SamplingParams, with mu = 2 * tau) and step() calls tce_sample_mirostat_f16 -- still two launches; mu lives on the device and
    moves with every token the slot emits, under a captured graph too.  debug=True also keeps the mirostat records (mirostat_debug_row).  The constructor's `mirostat`
    argument is the CALL's field and stays refused when it is not 0."""

    def __init__(self, batch: int, vocab: int, log_stride: int, device, top_k_bound: int = 40, stop_ids=(), debug: bool = False, tfs_z: float = 1.0,
                 typical_p: float = 1.0, mirostat: int = 0, logprobs: bool = False, constraints: bool = False, stages: bool = False, mirostat_rows: bool = False):
        import torch
        if len(stop_ids) > 4:
            raise ValueError("at most 4 stop ids")
        self.batch, self.vocab, self.log_stride, self.top_k_bound, self.stop_ids = batch, vocab, int(log_stride), int(top_k_bound), [int(s) for s in stop_ids]
        self.tfs_z, self.typical_p, self.mirostat = tfs_z, typical_p, mirostat
        need = int(capi.lib().tce_sample_workspace_bytes(batch, vocab))
        if need == 0:
            raise ValueError("unsupported sampling shape (batch 1 .. 65535, vocab 1 .. 2^20)")
        self.rows = torch.zeros((batch, _ROW_WORDS), dtype=torch.int32, device=device)
        self.next_token = torch.zeros(batch, dtype=torch.int32, device=device)
        self.out_log = torch.full((batch, self.log_stride), -1, dtype=torch.int32, device=device)
        self.workspace = torch.zeros(need, dtype=torch.uint8, device=device)
        self.uniform_override = None  # fp32 [batch] on the device: replaces the generator (tests)
        self.debug = torch.zeros((batch, _DEBUG_WORDS), dtype=torch.int32, device=device) if debug else None
        self.logprobs = bool(logprobs)
        self.out_logprob = self.last_lse = self.partials = None
        if self.logprobs:
            self.out_logprob = torch.full((batch, self.log_stride), float("nan"), dtype=torch.float32, device=device)
            self.last_lse = torch.full((batch,), float("nan"), dtype=torch.float32, device=device)
            self.partials = torch.empty(int(capi.lib().tce_logprobs_workspace_bytes(batch, vocab)), dtype=torch.uint8, device=device)  # (need not be zeroed)
        self.constraints = bool(constraints)
        self.crows = self.table = self.violations_word = None
        if self.constraints:
            from .constrain import AutomatonTable
            self.crows = torch.zeros((batch, C.sizeof(capi.ConstraintRow) // 4), dtype=torch.int32, device=device)
            self.crows[:, 0] = -1  # every row unconstrained
            self.table = AutomatonTable(vocab, device)
            self.violations_word = torch.zeros(1, dtype=torch.int32, device=device)
        self.mirostat_rows = bool(mirostat_rows)
        self.stages = bool(stages) or self.mirostat_rows
        self.mrows = self.mdebug = None
        if self.mirostat_rows:
            self.mrows = torch.zeros((batch, _MIRO_WORDS), dtype=torch.int32, device=device)  # every slot mode 0: off
            self.mdebug = torch.zeros((batch, C.sizeof(capi.MirostatDebug) // 4), dtype=torch.int32, device=device) if debug else None
        self.srows = self.sdebug = None
        if self.stages:
            self.srows = torch.ones((batch, 2), dtype=torch.float32, device=device)  # every slot (1.0, 1.0): off
            self.sdebug = torch.zeros((batch, C.sizeof(capi.StageDebug) // 4), dtype=torch.int32, device=device) if debug else None

    def stage_block(self, debug=None) -> capi.SampleStages:
        """struct tce_sample_stages over this sampler's stage rows (debug: another record array -- the verifier's, per virtual row)."""
        debug = self.sdebug if debug is None else debug
        return capi.SampleStages(rows=self.srows.data_ptr(), debug=debug.data_ptr() if debug is not None else None)

    def mirostat_block(self) -> capi.SampleMirostat:
        """struct tce_sample_mirostat over this sampler's mirostat rows"""
        return capi.SampleMirostat(rows=self.mrows.data_ptr(), debug=self.mdebug.data_ptr() if self.mdebug is not None else None)

    def constraint(self) -> capi.Constraint:
        """struct tce_constraint over this sampler's table, rows and violations word (n_fsm is the table's size: a free entry has no states and is refused on the device)."""
        return capi.Constraint(fsms=self.table.fsms.data_ptr(), n_fsm=capi.TCE_FSM_MAX, rows=self.crows.data_ptr(), violations=self.violations_word.data_ptr())

    def check_constraint(self, automaton, logit_bias) -> list:
        """set_row's refusals for automaton / logit_bias, without a write: returns the bias as [(id, value)]."""
        from .constrain import check_bias
        if not self.constraints:
            if automaton is not None or logit_bias:
                raise ValueError("automaton / logit_bias: the sampler was built without constraints=True")
            return []
        if automaton is not None:
            self.table.start(automaton)
        return check_bias(logit_bias, self.vocab)

    def violations(self) -> int:
        """Rows the device found in an invalid constraint state (rule 6) since the sampler was made: 0 unless a row or a descriptor was written from outside."""
        return int(self.violations_word.cpu().numpy().view(np.uint32)[0]) if self.constraints else 0

    def logprob_out(self, partials=None) -> capi.LogprobOut:
        """struct tce_logprob_out over this sampler's arrays (partials: another workspace -- the verifier's, for batch * rows_per_seq rows)."""
        return capi.LogprobOut(out_logprob=self.out_logprob.data_ptr(), last_lse=self.last_lse.data_ptr(), partials=(self.partials if partials is None else partials).data_ptr())

    def set_row(self, slot: int, params: SamplingParams, seed: int, max_new: int, prompt_ids=(), automaton: int | None = None, logit_bias=None) -> None:
        """The slot changes hands: one stream-ordered copy of its row (parameters, a fresh ring with the prompt pushed, counters at zero) and, with constraints=True,
        one of its constraint row: automaton (an index of table.register, None: unconstrained) in its start state, logit_bias ({id: value} or [(id, value)], <= 16)."""
        import torch
        params.check(self.top_k_bound, stages=self.stages, mirostat_rows=self.mirostat_rows)
        if not 1 <= max_new <= self.log_stride:
            raise ValueError(f"max_new {max_new}: 1 .. {self.log_stride}")
        bias = self.check_constraint(automaton, logit_bias)
        row = make_row(params, seed, max_new, prompt_ids)
        host = torch.from_numpy(np.frombuffer(bytes(row), dtype=np.int32).copy())
        self.rows[slot].copy_(host)
        if self.constraints:
            from .constrain import constraint_row
            cr = constraint_row(-1 if automaton is None else automaton, 0 if automaton is None else self.table.start(automaton), bias)
            self.crows[slot].copy_(torch.from_numpy(np.frombuffer(bytes(cr), dtype=np.int32).copy()))
            self.table.users.pop(slot, None)
            if automaton is not None:
                self.table.users[slot] = int(automaton)
        if self.stages:
            self.srows[slot].copy_(torch.tensor([params.tfs_z, params.typical_p], dtype=torch.float32))
        if self.mirostat_rows:
            self.mrows[slot].copy_(torch.from_numpy(np.frombuffer(bytes(make_mirostat_row(params)), dtype=np.int32).copy()))

    def step(self, logits, pos_device, pos_bound: int) -> None:
        """tce_sample_f16 on logits fp16 [batch][ld] (two launches on the current stream).  pos_device int32 [batch] is READ (activity) and WRITTEN (+1, or -1)."""
        import torch
        from .linear import _stream
        assert logits.dtype == torch.float16 and logits.is_contiguous() and logits.dim() == 2 and logits.shape[0] == self.batch and logits.shape[1] >= self.vocab
        assert pos_device.dtype == torch.int32 and pos_device.is_contiguous() and pos_device.numel() == self.batch
        assert logits.is_cuda and pos_device.is_cuda
        c = self.call(logits.data_ptr(), logits.shape[1], pos_device.data_ptr(), pos_bound)
        if self.mirostat_rows:
            capi.check(capi.sample_mirostat_f16(c, self.stage_block(), self.mirostat_block(), self.constraint() if self.constraints else None,
                                                self.logprob_out() if self.logprobs else None, _stream()))
        elif self.stages:
            capi.check(capi.sample_stages_f16(c, self.stage_block(), self.constraint() if self.constraints else None, self.logprob_out() if self.logprobs else None, _stream()))
        elif self.constraints:
            capi.check(capi.sample_constrained_f16(c, self.constraint(), self.logprob_out() if self.logprobs else None, _stream()))
        elif self.logprobs:
            capi.check(capi.sample_logprobs_f16(c, self.logprob_out(), _stream()))
        else:
            capi.check(capi.sample_f16(c, _stream()))

    def call(self, logits_ptr: int, ld: int, pos_ptr: int, pos_bound: int) -> capi.SampleCall:
        c = capi.SampleCall(logits=logits_ptr, ld=ld, vocab=self.vocab, batch=self.batch, top_k_bound=self.top_k_bound, rows=self.rows.data_ptr(), pos_device=pos_ptr,
                            pos_bound=int(pos_bound), log_stride=self.log_stride, next_token=self.next_token.data_ptr(), out_log=self.out_log.data_ptr(),
                            uniform_override=self.uniform_override.data_ptr() if self.uniform_override is not None else None,
                            debug=self.debug.data_ptr() if self.debug is not None else None, workspace=self.workspace.data_ptr(), n_stop=len(self.stop_ids),
                            mirostat=self.mirostat, tfs_z=self.tfs_z, typical_p=self.typical_p)
        for i, s in enumerate(self.stop_ids):
            c.stop_ids[i] = s
        return c

    # ---- reading state back (each synchronises) ----
    def row(self, slot: int) -> capi.SampleRow:
        return capi.SampleRow.from_buffer_copy(self.rows[slot].cpu().numpy().tobytes())

    def constraint_row(self, slot: int) -> capi.ConstraintRow:
        return capi.ConstraintRow.from_buffer_copy(self.crows[slot].cpu().numpy().tobytes())

    def debug_row(self, slot: int) -> capi.SampleDebug:
        return capi.SampleDebug.from_buffer_copy(self.debug[slot].cpu().numpy().tobytes())

    def stage_debug_row(self, slot: int) -> capi.StageDebug:
        return capi.StageDebug.from_buffer_copy(self.sdebug[slot].cpu().numpy().tobytes())

    def mirostat_row(self, slot: int) -> capi.MirostatRow:
        return capi.MirostatRow.from_buffer_copy(self.mrows[slot].cpu().numpy().tobytes())

    def mirostat_debug_row(self, slot: int) -> capi.MirostatDebug:
        return capi.MirostatDebug.from_buffer_copy(self.mdebug[slot].cpu().numpy().tobytes())

    def generated(self) -> np.ndarray:
        return self.rows[:, 10].cpu().numpy().astype(np.int64)  # word 10: tce_sample_row.generated


def embed_rows(table, token, out, pos_device, pos_bound: int, workspace) -> None:
    """tce_embed_rows_f16: out[b] = table[token[b]] for every active row (one launch on the current stream)."""
    import torch
    from .linear import _stream
    assert table.dtype == torch.float16 and table.is_contiguous() and table.dim() == 2 and out.dtype == torch.float16 and out.is_contiguous()
    assert token.dtype == torch.int32 and pos_device.dtype == torch.int32 and token.numel() == pos_device.numel() and out.numel() == token.numel() * table.shape[1]
    capi.check(capi.lib().tce_embed_rows_f16(table.data_ptr(), table.shape[0], table.shape[1], token.data_ptr(), out.data_ptr(), token.numel(), pos_device.data_ptr(),
                                             int(pos_bound), workspace.data_ptr(), _stream()))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# host bookkeeping
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
class SlotBook:
    """What the host knows about the slots between synchronisations: the position of the next token each live slot will process and how many tokens it may still
    produce.  run(n) asks it which key indices the next n replays can touch, so that pages are reserved BEFORE the replays and nothing is copied in between."""

    def __init__(self, batch: int, max_keys: int):
        self.batch, self.max_keys = batch, max_keys
        self.pos = [-1] * batch        # -1: free or retired
        self.generated = [0] * batch
        self.max_new = [0] * batch

    def live(self) -> list[int]:
        return [s for s in range(self.batch) if self.pos[s] >= 0]

    def admit(self, slot: int, prompt_len: int, max_new: int) -> None:
        if self.pos[slot] >= 0:
            raise ValueError(f"slot {slot} is live")
        if prompt_len < 1 or prompt_len >= self.max_keys or max_new < 1:
            raise ValueError(f"a prompt of 1 .. {self.max_keys - 1} tokens and max_new >= 1")
        self.pos[slot], self.generated[slot], self.max_new[slot] = prompt_len, 1, max_new  # (admission samples the first token)
        if max_new == 1:
            self.pos[slot] = -1

    def wanted(self, n: int) -> list[tuple[int, int]]:
        """[(slot, highest key index)] the next n replays may append: a live slot at position p with r tokens left processes positions p .. p + min(n, r) - 1,
        and never beyond the cache's last key (a row past it is inactive by the position rule)."""
        out = []
        for s in self.live():
            steps = min(n, self.max_new[s] - self.generated[s])
            if steps >= 1:
                out.append((s, min(self.pos[s] + steps - 1, self.max_keys - 1)))
        return out

    def reserve(self, allocator, n: int) -> list[list[int]]:
        """PageAllocator.reserve_many for the next n replays, all or nothing (PagePoolExhausted: nothing changed)."""
        w = self.wanted(n)
        return allocator.reserve_many(w) if w else []

    def update(self, pos_host, generated_host) -> list[int]:
        """After a synchronise: take the device's positions and counts; returns the slots that retired since the last update."""
        retired = []
        for s in range(self.batch):
            if self.pos[s] >= 0:
                self.generated[s] = int(generated_host[s])
                p = int(pos_host[s])
                if p < 0 or p >= self.max_keys:
                    retired.append(s)
                    p = -1
                self.pos[s] = p
        return retired

    def clear(self, slot: int) -> None:
        self.pos[slot], self.generated[slot], self.max_new[slot] = -1, 0, 0


def score_plan(prompts, free_slots, max_keys: int, vocab: int, chunk_rows: int = 256) -> dict:
    """BatchedGenerator.score's bookkeeping (host only): which prompts need rows ("work": those of >= 2 tokens), the free slot each takes, the pages to reserve
    [(slot, last key index)], the packed token row and its targets (the next token; -1 for a prompt's last row), the row chunks [(row0, rows)] of at most
    chunk_rows rows, and split(values [total rows]) -> one fp32 array of n - 1 values per prompt (empty for a 1-token prompt)."""
    if int(chunk_rows) < 1:
        raise ValueError("score: chunk_rows >= 1")
    prompts = [[int(t) for t in ids] for ids in prompts]
    for ids in prompts:
        if not 1 <= len(ids) <= max_keys:
            raise ValueError(f"a prompt of 1 .. {max_keys} tokens")
        if any(not 0 <= t < vocab for t in ids):
            raise ValueError("a prompt token lies outside the vocabulary")
    work = [i for i, ids in enumerate(prompts) if len(ids) >= 2]
    free_slots = list(free_slots)
    if len(work) > min(len(free_slots), capi.TCE_PREFILL_MAX_SEGMENTS):
        raise ValueError(f"score: {len(work)} prompts, {len(free_slots)} free slots (at most {capi.TCE_PREFILL_MAX_SEGMENTS} per call)")
    slots = free_slots[:len(work)]
    total = sum(len(prompts[i]) for i in work)
    chunk = max(1, min(int(chunk_rows), total))

    def split(values) -> list:
        out, r0 = [np.zeros(0, np.float32) for _ in prompts], 0
        for i in work:
            n = len(prompts[i])
            out[i] = np.asarray(values[r0:r0 + n - 1], np.float32).copy()
            r0 += n
        return out

    return {"prompts": prompts, "work": work, "slots": slots, "reserve": [(s, len(prompts[i]) - 1) for s, i in zip(slots, work)],
            "tokens": [t for i in work for t in prompts[i]], "targets": [t for i in work for t in prompts[i][1:] + [-1]], "chunk": chunk,
            "chunks": [(r0, min(chunk, total - r0)) for r0 in range(0, total, chunk)], "split": split}


def admission_chunks(lengths, chunk_rows: int, window: int | None = None, sinks: int | None = None) -> list[dict]:
    """The schedule of admit(..., chunk_rows=N) for prompts of `lengths` tokens (pure: no allocator, no device).  Round r takes rows [r N, min((r + 1) N, len)) of
    every prompt that still has some; per round, with i the prompt's index in `lengths`:
        "reserve"   [(i, c0 + m - 1)]   reserved first, all or nothing across the round (PageAllocator.reserve_many)
        "segments"  [(i, c0, m)]        embedded, then prefilled at position c0 through ALL layers
        "release"   [(i, c0 + m - W)]   then PageAllocator.release_behind -- only with window = W = the largest window when EVERY layer has one (else empty):
                                        the next chunk's first row sits at c0 + m and weighs keys from c0 + m - W + 1 on
    A slot's keys between a round's reserve and its release span at most W + N - 1 + (page_keys - 1) rows, so it holds at most ceil((W + N) / page_keys) + 1 pages,
    whatever the prompt's length.  sinks = S (the largest of the layers' sink counts; needs a window): the schedule is the same -- the caller's release_behind keeps
    the first ceil(S / page_keys) = 1 page besides, so the bound is ceil((W + N) / page_keys) + 2 pages."""
    if sinks is not None and (window is None or not 1 <= int(sinks) <= 16):
        raise ValueError(f"sinks {sinks}: None, or an integer 1 .. 16 beside a window")
    lengths = [int(n) for n in lengths]
    if int(chunk_rows) != chunk_rows or int(chunk_rows) < 1:
        raise ValueError(f"chunk_rows {chunk_rows}: None or an integer >= 1")
    if window is not None and int(window) < 1:
        raise ValueError(f"window {window}: None or an integer >= 1")
    if not lengths or min(lengths) < 1:
        raise ValueError("admission_chunks: prompts of at least one token")
    N, rounds = int(chunk_rows), []
    for c0 in range(0, max(lengths), N):
        segs = [(i, c0, min(N, n - c0)) for i, n in enumerate(lengths) if n > c0]
        rounds.append({"reserve": [(i, c + m - 1) for i, c, m in segs], "segments": segs,
                       "release": [] if window is None else [(i, c + m - int(window)) for i, c, m in segs]})
    return rounds


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the front
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
class _GeneratorBase:
    """What BatchedGenerator and speculative.SpeculativeGenerator share: the construction, the graph, admission, the replay loop and the read-outs.  A subclass gives
    token_step() (what one replay runs) and launches_per_token, and calls _capture() once its own buffers exist."""

    lora = None  # a LoraPool (BatchedGenerator / SpeculativeGenerator(..., lora=pool)): admit(..., adapter=) writes the slot's row_adapter word (LoraPool.set_slot: once per
    # row of the slot in a pool built for speculative rows), release() writes -1

    def __init__(self, decoders, final_gamma, lm_head, embed_table, max_new: int, eps: float | None, top_k_bound: int, stop_ids, rows_per_seq: int | None = None,
                 **sampler_kw):
        """rows_per_seq None: the token step carries one row per slot, and admission runs its head on the step's xn / logits.  An integer: hidden / xn / logits are
        batch * rows_per_seq rows and admission has batch rows of its own (_adm_xn / _adm_logits)."""
        import torch
        self.decoders = list(decoders)
        d0 = self.decoders[0]
        self.batch, self.hidden_size = d0.batch, d0.block.hidden
        self.allocator = getattr(d0, "allocator", None)
        assert all(getattr(d, "allocator", None) is self.allocator and d.batch == self.batch for d in self.decoders), "one allocator, one batch size"
        self.max_keys = d0.attention.max_keys
        self.pos_bound = self.max_keys - 1
        self.final_gamma, self.lm_head, self.embed_table = final_gamma, lm_head, embed_table
        self.eps = d0.block.eps if eps is None else eps
        self.vocab = embed_table.shape[0]
        assert embed_table.dtype == torch.float16 and embed_table.shape[1] == self.hidden_size and lm_head.in_features == self.hidden_size and lm_head.out_features >= self.vocab
        dev = embed_table.device
        self.device = dev
        self.sampler = Sampler(self.batch, self.vocab, max_new, dev, top_k_bound=top_k_bound, stop_ids=stop_ids, **sampler_kw)
        self.book = SlotBook(self.batch, self.max_keys)
        rows = self.batch * (rows_per_seq or 1)
        h = lambda n, width: torch.zeros((n, width), dtype=torch.float16, device=dev)
        self.pos = torch.full((self.batch,), -1, dtype=torch.int32, device=dev)
        self.hidden, self.xn, self.logits = h(rows, self.hidden_size), h(rows, self.hidden_size), h(rows, lm_head.out_features)
        self._adm_pos = torch.full((self.batch,), -1, dtype=torch.int32, device=dev)
        self._adm_hidden = h(self.batch, self.hidden_size)
        self._adm_xn, self._adm_logits = (self.xn, self.logits) if rows_per_seq is None else (h(self.batch, self.hidden_size), h(self.batch, lm_head.out_features))
        self._graph = None

    def _take_pool(self, lora) -> None:
        """lora=pool of a generator: the decoders' views must be this pool's layers, in order (None: no decoder may carry one)."""
        pools = [getattr(getattr(d, "lora", None), "pool", None) for d in self.decoders]
        if lora is None and any(p is not None for p in pools):
            raise ValueError("the decoders carry LoRA views: pass their pool as lora=")
        if lora is not None:
            if any(p is not lora for p in pools) or [d.lora.index for d in self.decoders] != list(range(len(self.decoders))) or lora.layers != len(self.decoders):
                raise ValueError("lora=pool: decoder i must be built with lora=pool.layer(i), one layer of the pool per decoder")
            self.lora = lora

    def _capture(self) -> None:
        """token_step once eagerly -- the warm-up: every row inactive, so nothing is embedded, appended or sampled; the gate/up form is settled --, then once into the
        graph run() replays."""
        import torch
        self.token_step()
        torch.cuda.synchronize()
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph):
            self.token_step()

    def _head(self, hidden, pos, xn, logits) -> None:
        """final norm -> lm_head -> sampling (which advances or retires `pos`), at M = batch"""
        from .linear import _stream, rmsnorm_half
        rmsnorm_half(hidden, self.final_gamma, self.eps, out=xn)
        capi.check(capi.w4a16_forward(self.lm_head.desc(xn, logits), _stream()))
        self.sampler.step(logits, pos, self.pos_bound)

    # ---- admission ----
    def admit(self, slot, prompt_ids=None, params: SamplingParams | None = None, seed: int = 0, max_new: int | None = None, chunk_rows: int | None = None,
              automaton: int | None = None, logit_bias=None, constraints: dict | None = None, adapter: int | None = None, adapters: dict | None = None) -> list[int]:
        """admit(slot, prompt_ids, params, seed, max_new), or admit([(slot, prompt_ids, params, seed, max_new), ...]) for several sequences through ONE prefill_many.
        The prompt is embedded, prefilled through every layer, the final norm and lm_head run on its last row and the first token is sampled; the slot's position
        becomes the prompt length.  Synchronises.  Returns the slots that retired on their first token.
        chunk_rows = N >= 1 (paged decoders): the prompts go through in chunks of at most N rows (admission_chunks) -- per chunk pages are reserved through its last
        key, all or nothing across the admissions, the chunk is embedded and prefilled at its position through ALL layers, and when every layer has a window the
        pages wholly behind it are given back before the next chunk.  A windowed slot then never holds more than ceil((max W + N) / page_keys) + 1 pages, so a prompt
        longer than the pool can be admitted; without windows only the activation rows are bounded.  PagePoolExhausted in a later chunk: the slots of this call are
        released and the generator is as it was before the call.  A chunked prefill is not bit-identical to the one-shot one (the prefill's tiling differs).
        constraints=True generators: automaton= (an index of sampler.table.register) and logit_bias= ({id: value} or [(id, value)]) for the single form, constraints=
        {slot: (automaton index or None, bias or None)} for the list form; the slot starts in the automaton's start state and the FIRST token is already constrained.
        lora=pool generators: adapter= (an index of the pool, None: the base model) for the single form, adapters={slot: index} for the list form (a slot it does not
        name runs the base model).  The slot's row_adapter word is written BEFORE the prefill, so the prompt's rows and the first token already run on the adapter; the
        captured graph reads the word, so no admission captures again."""
        import torch
        if prompt_ids is not None and adapters is not None or prompt_ids is None and adapter is not None:
            raise ValueError("admit: adapter= goes with the single form, adapters={slot: index} with the list form")
        lora_of = {int(slot): adapter} if prompt_ids is not None else {int(k): v for k, v in (adapters or {}).items()}
        if self.lora is None and any(a is not None for a in lora_of.values()):
            raise ValueError("admit: adapter= / adapters=: the generator was built without lora=pool")
        for a in lora_of.values():
            if a is not None and (int(a) != a or not 0 <= int(a) < self.lora.max_adapters):
                raise ValueError(f"admit: adapter {a} of {self.lora.max_adapters} (None: the base model)")
        if prompt_ids is not None and constraints is not None or prompt_ids is None and (automaton is not None or logit_bias):
            raise ValueError("admit: automaton= / logit_bias= go with the single form, constraints={slot: (automaton, bias)} with the list form")
        cons = {int(slot): (automaton, logit_bias)} if prompt_ids is not None else {int(k): tuple(v) for k, v in (constraints or {}).items()}
        adm = slot if prompt_ids is None else [(slot, prompt_ids, params, seed, max_new)]
        adm = [(int(s), [int(t) for t in ids], p or SamplingParams(), int(sd), int(self.sampler.log_stride if mn is None else mn)) for s, ids, p, sd, mn in adm]
        if len({s for s, *_ in adm}) != len(adm):
            raise ValueError("admit: a slot is named twice")
        if any(s not in {sl for sl, *_ in adm} for s in lora_of):
            raise ValueError("admit: adapters names a slot that is not admitted")
        for s, ids, p, sd, mn in adm:
            if not 0 <= s < self.batch:
                raise IndexError(f"slot {s} of {self.batch}")
            if self.book.pos[s] >= 0:
                raise ValueError(f"slot {s} is live")
            if any(not 0 <= t < self.vocab for t in ids):
                raise ValueError("a prompt token lies outside the vocabulary")
            p.check(self.sampler.top_k_bound, stages=getattr(self.sampler, "stages", False),  # (a sampler stand-in without the attribute runs no stage)
                    mirostat_rows=getattr(self.sampler, "mirostat_rows", False))
            if any(c is not None for c in cons.get(s, ())):  # (the existing call forms read nothing new of the sampler)
                self.sampler.check_constraint(*cons[s])
            if not 1 <= len(ids) < self.max_keys or not 1 <= mn <= self.sampler.log_stride:
                raise ValueError(f"a prompt of 1 .. {self.max_keys - 1} tokens and max_new 1 .. {self.sampler.log_stride}")
        if chunk_rows is not None:
            if self.allocator is None:
                raise ValueError("admit: chunk_rows needs paged decoders")
            if int(chunk_rows) != chunk_rows or int(chunk_rows) < 1:
                raise ValueError(f"chunk_rows {chunk_rows}: None or an integer >= 1")
        if self.allocator is not None:  # all or nothing, before anything changes
            if any(self.allocator.pages[s] or self.allocator.gone[s] for s, *_ in adm):
                raise ValueError("admit: a slot still holds pages (release it first)")
            if chunk_rows is None:
                self.allocator.reserve_many([(s, len(ids) - 1) for s, ids, *_ in adm])
        if self.lora is not None:
            for s, *_ in adm:  # every admitted slot's word, -1 included: before the prefill
                self.lora.set_slot(s, lora_of.get(s))

        def embedded(ids):
            tok = torch.tensor(ids, dtype=torch.int32).to(self.device)
            r = torch.empty((len(ids), self.hidden_size), dtype=torch.float16, device=self.device)
            embed_rows(self.embed_table, tok, r, torch.zeros(len(ids), dtype=torch.int32, device=self.device), 0, self.sampler.workspace)
            return r

        if chunk_rows is not None:
            rows = self._prefill_chunks(adm, int(chunk_rows), embedded)  # (each prompt's LAST chunk: its last row is the head's input)
        else:
            rows = [embedded(ids) for s, ids, *_ in adm]
            for d in self.decoders:
                d.prefill_many([(s, r, 0) for (s, *_), r in zip(adm, rows)])
        self._adm_pos.fill_(-1)
        for (s, ids, p, sd, mn), r in zip(adm, rows):
            self.sampler.set_row(s, p, sd, mn, ids, *(cons[s] if any(c is not None for c in cons.get(s, ())) else ()))
            self.sampler.out_log[s].fill_(-1)
            if self.sampler.logprobs:
                self.sampler.out_logprob[s].fill_(float("nan"))
            self._adm_hidden[s].copy_(r[-1])
            self._adm_pos[s] = len(ids) - 1
        self._head(self._adm_hidden, self._adm_pos, self._adm_xn, self._adm_logits)  # the first token: the sampler leaves len(ids) -- or -1 -- in the admitted slots' words
        slots = torch.tensor([s for s, *_ in adm], dtype=torch.int64, device=self.device)
        self.pos.index_copy_(0, slots, self._adm_pos.index_select(0, slots))
        self._admitted([(s, ids) for s, ids, *_ in adm])
        for s, ids, p, sd, mn in adm:
            self.book.admit(s, len(ids), mn)
        return self._sync()

    def _prefill_chunks(self, adm, chunk_rows: int, embedded) -> list:
        """admit's chunked prefill (admission_chunks is the schedule).  Returns every prompt's last chunk of rows, after all layers.  Nothing of the generator but the
        allocator changes here (and, with a pool, the admitted slots' adapter words, which admit wrote just before), so on any failure releasing this call's slots
        and writing their words back to -1 restores the state before the call."""
        windows = [getattr(d, "window", None) for d in self.decoders]
        window = None if any(w is None for w in windows) else max(windows)
        keep = self._keep_pages()
        last = [None] * len(adm)
        try:
            for rnd in admission_chunks([len(ids) for _, ids, *_ in adm], chunk_rows, window, self._max_sinks() if window is not None else None):
                self.allocator.reserve_many([(adm[i][0], upto) for i, upto in rnd["reserve"]])
                chunk = [(adm[i][0], embedded(adm[i][1][c0:c0 + m]), c0) for i, c0, m in rnd["segments"]]
                for d in self.decoders:
                    d.prefill_many(chunk)
                for (i, _, _), (_, r, _) in zip(rnd["segments"], chunk):
                    last[i] = r
                for i, key in rnd["release"]:
                    self.allocator.release_behind(adm[i][0], key, keep_pages=keep)
        except Exception:
            for s, *_ in adm:
                self.allocator.release(s)
                if self.lora is not None:  # (admit wrote the slot's word in front of the prefill: a free slot's word is -1)
                    self.lora.set_slot(s, None)
            raise
        return last

    def _admitted(self, admitted) -> None:
        """A subclass's own record of [(slot, prompt ids)], the first tokens sampled (sampler.next_token)."""

    # ---- running ----
    def run(self, n: int) -> list[int]:
        """n replays of the token step for every live slot: pages for the positions they can touch are reserved first (all or nothing), then the step is replayed n
        times with no host synchronisation and no host-to-device copy in between, then ONE synchronise.  Returns the slots that retired (a stop id, or their budget)."""
        if n < 1:
            raise ValueError("run: n >= 1")
        if self.allocator is not None:
            self._release_behind()
            self.book.reserve(self.allocator, n)
        for _ in range(n):
            if self._graph is not None:
                self._graph.replay()
            else:
                self.token_step()
            self._replayed()
        retired = self._sync()
        if self.allocator is not None:
            self._release_behind()
        return retired

    def _max_sinks(self) -> int | None:
        """The largest sink count of the layers (None: no layer has attention sinks)."""
        sinks = [s for s in (getattr(d, "sinks", None) for d in self.decoders) if s is not None]
        return max(sinks) if sinks else None

    def _keep_pages(self) -> int:
        """release_behind's keep_pages: the pages that hold the layers' sinks, ceil(max S / page_keys) (0: no layer has any)."""
        s = self._max_sinks()
        return 0 if s is None or self.allocator is None else -(-s // self.allocator.page_keys)

    def _release_behind(self) -> None:
        """Sliding windows: when EVERY layer has one, no layer weighs a key below pos - max(windows) + 1 of a live slot at position pos again -- the pages wholly below
        go back to the pool (PageAllocator.release_behind; host bookkeeping only: the table words stay, so the captured graph stays valid).  Between bursts a slot then
        holds at most ceil((max W + n) / page_keys) + 1 pages.  One unwindowed layer: nothing is released."""
        windows = [getattr(d, "window", None) for d in self.decoders]
        if any(w is None for w in windows):
            return
        for s in self.book.live():
            self.allocator.release_behind(s, self.book.pos[s] - max(windows) + 1, keep_pages=self._keep_pages())

    def _replayed(self) -> None:
        """Behind every replay of run(): a subclass's stream-ordered device work (no synchronisation)."""

    def _sync(self) -> list[int]:
        return self.book.update(self.pos.cpu().numpy(), self.sampler.generated())

    def tokens(self, slot: int) -> list[int]:
        """The token ids the slot's sequence has produced so far (since its admission)."""
        n = int(self.sampler.generated()[slot])
        return self.sampler.out_log[slot, :n].cpu().numpy().tolist()

    def logprobs(self, slot: int) -> np.ndarray:
        """fp32, one value per token of tokens(slot): the token's log-probability under the raw logits it was drawn from (logprob_reference's definition; the token
        sampled at admission included).  Needs logprobs=True."""
        if not self.sampler.logprobs:
            raise ValueError("logprobs: the generator was built without logprobs=True")
        n = int(self.sampler.generated()[slot])
        return self.sampler.out_logprob[slot, :n].cpu().numpy()

    def release(self, slot: int) -> list[int]:
        """The slot is free again: its position word is -1 and (paged) its pages go back to the pool; returns them."""
        self.pos[slot] = -1
        if self.lora is not None:
            self.lora.set_slot(slot, None)
        self.book.clear(slot)
        return self.allocator.release(slot) if self.allocator is not None else []

    def violations(self) -> int:
        """Rows the sampler found in an invalid constraint state (Sampler.violations; 0 without constraints=True)."""
        return self.sampler.violations()

    def embed_violations(self) -> int:
        """Token ids tce_embed_rows_f16 refused since the workspace was made (0 unless something wrote next_token from outside)."""
        return int(self.sampler.workspace[:4].cpu().numpy().view(np.uint32)[0])


class BatchedGenerator(_GeneratorBase):
    """decoders: one PagedBatchedDecoder per layer over ONE PageAllocator, or one BatchedDecoder per layer.  final_gamma fp32 [hidden], lm_head a Linear_half_int4
    [vocab][hidden], embed_table fp16 [vocab][hidden] (the reference's fp32 table rounded once).  graph=True captures the token step once (at construction, every row
    inactive) and run() replays it: one replay is one token for every live slot."""

    def __init__(self, decoders, final_gamma, lm_head, embed_table, max_new: int, eps: float | None = None, top_k_bound: int = 40, stop_ids=(), graph: bool = True,
                 debug: bool = False, logprobs: bool = False, constraints: bool = False, lora=None, stages: bool = False, mirostat_rows: bool = False):
        """stages=True: the sampler runs tce_sample_stages_f16 and every admission's SamplingParams may carry its own tfs_z / typical_p (Sampler).  mirostat_rows=True
        (implies stages): the sampler runs tce_sample_mirostat_f16 and an admission's SamplingParams may carry mirostat 1 or 2 with its tau / eta; the slot's mu starts at
        2 * tau and lives on the device, so a replay moves it with no host round trip and no admission captures again.  lora: the LoraPool whose layer views the decoders were built with (decoder i: lora=pool.layer(i)); None: the base model, every launch as before.  A
        gate_up=True pool adapts gate/up too (15 L + 5 launches per token instead of 13 L + 5).  lm_head and the embedding are not adapted."""
        super().__init__(decoders, final_gamma, lm_head, embed_table, max_new, eps, top_k_bound, stop_ids, debug=debug, logprobs=logprobs, constraints=constraints, stages=stages,
                         mirostat_rows=mirostat_rows)
        self._take_pool(lora)
        self.score_keep_logits = False  # a debug hook (tests): score() keeps a copy of every chunk's logits in score_logits, the last chunk's last
        self.score_logits: list = []
        self.launches_per_token = 1 + self.decoders[0].LAUNCHES * len(self.decoders) + 1 + 1 + 2
        if graph:
            self._capture()

    # ---- one token for every live row ----
    def token_step(self) -> None:
        embed_rows(self.embed_table, self.sampler.next_token, self.hidden, self.pos, self.pos_bound, self.sampler.workspace)
        for d in self.decoders:
            d.step(self.hidden, self.pos, self.pos_bound)
        self._head(self.hidden, self.pos, self.xn, self.logits)

    # ---- scoring ----
    def free_slots(self) -> list[int]:
        """Slots that are neither live nor still holding pages."""
        return [s for s in range(self.batch) if self.book.pos[s] < 0 and not (self.allocator is not None and self.allocator.pages[s])]

    def score(self, prompts, chunk_rows: int = 256, adapter: int | None = None) -> list[np.ndarray]:
        """For each prompt of n tokens the n - 1 values logprob(token[i + 1] | token[.. i]) (fp32; empty for a 1-token prompt), logprob_reference's definition on the
        logits this call produces.  The prompts take free slots and pages, all or nothing (PagePoolExhausted, or ValueError when there are fewer free slots than
        prompts: nothing changed), are embedded and run through every layer by ONE prefill_many; then, in chunks of at most chunk_rows rows: final norm -> lm_head at
        M = chunk -> tce_logprobs_f16 with the next tokens as targets (-1 for a prompt's last row), so at most chunk_rows * ld * 2 bytes of logits exist and none leave
        the device.  Slots and pages are released afterwards; ONE synchronise.  Live sequences are not disturbed.  Paged decoders only (fp16 or fp8_e4m3 pages).
        adapter (lora=pool generators): ALL the prompts are scored under that adapter of the pool (None: the base model); the slots' words are -1 again afterwards."""
        import torch
        from .linear import _stream, rmsnorm_half
        if self.allocator is None:
            raise ValueError("score: paged decoders only")
        if adapter is not None and (self.lora is None or int(adapter) != adapter or not 0 <= int(adapter) < self.lora.max_adapters):
            raise ValueError("score: adapter= needs a generator built with lora=pool and an index of that pool")
        plan = score_plan(prompts, self.free_slots(), self.max_keys, self.vocab, chunk_rows)
        prompts, work, slots = plan["prompts"], plan["work"], plan["slots"]
        if not work:
            return plan["split"](np.zeros(0, np.float32))
        self.allocator.reserve_many(plan["reserve"])  # all or nothing, before anything changes
        try:
            tok = torch.tensor(plan["tokens"], dtype=torch.int32).to(self.device)
            target = torch.tensor(plan["targets"], dtype=torch.int32).to(self.device)
            total = tok.numel()
            hidden = torch.empty((total, self.hidden_size), dtype=torch.float16, device=self.device)
            embed_rows(self.embed_table, tok, hidden, torch.zeros(total, dtype=torch.int32, device=self.device), 0, self.sampler.workspace)
            rows, r0 = [], 0
            for i in work:
                rows.append(hidden[r0:r0 + len(prompts[i])])
                r0 += len(prompts[i])
            if self.lora is not None:  # every slot it uses, -1 included, as admit does: nothing is assumed of a free slot's word
                for s in slots:
                    self.lora.set_slot(s, adapter)
            for d in self.decoders:
                d.prefill_many([(s, r, 0) for s, r in zip(slots, rows)])
            chunk = plan["chunk"]
            ld = self.lm_head.out_features
            xn = torch.empty((chunk, self.hidden_size), dtype=torch.float16, device=self.device)
            logits = torch.empty((chunk, ld), dtype=torch.float16, device=self.device)
            partials = torch.empty(int(capi.lib().tce_logprobs_workspace_bytes(chunk, self.vocab)), dtype=torch.uint8, device=self.device)
            values = torch.empty(total, dtype=torch.float32, device=self.device)
            self.score_logits = []
            for r0, m in plan["chunks"]:
                rmsnorm_half(hidden[r0:r0 + m], self.final_gamma, self.eps, out=xn[:m])
                capi.check(capi.w4a16_forward(self.lm_head.desc(xn[:m], logits[:m]), _stream()))
                capi.check(capi.logprobs_f16(logits.data_ptr(), ld, self.vocab, m, target[r0:].data_ptr(), values[r0:].data_ptr(), None, partials.data_ptr(), _stream()))
                if self.score_keep_logits:
                    self.score_logits.append(logits[:m].clone())
        finally:
            for s in slots:
                self.allocator.release(s)
                if self.lora is not None:
                    self.lora.set_slot(s, None)
        return plan["split"](values.cpu().numpy())  # (synchronises)


class HostDrivenLoop:
    """The same decoders driven from the host, greedy: every token the logits [B][vocab] are copied to the host, the lowest-id argmax is taken in numpy, the row is
    looked up in a host copy of the table and copied back.  A device synchronise and two copies per token -- what a caller had to do before tce_sample_f16 /
    tce_embed_rows_f16; the yardstick of tests/test_gpu_generate.py and scripts/generate_time.py."""

    def __init__(self, decoders, final_gamma, lm_head, embed_table, eps: float | None = None, stop_ids=()):
        import torch
        self.decoders = list(decoders)
        d0 = self.decoders[0]
        self.batch, self.allocator = d0.batch, getattr(d0, "allocator", None)
        self.max_keys = d0.attention.max_keys
        self.pos_bound = self.max_keys - 1
        self.final_gamma, self.lm_head = final_gamma, lm_head
        self.eps = d0.block.eps if eps is None else eps
        self.table_host = embed_table.cpu()
        self.vocab = embed_table.shape[0]
        dev = embed_table.device
        self.device = dev
        self.hidden = torch.zeros((self.batch, d0.block.hidden), dtype=torch.float16, device=dev)
        self.xn = torch.zeros_like(self.hidden)
        self.logits = torch.zeros((self.batch, lm_head.out_features), dtype=torch.float16, device=dev)
        self.pos_host = np.full(self.batch, -1, np.int32)
        self.pos = torch.from_numpy(self.pos_host.copy()).to(dev)
        self.next_token = np.zeros(self.batch, np.int64)
        self.out: list[list[int]] = [[] for _ in range(self.batch)]
        self.max_new = [0] * self.batch
        self.stop_ids = set(int(s) for s in stop_ids)

    def _argmax(self, rows_hidden) -> np.ndarray:
        from .linear import _stream, rmsnorm_half
        rmsnorm_half(rows_hidden, self.final_gamma, self.eps, out=self.xn)
        capi.check(capi.w4a16_forward(self.lm_head.desc(self.xn, self.logits), _stream()))
        lg = self.logits.cpu().numpy()[:, :self.vocab].astype(np.float32)  # (synchronises)
        return np.argmax(lg, axis=1)  # the first maximum = the lowest id

    def _take(self, slot: int, tok: int) -> None:
        self.out[slot].append(tok)
        self.next_token[slot] = tok
        if tok in self.stop_ids or len(self.out[slot]) >= self.max_new[slot]:
            self.pos_host[slot] = -1
        else:
            self.pos_host[slot] += 1

    def admit(self, slot, prompt_ids=None, max_new: int | None = None) -> None:
        """admit(slot, prompt_ids, max_new) or admit([(slot, prompt_ids, max_new), ...]): the prefill launches BatchedGenerator.admit makes for the same call (several
        sequences of a paged cache through one prefill_many), the first token chosen on the host."""
        import torch
        adm = slot if prompt_ids is None else [(slot, prompt_ids, max_new)]
        adm = [(int(s), [int(t) for t in ids], int(mn)) for s, ids, mn in adm]
        rows = [self.table_host[torch.tensor(ids, dtype=torch.int64)].to(self.device).contiguous() for _, ids, _ in adm]
        for d in self.decoders:
            d.prefill_many([(s, r, 0) for (s, _, _), r in zip(adm, rows)])
        last = torch.zeros_like(self.hidden)
        for (s, _, _), r in zip(adm, rows):
            last[s].copy_(r[-1])
        tok = self._argmax(last)
        for s, ids, mn in adm:
            self.out[s], self.max_new[s] = [], mn
            self.pos_host[s] = len(ids) - 1
            self._take(s, int(tok[s]))

    def step(self) -> None:
        import torch
        live = [s for s in range(self.batch) if self.pos_host[s] >= 0]
        if self.allocator is not None:
            for s in live:
                self.allocator.reserve(s, int(self.pos_host[s]))
        self.pos.copy_(torch.from_numpy(self.pos_host))
        rows = self.table_host[torch.from_numpy(self.next_token)]
        self.hidden.copy_(rows)  # host -> device
        for d in self.decoders:
            d.step(self.hidden, self.pos, self.pos_bound)
        tok = self._argmax(self.hidden)
        for s in live:
            self._take(s, int(tok[s]))

    def release(self, slot: int) -> None:
        self.pos_host[slot] = -1
        if self.allocator is not None:
            self.allocator.release(slot)
