"""Speculative decoding on the paged generator: T rows per sequence and step -- the certain next token plus up to T - 1 guessed continuations -- through the layers
at once, and a verifier that emits every token the plain loop (generate.py) would have emitted.

A decode token is a chain of dependent launches (7 L + 5) and memory round trips that no kernel can shorten from inside.  Here the chain is
spread over up to T tokens of the SAME sequence: the linears run at M = B T and still stream their weights once, the launch count does not change.

    1        tce_draft_ngram              rows (token, position) per sequence: row 0 = the next input, rows 1 .. = what followed the last occurrence of the
                                          sequence's most recent n-gram in its own history (prompt lookup; no second model)
    1        tce_embed_rows_f16           B T rows (inactive rows skipped)
    7 x L    the layers                   SpeculativeDecoder: BatchedDecoder.step's seven launches at B T rows, tce_attention_decode_step_paged_rows_* as launch 3
                                          (lora=: + 6 per layer, + 8 with a gate_up=True pool; the T rows of a slot carry the slot's adapter word)
    1        tce_rmsnorm_half             the final norm
    1        tce_w4a16_forward            lm_head at M = B T
    3        tce_sample_verify_f16        select for all rows, draw per row, walk the chain: 1 .. T tokens per sequence
                                          (stages=True: tce_sample_verify_stages_f16 -- the same three launches with the sequence's tail-free / typical pair on every row)
                                          (mirostat_rows=True: tce_sample_verify_mirostat_f16 -- FOUR launches: a mirostat sequence's rows are walked in order with mu carried)

LOSSLESS by construction: row t is sampled with the window and the Philox counter (seed, index of the token in its sequence) the plain loop would use, and a draft is
kept only if it EQUALS the token sampled in front of it.  There is no draft distribution and no rejection sampling; draft models and tree drafts are not built.

    ngram_draft_reference, verify_reference   the two device pieces restated in numpy (verify_reference from sample_reference, ring_window and uniform only)
    SpecSlotBook                              which pages run(n) must reserve: positions up to p + n T - 1, whatever the budget (rejected rows are written too)
    SpeculativeDecoder                        PagedBatchedDecoder at B T rows
    SpeculativeGenerator                      BatchedGenerator's surface (admit / run / tokens / logprobs / release: one base class) + rows_per_seq, ngram, emitted_per_step()
    HostDrivenSpeculativeLoop                 the same decoders and launches run eagerly, logits to the host, drafts / sampling / acceptance in numpy: the yardstick
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import capi
from .linear import _stream, rmsnorm_half
from .paged_kv import PagedBatchDecodeAttention, PagedBatchedDecoder
from .generate import RING, Sampler, SamplingParams, SlotBook, _GeneratorBase, embed_rows, ring_window, sample_reference, uniform

MAX_ROWS = capi.TCE_SPEC_MAX_ROWS


def _check_rows(rows_per_seq: int, ngram: int = 1) -> None:
    if not 1 <= int(rows_per_seq) <= MAX_ROWS:
        raise ValueError(f"rows_per_seq {rows_per_seq}: 1 .. {MAX_ROWS} (tree drafts and longer chains are not built)")
    if not 1 <= int(ngram) <= 4:
        raise ValueError(f"ngram {ngram}: 1 .. 4")


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the two device pieces in numpy
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def ngram_draft_reference(history, p: int, ngram: int, rows_per_seq: int, pos_bound: int, script=None) -> tuple[np.ndarray, np.ndarray]:
    """tce_draft_ngram for one sequence: history[i] = the token processed at position i (valid up to index p), p its position.  Returns (row_token, row_pos), int32
    [rows_per_seq]; an inactive row is (0, -1).  script (a test hook): row t >= 1 takes script[p + t]; the first negative value ends the prefix."""
    _check_rows(rows_per_seq, ngram)
    T = int(rows_per_seq)
    tok, pos = np.zeros(T, np.int32), np.full(T, -1, np.int32)
    h = np.asarray(history, dtype=np.int64).reshape(-1)
    if p < 0 or p > pos_bound or p >= h.size:
        return tok, pos
    tok[0], pos[0] = h[p], p
    if script is not None:
        sc = np.asarray(script, dtype=np.int64).reshape(-1)
        for t in range(1, T):
            if p + t > pos_bound or p + t >= sc.size or sc[p + t] < 0:
                break
            tok[t], pos[t] = sc[p + t], p + t
        return tok, pos
    n = int(ngram)
    if p < n:
        return tok, pos
    best = -1
    for i in range(n - 1, p):
        if np.array_equal(h[i - n + 1:i + 1], h[p - n + 1:p + 1]):
            best = i  # (ascending: the most recent match stays)
    if best < 0:
        return tok, pos
    for t in range(1, T):
        if best + t > p or p + t > pos_bound:
            break
        tok[t], pos[t] = h[best + t], p + t
    return tok, pos


def verify_reference(logit_rows, drafts, ring, pushed: int, generated: int, params: SamplingParams, seed: int, stop_ids, max_new: int, uniforms=None,
                     log_stride: int | None = None) -> dict:
    """tce_sample_verify_f16 for one sequence: logit_rows fp16 [n][vocab] are its n active rows, drafts[t] the token row t + 1 was fed (n - 1 of them).  Row t is
    sampled as the plain loop samples token `generated + t`: the window of the ring with y_0 .. y_{t-1} pushed, the uniform keyed (seed, generated + t) -- or
    uniforms[t], a test hook.  Returns tokens (1 .. n of them), ring / pushed / generated after them, retired (a stop id or the budget) and accepted (the drafts kept)."""
    ring = np.array(ring, dtype=np.int32).copy()
    assert ring.shape == (RING,)
    n = len(logit_rows)
    drafts = [int(d) for d in drafts]
    assert n >= 1 and len(drafts) >= n - 1
    stop = {int(s) for s in stop_ids}
    pushed, generated = int(pushed), int(generated)
    tokens, retired = [], False
    for t in range(n):
        u = uniforms[t] if uniforms is not None else uniform(seed, generated)
        y = int(sample_reference(logit_rows[t], ring_window(ring, pushed, params.repeat_last_n), params, u)["token"])
        tokens.append(y)
        ring[pushed % RING] = y
        pushed += 1
        generated += 1
        if y in stop or generated >= max_new or (log_stride is not None and generated >= log_stride):
            retired = True
            break
        if t + 1 >= n or drafts[t] != y:
            break
    return {"tokens": tokens, "ring": ring, "pushed": pushed, "generated": generated, "retired": retired, "accepted": len(tokens) - 1}


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# host bookkeeping
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
class SpecSlotBook(SlotBook):
    """SlotBook for steps of rows_per_seq rows: a replay appends rows p .. p + T - 1 of a live slot whatever it then accepts -- rejected rows are written too and stay
    behind the position --, and moves p by 1 .. T.  So n replays can touch every key up to p + n T - 1, and the reservation does not depend on the budget."""

    def __init__(self, batch: int, max_keys: int, rows_per_seq: int):
        _check_rows(rows_per_seq)
        super().__init__(batch, max_keys)
        self.rows_per_seq = int(rows_per_seq)

    def wanted(self, n: int) -> list[tuple[int, int]]:
        return [(s, min(self.pos[s] + n * self.rows_per_seq - 1, self.max_keys - 1)) for s in self.live()]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the layers at B T rows
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _check_rows_window(who: str, allocator, rows_per_seq: int, window, sinks) -> None:
    """The two rules a rows attention object has beside PagedBatchDecodeAttention's: sinks need window >= rows_per_seq (the C entry point's rule: no key a call appends
    is then a sink key), and with a window -- with or without sinks -- every path is a device path, so the allocator's block table must be on the device."""
    if sinks is not None and window is not None and int(window) < int(rows_per_seq):
        raise ValueError(f"{who}: window {window} < rows_per_seq {rows_per_seq} beside attention sinks (sinks={sinks}): the multi-row sink step needs window >= rows_per_seq")
    if window is not None and not allocator.table.is_cuda:
        # (the unwindowed form may be built over a host table for bookkeeping tests; with a window every path of the class -- step, table_violations -- is a
        # device path, and a host table would only fail later, inside a launch wrapper)
        raise ValueError(f"{who}: a window{'' if sinks is None else ' beside attention sinks (sinks=' + str(sinks) + ')'} needs the allocator's block table on the device")


def rows_check_calls(n_active, last_pos, rows_per_seq: int, window: int | None, sinks: int | None = None) -> list[tuple[int | None, list[int]]]:
    """The table checks that cover a rows step: per sequence n_active[b] rows at consecutive positions that end at last_pos[b] (n_active 0: inactive).  Returns
    [(window argument, position words [batch])]: one tce_kv_block_table_check call each (window None: the unwindowed check), -1 for the sequences a call leaves out.
    Unwindowed rows follow words 0 .. last // page_keys: the check at the last position.  Windowed rows p .. p + n - 1 follow the union of
    [max(0, p + t - W + 1) // page_keys, (p + t) // page_keys], t < n -- contiguous, from row 0's first word to row n - 1's last --, which is what
    tce_kv_block_table_check_window follows for position p + n - 1 with window W + n - 1: one call per distinct n.
    sinks = S (beside a window): the same calls, each a tce_kv_block_table_check_sink with sinks S.  At position p + n - 1 with window W + n - 1 that check binds iff
    p >= S + W -- iff row 0 binds, hence iff every row does -- and then follows word 0 and words (p - W + 1) // page_keys .. (p + n - 1) // page_keys: exactly the union
    the rows follow.  Otherwise it follows words 0 .. (p + n - 1) // page_keys, a SUPERSET of the rows' words where the later rows bind -- sound, because nothing behind
    page 0 can have been given back before position S + W (tests/test_sink_rows_host.py holds both against an enumeration)."""
    _check_rows(rows_per_seq)
    n_active, last_pos = [int(n) for n in n_active], [int(p) for p in last_pos]
    assert len(n_active) == len(last_pos) and all(0 <= n <= rows_per_seq for n in n_active)
    if window is None:
        assert sinks is None, "sinks exist beside a window"
        return [(None, [p if n else -1 for n, p in zip(n_active, last_pos)])]
    return [(int(window) + n - 1, [p if m == n else -1 for m, p in zip(n_active, last_pos)]) for n in sorted(set(n_active) - {0})]


class PagedRowsDecodeAttention(PagedBatchDecodeAttention):
    """PagedBatchDecodeAttention whose step takes rows_per_seq rows per sequence (tce_attention_decode_step_paged_rows_f16 / _fp8): a workspace slice per virtual
    row; prefill and the copies are the parent's.  window=W: tce_attention_decode_step_paged_rows_window_f16 / _fp8 -- row t of a sequence at position p weighs keys
    max(0, p + t - W + 1) .. p + t, the call's own rows among them from the call itself.  Rejected drafts leave pool rows beyond the accepted position: the next
    call's rows start AT that position and take every key from there on from their own q/k/v rows, and each appends its own row, so a stale row is overwritten
    before any row weighs it -- with a window as without.  window=W, sinks=S (W >= rows_per_seq): tce_attention_decode_step_paged_rows_sink_f16 / _fp8 -- each row
    binds or not by its own position p + t >= S + W; a binding row weighs keys 0 .. S - 1 beside its window."""

    def __init__(self, allocator, heads, kv_heads, device, cos=None, sin=None, rows_per_seq: int = 1, **kw):
        _check_rows(rows_per_seq)
        _check_rows_window("PagedRowsDecodeAttention", allocator, rows_per_seq, kw.get("window"), kw.get("sinks"))
        super().__init__(allocator, heads, kv_heads, device, cos, sin, **kw)
        self.rows_per_seq = int(rows_per_seq)
        need = int(capi.lib().tce_attention_decode_batch_workspace_bytes(self.batch * self.rows_per_seq, heads, self.max_keys, self.hd))
        if need == 0:
            raise ValueError("unsupported batched attention shape")
        self.workspace = torch.zeros(need, dtype=torch.uint8, device=device)  # zeroed once
        self.slot_workspace_bytes = need // (self.batch * self.rows_per_seq)

    def step(self, qkv, pos_device, pos_bound: int, out=None):
        """qkv fp16 [batch * T][(heads + 2 kv_heads) * 128], pos_device int32 [batch * T]: the ROWS' positions (a prefix p, p + 1, ... per sequence, -1 behind
        it).  One launch."""
        return self._step(self._entry("tce_attention_decode_step_paged_rows"), self.rows_per_seq, qkv, pos_device, pos_bound, out)

    def table_violations(self, pos_device, pos_bound: int) -> int:
        """The table check for a rows step: pos_device int32 [batch * T], the ROWS' positions as step() takes them.  The words the step would follow that are not page
        numbers (0: sound), through rows_check_calls; waited for."""
        assert pos_device.dtype == torch.int32 and pos_device.numel() == self.batch * self.rows_per_seq
        rp = pos_device.view(self.batch, self.rows_per_seq).cpu().numpy()
        active = (rp >= 0) & (rp <= pos_bound)
        last = np.where(active, rp, -1).max(axis=1)
        tab, stride, pk, n = self._table_args()
        bad = 0
        for w, words in rows_check_calls(active.sum(axis=1), last, self.rows_per_seq, self.window, self.sinks):
            pos = torch.tensor(words, dtype=torch.int32, device=pos_device.device)
            fn = getattr(capi.lib(), self._entry("tce_kv_block_table_check"))
            capi.check(fn(tab, stride, pk, n, self.batch, C.c_void_p(pos.data_ptr()), int(pos_bound), C.c_void_p(self._violations.data_ptr()),
                          *(() if w is None else ((w,) if self.sinks is None else (w, self.sinks))), C.c_void_p(_stream())))
            bad += int(self._violations.item())
        return bad


class SpeculativeDecoder(PagedBatchedDecoder):
    """PagedBatchedDecoder whose step runs batch * rows_per_seq rows: the same seven launches (BatchedDecoder.step: hidden fp16 [batch * T][hidden], the position
    words tce_draft_ngram's row_pos int32 [batch * T]), the rows step as launch 3.  fp16 and fp8_e4m3 pages.  prefill / prefill_many are the parent's.  window: this
    layer's sliding window (the windowed rows step and the windowed prefill), None for full attention.  sinks: this layer's attention sinks beside the window (the
    rows-sink step and the sink prefill; window >= rows_per_seq), None for none; reported as .sinks."""

    def __init__(self, block, allocator, rows_per_seq: int, kv_dtype: str = "fp16", k_scale_log2: int = 0, v_scale_log2: int = 0, window: int | None = None, lora=None,
                 sinks: int | None = None):
        """lora: this layer's view of a LoraPool built with the same rows_per_seq (LoraPool(..., rows_per_seq=T).layer(i)): the T rows of a slot run on the slot's
        adapter -- 7 + 6 launches, 7 + 8 with a gate_up=True pool."""
        _check_rows(rows_per_seq)
        _check_rows_window("SpeculativeDecoder", allocator, rows_per_seq, window, sinks)  # (before `block` is touched)
        self.rows_per_seq = int(rows_per_seq)
        attention = PagedRowsDecodeAttention(allocator, block.heads, block.kv_heads, block.gamma1.device, block.attention.cos, block.attention.sin,
                                             rows_per_seq=rows_per_seq, kv_dtype=kv_dtype, k_scale_log2=k_scale_log2, v_scale_log2=v_scale_log2, window=window, sinks=sinks)
        super().__init__(block, allocator, attention=attention, rows=allocator.batch * self.rows_per_seq, lora=lora)


def draft_ngram(history, script, pos_device, pos_bound: int, rows_per_seq: int, ngram: int, row_token, row_pos) -> None:
    """tce_draft_ngram (one launch on the current stream): history / script int32 [batch][hist_stride] (script may be None), pos_device int32 [batch]."""
    for t in (history, pos_device, row_token, row_pos) + ((script,) if script is not None else ()):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda
    batch = pos_device.numel()
    assert history.dim() == 2 and history.shape[0] == batch and row_token.numel() == row_pos.numel() == batch * rows_per_seq
    assert script is None or tuple(script.shape) == tuple(history.shape)
    capi.check(capi.lib().tce_draft_ngram(history.data_ptr(), script.data_ptr() if script is not None else None, history.shape[1], pos_device.data_ptr(), int(pos_bound),
                                          batch, int(rows_per_seq), int(ngram), row_token.data_ptr(), row_pos.data_ptr(), _stream()))


class Verifier:
    """tce_sample_verify_f16 over a Sampler's per-sequence state: the workspace for batch * rows_per_seq rows and `emitted`.  A Sampler built with logprobs=True:
    tce_sample_verify_logprobs_f16 -- the same three launches --, which writes the sampler's out_logprob beside every emitted token (partials for batch * rows_per_seq
    rows live here)."""

    def __init__(self, sampler: Sampler, rows_per_seq: int, debug: bool = False):
        _check_rows(rows_per_seq)
        self.sampler, self.rows_per_seq = sampler, int(rows_per_seq)
        dev = sampler.rows.device
        size = capi.lib().tce_sample_verify_mirostat_workspace_bytes if getattr(sampler, "mirostat_rows", False) else capi.lib().tce_sample_verify_workspace_bytes
        need = int(size(sampler.batch, self.rows_per_seq, sampler.vocab))
        if need == 0:
            raise ValueError("unsupported verify shape (batch * rows_per_seq <= 65535, vocab <= 2^20)")
        self.workspace = torch.zeros(need, dtype=torch.uint8, device=dev)
        self.emitted = torch.zeros(sampler.batch, dtype=torch.int32, device=dev)
        self.uniform_override = None  # fp32 [batch * rows_per_seq] on the device (tests)
        self.debug = torch.zeros((sampler.batch * self.rows_per_seq, C.sizeof(capi.SampleDebug) // 4), dtype=torch.int32, device=dev) if debug else None
        self.partials = None
        self.sdebug = None  # a Sampler built with stages=True: tce_sample_verify_stages_f16, the stage records per virtual row
        if sampler.stages and debug:
            self.sdebug = torch.zeros((sampler.batch * self.rows_per_seq, C.sizeof(capi.StageDebug) // 4), dtype=torch.int32, device=dev)
        self.mdebug = None  # a Sampler built with mirostat_rows=True: tce_sample_verify_mirostat_f16 (four launches), the mirostat records per virtual row
        if getattr(sampler, "mirostat_rows", False) and debug:
            self.mdebug = torch.zeros((sampler.batch * self.rows_per_seq, C.sizeof(capi.MirostatDebug) // 4), dtype=torch.int32, device=dev)
        if sampler.logprobs:
            self.partials = torch.empty(int(capi.lib().tce_logprobs_workspace_bytes(sampler.batch * self.rows_per_seq, sampler.vocab)), dtype=torch.uint8, device=dev)

    def step(self, logits, row_token, row_pos, history, pos_device, pos_bound: int) -> None:
        """logits fp16 [batch * T][ld]; pos_device int32 [batch] (the sequences' positions) is read and written; three launches on the current stream."""
        s = self.sampler
        n = s.batch * self.rows_per_seq
        assert logits.dtype == torch.float16 and logits.is_contiguous() and logits.dim() == 2 and logits.shape[0] == n and logits.shape[1] >= s.vocab and logits.is_cuda
        for t, m in ((row_token, n), (row_pos, n), (pos_device, s.batch)):
            assert t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda and t.numel() == m
        assert history.dtype == torch.int32 and history.is_contiguous() and history.is_cuda and history.dim() == 2 and history.shape[0] == s.batch
        c = s.call(logits.data_ptr(), logits.shape[1], pos_device.data_ptr(), pos_bound)
        c.workspace = self.workspace.data_ptr()
        c.uniform_override = self.uniform_override.data_ptr() if self.uniform_override is not None else None
        c.debug = self.debug.data_ptr() if self.debug is not None else None
        v = capi.SampleVerifyCall(s=c, rows_per_seq=self.rows_per_seq, hist_stride=history.shape[1], row_token=row_token.data_ptr(), row_pos=row_pos.data_ptr(),
                                  history=history.data_ptr(), emitted=self.emitted.data_ptr())
        if getattr(s, "mirostat_rows", False):
            st = capi.SampleStages(rows=s.srows.data_ptr(), debug=self.sdebug.data_ptr() if self.sdebug is not None else None)
            mi = capi.SampleMirostat(rows=s.mrows.data_ptr(), debug=self.mdebug.data_ptr() if self.mdebug is not None else None)
            capi.check(capi.sample_verify_mirostat_f16(v, st, mi, s.constraint() if s.constraints else None, s.logprob_out(self.partials) if s.logprobs else None, _stream()))
        elif s.stages:
            st = capi.SampleStages(rows=s.srows.data_ptr(), debug=self.sdebug.data_ptr() if self.sdebug is not None else None)
            capi.check(capi.sample_verify_stages_f16(v, st, s.constraint() if s.constraints else None, s.logprob_out(self.partials) if s.logprobs else None, _stream()))
        elif s.constraints:
            capi.check(capi.sample_verify_constrained_f16(v, s.constraint(), s.logprob_out(self.partials) if s.logprobs else None, _stream()))
        elif s.logprobs:
            capi.check(capi.sample_verify_logprobs_f16(v, s.logprob_out(self.partials), _stream()))
        else:
            capi.check(capi.sample_verify_f16(v, _stream()))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the front
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
class SpeculativeGenerator(_GeneratorBase):
    """decoders: one SpeculativeDecoder per layer over ONE PageAllocator, all with the same rows_per_seq.  The token step is captured once in one torch.cuda.graph;
    one replay is 1 .. rows_per_seq tokens per live sequence.  script=True (a test hook) allocates `script` int32 [batch][hist_stride], -1 everywhere, which then
    REPLACES the n-gram lookup: row t of a sequence at position p is fed script[b][p + t].  admit / tokens / logprobs / release are BatchedGenerator's.
    Decoders with sliding windows: as in BatchedGenerator, run() gives back the pages wholly behind every layer's window around each burst.  Row 0 of the next
    replay sits at the synced position p and needs keys from p - W + 1 on, later rows and later replays only later keys, so SpecSlotBook.wanted and _release_behind
    are the plain loop's; a slot holds at most ceil((max W + n T) / page_keys) + 1 + keep_pages pages through run(n).  Decoders with attention sinks (SpeculativeDecoder(...,
    window=W, sinks=S)): the base class keeps the sinks' page (keep_pages = 1) beside the window's."""

    def __init__(self, decoders, final_gamma, lm_head, embed_table, max_new: int, ngram: int = 2, eps: float | None = None, top_k_bound: int = 40, stop_ids=(),
                 graph: bool = True, script: bool = False, record_steps: int = 4096, logprobs: bool = False,
                 constraints: bool = False, lora=None, stages: bool = False, mirostat_rows: bool = False):
        if lora is not None:  # first: a pool that was not built for rows, or for another T, is refused before anything else of the constructor runs
            T = getattr(lora, "rows_per_seq", None)
            decoders = list(decoders) if T is not None and decoders is not None else None
            if T is None or not decoders or T != getattr(decoders[0], "rows_per_seq", None):
                raise ValueError(f"SpeculativeGenerator: lora= takes a pool built for its speculative rows, LoraPool(..., rows_per_seq=T) with the decoders' T "
                                 f"(this pool: rows_per_seq={T})")
        decoders = list(decoders)
        for d in decoders:  # a layer with sinks must run the ROWS sink step: its attention object carries the count (SpeculativeDecoder(..., window=W, sinks=S) builds it so)
            sk = getattr(d, "sinks", None)
            if sk is not None and getattr(getattr(d, "attention", None), "sinks", None) != sk:
                raise ValueError(f"SpeculativeGenerator: a decoder reports sinks {sk} but its attention object does not carry them (build the layer as "
                                 f"SpeculativeDecoder(..., window=W, sinks=S))")
        for d in decoders:  # a windowed layer must run the windowed ROWS step: its attention object carries the window (SpeculativeDecoder(..., window=W) builds it so)
            w = getattr(d, "window", None)
            if w is not None and getattr(getattr(d, "attention", None), "window", None) != w:
                raise ValueError(f"SpeculativeGenerator: a decoder reports window {w} but its attention object does not carry it (build the layer as SpeculativeDecoder(..., window=W))")
        self.rows_per_seq, self.ngram = decoders[0].rows_per_seq, int(ngram)
        _check_rows(self.rows_per_seq, self.ngram)
        assert all(d.rows_per_seq == self.rows_per_seq for d in decoders), "one T"
        super().__init__(decoders, final_gamma, lm_head, embed_table, max_new, eps, top_k_bound, stop_ids, rows_per_seq=self.rows_per_seq, logprobs=logprobs,
                         constraints=constraints, stages=stages, mirostat_rows=mirostat_rows)
        self._take_pool(lora)
        B, T, dev = self.batch, self.rows_per_seq, self.device
        self.verifier = Verifier(self.sampler, T)
        self.book = SpecSlotBook(B, self.max_keys, T)
        self.hist_stride = self.max_keys + 8  # (the verifier writes index p + 1 + t <= max_keys)
        z = lambda *shape, fill=0: torch.full(shape, fill, dtype=torch.int32, device=dev)
        self.row_token, self.row_pos = z(B * T), z(B * T, fill=-1)
        self.history = z(B, self.hist_stride)
        self.script = z(B, self.hist_stride, fill=-1) if script else None
        self._emit_log = z(int(record_steps), B)
        self._steps, self._record = 0, True
        self.launches_per_token = 1 + 1 + decoders[0].LAUNCHES * len(decoders) + 1 + 1 + (4 if mirostat_rows else 3)  # (the mirostat verifier walks in a fourth launch)
        if graph:
            self._capture()

    # ---- one step: 1 .. T tokens for every live sequence ----
    def token_step(self) -> None:
        draft_ngram(self.history, self.script, self.pos, self.pos_bound, self.rows_per_seq, self.ngram, self.row_token, self.row_pos)
        embed_rows(self.embed_table, self.row_token, self.hidden, self.row_pos, self.pos_bound, self.sampler.workspace)
        for d in self.decoders:
            d.step(self.hidden, self.row_pos, self.pos_bound)
        rmsnorm_half(self.hidden, self.final_gamma, self.eps, out=self.xn)
        capi.check(capi.w4a16_forward(self.lm_head.desc(self.xn, self.logits), _stream()))
        self.verifier.step(self.logits, self.row_token, self.row_pos, self.history, self.pos, self.pos_bound)

    def _admitted(self, admitted) -> None:
        """The history rows the drafts are looked up in: the prompt, then the first token."""
        first = self.sampler.next_token.cpu().numpy()  # (synchronises)
        for s, ids in admitted:
            row = torch.tensor(ids + [int(first[s])], dtype=torch.int32)
            self.history[s, :row.numel()].copy_(row)

    def set_script(self, slot: int, tokens) -> None:
        """The test hook's row for `slot`: tokens[i] is fed as the draft for position i (-1: no draft from there on); the rest of the row is -1."""
        if self.script is None:
            raise ValueError("set_script: the generator was built without script=True")
        row = np.full(self.hist_stride, -1, np.int32)
        tokens = np.asarray(tokens, np.int32)[:self.hist_stride]
        row[:tokens.size] = tokens
        self.script[slot].copy_(torch.from_numpy(row))

    # ---- running ----
    def run(self, n: int, record: bool = True) -> list[int]:
        """n steps -- n .. n T tokens -- for every live slot: pages for positions up to p + n T - 1 are reserved first (all or nothing: PagePoolExhausted and nothing
        changed), then the step is replayed n times with no host synchronisation, then ONE synchronise.  record: a stream-ordered device copy of `emitted` behind every
        replay, for emitted_per_step() (no synchronisation).  Returns the slots that retired."""
        self._record = record
        return super().run(n)

    def _replayed(self) -> None:
        if self._record and self._steps < self._emit_log.shape[0]:
            self._emit_log[self._steps].copy_(self.verifier.emitted)
            self._steps += 1

    def emitted_per_step(self) -> np.ndarray:
        """int32 [recorded steps][batch]: the tokens every slot emitted in each recorded replay (0: inactive)."""
        return self._emit_log[:self._steps].cpu().numpy()


class HostDrivenSpeculativeLoop:
    """The same decoders and the same M = B T launches run eagerly, driven from the host: drafts (ngram_draft_reference), sampling and acceptance (verify_reference)
    in numpy on logits copied back every step.  The yardstick of tests/test_gpu_speculative.py and scripts/speculative_time.py."""

    def __init__(self, decoders, final_gamma, lm_head, embed_table, ngram: int = 2, eps: float | None = None, stop_ids=()):
        self.decoders = list(decoders)
        d0 = self.decoders[0]
        self.batch, self.allocator, self.rows_per_seq, self.ngram = d0.batch, d0.allocator, d0.rows_per_seq, int(ngram)
        _check_rows(self.rows_per_seq, self.ngram)
        self.max_keys = d0.attention.max_keys
        self.pos_bound = self.max_keys - 1
        self.final_gamma, self.lm_head = final_gamma, lm_head
        self.eps = d0.block.eps if eps is None else eps
        self.table_host = embed_table.cpu()
        self.vocab = embed_table.shape[0]
        dev = embed_table.device
        self.device = dev
        n = self.batch * self.rows_per_seq
        self.hidden = torch.zeros((n, d0.block.hidden), dtype=torch.float16, device=dev)
        self.xn = torch.zeros_like(self.hidden)
        self.logits = torch.zeros((n, lm_head.out_features), dtype=torch.float16, device=dev)
        self.row_pos = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.pos_host = np.full(self.batch, -1, np.int64)
        self.stop_ids = [int(s) for s in stop_ids]
        self.state: list[dict | None] = [None] * self.batch
        self.script: list | None = None  # [batch] rows (or None per slot): replaces the lookup, as SpeculativeGenerator's
        self.emitted: list[list[int]] = []

    def _logits(self, hidden, xn, out) -> np.ndarray:
        rmsnorm_half(hidden, self.final_gamma, self.eps, out=xn)
        capi.check(capi.w4a16_forward(self.lm_head.desc(xn, out), _stream()))
        return out.cpu().numpy()[:, :self.vocab]  # (synchronises)

    def admit(self, admissions) -> None:
        """[(slot, prompt_ids, params, seed, max_new)]: the prefill launches SpeculativeGenerator.admit makes for the same call, the first token sampled on the host."""
        adm = [(int(s), [int(t) for t in ids], p or SamplingParams(), int(sd), int(mn)) for s, ids, p, sd, mn in admissions]
        rows = [self.table_host[torch.tensor(ids, dtype=torch.int64)].to(self.device).contiguous() for _, ids, *_ in adm]
        for d in self.decoders:
            d.prefill_many([(s, r, 0) for (s, *_), r in zip(adm, rows)])
        last = torch.zeros((self.batch, self.hidden.shape[1]), dtype=torch.float16, device=self.device)
        for (s, *_), r in zip(adm, rows):
            last[s].copy_(r[-1])
        lg = self._logits(last, torch.empty_like(last), torch.empty((self.batch, self.logits.shape[1]), dtype=torch.float16, device=self.device))
        for s, ids, p, sd, mn in adm:
            ring = np.zeros(RING, np.int32)
            for i, t in enumerate(ids):
                ring[i % RING] = t
            st = {"params": p, "seed": sd, "max_new": mn, "ring": ring, "pushed": len(ids), "generated": 0, "out": [], "history": list(ids)}
            v = verify_reference(lg[s:s + 1], [], st["ring"], st["pushed"], 0, p, sd, self.stop_ids, mn)
            self._take(s, st, v, len(ids) - 1)
            self.state[s] = st

    def _take(self, slot: int, st: dict, v: dict, p: int) -> None:
        st["ring"], st["pushed"], st["generated"] = v["ring"], v["pushed"], v["generated"]
        st["out"] += v["tokens"]
        st["history"] = st["history"][:p + 1] + v["tokens"]
        self.pos_host[slot] = -1 if v["retired"] else p + len(v["tokens"])

    def step(self) -> None:
        T = self.rows_per_seq
        live = [s for s in range(self.batch) if 0 <= self.pos_host[s] <= self.pos_bound]
        if live:
            self.allocator.reserve_many([(s, min(int(self.pos_host[s]) + T - 1, self.max_keys - 1)) for s in live])
        tok, pos = np.zeros(self.batch * T, np.int64), np.full(self.batch * T, -1, np.int32)
        for s in live:
            sc = self.script[s] if self.script is not None else None
            tok[s * T:(s + 1) * T], pos[s * T:(s + 1) * T] = ngram_draft_reference(self.state[s]["history"], int(self.pos_host[s]), self.ngram, T, self.pos_bound, script=sc)
        self.row_pos.copy_(torch.from_numpy(pos))
        self.hidden.copy_(self.table_host[torch.from_numpy(tok)])  # host -> device
        for d in self.decoders:
            d.step(self.hidden, self.row_pos, self.pos_bound)
        lg = self._logits(self.hidden, self.xn, self.logits)
        emitted = [0] * self.batch
        for s in live:
            st, p = self.state[s], int(self.pos_host[s])
            n = int((pos[s * T:(s + 1) * T] >= 0).sum())
            v = verify_reference(lg[s * T:s * T + n], tok[s * T + 1:s * T + n], st["ring"], st["pushed"], st["generated"], st["params"], st["seed"], self.stop_ids,
                                 st["max_new"])
            self._take(s, st, v, p)
            emitted[s] = len(v["tokens"])
        self.emitted.append(emitted)

    def tokens(self, slot: int) -> list[int]:
        return list(self.state[slot]["out"])

    def release(self, slot: int) -> None:
        self.pos_host[slot] = -1
        self.allocator.release(slot)
