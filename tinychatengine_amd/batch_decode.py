"""Batched decode: B independent sequences per decoder-block step, each at its own position.

The linears already take a batch (tce_w4a16_forward streams the weights once for M rows); the attention step between q/k/v and o_proj is
tce_attention_decode_step_batch_f16: ONE launch for B sequences, each with its own position word, cache slot, q/k/v and output rows and workspace
slice.  Every active row computes, bit for bit, what tce_attention_decode_step_pos_f16 computes for that sequence alone with the same bound; a row
whose position word is < 0 or > pos_bound is inactive (zero output row, caches and counters untouched), so a fixed-B captured graph is a slot pool
in which a finished sequence is retired by writing -1.

A layer is SEVEN launches for the B rows, issued by ONE function, decoder_block.layer_body -- step() runs it on the decoder's persistent rows with the batched step as
launch 3 and _gate_up as launch 6, _prefill_rows (prefill, prefill_many) on per-call rows with the prefill attention and gate_up_by_rule, DecoderBlock.prefill on its own:

    1  input_layernorm                           tce_rmsnorm_half over B rows (the fused RMSNorm prologue is an M = 1 form)
    2  q/k/v projection                          tce_w4a16_forward, M = B
    3  RoPE + KV append + attention              tce_attention_decode_step_batch_f16
    4  o_proj + residual add                     tce_w4a16_forward, M = B, TCE_W4_ADD_TO_C (an inactive row adds exactly 0)
    5  post_attention_layernorm                  tce_rmsnorm_half
    6  gate/up + SiLU*mul                        tce_w4a16_forward, M = B, TCE_W4_SILU_MUL_PAIRS (gate, up and tce_silu_mul_half where the pairs are refused)
    7  down_proj + residual add                  tce_w4a16_forward, M = B, TCE_W4_ADD_TO_C

lora=<a LoraLayer> (lora.py): q/k/v, o_proj and down_proj are ADAPTED linears (layer_body's `linear`) -- tce_lora_shrink_f16 once the linear's input exists,
tce_lora_expand_add_f16 directly behind the base launch, each row on the adapter its row_adapter word names -- 7 + 6 launches.  lora=None: every launch is the one above.
A view of a gate_up=True pool: launch 6 becomes three -- the shrink on xn with gate's and up's A stacked, the gate_up linear WITHOUT the pair flag into [rows][2 * ffn]
and tce_lora_expand_silu_mul_f16 (both deltas in front of the nonlinearity, SiLU * mul for every row) -- 7 + 8 launches.  A pool built with rows_per_seq=T serves the
speculative step: rows = batch * T, a slot's word stands T times in row_adapter.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import capi
from .attention_ops import DecodeAttention
from .decoder_block import DecoderBlock, gate_up_by_rule, gate_up_three, layer_body
from .linear import _stream


class _SlotAttention(DecodeAttention):
    """DecodeAttention over one slot of a BatchDecodeAttention: the slot's caches and workspace slice (views, no copies)."""

    def __init__(self, parent: "BatchDecodeAttention", b: int):  # (no DecodeAttention.__init__: it would allocate caches of its own)
        self.heads, self.hd, self.max_keys, self.kv_heads = parent.heads, parent.hd, parent.max_keys, parent.kv_heads
        self.k_cache, self.v_cache = parent.k_cache[b], parent.v_cache[b]
        self.workspace = parent.workspace[b * parent.slot_workspace_bytes:(b + 1) * parent.slot_workspace_bytes]
        self.cos, self.sin, self.alpha_bits = parent.cos, parent.sin, parent.alpha_bits


class BatchDecodeAttention:
    """The attention step for `batch` sequences: caches [batch][kv_heads][max_keys][128] (slot b is exactly a single-sequence cache), a workspace of
    `batch` single-step workspaces zeroed once, shared RoPE tables."""

    def __init__(self, batch: int, heads: int, max_keys: int, device, cos: torch.Tensor | None = None, sin: torch.Tensor | None = None,
                 kv_heads: int | None = None, head_dim: int = 128):
        self.batch, self.heads, self.hd, self.max_keys = batch, heads, head_dim, max_keys
        self.kv_heads = heads if kv_heads is None else kv_heads
        need = int(capi.lib().tce_attention_decode_batch_workspace_bytes(batch, heads, max_keys, head_dim))
        if need == 0:
            raise ValueError("unsupported batched attention shape (head_dim must be 128, batch > 0)")
        self.slot_workspace_bytes = need // batch
        self.k_cache = torch.zeros((batch, self.kv_heads, max_keys, head_dim), dtype=torch.float16, device=device)
        self.v_cache = torch.zeros((batch, self.kv_heads, max_keys, head_dim), dtype=torch.float16, device=device)
        self.workspace = torch.zeros(need, dtype=torch.uint8, device=device)  # zeroed once: the per-(sequence, head) arrival counters
        self.cos, self.sin = cos, sin
        self.alpha_bits = int(np.array([1.0 / np.sqrt(head_dim)], np.float16).view(np.uint16)[0])

    def step(self, qkv: torch.Tensor, pos_device: torch.Tensor, pos_bound: int, out: torch.Tensor | None = None) -> torch.Tensor:
        """qkv fp16 [batch][(heads + 2 kv_heads) * 128] (the q/k/v linear's output at M = batch), pos_device int32 [batch] on the device (read when the
        kernel runs; every value that is to be active <= pos_bound), out fp16 [batch][heads * 128] (o_proj's input rows)."""
        rw = (self.heads + 2 * self.kv_heads) * self.hd
        assert qkv.dtype == torch.float16 and qkv.is_contiguous() and qkv.is_cuda and qkv.numel() == self.batch * rw
        assert pos_device.dtype == torch.int32 and pos_device.is_cuda and pos_device.is_contiguous() and pos_device.numel() == self.batch
        if out is None:
            out = torch.empty((self.batch, self.heads * self.hd), dtype=torch.float16, device=qkv.device)
        assert out.dtype == torch.float16 and out.is_contiguous() and out.is_cuda and out.numel() == self.batch * self.heads * self.hd
        p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
        capi.check(capi.lib().tce_attention_decode_step_batch_f16(p(qkv), p(self.k_cache), p(self.v_cache), p(self.cos), p(self.sin), p(out), p(self.workspace),
                                                                  self.batch, self.heads, self.kv_heads, self.hd, self.max_keys, p(pos_device), int(pos_bound),
                                                                  self.alpha_bits, C.c_void_p(_stream())))
        return out

    def slot(self, b: int) -> DecodeAttention:
        """A DecodeAttention over slot b's caches and workspace slice: its prefill() admits a sequence into the slot, its step() is the single-sequence yardstick."""
        if not 0 <= b < self.batch:
            raise IndexError(f"slot {b} of {self.batch}")
        return _SlotAttention(self, b)


class BatchedDecoder:
    """`batch` sequences through one decoder block: the linears and gammas of `block` (nothing in the block changes), caches of its own."""

    LAUNCHES = 7  # per layer and step, with the SiLU*mul pairs accepted (9 otherwise); with lora=: 7 + 6 (9 + 6 where the pairs are refused: the figure does not follow _gate_up's fallback);
    # with a gate_up=True pool: 7 + 8 (the adapted gate/up never asks for the pairs)

    def __init__(self, block: DecoderBlock, batch: int, attention=None, rows: int | None = None, lora=None):
        """attention: the step's attention object (default: a BatchDecodeAttention with contiguous caches of its own); rows: the rows one step carries, where that is
        not `batch` (the speculative step's batch * rows_per_seq); lora: this layer's view of a LoraPool (LoraPool.layer(i)), None for the base model alone.  The
        pool's rows_per_seq must be the step's: None for rows == batch, T for rows == batch * T."""
        self.block, self.batch, self.rows = block, batch, batch if rows is None else rows
        self.lora, self._lora_t, self._gate_up_y = lora, None, None
        if lora is not None:
            if self.rows != batch * (lora.pool.rows_per_seq or 1):
                raise ValueError(f"lora: a step of {self.rows} rows for {batch} slots, but the pool was built with rows_per_seq={lora.pool.rows_per_seq} "
                                 "(speculative rows take LoraPool(..., rows_per_seq=T), one row per slot the default pool)")
            lora.pool.bind(batch)  # the shared row_adapter words: one per slot, or one per row of a slot
            self._lora_t = lora.workspace(self.rows)
            self.LAUNCHES = BatchedDecoder.LAUNCHES + (8 if lora.gate_up else 6)
        dev = block.gamma1.device
        self.attention = attention if attention is not None else BatchDecodeAttention(batch, block.heads, block.attention.max_keys, dev, block.attention.cos,
                                                                                      block.attention.sin, kv_heads=block.kv_heads)
        e = lambda n: torch.empty((self.rows, n), dtype=torch.float16, device=dev)
        self.xn, self.qkv_out, self.attn_out = e(block.hidden), e((block.heads + 2 * block.kv_heads) * 128), e(block.hidden)
        self.act = e(block.ffn)
        self._up = None  # gate / up / SiLU*mul as three launches: up's output rows (only where the dispatcher refuses the pairs at M = rows)
        if lora is not None and lora.gate_up:
            self._gate_up_y = e(2 * block.ffn)  # the adapted gate/up: the base linear's pairs, in front of tce_lora_expand_silu_mul_f16

    def step(self, hidden: torch.Tensor, pos_device: torch.Tensor, pos_bound: int) -> None:
        """hidden fp16 [rows][hidden], updated in place (each row is its sequence's residual stream); pos_device int32 [rows], -1 for an inactive slot: its
        attention row is zero and its caches are untouched (its hidden row still passes through the MLP and means nothing).  Capturable in one
        torch.cuda.graph and replayable token after token with pos_device advanced on the device."""
        blk = self.block
        assert hidden.dtype == torch.float16 and hidden.is_contiguous() and tuple(hidden.shape) == (self.rows, blk.hidden)
        layer_body(blk, hidden, self.xn, self.qkv_out, self.attn_out, self.act, lambda qkv, attn: self.attention.step(qkv, pos_device, pos_bound, out=attn),
                   self._gate_up, lora=self.lora, t=self._lora_t, y=self._gate_up_y)  # (row_words None: the pool's own row_adapter, one word per row of the step)

    def _gate_up(self, xn: torch.Tensor, st: int) -> None:
        """The step's gate/up policy: ask for the SiLU*mul pairs, and where the dispatcher refuses them at M = rows fall back to the three launches FOR GOOD."""
        if self._up is None:
            rc = capi.w4a16_forward(self.block.gate_up.desc(xn, self.act, flags=capi.TCE_W4_SILU_MUL_PAIRS), st)
            if rc == capi.TCE_OK:
                return
            if rc == capi.TCE_ERR_HIP:
                capi.check(rc)
            self._up = torch.empty_like(self.act)  # refused before any launch: the three-launch form from now on
        gate_up_three(self.block, xn, self.act, self._up, st)

    def prefill(self, slot: int, rows: torch.Tensor, pos: int) -> None:
        """Admit a sequence into `slot`: rows fp16 [m][hidden] at positions pos .. pos + m - 1, updated in place -- DecoderBlock.prefill's launches on the
        slot's caches."""
        self._prefill_rows(rows, lambda qkv, attn: self.attention.slot(slot).prefill(qkv, pos, out=attn, causal=True), self._row_words([(slot, rows.shape[0])]))

    def prefill_many(self, admissions) -> None:
        """admissions [(slot, rows, pos)]: prefill once per sequence, in order (a contiguous cache takes one sequence per attention call; the paged decoder's
        prefill_many serves them all at M = all rows)."""
        for slot, rows, pos in admissions:
            self.prefill(slot, rows, pos)

    def _row_words(self, segments) -> torch.Tensor | None:
        """The prefill's per-row adapter words for segments [(slot, m)]: every row of an admission carries its SLOT's word, gathered on the device from the shared
        row_adapter tensor (written before the prefill; device-side copies only: nothing is read back and no host tensor is sent over).  None without a pool."""
        if self.lora is None:
            return None
        ra, T = self.lora.row_adapter, self.lora.pool.rows_per_seq or 1  # (a pool built for rows: the slot's FIRST word)
        return torch.cat([ra[slot * T:slot * T + 1].expand(m) for slot, m in segments])

    def _prefill_rows(self, rows: torch.Tensor, attend, row_words: torch.Tensor | None = None) -> None:
        """prefill's launches over `rows` -- layer_body on rows of this call's own; attend(qkv, attn) is the attention in the middle (the paged decoder's serves several
        sequences' rows at once).  row_words (with a pool): int32 [m], the adapter of every row -- the linears are adapted as in step()."""
        blk = self.block
        m = rows.shape[0]
        lora = self.lora if row_words is not None else None
        assert rows.dtype == torch.float16 and rows.is_contiguous() and rows.shape[1] == blk.hidden
        e = lambda n: torch.empty((m, n), dtype=torch.float16, device=rows.device)
        xn, qkv, attn, g, u = e(blk.hidden), e((blk.heads + 2 * blk.kv_heads) * 128), e(blk.hidden), e(blk.ffn), e(blk.ffn)
        t, y = (lora.workspace(m), e(2 * blk.ffn) if lora.gate_up else None) if lora else (None, None)
        layer_body(blk, rows, xn, qkv, attn, g, attend, lambda x, st: gate_up_by_rule(blk, x, g, u, st), lora=lora, t=t, row_words=row_words, y=y)
