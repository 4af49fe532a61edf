"""Paged KV cache for batched decode: keys and values in fixed-size pages drawn from one pool, a block table per sequence.

BatchDecodeAttention reserves [batch][kv_heads][max_keys][128] per K and V and layer: every slot holds max_keys rows for its whole life.  Here a layer holds two
pools [num_pages][kv_heads][page_keys][128] and the attention step (tce_attention_decode_step_paged_f16, csrc/attention_fast.hip) finds logical key j of
sequence b in row j % page_keys of page table[b][j // page_keys].  Memory follows the tokens that exist, a retired sequence's pages go back to the pool, and full
pages can be shared read-only between sequences (a common prompt).  The step is the batched step with another row base: every active row's output and appended
rows are bit-identical to tce_attention_decode_step_batch_f16 on contiguous caches with the same contents.

    PageAllocator              host bookkeeping (free list, reference counts, a page list per slot) + the device block table; ONE for all layers: every layer
                               uses the same page numbers in its own pools
    PagedBatchDecodeAttention  one layer's pools and workspace: step (one launch), prefill (tce_attention_prefill_paged_f16: the new rows of up to 16 sequences
                               straight into their pages, two launches), admit (scatter from a contiguous cache), read_back (gather), copy_rows
    PagedBatchedDecoder        BatchedDecoder's seven launches with the paged step as launch 3; prefill / prefill_many: BatchedDecoder.prefill's launches once for
                               the rows of all admitted sequences, the paged prefill in the middle (no staging cache, no gather, no scatter)

kv_dtype="fp8_e4m3": the pools hold OCP e4m3 bytes (include/tce_matmul.h, "FP8 pages") -- half the bytes held and streamed per token -- with one power-of-two scale
per pool, 2^k_scale_log2 and 2^v_scale_log2, exponents in [-8, 7].  dequant(byte) is exact in binary16 and the arithmetic behind it is the fp16 kernels'.
fp8_quantize_reference / fp8_dequantize_reference restate the format on the host.

window=W (PagedBatchDecodeAttention / PagedBatchedDecoder): sliding-window attention -- a row at position p weighs keys max(0, p - W + 1) .. p -- through the
*_window entry points; the pages wholly behind every layer's window are given back with PageAllocator.release_behind (generate._GeneratorBase.run does, and
admit(..., chunk_rows=N) does between the chunks of a prompt).

Trust: the step follows only table words 0 .. pos // page_keys of an active row (with a window: max(0, pos - W + 1) // page_keys .. pos // page_keys); everything else in the table may hold anything (a released slot's words stay as
they were).  It does not validate page numbers: PageAllocator writes only numbers in [0, num_pages), and PagedBatchDecodeAttention.table_violations runs
tce_kv_block_table_check for a caller who wants the table checked on the device before a launch.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import capi
from .attention_ops import DecodeAttention
from .batch_decode import BatchedDecoder
from .decoder_block import DecoderBlock
from .linear import _stream


FP8_SCALE_LOG2_MIN, FP8_SCALE_LOG2_MAX = -8, 7
KV_DTYPES = ("fp16", "fp8_e4m3")


def _check_scale_log2(e: int) -> int:
    if int(e) != e or not FP8_SCALE_LOG2_MIN <= int(e) <= FP8_SCALE_LOG2_MAX:
        raise ValueError(f"scale exponent {e}: an integer in [{FP8_SCALE_LOG2_MIN}, {FP8_SCALE_LOG2_MAX}]")
    return int(e)


def fp8_quantize_reference(x_f16, e: int) -> np.ndarray:
    """quant(x, e) = e4m3_rne(clamp(float(x) * 2^-e, -448, 448)) of a binary16 array (numpy or torch), as uint8 of the same shape: the product is exact in fp32, nearest
    with ties to the even mantissa, saturating (+-inf included), -0 stays 0x80, NaN becomes the NaN byte 0x7f.  tests/test_fp8_kv_host.py holds it to the format's
    definition for every finite binary16 value and every exponent."""
    e = _check_scale_log2(e)
    x = x_f16.detach().cpu().numpy() if isinstance(x_f16, torch.Tensor) else np.asarray(x_f16)
    if x.dtype != np.float16:
        raise TypeError("fp8_quantize_reference takes binary16")
    with np.errstate(invalid="ignore"):  # (NaN inputs pass through the product)
        x32 = np.ascontiguousarray(x.astype(np.float32) * np.float32(2.0 ** -e))
    out = torch.from_numpy(x32).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8).numpy().copy()
    out[np.isnan(x32)] = 0x7F
    return out


def fp8_dequantize_reference(b, e: int) -> np.ndarray:
    """dequant(b, e) = e4m3(b) * 2^e of a uint8 array (numpy or torch) as binary16 of the same shape -- exact for every finite byte; the NaN bytes 0x7f / 0xff give the
    NaN 0x7fff.  Built from sign / exponent / mantissa, not from a library conversion."""
    e = _check_scale_log2(e)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    if b.dtype != np.uint8:
        raise TypeError("fp8_dequantize_reference takes uint8")
    i = b.astype(np.int32)
    ex, m = (i >> 3) & 15, (i & 7).astype(np.float64)
    v = np.where(ex == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * np.exp2((ex - 7).astype(np.float64)))
    v = np.where(i & 0x80, -v, v) * 2.0 ** e
    out = v.astype(np.float16)  # (exact: every value is representable)
    assert np.array_equal(out.astype(np.float64), v)
    out = out.view(np.uint16).copy()
    out[(i & 0x7F) == 0x7F] = 0x7FFF
    return out.view(np.float16)


class PagePoolExhausted(MemoryError):
    """The pool has fewer free pages than the operation needs; nothing was changed."""


class PageAllocator:
    """`num_pages` pages of `page_keys` keys for `batch` slots of at most `max_pages_per_seq` pages each.  Works with device="cpu" (the table is then a host tensor)."""

    def __init__(self, num_pages: int, page_keys: int, batch: int, max_pages_per_seq: int, device, free_order=None):
        """free_order: the page numbers in the order they are handed out first (default 0, 1, 2, ...) -- a permutation of range(num_pages)."""
        if page_keys not in (16, 32, 64, 128, 256):
            raise ValueError(f"page_keys {page_keys}: a power of two from 16 to 256")
        if num_pages < 1 or batch < 1 or max_pages_per_seq < 1:
            raise ValueError("num_pages, batch and max_pages_per_seq must be positive")
        order = list(range(num_pages)) if free_order is None else [int(p) for p in free_order]
        if sorted(order) != list(range(num_pages)):
            raise ValueError("free_order must be a permutation of range(num_pages)")
        self.num_pages, self.page_keys, self.batch, self.max_pages_per_seq = num_pages, page_keys, batch, max_pages_per_seq
        self.free = order[::-1]  # a stack: pop() hands out order[0] first, and a released page is the next one handed out
        self.refcount = [0] * num_pages
        self.pages: list[list[int]] = [[] for _ in range(batch)]  # the pages a slot HOLDS, in key order: pages[slot][i] is its table word gone[slot] + i
        self.gone = [0] * batch  # leading pages of a slot that release_behind gave back (their table words stay as they are and are never followed again)
        self.kept: list[list[int]] = [[] for _ in range(batch)]  # release_behind(..., keep_pages=k): the slot's first k pages (table words 0 .. k - 1), still held though
                                                                  # they lie below `gone` -- the attention sinks' pages; between them and pages[slot][0] is the hole
        self.frozen = [0] * batch  # leading pages of a slot that are (or were) shared: read-only for it, never the target of an append
        self.table = torch.zeros((batch, max_pages_per_seq), dtype=torch.int32, device=device)

    # ---- queries ----
    @property
    def max_keys(self) -> int:
        return self.max_pages_per_seq * self.page_keys

    def pages_in_use(self) -> int:
        return self.num_pages - len(self.free)

    def appendable_pages(self, slot: int) -> list[int]:
        """The pages of `slot` that an append may write: those behind its shared prefix."""
        return self.pages[slot][max(0, self.frozen[slot] - self.gone[slot]):]

    def writable(self, slot: int, key0: int, nkeys: int) -> bool:
        """May an append write rows [key0, key0 + nkeys) of `slot`: every page they fall in exists, is held by this slot alone and lies behind its frozen prefix."""
        self._slot(slot)
        if key0 < 0 or nkeys < 1:
            return False
        first, last = key0 // self.page_keys - self.gone[slot], (key0 + nkeys - 1) // self.page_keys - self.gone[slot]
        if first < max(0, self.frozen[slot] - self.gone[slot]) or last >= len(self.pages[slot]):
            return False
        return all(self.refcount[p] == 1 for p in self.pages[slot][first:last + 1])

    def holds(self, slot: int, key0: int, nkeys: int) -> bool:
        """Does `slot` hold a page for every key of [key0, key0 + nkeys): reserved, and not given back by release_behind.  With kept pages (release_behind(...,
        keep_pages=k)): inside the kept pages or inside the tail, never across the hole between them."""
        self._slot(slot)
        if key0 < 0 or nkeys < 1:
            return False
        first, last = key0 // self.page_keys, (key0 + nkeys - 1) // self.page_keys
        if last < len(self.kept[slot]):
            return True
        return first >= self.gone[slot] and last < self.gone[slot] + len(self.pages[slot])

    # ---- operations ----
    def reserve_many(self, wanted: list[tuple[int, int]]) -> list[list[int]]:
        """reserve() for several slots, all or nothing: [(slot, upto_pos)] with distinct slots.  Every argument is checked and the pages are counted before anything
        changes; on PagePoolExhausted (or a bad argument) no slot, page or table word has changed.  Returns the pages added per entry."""
        slots = [s for s, _ in wanted]
        if len(set(slots)) != len(slots):
            raise ValueError("reserve_many: a slot is named twice")
        short = 0
        for slot, upto_pos in wanted:
            self._slot(slot)
            need = upto_pos // self.page_keys + 1
            if upto_pos < 0 or need > self.max_pages_per_seq:
                raise ValueError(f"key index {upto_pos} outside a slot's {self.max_keys} keys")
            if need <= self.gone[slot]:
                raise ValueError(f"slot {slot}: key {upto_pos} lies in a page that was given back")
            short += max(0, need - self.gone[slot] - len(self.pages[slot]))
        if short > len(self.free):
            raise PagePoolExhausted(f"{short} pages needed for slots {slots}, {len(self.free)} free")
        return [self.reserve(slot, upto_pos) for slot, upto_pos in wanted]

    def reserve(self, slot: int, upto_pos: int) -> list[int]:
        """Add pages to `slot` until key index `upto_pos` is covered; returns the pages added.  Only the changed table words are written (stream-ordered)."""
        self._slot(slot)
        need = upto_pos // self.page_keys + 1
        if upto_pos < 0 or need > self.max_pages_per_seq:
            raise ValueError(f"key index {upto_pos} outside a slot's {self.max_keys} keys")
        if need <= self.gone[slot]:
            raise ValueError(f"slot {slot}: key {upto_pos} lies in a page that was given back")
        have = self.gone[slot] + len(self.pages[slot])
        if need - have > len(self.free):
            raise PagePoolExhausted(f"{need - have} pages needed for slot {slot}, {len(self.free)} free")
        added = [self.free.pop() for _ in range(need - have)]
        for p in added:
            assert self.refcount[p] == 0
            self.refcount[p] = 1
        self.pages[slot] += added
        if added:
            self._write(slot, have, added)
        target = self.pages[slot][upto_pos // self.page_keys - self.gone[slot]]
        assert self.refcount[target] == 1 and upto_pos // self.page_keys >= self.frozen[slot], f"slot {slot}: key {upto_pos} lies in a shared page ({target})"
        return added

    def release(self, slot: int) -> list[int]:
        """Drop the slot's references; returns the pages that went back to the free list.  The slot's table words are left as they are (an inactive row's words are
        never followed)."""
        self._slot(slot)
        freed = []
        for p in self.kept[slot] + self.pages[slot]:
            assert self.refcount[p] > 0
            self.refcount[p] -= 1
            if self.refcount[p] == 0:
                freed.append(p)
        self.free += freed[::-1]  # (the slot's first page is the next one handed out)
        self.pages[slot] = []
        self.kept[slot] = []
        self.frozen[slot] = 0
        self.gone[slot] = 0
        return freed

    def release_behind(self, slot: int, key: int, keep_pages: int = 0) -> list[int]:
        """Drop the slot's references to the pages that lie WHOLLY below key index `key` (sliding-window attention: no layer weighs them any more); returns the pages
        that went back to the free list -- a shared page only loses this slot's reference.  The table words are left as they are: a windowed row never follows a word
        below its window's first key.  Idempotent; key <= 0 drops nothing; never more than the slot holds.  From then on the slot cannot be a fork's source.
        keep_pages = k > 0 (attention sinks): the slot's first k pages stay held -- they move to kept[slot], the pages between them and `key` go back; gone[slot] is
        still the table index of pages[slot][0].  The kept pages can only be established while nothing has been given back (gone == 0): a later call that asks for
        more than is kept raises ValueError (one that asks for fewer, or 0, keeps what is kept).  keep_pages=0 on a slot without kept pages: as it always was."""
        self._slot(slot)
        k = int(keep_pages)
        if k < 0:
            raise ValueError(f"keep_pages {keep_pages}: an integer >= 0")
        if self.gone[slot] and k > len(self.kept[slot]):
            raise ValueError(f"slot {slot}: keep_pages {k}, but it gave pages back while {len(self.kept[slot])} were kept (kept pages are established by the first release)")
        drop = min(max(int(key), 0) // self.page_keys - self.gone[slot], len(self.pages[slot]))
        keep = k if self.gone[slot] == 0 else 0  # (the first release: the first k pages of the tail are the ones to keep)
        if drop <= keep:
            return []
        freed = []
        for p in self.pages[slot][keep:drop]:
            assert self.refcount[p] > 0
            self.refcount[p] -= 1
            if self.refcount[p] == 0:
                freed.append(p)
        self.free += freed[::-1]
        if keep:
            self.kept[slot] = self.pages[slot][:keep]
        self.pages[slot] = self.pages[slot][drop:]
        self.gone[slot] += drop
        return freed

    def fork(self, src_slot: int, dst_slot: int, keys: int) -> list[tuple[int, int, int]]:
        """`dst_slot` (empty) starts as a copy of the first `keys` keys of `src_slot`: the full pages among them are shared (reference counts raised), a partial last
        page gets a fresh page of dst's own.  Returns the copies the caller must carry out in every layer: [(src page, dst page, rows)] (empty when keys is a
        multiple of page_keys)."""
        self._slot(src_slot)
        self._slot(dst_slot)
        if src_slot == dst_slot or self.pages[dst_slot] or self.gone[dst_slot]:
            raise ValueError("fork needs an empty destination slot other than the source")
        if self.gone[src_slot]:
            raise ValueError(f"slot {src_slot} gave its leading pages back (release_behind): it cannot be forked")
        if keys < 0 or keys > len(self.pages[src_slot]) * self.page_keys:
            raise ValueError(f"slot {src_slot} does not hold {keys} keys")
        full, rows = divmod(keys, self.page_keys)
        if rows and not self.free:
            raise PagePoolExhausted(f"1 page needed for slot {dst_slot}, 0 free")
        shared = self.pages[src_slot][:full]
        for p in shared:
            self.refcount[p] += 1
        mine, copies = list(shared), []
        if rows:
            fresh = self.free.pop()
            assert self.refcount[fresh] == 0
            self.refcount[fresh] = 1
            mine.append(fresh)
            copies.append((self.pages[src_slot][full], fresh, rows))
        self.pages[dst_slot] = mine
        self.frozen[dst_slot] = full
        self.frozen[src_slot] = max(self.frozen[src_slot], full)
        if mine:
            self._write(dst_slot, 0, mine)
        return copies

    def check_invariants(self) -> None:
        """No page both free and referenced, counts equal to the slot lists, no shared page appendable, the table's live words equal to the slot lists."""
        counts = [0] * self.num_pages
        for ps, kp in zip(self.pages, self.kept):
            assert len(ps) <= self.max_pages_per_seq and len(set(kp + ps)) == len(kp) + len(ps)
            for p in kp + ps:
                counts[p] += 1
        assert counts == self.refcount
        assert len(set(self.free)) == len(self.free) and all(self.refcount[p] == 0 for p in self.free)
        assert len(self.free) + sum(1 for c in counts if c) == self.num_pages
        host = self.table.cpu().numpy()
        for s, ps in enumerate(self.pages):
            assert all(self.refcount[p] == 1 for p in self.appendable_pages(s))
            assert self.gone[s] >= 0 and self.gone[s] + len(ps) <= self.max_pages_per_seq
            assert host[s, self.gone[s]:self.gone[s] + len(ps)].tolist() == ps
            assert len(self.kept[s]) <= self.gone[s] and host[s, :len(self.kept[s])].tolist() == self.kept[s]

    # ---- internals ----
    def _slot(self, slot: int) -> None:
        if not 0 <= slot < self.batch:
            raise IndexError(f"slot {slot} of {self.batch}")

    def _write(self, slot: int, first: int, pages: list[int]) -> None:
        # a copy on the current stream: ordered after the launches already issued that read the old words, before the ones issued next
        self.table[slot, first:first + len(pages)].copy_(torch.tensor(pages, dtype=torch.int32))


class PagedBatchDecodeAttention:
    """One layer's K and V pools and the step's workspace, over a PageAllocator's table."""

    def __init__(self, allocator: PageAllocator, heads: int, kv_heads: int | None, device, cos: torch.Tensor | None = None, sin: torch.Tensor | None = None,
                 kv_dtype: str = "fp16", k_scale_log2: int = 0, v_scale_log2: int = 0, window: int | None = None, sinks: int | None = None):
        """kv_dtype "fp16" (the default: today's pools and entry points) or "fp8_e4m3": uint8 pools of the same shape, every call through the fp8 entry points with
        the two scale exponents (integers in [-8, 7]; ignored for fp16).  window None: every key, through today's entry points; W >= 1: step, prefill and
        table_violations go through the *_window entry points (a row at position p weighs keys max(0, p - W + 1) .. p).  sinks None: as above; S in 1 .. 16 (needs a
        window): attention sinks, through the *_sink entry points -- a row at p >= S + W weighs keys 0 .. S - 1 (q rotated with row S + W - 1) beside its window, a row
        below weighs keys 0 .. p (include/tce_matmul.h).  The caller keeps the sequence's first page: PageAllocator.release_behind(..., keep_pages=1)."""
        if window is not None and (int(window) != window or int(window) < 1 or int(window) > 0x7fffffff):
            raise ValueError(f"window {window}: None or an integer >= 1")
        self.window = None if window is None else int(window)
        if sinks is not None and (window is None or int(sinks) != sinks or not 1 <= int(sinks) <= 16):
            raise ValueError(f"sinks {sinks}: None, or an integer 1 .. 16 beside a window")
        self.sinks = None if sinks is None else int(sinks)
        if kv_dtype not in KV_DTYPES:
            raise ValueError(f"kv_dtype {kv_dtype!r}: one of {KV_DTYPES}")
        self.kv_dtype, self.fp8 = kv_dtype, kv_dtype == "fp8_e4m3"
        self.k_scale_log2, self.v_scale_log2 = _check_scale_log2(k_scale_log2), _check_scale_log2(v_scale_log2)
        self.allocator, self.batch, self.heads, self.hd = allocator, allocator.batch, heads, 128
        self.kv_heads = heads if kv_heads is None else kv_heads
        self.page_keys, self.num_pages, self.max_keys = allocator.page_keys, allocator.num_pages, allocator.max_keys
        L = capi.lib()
        pool_bytes = L.tce_kv_pages_pool_bytes_fp8 if self.fp8 else L.tce_kv_pages_pool_bytes
        if int(pool_bytes(self.num_pages, self.kv_heads, self.page_keys, self.hd)) == 0:
            raise ValueError("unsupported page pool shape")
        need = int(L.tce_attention_decode_batch_workspace_bytes(self.batch, heads, self.max_keys, self.hd))
        if need == 0:
            raise ValueError("unsupported batched attention shape")
        self.k_pool = torch.zeros((self.num_pages, self.kv_heads, self.page_keys, self.hd), dtype=torch.uint8 if self.fp8 else torch.float16, device=device)
        self.v_pool = torch.zeros_like(self.k_pool)
        self.workspace = torch.zeros(need, dtype=torch.uint8, device=device)  # zeroed once: the per-(sequence, head) arrival counters
        self.slot_workspace_bytes = need // self.batch
        self.cos, self.sin = cos, sin
        self.alpha_bits = int(np.array([1.0 / np.sqrt(self.hd)], np.float16).view(np.uint16)[0])
        self._staging: DecodeAttention | None = None  # made on first use of staging(): nothing in this module asks for it
        self._prefill_ws: torch.Tensor | None = None
        self._violations = torch.zeros(1, dtype=torch.int32, device=device)

    def _scales(self) -> tuple:
        """The fp8 entry points' two extra arguments (in front of the stream); nothing for fp16."""
        return (self.k_scale_log2, self.v_scale_log2) if self.fp8 else ()

    def _window(self) -> tuple:
        """The *_window entry points' one extra argument (behind the scales, in front of the stream), the *_sink entry points' two; nothing without a window."""
        return () if self.window is None else ((self.window,) if self.sinks is None else (self.window, self.sinks))

    def _entry(self, name: str) -> str:
        """`name` or, with a window, its *_window form; with sinks, its *_sink form"""
        return name if self.window is None else name + ("_window" if self.sinks is None else "_sink")

    def _table_args(self):
        t = self.allocator.table
        assert t.is_cuda and t.device == self.k_pool.device
        return C.c_void_p(t.data_ptr()), t.shape[1], self.page_keys, self.num_pages

    def step(self, qkv: torch.Tensor, pos_device: torch.Tensor, pos_bound: int, out: torch.Tensor | None = None) -> torch.Tensor:
        """BatchDecodeAttention.step on the pages: one launch; the table is read when the kernel runs."""
        return self._step(self._entry("tce_attention_decode_step_paged"), None, qkv, pos_device, pos_bound, out)

    def _step(self, entry: str, rows_per_seq: int | None, qkv: torch.Tensor, pos_device: torch.Tensor, pos_bound: int, out: torch.Tensor | None) -> torch.Tensor:
        """The step's assertions and call, `entry`_f16 or _fp8, for batch * rows_per_seq rows (None: one row per sequence, and an entry point without that argument).
        With a window the caller's `entry` already carries the suffix (_entry): ..._paged_window, ..._paged_rows_window; with sinks ..._paged_sink, ..._paged_rows_sink."""
        n = self.batch * (rows_per_seq or 1)
        rw = (self.heads + 2 * self.kv_heads) * self.hd
        assert qkv.dtype == torch.float16 and qkv.is_contiguous() and qkv.is_cuda and qkv.numel() == n * rw
        assert pos_device.dtype == torch.int32 and pos_device.is_cuda and pos_device.is_contiguous() and pos_device.numel() == n
        if out is None:
            out = torch.empty((n, self.heads * self.hd), dtype=torch.float16, device=qkv.device)
        assert out.dtype == torch.float16 and out.is_contiguous() and out.is_cuda and out.numel() == n * self.heads * self.hd
        p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
        fn = getattr(capi.lib(), entry + ("_fp8" if self.fp8 else "_f16"))
        rows = () if rows_per_seq is None else (rows_per_seq,)
        capi.check(fn(p(qkv), p(self.k_pool), p(self.v_pool), *self._table_args(), p(self.cos), p(self.sin), p(out), p(self.workspace), self.batch, *rows, self.heads,
                      self.kv_heads, self.hd, p(pos_device), int(pos_bound), self.alpha_bits, *self._scales(), *self._window(), C.c_void_p(_stream())))
        return out

    def prefill(self, segments, qkv: torch.Tensor, out: torch.Tensor | None = None, causal: bool = True) -> torch.Tensor:
        """tce_attention_prefill_paged_f16: segments [(slot, pos, m)] (at most 16, distinct slots, pages reserved before), qkv fp16 [sum m][(heads + 2 kv_heads) * 128]
        with the segments' rows packed in that order.  ONE call, two launches: rows pos .. pos + m - 1 of every segment are appended to its pages and out
        [sum m][heads * 128] (o_proj's input rows) is returned -- each segment bit-identical to DecodeAttention.prefill of that sequence alone."""
        segs, total = capi.prefill_segments(segments)
        assert qkv.dtype == torch.float16 and qkv.is_contiguous() and qkv.dim() == 2 and qkv.is_cuda and tuple(qkv.shape) == (total, (self.heads + 2 * self.kv_heads) * self.hd)
        for slot, pos, m in segments:
            assert self.allocator.writable(slot, pos, m), f"slot {slot}: rows [{pos}, {pos} + {m}) are not all in pages of its own (reserve them; a shared page is read-only)"
        if out is None:
            out = torch.empty((total, self.heads * self.hd), dtype=torch.float16, device=qkv.device)
        assert out.dtype == torch.float16 and out.is_contiguous() and out.is_cuda and tuple(out.shape) == (total, self.heads * self.hd)
        L = capi.lib()
        need = int(L.tce_attention_prefill_paged_workspace_bytes(self.heads, total, self.hd))
        if self._prefill_ws is None or self._prefill_ws.numel() < need:
            self._prefill_ws = torch.empty(need, dtype=torch.uint8, device=qkv.device)
        t = self.allocator.table
        assert t.is_cuda and t.device == self.k_pool.device
        p = lambda x: C.c_void_p(x.data_ptr() if x is not None else 0)
        fn = getattr(L, self._entry("tce_attention_prefill_paged") + ("_fp8" if self.fp8 else "_f16"))
        capi.check(fn(p(qkv), 0, p(self.k_pool), p(self.v_pool), p(t), t.shape[0], t.shape[1], self.page_keys, self.num_pages, p(self.cos), p(self.sin),
                      1 if causal else 0, p(out), 0, p(self._prefill_ws), self.heads, self.kv_heads, self.hd, C.cast(segs, C.c_void_p), len(segments), total,
                      self.alpha_bits, *self._scales(), *self._window(), C.c_void_p(_stream())))
        return out

    def table_violations(self, pos_device: torch.Tensor, pos_bound: int) -> int:
        """tce_kv_block_table_check on the allocator's table, waited for: the number of words the step would follow that are not page numbers (0: sound)."""
        tab, stride, pk, n = self._table_args()
        fn = getattr(capi.lib(), self._entry("tce_kv_block_table_check"))
        capi.check(fn(tab, stride, pk, n, self.batch, C.c_void_p(pos_device.data_ptr()), int(pos_bound), C.c_void_p(self._violations.data_ptr()),
                      *self._window(), C.c_void_p(_stream())))
        return int(self._violations.item())

    def _row(self, slot: int) -> C.c_void_p:
        t = self.allocator.table
        if not 0 <= slot < self.batch:
            raise IndexError(f"slot {slot} of {self.batch}")
        return C.c_void_p(t.data_ptr() + slot * t.shape[1] * 4)

    def admit(self, slot: int, contiguous_attention, key0: int, nkeys: int) -> None:
        """Scatter rows [key0, key0 + nkeys) of a contiguous single-sequence cache pair (a DecodeAttention's k_cache / v_cache) into the slot's pages (reserved
        before: PageAllocator.reserve(slot, key0 + nkeys - 1))."""
        k, v = contiguous_attention.k_cache, contiguous_attention.v_cache
        assert k.dtype == v.dtype == torch.float16 and k.is_contiguous() and v.is_contiguous() and tuple(k.shape) == tuple(v.shape) and k.shape[0] == self.kv_heads
        assert self.allocator.holds(slot, key0, nkeys), "reserve the slot's pages first"
        p = lambda t: C.c_void_p(t.data_ptr())
        L = capi.lib()
        fn = L.tce_kv_pages_scatter_fp8 if self.fp8 else L.tce_kv_pages_scatter_f16  # (fp8: the contiguous side stays fp16, the rows are quantised on their way in)
        capi.check(fn(p(k), p(v), p(self.k_pool), p(self.v_pool), self._row(slot), self.allocator.table.shape[1], self.page_keys, self.num_pages, self.kv_heads,
                      self.hd, k.shape[1], int(key0), int(nkeys), *self._scales(), C.c_void_p(_stream())))

    def gather_into(self, slot: int, contiguous_attention, key0: int, nkeys: int) -> None:
        """The reverse of admit: the slot's rows [key0, key0 + nkeys) into a contiguous cache pair."""
        k, v = contiguous_attention.k_cache, contiguous_attention.v_cache
        assert k.dtype == v.dtype == torch.float16 and k.is_contiguous() and v.is_contiguous() and tuple(k.shape) == tuple(v.shape) and k.shape[0] == self.kv_heads
        assert self.allocator.holds(slot, key0, nkeys), "the slot does not hold these keys"
        p = lambda t: C.c_void_p(t.data_ptr())
        L = capi.lib()
        fn = L.tce_kv_pages_gather_fp8 if self.fp8 else L.tce_kv_pages_gather_f16  # (fp8: dequantised -- exactly -- into the fp16 pair)
        capi.check(fn(p(self.k_pool), p(self.v_pool), p(k), p(v), self._row(slot), self.allocator.table.shape[1], self.page_keys, self.num_pages, self.kv_heads,
                      self.hd, k.shape[1], int(key0), int(nkeys), *self._scales(), C.c_void_p(_stream())))

    def read_back(self, slot: int, keys: int) -> tuple[torch.Tensor, torch.Tensor]:
        """The slot's first `keys` keys as a fresh contiguous fp16 pair [kv_heads][keys][128] (fp8 pages: dequantised)."""
        class _Pair:
            pass
        pair = _Pair()
        pair.k_cache = torch.zeros((self.kv_heads, keys, self.hd), dtype=torch.float16, device=self.k_pool.device)
        pair.v_cache = torch.zeros_like(pair.k_cache)
        self.gather_into(slot, pair, 0, keys)
        return pair.k_cache, pair.v_cache

    def copy_rows(self, src_page: int, dst_page: int, rows: int) -> None:
        """PageAllocator.fork's copy for this layer: the first `rows` rows of every head of src_page into dst_page."""
        assert 0 <= src_page < self.num_pages and 0 <= dst_page < self.num_pages and src_page != dst_page and 0 < rows <= self.page_keys
        self.k_pool[dst_page, :, :rows].copy_(self.k_pool[src_page, :, :rows])
        self.v_pool[dst_page, :, :rows].copy_(self.v_pool[src_page, :, :rows])

    def staging(self) -> DecodeAttention:
        """A contiguous single-sequence cache of max_keys rows for a caller that wants one beside the pages (admit / gather_into; made on first use).  Prefill does
        not use it: PagedBatchDecodeAttention.prefill writes the pages directly."""
        if self._staging is None:
            self._staging = DecodeAttention(self.heads, self.hd, self.max_keys, self.k_pool.device, self.cos, self.sin, kv_heads=self.kv_heads)
        return self._staging

    def slot(self, b: int) -> DecodeAttention:
        """A DecodeAttention for slot b: the staging cache (the caller gathers before and scatters after: gather_into / admit)."""
        if not 0 <= b < self.batch:
            raise IndexError(f"slot {b} of {self.batch}")
        return self.staging()


class PagedBatchedDecoder(BatchedDecoder):
    """BatchedDecoder on a paged cache: the same seven launches per layer (BatchedDecoder.step itself, with PagedBatchDecodeAttention.step as launch 3), the same
    prefill launches with the paged prefill in the middle.  One PageAllocator serves the decoders of all layers."""

    def __init__(self, block: DecoderBlock, allocator: PageAllocator, kv_dtype: str = "fp16", k_scale_log2: int = 0, v_scale_log2: int = 0, attention=None,
                 rows: int | None = None, window: int | None = None, lora=None, sinks: int | None = None):
        """attention, rows: BatchedDecoder's (a subclass with an attention object of its own over the same allocator; the default is built here).  window: this layer's
        sliding window (PagedBatchDecodeAttention), None for full attention.  lora: BatchedDecoder's (this layer's view of a LoraPool: q/k/v, o_proj and down_proj
        become adapted linears in step, prefill and prefill_many; gate/up too with a gate_up=True pool)."""
        self.allocator = allocator
        if attention is None:
            attention = PagedBatchDecodeAttention(allocator, block.heads, block.kv_heads, block.gamma1.device, block.attention.cos, block.attention.sin, kv_dtype=kv_dtype,
                                                  k_scale_log2=k_scale_log2, v_scale_log2=v_scale_log2, window=window, sinks=sinks)
        elif window is not None and getattr(attention, "window", None) != window:
            raise ValueError("window: the attention object given was built with another one")
        elif sinks is not None and getattr(attention, "sinks", None) != sinks:
            raise ValueError("sinks: the attention object given was built with another count")
        super().__init__(block, allocator.batch, attention=attention, rows=rows, lora=lora)

    @property
    def window(self) -> int | None:
        return getattr(self.attention, "window", None)

    @property
    def sinks(self) -> int | None:
        return getattr(self.attention, "sinks", None)

    def prefill_many(self, admissions) -> None:
        """Admit several sequences at once: admissions [(slot, rows, pos)], at most 16, distinct slots; rows fp16 [m][hidden] at positions pos .. pos + m - 1, updated
        in place.  Pages are reserved for every sequence first, all or nothing (PagePoolExhausted: no slot changed; the allocator is shared, so the first layer's call
        reserves for all); then BatchedDecoder.prefill's launches run ONCE at M = all rows -- the weights are streamed once -- with the paged prefill in the middle."""
        blk = self.block
        if not 1 <= len(admissions) <= capi.TCE_PREFILL_MAX_SEGMENTS:
            raise ValueError(f"{len(admissions)} sequences: 1 .. {capi.TCE_PREFILL_MAX_SEGMENTS} per call")
        for _, rows, _ in admissions:
            assert rows.dtype == torch.float16 and rows.is_contiguous() and rows.dim() == 2 and rows.shape[1] == blk.hidden and rows.shape[0] >= 1
        self.allocator.reserve_many([(slot, pos + rows.shape[0] - 1) for slot, rows, pos in admissions])
        segments = [(slot, pos, rows.shape[0]) for slot, rows, pos in admissions]
        for slot, pos, m in segments:
            assert self.allocator.writable(slot, pos, m), f"slot {slot}: a chunk at key {pos} starts inside a shared page"
        packed = admissions[0][1] if len(admissions) == 1 else torch.cat([rows for _, rows, _ in admissions])
        self._prefill_rows(packed, lambda qkv, attn: self.attention.prefill(segments, qkv, out=attn, causal=True), self._row_words([(slot, m) for slot, _, m in segments]))
        if len(admissions) > 1:
            row0 = 0
            for _, rows, _ in admissions:
                rows.copy_(packed[row0:row0 + rows.shape[0]])
                row0 += rows.shape[0]

    def prefill(self, slot: int, rows: torch.Tensor, pos: int) -> None:
        """Admit a sequence into `slot`: prefill_many with one sequence.  The new rows pos .. pos + m - 1 go straight into the slot's pages (reserved here)."""
        self.prefill_many([(slot, rows, pos)])
