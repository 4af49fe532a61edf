"""A sparse mixture-of-experts FFN on W4A16 (csrc/w4a16_moe.hip, include/tce_matmul.h "Mixture of experts"): Mixtral / Qwen-MoE shaped layers on the batched path.

Which expert a row uses is decided per token on the device, so the layer is five launches with fixed grids that read the routing words when they run -- nothing is read
back, and a captured graph follows a routing that changes from replay to replay:

    route (2)   logits x . Wr[e] in fp32, the k largest (ties to the lower index, NaN below every number), softmax weights; the stable grouping of the pairs by expert
    gate_up     act[p] = silu_mul_half(fp16(gate_e . x_i), fp16(up_e . x_i))     pair p = i * k + s, e = ids[p]; fp16 [rows * k][ffn]
    down        y[p] = down_e . act[p]                                           fp32 [rows * k][hidden]
    combine     C[i] = fp16(float(C[i]) + sum_s w[i][s] * y[i * k + s])          the residual stream, in place

    moe_reference     the definition in numpy float64 on the stored values: the yardstick of the tests
    group_reference   the stable grouping (count, lists) of ids
    MoeWorkspace      the caller workspace of the five entry points and typed views of its six sections
    route / gate_up / down / combine_add    one entry point each, on torch tensors, on the current stream; route(parallel=True) / group_parallel: the grouping for
                      prompt-sized pair counts (csrc/w4a16_moe_group.hip: chunks of 1024 pairs, a workgroup each), the same count and lists; gate_up /
                      down(tiled=True): the tiled form for prompt-sized pair counts (csrc/w4a16_moe_tiled.hip: TILE_ROWS weight rows x TILE_PAIRS pairs per workgroup), bit-identical per pair to the other
    MoeFFN            the stacked expert tensors of one layer (synthetic weights, quantize_q4_6 per expert) and forward(xn, rows_inout): DecoderBlock(..., moe=)
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import capi, quantize

GROUP = 128
TILE_ROWS, TILE_PAIRS = capi.TCE_MOE_TILE_ROWS, capi.TCE_MOE_TILE_PAIRS  # the tiled form's tile (include/tce_matmul.h)


def _unpack_nibbles(words: np.ndarray) -> np.ndarray:
    w = np.ascontiguousarray(words).view(np.uint32)
    return ((w[..., None] >> (np.arange(8, dtype=np.uint32) * 4)) & 0xF).reshape(*w.shape[:-1], w.shape[-1] * 8)


def dequantize_stacked(qweight, scales, zeros) -> np.ndarray:
    """float64 [E][N][K] = scale * (code - zero point) of stacked q4_6 arrays (group size 128)"""
    codes = _unpack_nibbles(np.asarray(qweight)).astype(np.float64)
    ng = codes.shape[-1] // GROUP
    z = _unpack_nibbles(np.asarray(zeros))[..., :ng].astype(np.float64)
    s = np.asarray(scales).astype(np.float64)[..., :ng]
    return (codes - np.repeat(z, GROUP, axis=-1)) * np.repeat(s, GROUP, axis=-1)


def route_reference(x, Wr, k: int, renormalize: bool = True):
    """ids int32 [rows][k], weights float64 [rows][k], logits float64 [rows][E]: logits in float64 on the fp16 values; the k largest in descending order, ties (-0 == +0)
    to the lower expert index, a NaN below every number (NaNs among themselves: the lower index); w[s] = exp(l[ids[s]] - max l) / sum_e exp(l[e] - max l), max over the
    numbers; renormalize: divided by their sum in slot order."""
    x, Wr = np.asarray(x), np.asarray(Wr)
    assert x.dtype == Wr.dtype == np.float16 and 1 <= k <= Wr.shape[0]
    with np.errstate(all="ignore"):
        logits = x.astype(np.float64) @ Wr.astype(np.float64).T
    rows, E = logits.shape
    ids, w = np.zeros((rows, k), np.int32), np.zeros((rows, k), np.float64)
    for i in range(rows):
        l = logits[i]
        order = sorted(range(E), key=lambda e: (math.isnan(l[e]), 0.0 if math.isnan(l[e]) else -l[e], e))
        ids[i] = order[:k]
        with np.errstate(all="ignore"):
            num = l[~np.isnan(l)]
            p = np.exp(l - (num.max() if num.size else np.nan))
            p = p / p.sum()
            w[i] = p[ids[i]]
            if renormalize:
                tot = 0.0
                for s in range(k):
                    tot = tot + w[i, s]
                w[i] = w[i] / tot
    return ids, w, logits


def group_reference(ids, E: int):
    """count int32 [E], lists: per expert the pair indices p (row-major over ids) that name it, ascending; a word outside [0, E) is in no list"""
    flat = np.asarray(ids).reshape(-1)
    lists = [np.nonzero(flat == e)[0].astype(np.int32) for e in range(E)]
    return np.array([len(v) for v in lists], np.int32), lists


def moe_reference(x, Wr, gate_up, down, k: int, Cm, renormalize: bool = True, ids=None, weights=None) -> dict:
    """The definition in float64 on the stored values.  x fp16 [rows][hidden]; Wr fp16 [E][hidden]; gate_up / down: (qweight, scales, zeros) stacked q4_6 arrays
    ([E][2 ffn][..] with gate / up rows interleaved, [E][hidden][..]); Cm fp16 [rows][hidden].  ids / weights given: that routing instead of the reference's own (a
    word outside [0, E) is a skipped slot).  Returns ids, weights, act float64 [rows * k][ffn], y float64 [rows * k][hidden], out fp16 [rows][hidden] (ONE rounding)."""
    x, Cm = np.asarray(x), np.asarray(Cm)
    rid, rw, _ = route_reference(x, Wr, k, renormalize)
    ids = rid if ids is None else np.asarray(ids).reshape(rid.shape)
    weights = rw if weights is None else np.asarray(weights, np.float64).reshape(rw.shape)
    Wgu, Wd = dequantize_stacked(*gate_up), dequantize_stacked(*down)
    E, rows = Wgu.shape[0], x.shape[0]
    act, y = np.zeros((rows * k, Wgu.shape[1] // 2)), np.zeros((rows * k, Wd.shape[1]))
    acc = np.zeros((rows, Wd.shape[1]))
    xf = x.astype(np.float64)
    for i in range(rows):
        for s in range(k):
            e, p = int(ids[i, s]), i * k + s
            if not 0 <= e < E:
                continue
            gu = Wgu[e] @ xf[i]
            g, u = gu[0::2], gu[1::2]
            act[p] = g / (1.0 + np.exp(-g)) * u
            y[p] = Wd[e] @ act[p]
            acc[i] += weights[i, s] * y[p]
    with np.errstate(over="ignore"):
        out = (Cm.astype(np.float64) + acc).astype(np.float16)
    return {"ids": ids, "weights": weights, "act": act, "y": y, "out": out}


def workspace_offsets(rows: int, k: int, E: int, n_max: int) -> list:
    """the six sections' byte offsets and the total (include/tce_matmul.h: each section rounded up to 256 bytes)"""
    P, offs = rows * k, [0]
    for s in (P * 4, P * 4, E * 4, E * P * 4, P * n_max * 2, P * n_max * 4):
        offs.append(offs[-1] + ((s + 255) & ~255))
    return offs


class MoeWorkspace:
    """The workspace of the five entry points for (rows, k, E, n_max) and views of its sections (include/tce_matmul.h: ids int32 [P], weights fp32 [P], count int32 [E],
    list int32 [E][P], act fp16 [P][ffn], y fp32 [P][N], each rounded up to 256 bytes).  device="cpu": host memory, for the layout tests."""

    def __init__(self, rows: int, k: int, E: int, n_max: int, device, buf=None):
        """buf: 256-byte aligned uint8 memory of at least `bytes` bytes to lay the sections over (MoeFFN's shared buffer); None: memory of its own, zeroed"""
        import torch
        self.rows, self.k, self.E, self.n_max, self.P = int(rows), int(k), int(E), int(n_max), int(rows) * int(k)
        self.offsets = workspace_offsets(self.rows, self.k, self.E, self.n_max)
        self.bytes = self.offsets[-1]
        if buf is None:
            buf = torch.zeros(self.bytes + 256, dtype=torch.uint8, device=device)
            buf = buf[(-buf.data_ptr()) % 256:]
        assert buf.data_ptr() % 256 == 0 and buf.numel() >= self.bytes
        self.buf = buf[:self.bytes]

    def _view(self, section: int, dtype, *shape):
        n = int(np.prod(shape)) * dtype.itemsize
        return self.buf[self.offsets[section]:self.offsets[section] + n].view(dtype).view(*shape)

    @property
    def ids(self):
        import torch
        return self._view(0, torch.int32, self.rows, self.k)

    @property
    def weights(self):
        import torch
        return self._view(1, torch.float32, self.rows, self.k)

    @property
    def count(self):
        import torch
        return self._view(2, torch.int32, self.E)

    @property
    def list(self):
        import torch
        return self._view(3, torch.int32, self.E, self.P)

    def act(self, ffn: int):
        import torch
        return self._view(4, torch.float16, self.P, ffn)

    def y(self, n: int):
        import torch
        return self._view(5, torch.float32, self.P, n)

    def write_routing(self, ids, weights) -> None:
        """a routing the caller states itself: ids / weights and the grouping group_reference gives for them (tests; tce_moe_route_f16 writes all four on the device)"""
        import torch
        ids = np.asarray(ids, np.int32).reshape(self.rows, self.k)
        count, lists = group_reference(ids, self.E)
        table = np.zeros((self.E, self.P), np.int32)
        for e, v in enumerate(lists):
            table[e, :len(v)] = v
        for dst, src in ((self.ids, ids), (self.weights, np.asarray(weights, np.float32).reshape(self.rows, self.k)), (self.count, count), (self.list, table)):
            dst.copy_(torch.from_numpy(src))


def _ptr(t) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


def _st() -> C.c_void_p:
    from .linear import _stream
    return C.c_void_p(_stream())


def route(x, Wr, ws: MoeWorkspace, renormalize: bool = True, parallel: bool = False) -> None:
    """tce_moe_route_f16 (parallel: tce_moe_route_parallel_f16, the same bits in three launches, the grouping's two of ceil(P / 1024) workgroups each): x fp16
    [rows][hidden] (row stride x.stride(0)), Wr fp16 [E][hidden] -> ws.ids, ws.weights, ws.count, ws.list"""
    import torch
    assert x.dtype == Wr.dtype == torch.float16 and x.dim() == 2 and x.stride(1) == 1 and Wr.is_contiguous() and x.shape == (ws.rows, Wr.shape[1]) and Wr.shape[0] == ws.E
    fn = capi.lib().tce_moe_route_parallel_f16 if parallel else capi.lib().tce_moe_route_f16
    capi.check(fn(_ptr(x), x.stride(0), _ptr(Wr), ws.rows, Wr.shape[1], ws.E, ws.k, int(bool(renormalize)), ws.n_max, _ptr(ws.buf), _st()))


def group_parallel(ws: MoeWorkspace) -> None:
    """tce_moe_group_parallel: ws.ids -> ws.count, ws.list (group_reference's grouping; the head of ws.y is its scratch)"""
    capi.check(capi.lib().tce_moe_group_parallel(ws.rows, ws.k, ws.E, ws.n_max, _ptr(ws.buf), _st()))


def _stacked(arrays, E: int):
    import torch
    qw, sc, zp = arrays
    assert qw.dtype == zp.dtype == torch.int32 and sc.dtype == torch.float16 and all(a.is_contiguous() and a.dim() == 3 and a.shape[0] == E for a in arrays)
    N, K = qw.shape[1], qw.shape[2] * 8
    zw = quantize.calculate_zeros_width(K, GROUP)
    assert tuple(sc.shape) == (E, N, zw * 8) and tuple(zp.shape) == (E, N, zw), "stacked q4_6 arrays with the default strides"
    return N, K


def gate_up(x, arrays, ws: MoeWorkspace, flags: int = 0, tiled: bool = False) -> None:
    """tce_moe_gate_up_f16 (tiled: tce_moe_gate_up_tiled_f16, the same bits): x fp16 [rows][K], arrays (qweight int32 [E][N][K/8], scales fp16, zeros int32) with gate /
    up rows interleaved -> ws.act(N / 2)"""
    import torch
    N, K = _stacked(arrays, ws.E)
    assert x.dtype == torch.float16 and x.dim() == 2 and x.stride(1) == 1 and tuple(x.shape) == (ws.rows, K)
    capi.check((capi.lib().tce_moe_gate_up_tiled_f16 if tiled else capi.lib().tce_moe_gate_up_f16)(_ptr(x), x.stride(0), *(_ptr(a) for a in arrays), ws.rows, ws.k, ws.E, N, K, GROUP, flags, ws.n_max, _ptr(ws.buf), _st()))


def down(arrays, ws: MoeWorkspace, flags: int = 0, tiled: bool = False) -> None:
    """tce_moe_down_f16 (tiled: tce_moe_down_tiled_f16, the same bits): ws.act(K) -> ws.y(N)"""
    N, K = _stacked(arrays, ws.E)
    capi.check((capi.lib().tce_moe_down_tiled_f16 if tiled else capi.lib().tce_moe_down_f16)(*(_ptr(a) for a in arrays), ws.rows, ws.k, ws.E, N, K, GROUP, flags, ws.n_max, _ptr(ws.buf), _st()))


def combine_add(Cm, ws: MoeWorkspace) -> None:
    """tce_moe_combine_add_f16: Cm fp16 [ws.rows][N] (row stride Cm.stride(0)), in place, from ws.ids, ws.weights and ws.y(N)"""
    import torch
    assert Cm.dtype == torch.float16 and Cm.dim() == 2 and Cm.stride(1) == 1 and Cm.shape[0] == ws.rows
    capi.check(capi.lib().tce_moe_combine_add_f16(_ptr(Cm), Cm.stride(0), ws.rows, ws.k, ws.E, Cm.shape[1], ws.n_max, _ptr(ws.buf), _st()))


class MoeFFN:
    """One layer's experts: Wr fp16 [E][hidden]; gate_up = (qweight int32 [E][2 ffn][hidden / 8], scales, zeros) with row 2n = gate n, row 2n + 1 = up n;
    down = (qweight int32 [E][hidden][ffn / 8], scales, zeros).  Synthetic weights, quantize_q4_6 per expert, as DecoderBlock's; nothing loads a checkpoint."""

    LAUNCHES = 5  # route (logits + selection, grouping), gate_up, down, combine; a forward of PARALLEL_GROUP_FROM_PAIRS pairs or more: 6 (the grouping is two launches)
    # forward runs the two contractions in the tiled form from this many pairs (rows * top_k) on; None: never.  From profiles/moe_tiled/moe_tiled_time.jsonl: the smallest
    # measured P from which the tiled pair of launches beats the pass pair at every larger measured point by more than the repeats' spreads (slower at P = 32 and 128)
    TILED_FROM_PAIRS = 256
    # forward routes with the parallel grouping (route(parallel=True): one launch more than LAUNCHES) from this many pairs on; None: never.  The same rule on
    # profiles/moe_group/moe_group_time.jsonl, over both measured routers (E = 8, k = 2 and E = 64, k = 8): slower at P = 32 (8.8 -> 9.4, 20.6 -> 23.9 us), level at
    # P = 128 with 64 experts (26.8 -> 26.4 us) and 1.6x faster with 8, then faster everywhere: 295 -> 16 us at 4096 pairs
    PARALLEL_GROUP_FROM_PAIRS = 128

    def __init__(self, hidden: int, ffn: int, experts: int, top_k: int, device, renormalize: bool = True, seed: int = 0, tiled_from=None, parallel_group_from=None):
        """tiled_from: the pair count from which forward uses the tiled form (0: always); None: the class default TILED_FROM_PAIRS.  Both forms give the same bits.
        parallel_group_from: the same for the parallel grouping of the route (class default PARALLEL_GROUP_FROM_PAIRS); the same bits again."""
        import torch
        for name, v in (("tiled_from", tiled_from), ("parallel_group_from", parallel_group_from)):
            if v is not None and int(v) < 0:
                raise ValueError(f"{name} {v}: a pair count >= 0, or None for the default")
        self.tiled_from = None if tiled_from is None else int(tiled_from)
        self.parallel_group_from = None if parallel_group_from is None else int(parallel_group_from)
        if not 1 <= int(top_k) <= capi.TCE_MOE_MAX_TOP_K or not int(top_k) <= int(experts) <= capi.TCE_MOE_MAX_EXPERTS:
            raise ValueError(f"top_k {top_k} of {experts} experts: 1 <= top_k <= {capi.TCE_MOE_MAX_TOP_K}, top_k <= experts <= {capi.TCE_MOE_MAX_EXPERTS}")
        if hidden % GROUP or ffn % GROUP:
            raise ValueError(f"hidden {hidden}, ffn {ffn}: multiples of the group size {GROUP} (both are a contraction's K)")
        self.hidden, self.ffn, self.experts, self.top_k, self.renormalize, self.device = int(hidden), int(ffn), int(experts), int(top_k), bool(renormalize), torch.device(device)
        g = torch.Generator(device=device).manual_seed(seed)
        rnd = lambda n, kk: torch.empty(n, kk, device=device).normal_(0.0, kk ** -0.5, generator=g)
        il = lambda a, b: torch.stack((a, b), dim=1).reshape(2 * a.shape[0], *a.shape[1:])  # Linear_half_int4.interleave's row order
        gu, dn = [], []
        for _ in range(self.experts):
            ga, ub = quantize.quantize_q4_6(rnd(ffn, hidden)), quantize.quantize_q4_6(rnd(ffn, hidden))
            gu.append(tuple(il(a, b) for a, b in zip(ga, ub)))
            dn.append(quantize.quantize_q4_6(rnd(hidden, ffn)))
        self.gate_up = tuple(torch.stack([t[j] for t in gu]).contiguous() for j in range(3))
        self.down = tuple(torch.stack([t[j] for t in dn]).contiguous() for j in range(3))
        self.Wr = torch.empty(self.experts, hidden, device=device).normal_(0.0, 1.0, generator=g).half()
        z8 = all(bool((a[2] == -2004318072).all().item()) for a in (self.gate_up, self.down))  # verified once, as Linear_half_int4 does
        self.flags = capi.TCE_W4_ZERO_POINT_IS_8 if z8 else 0
        self._buf, self._retired = None, []

    def workspace(self, m: int) -> MoeWorkspace:
        """The workspace for m rows: views of ONE buffer, the largest any call has needed so far (a prefill of many lengths keeps one buffer, not one per length).
        When it has to grow, the smaller buffer is kept alive -- a graph captured on it goes on replaying -- and later calls use the new one.  What a forward left
        behind is readable through workspace(m) until the next forward of any m.  The buffer belongs to the layer: every decoder that holds the block shares it, so
        two streams must not run one block at the same time."""
        n_max = max(self.hidden, self.ffn)
        need = workspace_offsets(m, self.top_k, self.experts, n_max)[-1]
        if self._buf is None or self._buf.numel() < need:
            import torch
            if self._buf is not None:
                self._retired.append(self._buf)
            buf = torch.zeros(need + 256, dtype=torch.uint8, device=self.device)
            self._buf = buf[(-buf.data_ptr()) % 256:][:need]
        return MoeWorkspace(m, self.top_k, self.experts, n_max, self.device, buf=self._buf)

    def forward(self, xn, rows_inout) -> None:
        """xn fp16 [m][hidden], the normalised rows; rows_inout fp16 [m][hidden], the residual stream, updated in place.  Five launches on the current stream; six from
        parallel_group_from pairs on (the parallel grouping is two launches)."""
        ws = self.workspace(xn.shape[0])
        frm = self.TILED_FROM_PAIRS if self.tiled_from is None else self.tiled_from
        tiled = frm is not None and ws.P >= frm
        frm = self.PARALLEL_GROUP_FROM_PAIRS if self.parallel_group_from is None else self.parallel_group_from
        route(xn, self.Wr, ws, self.renormalize, parallel=frm is not None and ws.P >= frm)
        gate_up(xn, self.gate_up, ws, self.flags, tiled)
        down(self.down, ws, self.flags, tiled)
        combine_add(rows_inout, ws)
