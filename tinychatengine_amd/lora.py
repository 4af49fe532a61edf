"""Multi-LoRA: per-slot fp16 adapters beside the W4A16 linears of the batched decode path.

The base weights are AWQ-packed int4, so a LoRA delta cannot be merged into them: an adapter is a run-time path.  An adapted linear is the base launch plus two
(csrc/lora.hip, include/tce_matmul.h "Multi-LoRA"):

    shrink   t[i][j] = sum_k x[i][k] * A[a][j][k]                                      fp32 [rows][R], never rounded to fp16
    expand   C[i][n] = fp16(float(C[i][n]) + scale[a] * sum_j t[i][j] * B[a][j][n])    in place, directly behind the base launch

with a = row_adapter[i], an int32 word per row that lives ON THE DEVICE: the rows of one launch pick different adapters, a word outside [0, n_adapters) (-1: "no
adapter") leaves its row untouched, and a captured graph follows a slot that changes its adapter without being captured again.

    lora_reference   the definition in numpy float64 plus the one rounding to fp16: the yardstick of the tests
    shrink, expand_add   the two launches on torch tensors (one launch each, on the current stream)
    pack_adapter     PEFT-style per-projection arrays -> the pool's per-target A [R][K] / B [R][N] (host only)
    LoraPool         fixed device storage for `max_adapters` adapters of every layer; load / unload are stream-ordered copies into it
    LoraLayer        one layer's view of the pool + the shared row_adapter tensor: what BatchedDecoder / PagedBatchedDecoder take as lora=

Targets: "qkv" (q_proj, k_proj and v_proj served as ONE adapted linear, because the project runs q/k/v as one fused linear: A is the three As stacked, R = 3 * rank, and B
is block-structured with zeros off the blocks), "o" and "down".  gate_proj / up_proj are refused by a default pool: the fused SiLU * mul epilogue has no place for a
delta in front of the nonlinearity.  lm_head and the embedding are not adapted.

LoraPool(..., gate_up=True) holds a fourth target, "gate_up": A is gate's and up's As stacked ([2 * rank][hidden]: ONE shrink on the shared input), Bg and Bu are
[rank][ffn] each, and the adapted gate/up is three launches -- the shrink, the base gate_up linear WITHOUT the pair flag (y fp16 [rows][2 * ffn], column 2n = gate n,
column 2n + 1 = up n) and tce_lora_expand_silu_mul_f16, which adds both deltas in front of the nonlinearity and writes SiLU(g) * u for EVERY row:

    expand_silu_mul          the launch on torch tensors
    lora_gate_up_reference   its definition in float64, the two roundings to fp16, then the oracle's SiLU * mul (silu_mul_reference restates it)

LoraPool(..., rows_per_seq=T) serves the speculative step: row_adapter is int32 [batch * T], the T rows of a slot carry the slot's word (set_slot writes it T times;
no launch is added: the host writes the word anyway).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

TARGETS = ("qkv", "o", "down")
PROJECTIONS = ("q_proj", "k_proj", "v_proj", "o_proj", "down_proj")
REFUSED_PROJECTIONS = ("gate_proj", "up_proj")  # by a pool built without gate_up=True
GATE_UP = "gate_up"                             # the fourth target of a gate_up=True pool: A [2 * rank][hidden]; Bg, Bu [rank][ffn]
NO_ADAPTER = -1


def lora_reference(x, A, B, scale, row_adapter, Cm) -> np.ndarray:
    """The definition: x fp16 [rows][K], A fp16 [n][R][K], B fp16 [n][R][N], scale fp32 [n], row_adapter integers [rows], Cm fp16 [rows][N] -> fp16 [rows][N].
    Every product and sum in float64, ONE rounding to fp16 at the end; a row whose word lies outside [0, n) keeps the bits of Cm."""
    x, A, B, Cm = (np.asarray(v) for v in (x, A, B, Cm))
    assert x.dtype == A.dtype == B.dtype == Cm.dtype == np.float16
    scale = np.asarray(scale, np.float32)
    out = Cm.copy()
    for i, a in enumerate(np.asarray(row_adapter).astype(np.int64).tolist()):
        if 0 <= a < A.shape[0]:
            t = A[a].astype(np.float64) @ x[i].astype(np.float64)
            with np.errstate(over="ignore"):
                out[i] = (Cm[i].astype(np.float64) + np.float64(scale[a]) * (t @ B[a].astype(np.float64))).astype(np.float16)
    return out


def silu_mul_reference(g, u) -> np.ndarray:
    """SiLuMul_half as the oracle states it (oracle/tce_oracle.c, orc_silu_mul_half), in numpy: every operation rounded to binary16 -- e = h(exp(-g)), d = h(1 + e),
    r = h(1 / d) with the quotient formed in double, sv = h(g * r), out = h(sv * u).  The oracle takes the C library's expf; numpy's float32 exp may differ from it in
    the last float bit, which shows only where that float sits on a binary16 rounding boundary -- a test that needs the oracle's bits passes its function instead."""
    h = lambda v: np.asarray(v).astype(np.float16)
    g, u = np.asarray(g, np.float16), np.asarray(u, np.float16)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        gf = g.astype(np.float32)
        e = h(np.exp(-gf))
        d = h(np.float32(1.0) + e.astype(np.float32))
        r = h(1.0 / d.astype(np.float64))
        sv = h(gf * r.astype(np.float32))
        return h(sv.astype(np.float32) * u.astype(np.float32))


def lora_gate_up_reference(x, A, Bg, Bu, scale, row_adapter, y, silu_mul=silu_mul_reference) -> np.ndarray:
    """The gate/up definition: x fp16 [rows][K], A fp16 [n][2R][K] (rows 0 .. R-1 gate's, R .. 2R-1 up's), Bg / Bu fp16 [n][R][N], scale fp32 [n], row_adapter integers
    [rows], y fp16 [rows][2N] (what the base gate_up linear left behind: column 2n = gate n, column 2n + 1 = up n) -> fp16 [rows][N].  Every product and sum in float64,
    ONE rounding to fp16 each for g and u (a row whose word lies outside [0, n) takes y's bits), then the oracle's SiLU * mul on (g, u): silu_mul(g, u) -> fp16, by
    default its numpy restatement above (the package does not import the oracle; the tests pass Oracle().silu_mul_half)."""
    x, A, Bg, Bu, y = (np.asarray(v) for v in (x, A, Bg, Bu, y))
    assert x.dtype == A.dtype == Bg.dtype == Bu.dtype == y.dtype == np.float16 and A.shape[1] == 2 * Bg.shape[1] and Bg.shape == Bu.shape and y.shape[1] == 2 * Bg.shape[2]
    scale = np.asarray(scale, np.float32)
    R = Bg.shape[1]
    g, u = y[:, 0::2].copy(), y[:, 1::2].copy()
    for i, a in enumerate(np.asarray(row_adapter).astype(np.int64).tolist()):
        if 0 <= a < A.shape[0]:
            t = A[a].astype(np.float64) @ x[i].astype(np.float64)
            with np.errstate(over="ignore"):
                g[i] = (g[i].astype(np.float64) + np.float64(scale[a]) * (t[:R] @ Bg[a].astype(np.float64))).astype(np.float16)
                u[i] = (u[i].astype(np.float64) + np.float64(scale[a]) * (t[R:] @ Bu[a].astype(np.float64))).astype(np.float16)
    return np.asarray(silu_mul(np.ascontiguousarray(g), np.ascontiguousarray(u)), np.float16).reshape(g.shape)


def _ptr(t) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


def shrink(x, A, row_adapter, t, rows: int | None = None) -> None:
    """tce_lora_shrink_f16: x fp16 [rows][K] (row stride x.stride(0)), A fp16 [n][R][K], row_adapter int32 [rows], t fp32 [rows][R]."""
    import torch
    from .linear import _stream
    assert x.dtype == A.dtype == torch.float16 and t.dtype == torch.float32 and row_adapter.dtype == torch.int32
    assert x.dim() == 2 and x.stride(1) == 1 and A.is_contiguous() and A.dim() == 3 and t.is_contiguous() and row_adapter.is_contiguous()
    rows = x.shape[0] if rows is None else rows
    assert row_adapter.numel() >= rows and t.numel() >= rows * A.shape[1] and x.shape[1] == A.shape[2]
    capi.check(capi.lib().tce_lora_shrink_f16(_ptr(x), x.stride(0), _ptr(A), _ptr(row_adapter), _ptr(t), rows, A.shape[2], A.shape[1], A.shape[0], C.c_void_p(_stream())))


def expand_add(t, B, scale, row_adapter, Cm, rows: int | None = None) -> None:
    """tce_lora_expand_add_f16: t fp32 [rows][R], B fp16 [n][R][N], scale fp32 [n], row_adapter int32 [rows], Cm fp16 [rows][N] (row stride Cm.stride(0)), in place."""
    import torch
    from .linear import _stream
    assert Cm.dtype == B.dtype == torch.float16 and t.dtype == scale.dtype == torch.float32 and row_adapter.dtype == torch.int32
    assert Cm.dim() == 2 and Cm.stride(1) == 1 and B.is_contiguous() and B.dim() == 3 and t.is_contiguous() and row_adapter.is_contiguous() and scale.is_contiguous()
    rows = Cm.shape[0] if rows is None else rows
    assert row_adapter.numel() >= rows and t.numel() >= rows * B.shape[1] and Cm.shape[1] == B.shape[2] and scale.numel() == B.shape[0]
    capi.check(capi.lib().tce_lora_expand_add_f16(_ptr(t), _ptr(B), _ptr(scale), _ptr(row_adapter), _ptr(Cm), Cm.stride(0), rows, B.shape[2], B.shape[1], B.shape[0],
                                                  C.c_void_p(_stream())))


def expand_silu_mul(t, Bg, Bu, scale, row_adapter, y, Cm, rows: int | None = None) -> None:
    """tce_lora_expand_silu_mul_f16: t fp32 [rows][2R], Bg / Bu fp16 [n][R][N], scale fp32 [n], row_adapter int32 [rows], y fp16 [rows][2N] (row stride y.stride(0), only
    read), Cm fp16 [rows][N] (row stride Cm.stride(0)): SiLU(g) * u of every row, g and u with the row's deltas added."""
    import torch
    from .linear import _stream
    assert Cm.dtype == y.dtype == Bg.dtype == Bu.dtype == torch.float16 and t.dtype == scale.dtype == torch.float32 and row_adapter.dtype == torch.int32
    assert Cm.dim() == y.dim() == 2 and Cm.stride(1) == y.stride(1) == 1 and Bg.is_contiguous() and Bu.is_contiguous() and Bg.dim() == 3 and Bg.shape == Bu.shape
    assert t.is_contiguous() and row_adapter.is_contiguous() and scale.is_contiguous()
    rows = Cm.shape[0] if rows is None else rows
    n, R, N = Bg.shape
    assert row_adapter.numel() >= rows and t.numel() >= rows * 2 * R and y.shape[0] >= rows and Cm.shape[1] == N and y.shape[1] == 2 * N and scale.numel() == n
    capi.check(capi.lib().tce_lora_expand_silu_mul_f16(_ptr(t), _ptr(Bg), _ptr(Bu), _ptr(scale), _ptr(row_adapter), _ptr(y), y.stride(0), _ptr(Cm), Cm.stride(0), rows, N, R, n,
                                                       C.c_void_p(_stream())))


def _shapes(block_shapes) -> dict:
    """hidden / heads / kv_heads / ffn from a dict or from anything with these attributes (a DecoderBlock); head_dim is 128."""
    get = (lambda k: block_shapes[k]) if isinstance(block_shapes, dict) else (lambda k: getattr(block_shapes, k))
    hidden, heads, ffn = int(get("hidden")), int(get("heads")), int(get("ffn"))
    kv = get("kv_heads")
    kv_heads = heads if kv is None else int(kv)
    return {"hidden": hidden, "heads": heads, "kv_heads": kv_heads, "ffn": ffn, "q": heads * 128, "kv": kv_heads * 128}


def target_shapes(block_shapes, rank: int, gate_up: bool = False) -> dict:
    """{target: (R, K, N)} of a pool of padded rank `rank`; gate_up: the fourth target too -- R = 2 * rank is the SHRINK's (A [2 * rank][hidden]); Bg and Bu are
    [rank][N] each"""
    s = _shapes(block_shapes)
    out = {"qkv": (3 * rank, s["hidden"], s["q"] + 2 * s["kv"]), "o": (rank, s["q"], s["hidden"]), "down": (rank, s["ffn"], s["hidden"])}
    if gate_up:
        out[GATE_UP] = (2 * rank, s["hidden"], s["ffn"])
    return out


def pack_adapter(block_shapes, rank: int, weights: dict, gate_up: bool = False) -> dict:
    """One layer of one adapter: weights {projection: (A [r][in], B [out][r])} in PEFT's orientation (lora_A.weight, lora_B.weight), any subset of PROJECTIONS, every
    r <= rank -> {target: (A fp16 [R][K], B fp16 [R][N])}.  A smaller rank is zero-padded, a missing projection is zeros.  qkv: the As stacked (rows p * rank .. of
    projection p), B block-structured -- rows p * rank .. hold projection p's B transposed in ITS columns of the fused output, zeros elsewhere.
    gate_up=True: gate_proj and up_proj are accepted too and the result has "gate_up": (A fp16 [2 * rank][hidden] -- gate's rows, then up's --, Bg fp16 [rank][ffn],
    Bu fp16 [rank][ffn]): segmented, no zero block."""
    s = _shapes(block_shapes)
    for name in weights:
        if name in REFUSED_PROJECTIONS and not gate_up:
            raise ValueError(f"{name}: gate / up adapters are not built (the fused SiLU * mul epilogue has no place for a delta in front of the nonlinearity)")
        if name not in PROJECTIONS + (REFUSED_PROJECTIONS if gate_up else ()):
            raise ValueError(f"{name}: not one of {PROJECTIONS + (REFUSED_PROJECTIONS if gate_up else ())}")
    shp = target_shapes(s, rank, gate_up)
    out = {t: (np.zeros((R, K), np.float16), np.zeros((R, N), np.float16)) for t, (R, K, N) in shp.items() if t != GATE_UP}
    if gate_up:
        out[GATE_UP] = (np.zeros((2 * rank, s["hidden"]), np.float16), np.zeros((rank, s["ffn"]), np.float16), np.zeros((rank, s["ffn"]), np.float16))
    place = {"gate_proj": (GATE_UP, 0, 0, s["ffn"]), "up_proj": (GATE_UP, rank, 0, s["ffn"]),
             "q_proj": ("qkv", 0, 0, s["q"]), "k_proj": ("qkv", rank, s["q"], s["kv"]), "v_proj": ("qkv", 2 * rank, s["q"] + s["kv"], s["kv"]),
             "o_proj": ("o", 0, 0, s["hidden"]), "down_proj": ("down", 0, 0, s["hidden"])}
    for name, (a, b) in weights.items():
        target, j0, n0, n = place[name]
        a, b = np.asarray(a), np.asarray(b)
        K = shp[target][1]
        if a.ndim != 2 or b.ndim != 2 or a.shape[1] != K or b.shape[0] != n or a.shape[0] != b.shape[1] or not 1 <= a.shape[0] <= rank:
            raise ValueError(f"{name}: A {a.shape} / B {b.shape}; expected A [r][{K}], B [{n}][r] with 1 <= r <= {rank}")
        r = a.shape[0]
        out[target][0][j0:j0 + r] = a.astype(np.float16)
        if target == GATE_UP:
            out[target][1 if name == "gate_proj" else 2][:r] = b.astype(np.float16).T
        else:
            out[target][1][j0:j0 + r, n0:n0 + n] = b.astype(np.float16).T
    return out


class LoraLayer:
    """One layer's view of a LoraPool: per target the device tensors A [max_adapters][R][K] and B [max_adapters][R][N], the pool's scale [max_adapters] and its
    row_adapter words.  What BatchedDecoder(..., lora=) and PagedBatchedDecoder(..., lora=) take."""

    def __init__(self, pool: "LoraPool", index: int):
        self.pool, self.index = pool, index
        self.A = {t: pool.A[t][index] for t in pool.A}
        self.B = {t: pool.B[t][index] for t in TARGETS}
        self.gate_up = pool.gate_up  # the fourth target: A["gate_up"] [max_adapters][2 * rank][hidden], Bg / Bu [max_adapters][rank][ffn]
        self.Bg, self.Bu = (pool.Bg[index], pool.Bu[index]) if pool.gate_up else (None, None)
        self.scale = pool.scale

    @property
    def row_adapter(self):
        return self.pool.row_adapter

    def workspace(self, rows: int) -> dict:
        """{target: t fp32 [rows][R]} for `rows` rows (the shrink's output; need not be zeroed); "gate_up": [rows][2 * rank]"""
        import torch
        return {t: torch.empty((rows, self.A[t].shape[1]), dtype=torch.float32, device=self.pool.device) for t in self.A}

    def shrink(self, target: str, x, t, row_adapter=None) -> None:
        shrink(x, self.A[target], self.row_adapter if row_adapter is None else row_adapter, t)

    def expand_add(self, target: str, t, Cm, row_adapter=None) -> None:
        expand_add(t, self.B[target], self.scale, self.row_adapter if row_adapter is None else row_adapter, Cm)

    def expand_silu_mul(self, t, y, Cm, row_adapter=None) -> None:
        """gate_up=True pools: t = the shrink of "gate_up", y the base gate_up linear's [rows][2 * ffn], Cm [rows][ffn]"""
        expand_silu_mul(t, self.Bg, self.Bu, self.scale, self.row_adapter if row_adapter is None else row_adapter, y, Cm)


class LoraPool:
    """Fixed storage for `max_adapters` adapters of padded rank `rank` for `layers` decoder blocks of one shape (block_shapes: hidden / heads / kv_heads / ffn as a dict,
    or a DecoderBlock).  Per target [layers][max_adapters][R][K] and [layers][max_adapters][R][N] fp16, scale fp32 [max_adapters] (alpha / r), zeros until loaded: an
    adapter that was never loaded adds exactly 0.  Works with device="cpu" (host tensors: packing and bookkeeping tests).

    row_adapter: int32 [batch] on the device, one word per SLOT, -1 everywhere; made by bind(batch) -- the decoders call it -- and shared by every layer.  A captured
    graph reads it, and load / unload are stream-ordered copies into the fixed tensors above, so neither a new adapter nor a slot that changes its adapter captures again.

    gate_up=True: the fourth target (A["gate_up"] [layers][max_adapters][2 * rank][hidden], Bg and Bu [layers][max_adapters][rank][ffn]); load accepts gate_proj and
    up_proj, and the decoders run gate/up as shrink + base linear + tce_lora_expand_silu_mul_f16.  False (the default): gate_proj / up_proj are refused, as before.
    rows_per_seq=T: a pool for the speculative step -- row_adapter is int32 [batch * T] and a slot's word stands T times (set_slot).  None (the default): one word per
    slot; such a pool is not built for rows."""

    def __init__(self, block_shapes, layers: int, max_adapters: int, rank: int, device, gate_up: bool = False, rows_per_seq: int | None = None):
        import torch
        if int(rank) != rank or rank < 8 or rank % 8 != 0 or 3 * rank > capi.TCE_LORA_MAX_RANK:
            raise ValueError(f"rank {rank}: a multiple of 8 from 8 to {capi.TCE_LORA_MAX_RANK // 3} (the fused q/k/v runs at 3 * rank <= {capi.TCE_LORA_MAX_RANK})")
        if not 1 <= int(max_adapters) <= capi.TCE_LORA_MAX_ADAPTERS:
            raise ValueError(f"max_adapters {max_adapters}: 1 .. {capi.TCE_LORA_MAX_ADAPTERS}")
        if int(layers) < 1:
            raise ValueError("layers >= 1")
        if rows_per_seq is not None and (int(rows_per_seq) != rows_per_seq or not 1 <= int(rows_per_seq) <= capi.TCE_SPEC_MAX_ROWS):
            raise ValueError(f"rows_per_seq {rows_per_seq}: None or 1 .. {capi.TCE_SPEC_MAX_ROWS} (the speculative step's rows per sequence)")
        self.shapes, self.layers, self.max_adapters, self.rank, self.device = _shapes(block_shapes), int(layers), int(max_adapters), int(rank), torch.device(device)
        self.gate_up, self.rows_per_seq = bool(gate_up), None if rows_per_seq is None else int(rows_per_seq)
        self.target_shapes = target_shapes(self.shapes, self.rank, self.gate_up)
        z = lambda *shape, dtype=torch.float16: torch.zeros(shape, dtype=dtype, device=self.device)
        self.A = {t: z(self.layers, self.max_adapters, R, K) for t, (R, K, N) in self.target_shapes.items()}
        self.B = {t: z(self.layers, self.max_adapters, R, N) for t, (R, K, N) in self.target_shapes.items() if t != GATE_UP}
        self.Bg = z(self.layers, self.max_adapters, self.rank, self.shapes["ffn"]) if self.gate_up else None
        self.Bu = z(self.layers, self.max_adapters, self.rank, self.shapes["ffn"]) if self.gate_up else None
        self.scale = z(self.max_adapters, dtype=torch.float32)
        self.row_adapter = None
        self.loaded: dict[int, float] = {}  # index -> alpha / r

    def bind(self, batch: int):
        """The shared row_adapter tensor for `batch` slots (made on the first call; every decoder of a pool has the same batch): batch * rows_per_seq words in a pool
        built for rows."""
        import torch
        words = int(batch) * (self.rows_per_seq or 1)
        if self.row_adapter is None:
            self.row_adapter = torch.full((words,), NO_ADAPTER, dtype=torch.int32, device=self.device)
        elif self.row_adapter.numel() != words:
            raise ValueError(f"the pool's row_adapter serves {self.row_adapter.numel() // (self.rows_per_seq or 1)} slots, not {batch}")
        return self.row_adapter

    def set_slot(self, slot: int, adapter: int | None) -> None:
        """The slot's word (None: -1, the base model), once per row of the slot: a stream-ordered fill of row_adapter[slot * T : (slot + 1) * T] (T = rows_per_seq or 1)"""
        T = self.rows_per_seq or 1
        self.row_adapter[int(slot) * T:(int(slot) + 1) * T] = NO_ADAPTER if adapter is None else int(adapter)

    def layer(self, index: int) -> LoraLayer:
        if not 0 <= index < self.layers:
            raise IndexError(f"layer {index} of {self.layers}")
        return LoraLayer(self, index)

    def _index(self, index) -> int:
        if int(index) != index or not 0 <= int(index) < self.max_adapters:
            raise IndexError(f"adapter {index} of {self.max_adapters}")
        return int(index)

    def load(self, index: int, weights, alpha: float) -> None:
        """weights: one {projection: (A [r][in], B [out][r])} per layer (a list, or {layer: {...}}; a missing layer or projection is zeros), PEFT's orientation; one r
        for the whole adapter; scale = alpha / r.  Everything is checked and packed on the host first; then one stream-ordered copy per layer and target."""
        import torch
        index = self._index(index)
        per_layer = dict(enumerate(weights)) if isinstance(weights, (list, tuple)) else {int(k): v for k, v in weights.items()}
        if any(not 0 <= l < self.layers for l in per_layer):
            raise ValueError(f"weights name a layer outside 0 .. {self.layers - 1}")
        ranks = {np.asarray(a).shape[0] for w in per_layer.values() for a, _ in w.values() if np.asarray(a).ndim == 2}
        packed = {l: pack_adapter(self.shapes, self.rank, w, self.gate_up) for l, w in per_layer.items()}
        if len(ranks) != 1:
            raise ValueError(f"one rank per adapter (got {sorted(ranks)}): scale = alpha / r is one number")
        scale = float(alpha) / ranks.pop()
        zero = pack_adapter(self.shapes, self.rank, {}, self.gate_up)
        for l in range(self.layers):
            for t, (a, *bs) in packed.get(l, zero).items():
                self.A[t][l, index].copy_(torch.from_numpy(a))
                for dst, b in zip((self.Bg, self.Bu) if t == GATE_UP else (self.B[t],), bs):
                    dst[l, index].copy_(torch.from_numpy(b))
        self.scale[index:index + 1].copy_(torch.tensor([scale], dtype=torch.float32))
        self.loaded[index] = scale

    def unload(self, index: int) -> None:
        """The adapter is zeros again (A, B and scale): a slot still on it computes the base model (an add of 0)."""
        index = self._index(index)
        for t in self.A:
            self.A[t][:, index].zero_()
            for b in (self.Bg, self.Bu) if t == GATE_UP else (self.B[t],):
                b[:, index].zero_()
        self.scale[index:index + 1].zero_()
        self.loaded.pop(index, None)
