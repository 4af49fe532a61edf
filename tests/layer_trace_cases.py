"""The calls a decoder layer issues, recorded as data on a host without a device -- shared by scripts/layer_trace_record.py (which writes
tests/golden/layer_trace_parent.json from the commit BEFORE a change to the host code) and tests/test_layer_trace_host.py (which holds the tree to that file).

Nothing is launched.  A DecoderBlock made without its constructor carries stub linears whose desc(...) returns a record; the attention objects and the allocator are
stubs; capi.w4a16_forward, capi.lib() (tce_silu_mul_half and the three tce_lora_* entries lora.py calls), rmsnorm_half and _stream are patched wherever the decoders
look them up; the pool is a LoraPool(device="cpu").  Every event names its tensor arguments by ROLE, never by address:

* the caller's tensors, the gammas and the pool's tensors are registered under their names (hidden, rows, gamma1, A[qkv], scale, row_adapter, ...);
* any other tensor is named when it is first WRITTEN, after the call that writes it (the first norm's output is xn, the q/k/v linear's qkv_out, gate's act, up's up, the
  unfused gate_up linear's y, a shrink's t[target], ...) and keeps that name while it lives: a second tensor in the same role is xn#2, a tensor that is read before
  anything wrote it is unknown (packed_rows where it is the residual rows the first norm reads: prefill_many's concatenation).  Step cases and the DecoderBlock.prefill case keep the names across calls, so a persistent buffer must come back under its name;
  BatchedDecoder.prefill's per-call buffers are named anew at every layer pass (TRACE.fresh_per_layer).
* a row_adapter argument that is not the pool's tensor is recorded as row_words with its VALUES (read from host memory through the pointer).
"""
import ctypes as C

import torch

from tinychatengine_amd import batch_decode, capi, decoder_block, generate, linear, lora, paged_kv
from tinychatengine_amd.batch_decode import BatchedDecoder
from tinychatengine_amd.decoder_block import DecoderBlock
from tinychatengine_amd.lora import LoraPool
from tinychatengine_amd.paged_kv import PagedBatchedDecoder

STREAM = 0x5EED
HIDDEN, HEADS, KV_HEADS, FFN, BATCH, MAX_KEYS = 128, 1, 1, 256, 4, 64
SHAPES = {"hidden": HIDDEN, "heads": HEADS, "kv_heads": KV_HEADS, "ffn": FFN}
FLAGS = {capi.TCE_W4_SILU_MUL_PAIRS: "SILU_MUL_PAIRS", capi.TCE_W4_ADD_TO_C: "ADD_TO_C"}
OUT_ROLE = {"qkv": "qkv_out", "gate": "act", "up": "up", "lm_head": "logits"}


def _ptr(v) -> int:
    if isinstance(v, torch.Tensor):
        return v.data_ptr()
    return int(v.value or 0) if isinstance(v, C.c_void_p) else int(v or 0)


class Trace:
    def __init__(self, mp):
        self.events, self.fixed, self.names, self.keep = [], {}, {}, []
        self.pair_rc, self.fresh_per_layer, self.pool = capi.TCE_OK, False, None
        mp.setattr(capi, "w4a16_forward", self._forward)
        mp.setattr(capi, "lib", lambda: self)
        for mod in (linear, batch_decode, decoder_block, lora, paged_kv, generate):
            for nm, fn in (("rmsnorm_half", self._rmsnorm), ("_stream", lambda: STREAM)):
                if hasattr(mod, nm):
                    mp.setattr(mod, nm, fn)

    # ---- names ----
    def fix(self, t, name: str):
        self.keep.append(t)
        self.fixed[t.data_ptr()] = name
        return t

    def name(self, v, written_as: str | None = None) -> str:
        if isinstance(v, torch.Tensor):
            self.keep.append(v)  # (kept alive: no later tensor takes its address)
        p = _ptr(v)
        if p in self.fixed:
            return self.fixed[p]
        if p not in self.names:
            role, k = written_as or "unknown", 1
            while (role if k == 1 else f"{role}#{k}") in self.names.values():
                k += 1
            self.names[p] = role if k == 1 else f"{role}#{k}"
        return self.names[p]

    def seen(self, t) -> str | None:
        return None if t is None else self.names.get(t.data_ptr(), "never used")

    def _words(self, ra, rows: int):
        p = _ptr(ra)
        if self.pool is not None and self.pool.row_adapter is not None and p == self.pool.row_adapter.data_ptr():
            return "row_adapter"
        return {"row_words": list((C.c_int32 * rows).from_address(p))}

    def mark(self, what: str) -> None:
        self.events.append({"call": "--", "what": what})

    # ---- the patched calls ----
    def _rmsnorm(self, x, gamma, eps, out=None):
        if self.fresh_per_layer and self.fixed.get(gamma.data_ptr()) == "gamma1":
            self.names = {}
        self.events.append({"call": "rmsnorm_half", "x": self.name(x, "packed_rows"), "gamma": self.name(gamma), "eps": eps, "out": self.name(out, "xn"), "rows": x.shape[0]})
        return out

    def _forward(self, d, st):
        pairs = bool(d["flags"] & capi.TCE_W4_SILU_MUL_PAIRS)
        role = ("act" if pairs else "y") if d["linear"] == "gate_up" else OUT_ROLE.get(d["linear"])
        rc = self.pair_rc if d["linear"] == "gate_up" and pairs else capi.TCE_OK
        self.events.append({"call": "w4a16_forward", "linear": d["linear"], "x": self.name(d["x"]), "out": self.name(d["out"], role),
                            "flags": [n for f, n in FLAGS.items() if d["flags"] & f] + ([d["flags"] & ~sum(FLAGS)] if d["flags"] & ~sum(FLAGS) else []),
                            "rows": d["x"].shape[0], "stream": st == STREAM, "rc": rc})
        return rc

    def tce_last_error(self):
        return b"stub"

    def tce_silu_mul_half(self, g, u, n, st):
        self.events.append({"call": "tce_silu_mul_half", "g": self.name(g), "u": self.name(u), "numel": n, "stream": _ptr(st) == STREAM})
        return 0

    def tce_lora_shrink_f16(self, x, ldx, A, ra, t, rows, K, R, n, st):
        a = self.name(A)
        self.events.append({"call": "tce_lora_shrink_f16", "x": self.name(x), "ldx": ldx, "A": a, "row_adapter": self._words(ra, rows), "t": self.name(t, "t[" + a[2:-1] + "]"),
                            "rows": rows, "K": K, "R": R, "n": n, "stream": _ptr(st) == STREAM})
        return 0

    def tce_lora_expand_add_f16(self, t, B, scale, ra, Cm, ldc, rows, N, R, n, st):
        self.events.append({"call": "tce_lora_expand_add_f16", "t": self.name(t), "B": self.name(B), "scale": self.name(scale), "row_adapter": self._words(ra, rows),
                            "C": self.name(Cm), "ldc": ldc, "rows": rows, "N": N, "R": R, "n": n, "stream": _ptr(st) == STREAM})
        return 0

    def tce_lora_expand_silu_mul_f16(self, t, Bg, Bu, scale, ra, y, ldy, Cm, ldc, rows, N, R, n, st):
        self.events.append({"call": "tce_lora_expand_silu_mul_f16", "t": self.name(t), "Bg": self.name(Bg), "Bu": self.name(Bu), "scale": self.name(scale),
                            "row_adapter": self._words(ra, rows), "y": self.name(y), "ldy": ldy, "C": self.name(Cm, "act"), "ldc": ldc, "rows": rows, "N": N, "R": R, "n": n,
                            "stream": _ptr(st) == STREAM})
        return 0


# ---- stubs ----
class _Linear:
    def __init__(self, name, n, k, packed=None):
        self.name, self.out_features, self.in_features, self.packed = name, n, k, packed

    def desc(self, x, out, ldc=0, flags=0, **kw):
        assert not kw and ldc == 0, "the traced layer passes x, out and flags only"
        return {"linear": self.name, "x": x, "out": out, "flags": int(flags)}


class _Attention:
    """every attention object a decoder can hold, as one stub: the contiguous step / slot(b).prefill, the paged prefill(segments, ...), the block's own prefill"""
    max_keys, cos, sin, window = MAX_KEYS, None, None, None

    def __init__(self, tr, what="attention"):
        self.tr, self.what = tr, what

    def step(self, qkv, pos_device, pos_bound, out=None):
        self.tr.events.append({"call": self.what + ".step", "qkv": self.tr.name(qkv), "pos": self.tr.name(pos_device), "pos_bound": pos_bound, "out": self.tr.name(out, "attn_out")})
        return out

    def slot(self, b):
        return _Attention(self.tr, f"{self.what}.slot({b})")

    def prefill(self, a, b, out=None, causal=None):
        qkv, where = (b, {"segments": [list(s) for s in a]}) if isinstance(b, torch.Tensor) else (a, {"pos": b})
        self.tr.events.append({"call": self.what + ".prefill", **where, "qkv": self.tr.name(qkv), "out": self.tr.name(out, "attn_out"), "causal": causal})
        return out


class _Allocator:
    def __init__(self, tr):
        self.tr, self.batch, self.pages, self.gone = tr, BATCH, [[] for _ in range(BATCH)], [0] * BATCH

    def reserve_many(self, wanted):
        self.tr.events.append({"call": "allocator.reserve_many", "wanted": [list(w) for w in wanted]})

    def writable(self, slot, pos, m):
        return True


def block(tr, packed: bool) -> DecoderBlock:
    b = object.__new__(DecoderBlock)
    b.hidden, b.heads, b.kv_heads, b.ffn, b.eps = HIDDEN, HEADS, KV_HEADS, FFN, 1e-6
    b.gamma1, b.gamma2 = tr.fix(torch.ones(HIDDEN), "gamma1"), tr.fix(torch.ones(HIDDEN), "gamma2")
    qkv_n = (HEADS + 2 * KV_HEADS) * 128
    b.qkv, b.o, b.down = _Linear("qkv", qkv_n, HIDDEN), _Linear("o", HIDDEN, HIDDEN), _Linear("down", HIDDEN, FFN)
    b.gate, b.up, b.gate_up = _Linear("gate", FFN, HIDDEN), _Linear("up", FFN, HIDDEN), _Linear("gate_up", 2 * FFN, HIDDEN, packed=object() if packed else None)
    b.attention = _Attention(tr, "block.attention")
    return b


def pool(tr, kind: str, rows_per_seq=None):
    """"none" / "default" / "gate_up"; the pool's tensors under their names"""
    if kind == "none":
        return None
    p = LoraPool(SHAPES, 1, 2, 8, "cpu", gate_up=kind == "gate_up", rows_per_seq=rows_per_seq)
    lv = p.layer(0)
    for t in lv.A:
        tr.fix(lv.A[t], f"A[{t}]")
    for t in lv.B:
        tr.fix(lv.B[t], f"B[{t}]")
    if p.gate_up:
        tr.fix(lv.Bg, "Bg"), tr.fix(lv.Bu, "Bu")
    tr.fix(p.scale, "scale")
    tr.pool = p
    return p


def rows(tr, m: int, name: str = "rows"):
    return tr.fix(torch.zeros((m, HIDDEN), dtype=torch.float16), name)


def decoder(tr, kind: str, packed: bool = False, paged: bool = False, rows_per_seq=None, blk=None):
    p = pool(tr, kind, rows_per_seq)
    blk = blk if blk is not None else block(tr, packed)
    view = None if p is None else p.layer(0)
    n = None if rows_per_seq is None else BATCH * rows_per_seq
    if paged:
        return PagedBatchedDecoder(blk, _Allocator(tr), attention=_Attention(tr), rows=n, lora=view)
    return BatchedDecoder(blk, BATCH, attention=_Attention(tr), rows=n, lora=view)


def _buffers(tr, d) -> dict:
    """the decoder's persistent buffers under the names the trace gave them"""
    return {"call": "buffers", "xn": tr.seen(d.xn), "qkv_out": tr.seen(d.qkv_out), "attn_out": tr.seen(d.attn_out), "act": tr.seen(d.act), "_up": tr.seen(d._up),
            "_gate_up_y": tr.seen(d._gate_up_y), "_lora_t": None if d._lora_t is None else {k: tr.seen(v) for k, v in d._lora_t.items()}, "LAUNCHES": d.LAUNCHES}


# ---- the cases: fn(tr) -> None, the events are tr.events ----
def _step(tr, kind, pair_rc=capi.TCE_OK):
    d = decoder(tr, kind)
    tr.pair_rc = pair_rc
    hidden = rows(tr, BATCH, "hidden")
    pos = tr.fix(torch.zeros(BATCH, dtype=torch.int32), "pos_device")
    for i in range(2):
        tr.mark(f"step {i}")
        try:
            d.step(hidden, pos, MAX_KEYS - 1)
        except capi.TceError as e:
            tr.events.append({"call": "raised", "type": "TceError", "code": e.code})
            break
    tr.events.append(_buffers(tr, d))


def _prefill(tr, kind, m, packed):
    tr.fresh_per_layer = True
    d = decoder(tr, kind, packed=packed)
    if d.lora is not None:
        d.lora.row_adapter.copy_(torch.tensor([7, -1, 3, 5], dtype=torch.int32))
    d.prefill(2, rows(tr, m), 4)


def _paged_many(tr, rows_per_seq):
    tr.fresh_per_layer = True
    d = decoder(tr, "default", paged=True, rows_per_seq=rows_per_seq)
    d.lora.row_adapter.copy_(torch.arange(10, 10 + d.lora.row_adapter.numel(), dtype=torch.int32))
    d.prefill_many([(2, rows(tr, 2, "rows a"), 0), (0, rows(tr, 3, "rows b"), 5)])


def _block_prefill(tr):
    b = block(tr, packed=True)
    for m in (3, 130, 3):
        tr.mark(f"m = {m}")
        b.prefill(rows(tr, m, f"rows m{m}"), 1)


def _two_admissions(tr, via_many: bool):
    """two sequences into a contiguous decoder: two prefill calls, or -- the same launches -- one prefill_many"""
    tr.fresh_per_layer = True
    d = decoder(tr, "default")
    d.lora.row_adapter.copy_(torch.tensor([7, -1, 3, 5], dtype=torch.int32))
    adm = [(3, rows(tr, 2, "rows a"), 0), (0, rows(tr, 3, "rows b"), 0)]
    if via_many:
        d.prefill_many(adm)
    else:
        for slot, r, pos in adm:
            d.prefill(slot, r, pos)


def _host_loop_admit(tr, paged: bool, mp):
    """HostDrivenLoop.admit with two sequences over two layers: which prefill launches the admission makes"""
    tr.fresh_per_layer = True
    decs = [decoder(tr, "none", paged=paged, blk=block(tr, False)) for _ in range(2)]
    if paged:
        for d in decs:
            d.allocator = decs[0].allocator
    table = torch.zeros((16, HIDDEN), dtype=torch.float16)
    loop = generate.HostDrivenLoop(decs, tr.fix(torch.ones(HIDDEN), "final_gamma"), _Linear("lm_head", 16, HIDDEN), table)
    loop.admit([(1, [3, 4, 5], 4), (2, [6, 7], 4)])


def _generator_admit(tr, paged: bool, mp):
    """_GeneratorBase.admit with two sequences over two layers (a BatchedGenerator made without its constructor: no sampler, no graph): the prefill launches"""
    tr.fresh_per_layer = True
    decs = [decoder(tr, "none", paged=paged, blk=block(tr, False)) for _ in range(2)]
    g = object.__new__(generate.BatchedGenerator)
    g.decoders, g.batch, g.vocab, g.max_keys, g.hidden_size, g.device = decs, BATCH, 16, MAX_KEYS, HIDDEN, torch.device("cpu")
    g.allocator = decs[0].allocator if paged else None
    g.embed_table = torch.zeros((16, HIDDEN), dtype=torch.float16)
    g.book = generate.SlotBook(BATCH, MAX_KEYS)

    class _Sampler:
        log_stride, top_k_bound, logprobs, workspace = 8, 40, False, None
        out_log = torch.zeros((BATCH, 8), dtype=torch.int32)

        def set_row(self, *a):
            pass
    g.sampler = _Sampler()
    g.pos = torch.full((BATCH,), -1, dtype=torch.int32)
    g._adm_pos, g._adm_hidden = torch.full((BATCH,), -1, dtype=torch.int32), torch.zeros((BATCH, HIDDEN), dtype=torch.float16)
    g._adm_xn = g._adm_logits = None
    g._head = lambda *a: tr.mark("head")
    g._sync = lambda: []
    mp.setattr(generate, "embed_rows", lambda table, tok, out, *a: tr.events.append({"call": "embed_rows", "rows": out.shape[0]}))
    g.admit([(1, [3, 4, 5], None, 0, 4), (2, [6, 7], None, 0, 4)])


def cases() -> dict:
    """{name: fn(tr, mp)}: the cases of tests/golden/layer_trace_parent.json"""
    out = {}
    for kind in ("none", "default", "gate_up"):
        out[f"step/{kind}"] = lambda tr, mp, kind=kind: _step(tr, kind)
        for m, packed in ((3, False), (130, True)) + (((130, False),) if kind == "none" else ()):
            out[f"prefill/contiguous/{kind}/m{m}{'/packed' if packed else ''}"] = lambda tr, mp, kind=kind, m=m, packed=packed: _prefill(tr, kind, m, packed)
    out["step/none/pairs_refused"] = lambda tr, mp: _step(tr, "none", capi.TCE_ERR_UNSUPPORTED_SHAPE)
    out["step/default/pairs_refused"] = lambda tr, mp: _step(tr, "default", capi.TCE_ERR_UNSUPPORTED_SHAPE)
    out["step/none/pairs_hip_error"] = lambda tr, mp: _step(tr, "none", capi.TCE_ERR_HIP)
    out["prefill_many/paged/default"] = lambda tr, mp: _paged_many(tr, None)
    out["prefill_many/paged/default/rows_per_seq3"] = lambda tr, mp: _paged_many(tr, 3)
    out["block_prefill/m3,m130,m3"] = lambda tr, mp: _block_prefill(tr)
    out["two_admissions/contiguous"] = lambda tr, mp: _two_admissions(tr, False)
    for paged in (False, True):
        where = "paged" if paged else "contiguous"
        out[f"host_loop_admit/{where}"] = lambda tr, mp, paged=paged: _host_loop_admit(tr, paged, mp)
        out[f"generator_admit/{where}"] = lambda tr, mp, paged=paged: _generator_admit(tr, paged, mp)
    return out


def run(fn) -> list:
    """the events of one case, under patches of its own"""
    import pytest
    with pytest.MonkeyPatch.context() as mp:
        tr = Trace(mp)
        fn(tr, mp)
        return tr.events
