"""The decoder layer's residual rows, as SHA-256 digests, for every caller of the layer's launch sequence -- shared by scripts/layer_bits_record.py (which writes
tests/golden/layer_bits_parent.json from the commit BEFORE a host-side change) and tests/test_gpu_layer_bits.py (which holds the tree to that file).

The tiny model of tests/test_gpu_generate.py (2 layers, hidden 512, 4 query heads over 1 key / value head, ffn 1408, batch 4, 16-key pages) with max_keys 256 and 24
pages, so a 130-row prompt fits; prepacked weights; the adapters of tests/test_gpu_lora_generate.py (default pool) and tests/test_gpu_lora_rows_generate.py
(gate_up=True pools).  Every case builds decoders of its own (fresh caches) over the shared blocks and runs the rows through BOTH layers."""
import hashlib

import numpy as np
import torch

HD = 128
HIDDEN, HEADS, KV_HEADS, FFN, LAYERS = 512, 4, 1, 1408, 2
MAX_KEYS, PAGE_KEYS, BATCH, NUM_PAGES = 256, 16, 4, 24
RANK, MAX_ADAPTERS, T = 8, 4, 3
WORDS = [0, -1, 1, 2]
DIMS = {"q_proj": (HIDDEN, HEADS * HD), "k_proj": (HIDDEN, KV_HEADS * HD), "v_proj": (HIDDEN, KV_HEADS * HD), "o_proj": (HEADS * HD, HIDDEN), "down_proj": (FFN, HIDDEN),
        "gate_proj": (HIDDEN, FFN), "up_proj": (HIDDEN, FFN)}
FIVE = ("q_proj", "k_proj", "v_proj", "o_proj", "down_proj")


def _adapter(seed, names, r=RANK, gain=0.5):
    rng = np.random.default_rng(seed)
    return [{nm: ((rng.normal(0, 1, (r, DIMS[nm][0])) * DIMS[nm][0] ** -0.5).astype(np.float16), (rng.normal(0, 1, (DIMS[nm][1], r)) * gain).astype(np.float16)) for nm in names}
            for _ in range(LAYERS)]


class Model:
    def __init__(self, dev, seed=40 + HIDDEN):
        from tinychatengine_amd.decoder_block import DecoderBlock
        rng = np.random.default_rng(seed)
        ang = rng.uniform(0, 2 * np.pi, (MAX_KEYS, HD // 2))
        cos = torch.from_numpy(np.concatenate([np.cos(ang), np.cos(ang)], axis=1).astype(np.float16)).to(dev)
        sin = torch.from_numpy(np.concatenate([np.sin(ang), np.sin(ang)], axis=1).astype(np.float16)).to(dev)
        self.dev = dev
        self.blocks = [DecoderBlock(HIDDEN, HEADS, FFN, MAX_KEYS, dev, cos, sin, seed=seed + i, kv_heads=KV_HEADS) for i in range(LAYERS)]

    def pool(self, kind, rows_per_seq=None):
        """"none": None; "default": adapter 0 on the five projections, adapter 1 the same at rank 4, 2 left as zeros; "gate_up": adapter 0 on all seven, adapter 1
        gate_proj / up_proj only at rank 4, 2 left as zeros"""
        from tinychatengine_amd.lora import LoraPool
        if kind == "none":
            return None
        pool = LoraPool(self.blocks[0], LAYERS, MAX_ADAPTERS, RANK, self.dev, gate_up=kind == "gate_up", rows_per_seq=rows_per_seq)
        pool.load(0, _adapter(1, tuple(DIMS) if kind == "gate_up" else FIVE), alpha=8.0)
        pool.load(1, _adapter(2, ("gate_proj", "up_proj") if kind == "gate_up" else FIVE, r=4), alpha=8.0)
        return pool

    def decoders(self, paged, pool, rows_per_seq=None):
        from tinychatengine_amd.batch_decode import BatchedDecoder
        from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchedDecoder
        from tinychatengine_amd.speculative import SpeculativeDecoder
        view = (lambda i: None) if pool is None else pool.layer
        if not paged:
            decs = [BatchedDecoder(b, BATCH, lora=view(i)) for i, b in enumerate(self.blocks)]
        else:
            alloc = PageAllocator(NUM_PAGES, PAGE_KEYS, BATCH, MAX_KEYS // PAGE_KEYS, self.dev)
            if rows_per_seq is None:
                decs = [PagedBatchedDecoder(b, alloc, lora=view(i)) for i, b in enumerate(self.blocks)]
            else:
                decs = [SpeculativeDecoder(b, alloc, rows_per_seq, lora=view(i)) for i, b in enumerate(self.blocks)]
        if pool is not None:
            for s, w in enumerate(WORDS):
                pool.set_slot(s, None if w < 0 else w)
        return decs

    def rows(self, m, seed):
        g = torch.Generator(device=self.dev).manual_seed(seed)
        return torch.empty((m, HIDDEN), device=self.dev).normal_(0, 1, generator=g).half()


def _sha(*tensors) -> str:
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def _steps(model, paged, kind):
    """one step at position 0 and a second at position 1 -> two digests"""
    decs = model.decoders(paged, model.pool(kind))
    out = []
    for p in (0, 1):
        if paged:
            decs[0].allocator.reserve_many([(s, p) for s in range(BATCH)])
        h = model.rows(BATCH, 3 + p)
        pos = torch.full((BATCH,), p, dtype=torch.int32, device=model.dev)
        for d in decs:
            d.step(h, pos, MAX_KEYS - 1)
        out.append(_sha(h))
    return out


def _spec_steps(model):
    """SpeculativeDecoder.step, T rows per slot at positions p .. p + T - 1, p = 0 and then p = T; a gate_up=True pool built for rows"""
    decs = model.decoders(True, model.pool("gate_up", rows_per_seq=T), rows_per_seq=T)
    out = []
    for p in (0, T):
        decs[0].allocator.reserve_many([(s, p + T - 1) for s in range(BATCH)])
        h = model.rows(BATCH * T, 5 + p)
        pos = torch.tensor([p + t for _ in range(BATCH) for t in range(T)], dtype=torch.int32, device=model.dev)
        for d in decs:
            d.step(h, pos, MAX_KEYS - 1)
        out.append(_sha(h))
    return out


def _prefill(model, paged, kind, m):
    decs = model.decoders(paged, model.pool(kind))
    rows = model.rows(m, 10 + m)
    for d in decs:
        d.prefill(0 if m == 5 else 2, rows, 0)  # (words 0 and 1: both slots carry an adapter)
    return [_sha(rows)]


def _prefill_many(model):
    decs = model.decoders(True, model.pool("default"))
    adm = [(0, model.rows(5, 21), 0), (2, model.rows(7, 22), 0)]
    for d in decs:
        d.prefill_many(adm)
    return [_sha(adm[0][1], adm[1][1])]


def _block_prefill(model, m):
    rows = model.rows(m, 30 + m)
    for b in model.blocks:
        b.prefill(rows, 0)
    return [_sha(rows)]


def cases() -> dict:
    """{name: fn(model) -> [digest, ...]}; a case with several digests stands in the file as name/0, name/1"""
    out = {}
    for paged in (False, True):
        where = "paged" if paged else "contiguous"
        for kind in ("none", "default", "gate_up"):
            out[f"step/{where}/{kind}"] = lambda m, paged=paged, kind=kind: _steps(m, paged, kind)
        for kind in ("none", "default"):
            for rows in (5, 130):
                out[f"prefill/{where}/{kind}/m{rows}"] = lambda m, paged=paged, kind=kind, rows=rows: _prefill(m, paged, kind, rows)
    out["speculative_step/T3/gate_up_rows"] = _spec_steps
    out["prefill_many/paged/default/m5+m7"] = _prefill_many
    for rows in (5, 130):
        out[f"block_prefill/m{rows}"] = lambda m, rows=rows: _block_prefill(m, rows)
    return out


def run(model, name: str) -> dict:
    digests = cases()[name](model)
    return {f"{name}/{i}": d for i, d in enumerate(digests)}
