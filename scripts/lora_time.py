#!/usr/bin/env python3
"""Multi-LoRA on the clock, in ONE process on Llama-3-8B's shapes (hidden 4096, 32 query / 8 key-value heads, ffn 14336, vocabulary 128256; --layers N, default 32),
64-key pages, adapters of rank 16 (the fused q/k/v runs at R = 48), 16 adapters resident.

    replay     BatchedGenerator.run under the captured graph at B = 1 / 4 / 16 around 512 keys, four forms that ALTERNATE, REPEATS times:
                 none         lora=None: the 7 L + 5 launches the loop had
                 off          a pool, every slot's word -1: 13 L + 5 launches, the 6 L new ones leave at once
                 one          every slot on adapter 0
                 own          slot b on adapter b
               (`off`, `one` and `own` are ONE generator and ONE graph: only the words change.  `none` has decoders of its own over the same blocks and allocator.)
               device events around TOKENS tokens after WARMUP
    pair       tce_lora_shrink_f16 + tce_lora_expand_add_f16 alone per target (qkv 4096 -> 6144 at R 48, o 4096 -> 4096 and down 14336 -> 4096 at R 16), B rows, the
               words of `off` / `one` / `own`: PAIRS pairs captured in one graph, device events around its replays

EXPECTATION (written down before the first run, to be confirmed or refuted by the numbers):
  * `off` costs the launch boundaries of 6 launches per layer over `none` -- a few microseconds each under a graph, so some tens of microseconds per layer-dozen,
    independent of B;
  * `own` at B = 16 costs that plus the adapters' bytes, about 16 * R * (K + N) * 2 per target: 15.7 MB (qkv) + 4.2 MB (o) + 9.4 MB (down) = 29 MB per layer against the
    layer's ~110 MB of int4 base weights, i.e. of the order of +25 % of the layers' stream if the two kernels ran at the base kernels' bandwidth; they will not (few workgroups, each a short dependent chain of loads), so more than that is expected;
  * `one` reads ONE adapter's bytes whatever B is (rows that share an adapter share its read within a block of 4 rows, and the blocks after the first find it in the L2): close to `off`.

    python scripts/lora_time.py [--layers N] [OUT.jsonl]
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BATCHES = (1, 4, 16)
CONTEXT, PAGE_KEYS = 512, 64
REPEATS = 3
TOKENS, WARMUP = 50, 5
PAIRS = 50
HIDDEN, HEADS, KV_HEADS, FFN, VOCAB = 4096, 32, 8, 14336, 128256
RANK, ADAPTERS = 16, 16
FORMS = ("none", "off", "one", "own")


def words(form, B):
    return [-1] * B if form == "off" else [0] * B if form == "one" else list(range(B))


def main():
    argv = sys.argv[1:]
    layers = 32
    if "--layers" in argv:
        i = argv.index("--layers")
        layers = int(argv[i + 1])
        del argv[i:i + 2]
    out_path = argv[0] if argv else None
    import numpy as np
    import torch
    from tinychatengine_amd import capi
    from tinychatengine_amd.decoder_block import DecoderBlock
    from tinychatengine_amd.generate import BatchedGenerator, SamplingParams
    from tinychatengine_amd.linear import Linear_half_int4
    from tinychatengine_amd.lora import TARGETS, LoraPool
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchedDecoder
    assert torch.cuda.is_available(), "a GPU measurement: no device, no number"
    capi.lib()
    dev = torch.device("cuda:0")
    hd = 128
    ang = np.random.default_rng(0).uniform(0, 2 * np.pi, (CONTEXT, hd // 2))
    cos = torch.from_numpy(np.concatenate([np.cos(ang), np.cos(ang)], axis=1).astype(np.float16)).to(dev)
    sin = torch.from_numpy(np.concatenate([np.sin(ang), np.sin(ang)], axis=1).astype(np.float16)).to(dev)
    blocks = [DecoderBlock(HIDDEN, HEADS, FFN, CONTEXT, dev, cos, sin, seed=100 + i, kv_heads=KV_HEADS) for i in range(layers)]
    g = torch.Generator(device=dev).manual_seed(7)
    final_gamma = (1.0 + 0.1 * torch.empty(HIDDEN, device=dev).normal_(0, 1, generator=g)).float()
    lm_head = Linear_half_int4.from_float(torch.empty(VOCAB, HIDDEN, device=dev).normal_(0.0, HIDDEN ** -0.5, generator=g)).prepack()
    table = torch.empty(VOCAB, HIDDEN, device=dev).normal_(0.0, 1.0, generator=g).half()
    lines = []

    def emit(rec):
        rec.update({"layers": layers, "hidden": HIDDEN, "rank": RANK, "adapters": ADAPTERS})
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec) + "\n")

    def timed(run, n):
        a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        run(n)
        b_.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b_) / n

    def filled_pool():
        """every adapter dense and small (the device's random numbers: what is timed does not depend on the values; the fused q/k/v keeps its zero blocks' BYTES)"""
        pool = LoraPool(blocks[0], layers, ADAPTERS, RANK, dev)
        for t in TARGETS:
            pool.A[t].normal_(0, 0.01)
            pool.B[t].normal_(0, 0.01)
        pool.scale.fill_(2.0)
        return pool

    pages_per_seq = CONTEXT // PAGE_KEYS
    for B in BATCHES:
        num_pages = 2 * B * pages_per_seq
        alloc = PageAllocator(num_pages, PAGE_KEYS, B, pages_per_seq, dev, free_order=np.random.default_rng(B).permutation(num_pages).tolist())
        for i in range(pages_per_seq):
            for b in range(B):
                alloc.reserve(b, (i + 1) * PAGE_KEYS - 1)
        pool = filled_pool()
        decs = {"none": [PagedBatchedDecoder(b, alloc) for b in blocks], "pool": [PagedBatchedDecoder(b, alloc, lora=pool.layer(i)) for i, b in enumerate(blocks)]}
        for ds in decs.values():
            for dp in ds:
                dp.attention.k_pool.normal_(0, 0.8)
                dp.attention.v_pool.normal_(0, 0.8)
        gens = {"none": BatchedGenerator(decs["none"], final_gamma, lm_head, table, max_new=1 << 12, graph=True),
                "pool": BatchedGenerator(decs["pool"], final_gamma, lm_head, table, max_new=1 << 12, graph=True, lora=pool)}
        start = CONTEXT - (TOKENS + WARMUP) - 4  # the timed tokens end just below CONTEXT keys

        def place(form):
            gen = gens["none" if form == "none" else "pool"]
            for b in range(B):
                gen.sampler.set_row(b, SamplingParams(), 1000 + b, 1 << 12, [b + 1])
            gen.pos.fill_(start)
            gen.book.pos = [start] * B
            gen.book.max_new = [1 << 12] * B
            gen.book.generated = [0] * B
            if form != "none":
                pool.row_adapter.copy_(torch.tensor(words(form, B), dtype=torch.int32))
            return gen

        for rep in range(REPEATS):
            for form in FORMS:  # the forms alternate
                gen = place(form)
                gen.run(WARMUP)
                ms = timed(gen.run, TOKENS)
                emit({"what": "BatchedGenerator.run (graph), one replay = one token", "form": "replay", "lora": form, "batch": B, "keys": CONTEXT, "repeat": rep,
                      "ms_per_token": round(ms, 4), "launches_per_token": gen.launches_per_token})
        # the two new launches alone, per target: PAIRS pairs in one graph
        lv = pool.layer(0)
        shapes = pool.target_shapes
        for target in TARGETS:
            R, K, N = shapes[target]
            x = torch.randn(B, K, device=dev).half()
            c = torch.randn(B, N, device=dev).half()
            t = torch.empty(B, R, dtype=torch.float32, device=dev)

            def pairs():
                for _ in range(PAIRS):
                    lv.shrink(target, x, t)
                    lv.expand_add(target, t, c)
            pool.row_adapter.fill_(-1)
            pairs()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                pairs()

            def replay(n):
                for _ in range(n):
                    graph.replay()
            for rep in range(REPEATS):
                for form in FORMS[1:]:
                    pool.row_adapter.copy_(torch.tensor(words(form, B), dtype=torch.int32))
                    c.normal_(0, 1)  # (the expand accumulates into c: keep it finite)
                    replay(2)
                    us = timed(replay, 10) * 1e3 / PAIRS
                    touched = 0 if form == "off" else (1 if form == "one" else B) * R * (K + N) * 2
                    emit({"what": "tce_lora_shrink_f16 + tce_lora_expand_add_f16 alone (graph of %d pairs)" % PAIRS, "form": "pair", "target": target, "R": R, "K": K, "N": N,
                          "lora": form, "batch": B, "repeat": rep, "us_per_pair": round(us, 2), "adapter_bytes": touched})
            del graph
        del gens, decs, alloc, pool
        torch.cuda.empty_cache()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.writelines(lines)


if __name__ == "__main__":
    main()
