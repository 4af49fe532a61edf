#!/usr/bin/env python3
"""Generation on the clock: what one token costs once the loop is closed on the device, in ONE process on Llama-3-8B's shapes (32 layers, hidden 4096, 32 query /
8 key-value heads, ffn 14336, vocabulary 128256), B in {8, 16}, around 512 and 2048 keys, 64-key pages.  Three forms on the SAME decoders, alternating, REPEATS times:

    generate   BatchedGenerator.run: embed + 32 x 7 launches + final norm + lm_head + tce_sample_f16 in one captured graph, one replay per token, no host round trip
               (sampled: k 40, top_p 0.95, temp 0.8, repeat 1.1 -- the reference's defaults)
    host       HostDrivenLoop.step: the same launches eagerly, then logits [B][128256] copied to the host, a numpy argmax, the rows looked up on the host and copied
               back -- a synchronise and two copies per token: the only way to continue a sequence before tce_sample_f16 / tce_embed_rows_f16, the baseline
    layers     the layers-only graph step as scripts/paged_decode_time.py times it: what the final norm, lm_head, sampling and the embedding add

    python scripts/generate_time.py [OUT.jsonl]           device events around 50 tokens after 5 warm-up tokens, per form and repeat
    python scripts/generate_time.py --eager [OUT.jsonl]   B = 16, 2048 keys, the generator's launches without a graph, 10 tokens: the driver for a
                                                          rocprofv3 --kernel-trace --stats run of its own (the sampling and embedding launches beside lm_head's)

The caches hold random numbers and the positions are set, not reached: a 2048-token prefill of 16 prompts is not what is timed here.
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BATCHES = (8, 16)
CONTEXTS = (512, 2048)
PAGE_KEYS = 64
REPEATS = 3
TOKENS, WARMUP = 50, 5
LAYERS, HIDDEN, HEADS, KV_HEADS, FFN, VOCAB = 32, 4096, 32, 8, 14336, 128256


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    eager = "--eager" in sys.argv
    out_path = args[0] if args else None
    import numpy as np
    import torch
    from tinychatengine_amd import capi
    from tinychatengine_amd.decoder_block import DecoderBlock
    from tinychatengine_amd.generate import BatchedGenerator, HostDrivenLoop, SamplingParams
    from tinychatengine_amd.linear import Linear_half_int4
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchedDecoder
    assert torch.cuda.is_available(), "a GPU measurement: no device, no number"
    capi.lib()
    dev = torch.device("cuda:0")
    hd, ctx_max = 128, max(CONTEXTS)
    ang = np.random.default_rng(0).uniform(0, 2 * np.pi, (ctx_max, hd // 2))
    cos = torch.from_numpy(np.concatenate([np.cos(ang), np.cos(ang)], axis=1).astype(np.float16)).to(dev)
    sin = torch.from_numpy(np.concatenate([np.sin(ang), np.sin(ang)], axis=1).astype(np.float16)).to(dev)
    blocks = [DecoderBlock(HIDDEN, HEADS, FFN, ctx_max, dev, cos, sin, seed=100 + i, kv_heads=KV_HEADS) for i in range(LAYERS)]
    g = torch.Generator(device=dev).manual_seed(7)
    final_gamma = (1.0 + 0.1 * torch.empty(HIDDEN, device=dev).normal_(0, 1, generator=g)).float()
    lm_head = Linear_half_int4.from_float(torch.empty(VOCAB, HIDDEN, device=dev).normal_(0.0, HIDDEN ** -0.5, generator=g)).prepack()
    table = torch.empty(VOCAB, HIDDEN, device=dev).normal_(0.0, 1.0, generator=g).half()
    lines = []

    def emit(rec):
        rec.update({"layers": LAYERS, "hidden": HIDDEN, "heads": HEADS, "kv_heads": KV_HEADS, "ffn": FFN, "vocab": VOCAB, "page_keys": PAGE_KEYS})
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec) + "\n")

    def timed(run, tokens):
        a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        run(tokens)
        b_.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b_) / tokens

    for B in ((16,) if eager else BATCHES):
        pages_per_seq = ctx_max // PAGE_KEYS
        num_pages = 2 * B * pages_per_seq
        alloc = PageAllocator(num_pages, PAGE_KEYS, B, pages_per_seq, dev, free_order=np.random.default_rng(B).permutation(num_pages).tolist())
        for i in range(pages_per_seq):  # slot by slot in turn: a sequence's pages are scattered over the pool
            for b in range(B):
                alloc.reserve(b, (i + 1) * PAGE_KEYS - 1)
        paged = [PagedBatchedDecoder(b, alloc) for b in blocks]
        for dp in paged:
            dp.attention.k_pool.normal_(0, 0.8)
            dp.attention.v_pool.normal_(0, 0.8)
        gen = BatchedGenerator(paged, final_gamma, lm_head, table, max_new=1 << 14, graph=not eager)
        host = HostDrivenLoop(paged, final_gamma, lm_head, table)
        for b in range(B):
            gen.sampler.set_row(b, SamplingParams(), 1000 + b, 1 << 14, [b + 1])
            host.max_new[b] = 1 << 30
        h0 = torch.randn(B, HIDDEN, device=dev).to(torch.float16)
        h = h0.clone()
        pos_fixed = torch.zeros(B, dtype=torch.int32, device=dev)
        for ctx in ((2048,) if eager else CONTEXTS):
            start = ctx - (TOKENS + WARMUP) - 4  # the timed tokens end just below ctx keys

            def run_generate(n):
                gen.run(n)

            def run_host(n):
                for _ in range(n):
                    host.step()

            def place():
                gen.pos.fill_(start)
                gen.book.pos = [start] * B
                gen.book.max_new = [1 << 14] * B
                gen.book.generated = [int(v) for v in gen.sampler.generated()]
                host.pos_host[:] = start
            if eager:
                place()
                gen.run(10)
                emit({"what": "eager generator tokens for a kernel trace", "batch": B, "keys": ctx, "tokens": 10, "launches_per_token": gen.launches_per_token})
                continue
            pos_fixed.fill_(ctx - 1)

            def layers_step():
                h.copy_(h0)
                for d in paged:
                    d.step(h, pos_fixed, ctx - 1)
            layers_step()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                layers_step()

            def run_layers(n):
                for _ in range(n):
                    graph.replay()
            forms = {"generate": run_generate, "host": run_host, "layers": run_layers}
            for rep in range(REPEATS):
                for form, run in forms.items():  # the forms alternate
                    place()
                    run(WARMUP)
                    ms = timed(run, TOKENS)
                    emit({"what": {"generate": "BatchedGenerator.run (graph, device sampling)", "host": "HostDrivenLoop.step (logits to the host, numpy argmax, rows copied back)",
                                   "layers": "PagedBatchedDecoder.step x 32 (graph, no lm_head)"}[form], "form": form, "batch": B, "keys": ctx, "repeat": rep,
                          "ms_per_token": round(ms, 4), "tokens_per_s": round(B * 1e3 / ms, 1),
                          "launches_per_token": gen.launches_per_token if form != "layers" else LAYERS * PagedBatchedDecoder.LAUNCHES})
            del graph
        del gen, host, paged, alloc
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            f.writelines(lines)


if __name__ == "__main__":
    main()
