#!/usr/bin/env python3
"""Log-probabilities on the clock, in ONE process on Llama-3-8B's shapes (hidden 4096, 32 query / 8 key-value heads, ffn 14336, vocabulary 128256; --layers N,
default 32 -- what is timed here sits behind the layers and does not depend on their number), 64-key pages.

    replay     BatchedGenerator.run under the captured graph with logprobs on (tce_sample_logprobs_f16) against off (tce_sample_f16: the code it was), at B = 1 / 4 / 16
               around 512 keys; the two generators share the decoders and alternate, REPEATS times; device events around TOKENS tokens after WARMUP
    head       the sampling call alone on fixed logits [B][128256], on against off, the same alternation (2 launches either way): what the LSE adds where it is added
    score      tce_logprobs_f16's two launches on one 256-row chunk of logits [256][128256] (score() makes them once per chunk), beside lm_head at M = 256, which
               produces the chunk
    delta      BatchedGenerator.score on e4m3 pages against fp16 pages, the same synthetic model and prompts: mean and maximum |difference of logprob|.  REPORTED,
               never asserted -- it depends on the data --, and synthetic Gaussian weights say NOTHING about a real model's perplexity on e4m3 pages: the figure shows
               that the measure exists and what it costs, not what a model loses.

    python scripts/logprob_time.py [--layers N] [OUT.jsonl]
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
HIDDEN, HEADS, KV_HEADS, FFN, VOCAB = 4096, 32, 8, 14336, 128256
CHUNK_ROWS = 256
SCORE_PROMPTS, SCORE_TOKENS = 4, 128


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
    from tinychatengine_amd.generate import BatchedGenerator, Sampler, SamplingParams, perplexity
    from tinychatengine_amd.linear import Linear_half_int4, _stream
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
        rec.update({"layers": layers, "hidden": HIDDEN, "vocab": VOCAB})
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

    pages_per_seq = CONTEXT // PAGE_KEYS
    for B in BATCHES:
        num_pages = 2 * B * pages_per_seq
        alloc = PageAllocator(num_pages, PAGE_KEYS, B, pages_per_seq, dev, free_order=np.random.default_rng(B).permutation(num_pages).tolist())
        for i in range(pages_per_seq):
            for b in range(B):
                alloc.reserve(b, (i + 1) * PAGE_KEYS - 1)
        paged = [PagedBatchedDecoder(b, alloc) for b in blocks]
        for dp in paged:
            dp.attention.k_pool.normal_(0, 0.8)
            dp.attention.v_pool.normal_(0, 0.8)
        gens = {on: BatchedGenerator(paged, final_gamma, lm_head, table, max_new=1 << 12, graph=True, logprobs=on) for on in (False, True)}
        start = CONTEXT - (TOKENS + WARMUP) - 4  # the timed tokens end just below CONTEXT keys

        def place(gen):
            for b in range(B):
                gen.sampler.set_row(b, SamplingParams(), 1000 + b, 1 << 12, [b + 1])
            gen.pos.fill_(start)
            gen.book.pos = [start] * B
            gen.book.max_new = [1 << 12] * B
            gen.book.generated = [0] * B

        for rep in range(REPEATS):
            for on in (False, True):  # the two forms alternate
                place(gens[on])
                gens[on].run(WARMUP)
                ms = timed(gens[on].run, TOKENS)
                emit({"what": "BatchedGenerator.run (graph), one replay = one token", "form": "replay", "logprobs": on, "batch": B, "keys": CONTEXT, "repeat": rep,
                      "ms_per_token": round(ms, 4), "launches_per_token": gens[on].launches_per_token})
        # the sampling call alone, on fixed logits
        logits = (torch.randn(B, VOCAB, device=dev) * 2.5).half()
        samplers = {on: Sampler(B, VOCAB, 4096, dev, logprobs=on) for on in (False, True)}
        pos = torch.zeros(B, dtype=torch.int32, device=dev)

        def head(s):
            def run(n):
                for _ in range(n):
                    s.step(logits, pos, 1 << 30)
            return run
        for rep in range(REPEATS):
            for on in (False, True):
                for b in range(B):
                    samplers[on].set_row(b, SamplingParams(), 1000 + b, 4096, [b + 1])
                pos.fill_(0)
                head(samplers[on])(WARMUP)
                us = timed(head(samplers[on]), 200) * 1e3
                emit({"what": "tce_sample_logprobs_f16 / tce_sample_f16 alone (2 launches, eager)", "form": "head", "logprobs": on, "batch": B, "repeat": rep,
                      "us_per_call": round(us, 2)})
        del gens, paged, alloc, samplers
        torch.cuda.empty_cache()

    # scoring: the two launches per 256-row chunk, beside the lm_head launch that produces the chunk
    xn = torch.randn(CHUNK_ROWS, HIDDEN, device=dev).half()
    logits = torch.empty((CHUNK_ROWS, VOCAB), dtype=torch.float16, device=dev)
    target = torch.randint(0, VOCAB, (CHUNK_ROWS,), device=dev, dtype=torch.int32)
    out = torch.empty(CHUNK_ROWS, dtype=torch.float32, device=dev)
    partials = torch.empty(int(capi.lib().tce_logprobs_workspace_bytes(CHUNK_ROWS, VOCAB)), dtype=torch.uint8, device=dev)

    def run_head(n):
        for _ in range(n):
            capi.check(capi.w4a16_forward(lm_head.desc(xn, logits), _stream()))

    def run_score(n):
        for _ in range(n):
            capi.check(capi.logprobs_f16(logits.data_ptr(), VOCAB, VOCAB, CHUNK_ROWS, target.data_ptr(), out.data_ptr(), None, partials.data_ptr(), _stream()))
    for rep in range(REPEATS):
        for form, run in (("lm_head at M = 256", run_head), ("tce_logprobs_f16 (2 launches), 256 rows", run_score)):
            run(3)
            emit({"what": form, "form": "score", "rows": CHUNK_ROWS, "repeat": rep, "us_per_call": round(timed(run, 20) * 1e3, 2),
                  "logits_bytes": CHUNK_ROWS * VOCAB * 2})
    del xn, logits

    # e4m3 pages against fp16 pages through score(): reported, not asserted
    rng = np.random.default_rng(11)
    prompts = [rng.integers(0, VOCAB, SCORE_TOKENS).tolist() for _ in range(SCORE_PROMPTS)]
    values = {}
    for kv_dtype in ("fp16", "fp8_e4m3"):
        alloc = PageAllocator(SCORE_PROMPTS * pages_per_seq, PAGE_KEYS, SCORE_PROMPTS, pages_per_seq, dev)
        kw = dict(kv_dtype=kv_dtype, k_scale_log2=-1, v_scale_log2=-1) if kv_dtype != "fp16" else {}
        gen = BatchedGenerator([PagedBatchedDecoder(b, alloc, **kw) for b in blocks], final_gamma, lm_head, table, max_new=8, graph=False)
        values[kv_dtype] = np.concatenate(gen.score(prompts, chunk_rows=CHUNK_ROWS))
        del gen, alloc
        torch.cuda.empty_cache()
    d = np.abs(values["fp16"].astype(np.float64) - values["fp8_e4m3"].astype(np.float64))
    emit({"what": "score() on e4m3 pages against fp16 pages, SYNTHETIC Gaussian weights and random prompts: says nothing about a real model's perplexity",
          "form": "delta", "prompts": SCORE_PROMPTS, "tokens_per_prompt": SCORE_TOKENS, "values": int(d.size), "mean_abs_delta_logprob": float(d.mean()),
          "max_abs_delta_logprob": float(d.max()), "perplexity_fp16": perplexity(values["fp16"]), "perplexity_fp8_e4m3": perplexity(values["fp8_e4m3"])})
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.writelines(lines)


if __name__ == "__main__":
    main()
