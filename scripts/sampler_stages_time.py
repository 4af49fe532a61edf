#!/usr/bin/env python3
"""Tail-free and typical sampling on the clock, in ONE process on Llama-3-8B's shapes (hidden 4096, 32 query / 8 key-value heads, ffn 14336, vocabulary 128256;
--layers N, default 2 -- what is timed here sits behind the layers and does not depend on their number), 64-key pages.

    replay     BatchedGenerator.run under the captured graph at B = 1 / 4 / 16 around 512 keys, three forms that share the decoders and ALTERNATE, REPEATS times:
                 off          stages=False: tce_sample_f16, the code it was
                 identity     stages=True, every row at (1.0, 1.0): tce_sample_stages_f16 running no stage
                 stages       stages=True, every row at (tfs_z 0.95, typical_p 0.9): both stages on the 40 candidates
               device events around TOKENS tokens after WARMUP
    head       the sampler's two launches alone on fixed logits [B][128256], the same three forms, the same alternation

The yardstick is `off` in the same process.  A difference smaller than the spread of a form's own repeats is "within noise".

EXPECTATION (written down before the first run, to be confirmed or refuted by the numbers): the stages are work on at most 256 -- here 40 -- elements in one
workgroup's LDS, a dozen barriers and three short sequential walks, behind a search that already costs about 50 counting rounds with a barrier each and a select
launch that reads the whole vocabulary; `identity` adds two LDS copies and one 8-byte load.  So `identity` and `stages` should sit within the run-to-run spread of
`off` in the replay, and within a few percent of it in the head.

    python scripts/sampler_stages_time.py [--layers N] [OUT.jsonl]
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
FORMS = ("off", "identity", "stages")
PAIR = {"off": (1.0, 1.0), "identity": (1.0, 1.0), "stages": (0.95, 0.9)}


def main():
    argv = sys.argv[1:]
    layers = 2
    if "--layers" in argv:
        i = argv.index("--layers")
        layers = int(argv[i + 1])
        del argv[i:i + 2]
    out_path = argv[0] if argv else None
    import numpy as np
    import torch
    from tinychatengine_amd import capi
    from tinychatengine_amd.decoder_block import DecoderBlock
    from tinychatengine_amd.generate import BatchedGenerator, Sampler, SamplingParams
    from tinychatengine_amd.linear import Linear_half_int4
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

    def set_rows(sampler, form, B, max_new):
        z, typ = PAIR[form]
        for b in range(B):
            sampler.set_row(b, SamplingParams(tfs_z=z, typical_p=typ), 1000 + b, max_new, [b + 1])

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
        gens = {form: BatchedGenerator(paged, final_gamma, lm_head, table, max_new=1 << 12, graph=True, stages=form != "off") for form in FORMS}
        start = CONTEXT - (TOKENS + WARMUP) - 4  # the timed tokens end just below CONTEXT keys

        def place(form):
            gen = gens[form]
            set_rows(gen.sampler, form, B, 1 << 12)
            gen.pos.fill_(start)
            gen.book.pos = [start] * B
            gen.book.max_new = [1 << 12] * B
            gen.book.generated = [0] * B

        for rep in range(REPEATS):
            for form in FORMS:  # the forms alternate
                place(form)
                gens[form].run(WARMUP)
                ms = timed(gens[form].run, TOKENS)
                emit({"what": "BatchedGenerator.run (graph), one replay = one token", "form": "replay", "stages": form, "batch": B, "keys": CONTEXT, "repeat": rep,
                      "ms_per_token": round(ms, 4), "launches_per_token": gens[form].launches_per_token})
        # the sampler's two launches alone, on fixed logits
        logits = (torch.randn(B, VOCAB, device=dev) * 2.5).half()
        samplers = {form: Sampler(B, VOCAB, 4096, dev, stages=form != "off") for form in FORMS}
        pos = torch.zeros(B, dtype=torch.int32, device=dev)

        def head(s):
            def run(n):
                for _ in range(n):
                    s.step(logits, pos, 1 << 30)
            return run
        for rep in range(REPEATS):
            for form in FORMS:
                set_rows(samplers[form], form, B, 4096)
                pos.fill_(0)
                head(samplers[form])(WARMUP)
                us = timed(head(samplers[form]), 200) * 1e3
                emit({"what": "tce_sample_stages_f16 / tce_sample_f16 alone (2 launches, eager)", "form": "head", "stages": form, "batch": B, "repeat": rep,
                      "us_per_call": round(us, 2)})
        del gens, paged, alloc, samplers
        torch.cuda.empty_cache()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.writelines(lines)


if __name__ == "__main__":
    main()
