#!/usr/bin/env python3
"""Mirostat on the clock, in ONE process on Llama-3-8B's shapes (hidden 4096, 32 query / 8 key-value heads, ffn 14336, vocabulary 128256; --layers N, default 2 --
what is timed here sits behind the layers and does not depend on their number), 64-key pages.

    replay     BatchedGenerator.run under the captured graph at B = 1 / 4 / 16 around 512 keys, four forms that share the decoders and ALTERNATE, REPEATS times:
                 off          stages=True, mirostat_rows=False: tce_sample_stages_f16 at (1.0, 1.0), the code it was
                 mode0        mirostat_rows=True, every row mode 0: tce_sample_mirostat_f16 running no mirostat
                 mode1        every row mirostat 1 (tau 5, eta 0.1, m 100) on its 40 candidates
                 mode2        every row mirostat 2 (tau 5, eta 0.1)
               device events around TOKENS tokens after WARMUP
    head       the sampler's two launches alone on fixed logits [B][128256], the same four forms, the same alternation

The yardstick is `off` in the same process.  A difference smaller than the spread of a form's own repeats is "within noise" (DESIGN.md section 5).
    spec       SpeculativeGenerator.run under the captured graph, B = 4, T = 4 (M = 16 rows), scripted wrong drafts (all T rows of a slot active, one token kept per
               step), four forms alternating: off (stages=True, tce_sample_verify_stages_f16: 3 sampler launches), mode0 / mode1 / mode2 with mirostat_rows=True
               (tce_sample_verify_mirostat_f16: 4 launches, a mirostat sequence's rows walked in order with mu carried)

EXPECTATION (written down before the first run, to be confirmed or refuted by the numbers): `mode0` adds one 4-byte load of the row's mode and a uniform branch to
the STG = true draw kernel, so it should sit within the run-to-run spread of `off`.  `mode2` replaces two softmaxes and a top-p walk by one softmax, a log2f per
candidate and two short walks: level with `off` or below it.  `mode1` adds two logf per candidate, a 39-term walk and three fp64 pow calls per row: a microsecond or
two in the head, invisible in the replay.  The speculative replay gains one launch with the flag (about 2 us of launch and boundary even where no row runs
mirostat), and for mirostat sequences the walk does T rows one after the other in one workgroup, where the draw launch did them side by side: a few microseconds more.

    python scripts/mirostat_time.py [--layers N] [OUT.jsonl]
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
SPEC_B, SPEC_T, SPEC_STEPS = 4, 4, 20
HIDDEN, HEADS, KV_HEADS, FFN, VOCAB = 4096, 32, 8, 14336, 128256
FORMS = ("off", "mode0", "mode1", "mode2")
MODE = {"off": 0, "mode0": 0, "mode1": 1, "mode2": 2}


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
    from tinychatengine_amd.speculative import SpeculativeDecoder, SpeculativeGenerator
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
        for b in range(B):
            sampler.set_row(b, SamplingParams(mirostat=MODE[form]), 1000 + b, max_new, [b + 1])

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
        gens = {form: BatchedGenerator(paged, final_gamma, lm_head, table, max_new=1 << 12, graph=True, stages=True, mirostat_rows=form != "off") for form in FORMS}
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
                emit({"what": "BatchedGenerator.run (graph), one replay = one token", "form": "replay", "mirostat": form, "batch": B, "keys": CONTEXT, "repeat": rep,
                      "ms_per_token": round(ms, 4), "launches_per_token": gens[form].launches_per_token})
        # the sampler's two launches alone, on fixed logits
        logits = (torch.randn(B, VOCAB, device=dev) * 2.5).half()
        samplers = {form: Sampler(B, VOCAB, 4096, dev, stages=True, mirostat_rows=form != "off") for form in FORMS}
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
                emit({"what": "tce_sample_mirostat_f16 / tce_sample_stages_f16 alone (2 launches, eager)", "form": "head", "mirostat": form, "batch": B, "repeat": rep,
                      "us_per_call": round(us, 2)})
        del gens, paged, alloc, samplers
        torch.cuda.empty_cache()
    # ---- one speculative replay, T = 4, with and without the flag ----
    B, T = SPEC_B, SPEC_T
    num_pages = 2 * B * pages_per_seq
    alloc = PageAllocator(num_pages, PAGE_KEYS, B, pages_per_seq, dev, free_order=np.random.default_rng(B).permutation(num_pages).tolist())
    for i in range(pages_per_seq):
        for b in range(B):
            alloc.reserve(b, (i + 1) * PAGE_KEYS - 1)
    decs = [SpeculativeDecoder(b, alloc, T) for b in blocks]
    for dp in decs:
        dp.attention.k_pool.normal_(0, 0.8)
        dp.attention.v_pool.normal_(0, 0.8)
    gens = {flag: SpeculativeGenerator(decs, final_gamma, lm_head, table, max_new=1 << 12, graph=True, script=True, stages=True, mirostat_rows=flag) for flag in (False, True)}
    start = CONTEXT - (SPEC_STEPS + WARMUP) * T - 8
    for rep in range(REPEATS):
        for form in FORMS:
            gen = gens[form != "off"]
            set_rows(gen.sampler, form, B, 1 << 12)
            gen.pos.fill_(start)
            gen.book.pos = [start] * B
            gen.book.max_new = [1 << 12] * B
            gen.book.generated = [0] * B
            gen.history.fill_(1)
            gen.script.fill_(5)  # every row t >= 1 is fed a (wrong) draft: all T rows of a slot are active, a step emits one token
            gen.run(WARMUP, record=False)
            ms = timed(lambda n: gen.run(n, record=False), SPEC_STEPS)
            emit({"what": "SpeculativeGenerator.run (graph), one replay = one step of T rows per slot (scripted wrong drafts: all T rows active, one token kept)", "form": "spec",
                  "mirostat": form, "batch": B, "rows_per_seq": T, "keys": CONTEXT, "repeat": rep, "ms_per_step": round(ms, 4), "launches_per_step": gen.launches_per_token})
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.writelines(lines)


if __name__ == "__main__":
    main()
