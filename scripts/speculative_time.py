#!/usr/bin/env python3
"""Speculative decoding on the clock: SpeculativeGenerator (T rows per sequence and replay) against BatchedGenerator (one row) in ONE process on Llama-3-8B's shapes
(32 layers, hidden 4096, 32 query / 8 key-value heads, ffn 14336, vocabulary 128256), B in {1, 4, 16}, around 512 and 2048 keys, T in {2, 4, 8}, 64-key pages.
The forms alternate, REPEATS times, device events around STEPS replays after WARMUP:

    plain      BatchedGenerator.run: 7 L + 5 launches, one token per sequence and replay
    spec       SpeculativeGenerator.run: 7 L + 7 launches at M = B T, 1 .. T tokens per sequence and replay.  The script hook decides how many: a discovery run with
               an all -1 script records each slot's plain tokens from the placed position; the timed runs feed them back as drafts
                   accept=none   every draft wrong: the rows are computed and rejected, one token per replay
                   accept=half   replays alternate between all drafts right and the first one wrong: (T - 1) / 2 drafts accepted per replay on average
                   accept=all    every draft right: T tokens per replay
               tokens are COUNTED from the device's `generated` words, not assumed.
    (i)  replay_ratio = ms per spec replay / ms per plain replay: the break-even acceptance is (replay_ratio - 1) / (T - 1) of the drafts
    (ii) tokens_per_s per form

    python scripts/speculative_time.py [OUT.jsonl]                 the sweep
    python scripts/speculative_time.py --attention [OUT.jsonl]     the attention launch alone: the rows form against T single-row launches (one layer, graph replays)
    python scripts/speculative_time.py --quick ...                 B = 4, 512 keys, T = 4 only

The caches hold random numbers and the positions are set, not reached, as in scripts/generate_time.py.
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BATCHES = (1, 4, 16)
CONTEXTS = (512, 2048)
ROWS = (2, 4, 8)
PAGE_KEYS = 64
REPEATS = 3
STEPS, WARMUP = 24, 3
LAYERS, HIDDEN, HEADS, KV_HEADS, FFN, VOCAB = 32, 4096, 32, 8, 14336, 128256


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    quick, attention_only = "--quick" in sys.argv, "--attention" in sys.argv
    out_path = args[0] if args else None
    import numpy as np
    import torch
    from tinychatengine_amd import capi
    from tinychatengine_amd.decoder_block import DecoderBlock
    from tinychatengine_amd.generate import BatchedGenerator, SamplingParams
    from tinychatengine_amd.linear import Linear_half_int4
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchDecodeAttention, PagedBatchedDecoder
    from tinychatengine_amd.speculative import PagedRowsDecodeAttention, SpeculativeDecoder, SpeculativeGenerator
    assert torch.cuda.is_available(), "a GPU measurement: no device, no number"
    capi.lib()
    dev = torch.device("cuda:0")
    batches, contexts, rows = ((4,), (512,), (4,)) if quick else (BATCHES, CONTEXTS, ROWS)
    hd, ctx_max = 128, max(contexts)
    ang = np.random.default_rng(0).uniform(0, 2 * np.pi, (ctx_max, hd // 2))
    cos = torch.from_numpy(np.concatenate([np.cos(ang), np.cos(ang)], axis=1).astype(np.float16)).to(dev)
    sin = torch.from_numpy(np.concatenate([np.sin(ang), np.sin(ang)], axis=1).astype(np.float16)).to(dev)
    lines = []

    def emit(rec):
        rec.update({"layers": LAYERS, "hidden": HIDDEN, "heads": HEADS, "kv_heads": KV_HEADS, "ffn": FFN, "vocab": VOCAB, "page_keys": PAGE_KEYS})
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

    def allocator(B):
        pages_per_seq = ctx_max // PAGE_KEYS
        num_pages = B * pages_per_seq
        alloc = PageAllocator(num_pages, PAGE_KEYS, B, pages_per_seq, dev, free_order=np.random.default_rng(B).permutation(num_pages).tolist())
        for i in range(pages_per_seq):  # slot by slot in turn: a sequence's pages are scattered over the pool
            for b in range(B):
                alloc.reserve(b, (i + 1) * PAGE_KEYS - 1)
        return alloc

    if attention_only:
        for B in batches:
            alloc = allocator(B)
            for ctx in contexts:
                for T in rows:
                    R = PagedRowsDecodeAttention(alloc, HEADS, KV_HEADS, dev, cos, sin, rows_per_seq=T)
                    S = PagedBatchDecodeAttention(alloc, HEADS, KV_HEADS, dev, cos, sin)
                    for P in (R, S):
                        P.k_pool.normal_(0, 0.8)
                        P.v_pool.normal_(0, 0.8)
                    qkv = torch.randn(B * T, (HEADS + 2 * KV_HEADS) * hd, device=dev).half()
                    start = ctx - T - 1
                    pos_rows = (torch.arange(T, dtype=torch.int32, device=dev)[None, :] + start).repeat(B, 1).reshape(-1).contiguous()
                    pos_t = [torch.full((B,), start + t, dtype=torch.int32, device=dev) for t in range(T)]
                    q_t = [qkv.view(B, T, -1)[:, t].contiguous() for t in range(T)]
                    out_r, out_s = torch.empty(B * T, HEADS * hd, dtype=torch.float16, device=dev), torch.empty(B, HEADS * hd, dtype=torch.float16, device=dev)

                    def rows_form():
                        R.step(qkv, pos_rows, ctx - 1, out=out_r)

                    def single_steps():
                        for t in range(T):
                            S.step(q_t[t], pos_t[t], ctx - 1, out=out_s)
                    graphs = {}
                    for name, fn in (("rows", rows_form), ("single", single_steps)):
                        fn()
                        torch.cuda.synchronize()
                        graphs[name] = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(graphs[name]):
                            for _ in range(10):
                                fn()
                    for rep in range(REPEATS):
                        for name, gr in graphs.items():
                            gr.replay()
                            ms = timed(lambda n: [gr.replay() for _ in range(n)], 20) / 10
                            emit({"what": "attention launch alone: " + ("one rows launch" if name == "rows" else f"{T} single-row launches"), "form": name, "batch": B,
                                  "keys": ctx, "rows_per_seq": T, "repeat": rep, "us": round(ms * 1e3, 2)})
                    del R, S, graphs
            del alloc
    else:
        blocks = [DecoderBlock(HIDDEN, HEADS, FFN, ctx_max, dev, cos, sin, seed=100 + i, kv_heads=KV_HEADS) for i in range(LAYERS)]
        g = torch.Generator(device=dev).manual_seed(7)
        final_gamma = (1.0 + 0.1 * torch.empty(HIDDEN, device=dev).normal_(0, 1, generator=g)).float()
        lm_head = Linear_half_int4.from_float(torch.empty(VOCAB, HIDDEN, device=dev).normal_(0.0, HIDDEN ** -0.5, generator=g)).prepack()
        table = torch.empty(VOCAB, HIDDEN, device=dev).normal_(0.0, 1.0, generator=g).half()
        big = 1 << 12
        for B in batches:
            alloc = allocator(B)
            paged = [PagedBatchedDecoder(b, alloc) for b in blocks]
            for dp in paged:
                dp.attention.k_pool.normal_(0, 0.8)
                dp.attention.v_pool.normal_(0, 0.8)
            plain = BatchedGenerator(paged, final_gamma, lm_head, table, max_new=big)
            for T in rows:
                spec_dec = [SpeculativeDecoder(b, alloc, T) for b in blocks]
                for ds, dp in zip(spec_dec, paged):
                    ds.attention.k_pool.copy_(dp.attention.k_pool)
                    ds.attention.v_pool.copy_(dp.attention.v_pool)
                spec = SpeculativeGenerator(spec_dec, final_gamma, lm_head, table, max_new=big, script=True)
                for ctx in contexts:
                    start = ctx - (STEPS + WARMUP) * T - 4  # the timed tokens end just below ctx keys even when every draft is accepted

                    def place_plain():
                        for b in range(B):
                            plain.sampler.set_row(b, SamplingParams(), 1000 + b, big, [b + 1])
                        plain.pos.fill_(start)
                        plain.sampler.next_token.copy_(torch.arange(1, B + 1, dtype=torch.int32))
                        plain.book.pos, plain.book.max_new, plain.book.generated = [start] * B, [big] * B, [0] * B

                    def place_spec():
                        for b in range(B):
                            spec.sampler.set_row(b, SamplingParams(), 1000 + b, big, [b + 1])
                        spec.pos.fill_(start)
                        spec.history[:, start].copy_(torch.arange(1, B + 1, dtype=torch.int32))
                        spec.book.pos, spec.book.max_new, spec.book.generated = [start] * B, [big] * B, [0] * B

                    # discovery: the plain tokens from the placed position, one per replay
                    need = (STEPS + WARMUP) * T
                    spec.script.fill_(-1)
                    place_spec()
                    spec.run(need, record=False)
                    found = spec.sampler.out_log[:, :need].clone()  # token index j sits at position start + 1 + j
                    scripts = {}
                    for mode in ("none", "half", "all"):
                        sc = torch.full_like(spec.script, -1)
                        good = found.clone()
                        if mode == "none":
                            good = (good + 1) % VOCAB
                        elif mode == "half":  # replays alternate: all right (T tokens), the first draft wrong (1 token)
                            j, k = 0, 0
                            while j < need:
                                if k % 2:
                                    good[:, j] = (good[:, j] + 1) % VOCAB
                                j += 1 if k % 2 else T
                                k += 1
                        sc[:, start + 1:start + 1 + need] = good
                        scripts[mode] = sc

                    def run_plain(n):
                        plain.run(n)

                    def run_spec(n):
                        spec.run(n, record=False)
                    for rep in range(REPEATS):
                        for form in ("plain", "none", "half", "all"):  # the forms alternate
                            if form == "plain":
                                place_plain()
                                run_plain(WARMUP)
                                before = plain.sampler.generated().sum()
                                ms = timed(run_plain, STEPS)
                                made = int(plain.sampler.generated().sum() - before)
                                plain_ms = ms
                            else:
                                spec.script.copy_(scripts[form])
                                place_spec()
                                run_spec(WARMUP)
                                before = spec.sampler.generated().sum()
                                ms = timed(run_spec, STEPS)
                                made = int(spec.sampler.generated().sum() - before)
                            emit({"what": "BatchedGenerator.run" if form == "plain" else f"SpeculativeGenerator.run, accept={form}", "form": form, "batch": B, "keys": ctx,
                                  "rows_per_seq": 1 if form == "plain" else T, "repeat": rep, "ms_per_replay": round(ms, 4), "tokens": made,
                                  "tokens_per_replay_and_sequence": round(made / (STEPS * B), 3), "tokens_per_s": round(made * 1e3 / (ms * STEPS), 1),
                                  "replay_ratio": None if form == "plain" else round(ms / plain_ms, 4),
                                  "launches_per_replay": plain.launches_per_token if form == "plain" else spec.launches_per_token})
                del spec, spec_dec
                torch.cuda.empty_cache()
            del plain, paged, alloc
            torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            f.writelines(lines)


if __name__ == "__main__":
    main()
