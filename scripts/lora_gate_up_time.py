#!/usr/bin/env python3
"""Gate/up adapters and adapters on speculative rows on the clock, beside the parent's three-target pool, in ONE process (scripts/lora_time.py's setting: Llama-3-8B's
shapes -- hidden 4096, 32 query / 8 key-value heads, ffn 14336, vocabulary 128256 --, --layers N, default 32, 64-key pages, rank 16, 16 adapters resident).

    replay     BatchedGenerator.run under the captured graph at B = 1 / 4 / 16 around 512 keys, six forms that ALTERNATE, REPEATS times:
                 pool3 off / one / own    the three-target pool (13 L + 5 launches): every word -1, every slot on adapter 0, slot b on adapter b
                 pool4 off / one / own    the gate_up=True pool (15 L + 5 launches), the same words
               (each pool is ONE generator and ONE graph: only the words change.  The two have decoders of their own over the same blocks and allocator.)
    launch     tce_lora_expand_silu_mul_f16 alone (gate/up: 4096 -> 2 x 14336 at R 16) against the composition it replaces -- tce_lora_expand_add_f16 on y with the
               block-structured B' [2R][2N] followed by tce_silu_mul_half on N columns (the de-interleave between them is left out, in the composition's favour) --,
               B rows, the words of off / one / own: LAUNCHES of each captured in one graph, forms alternating
    spec       SpeculativeGenerator.run under the captured graph, B = 4, T = 4 (M = 16 rows): lora=None against a gate_up=True pool built with rows_per_seq=4, every
               word -1 and every slot on its own adapter

EXPECTATION (written down before the first run; DESIGN.md 3.9 marks it CONFIRMED or REFUTED):
  * pool4 `off` over pool3 `off`: one more shrink + expand pair of launch boundaries per layer (the parent measured 3.2 us per pair under a graph), and the gate/up
    linear no longer fuses SiLU * mul: its [B][2 * 14336] fp16 output goes through memory once more (0.9 MB at B = 16) -- about 32 x 3.2 us = 0.1 ms per token, a
    little more at B = 16;
  * pool4 `own` at B = 16 over pool3 `own`: that plus 16 * 2R * (K + N) * 2 = 18.9 MB of adapter bytes per layer against the three existing targets' 29 MB -- of the
    order of two thirds of what pool3 `own` costs over pool3 `off`;
  * the new launch against the composition: no zero block is read (half the B bytes: 2 * R * N * 2 against 2R * 2N * 2 per adapter) and one launch boundary less;
  * spec: the rows pool costs what the plain pool costs at M = 16 -- the words are per row, nothing else changed.

    python scripts/lora_gate_up_time.py [--layers N] [OUT.jsonl]
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
LAUNCHES = 50
HIDDEN, HEADS, KV_HEADS, FFN, VOCAB = 4096, 32, 8, 14336, 128256
RANK, ADAPTERS = 16, 16
WORDS = ("off", "one", "own")
SPEC_B, SPEC_T, SPEC_STEPS = 4, 4, 20


def words(form, B, T=1):
    w = [-1] * B if form == "off" else [0] * B if form == "one" else list(range(B))
    return [a for a in w for _ in range(T)]


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
    from tinychatengine_amd.linear import Linear_half_int4, _stream
    from tinychatengine_amd.lora import LoraPool, expand_add, expand_silu_mul
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
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").close()

    def emit(rec):
        rec.update({"layers": layers, "hidden": HIDDEN, "rank": RANK, "adapters": ADAPTERS})
        print(json.dumps(rec), flush=True)
        if out_path:  # line by line: a run that is cut short keeps what it measured
            with open(out_path, "a") as f:
                f.write(json.dumps(rec) + "\n")

    def timed(run, n):
        a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        run(n)
        b_.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b_) / n

    def filled_pool(gate_up, rows_per_seq=None):
        """every adapter dense and small (the device's random numbers: what is timed does not depend on the values)"""
        pool = LoraPool(blocks[0], layers, ADAPTERS, RANK, dev, gate_up=gate_up, rows_per_seq=rows_per_seq)
        for t in pool.A:
            pool.A[t].normal_(0, 0.01)
        for b in list(pool.B.values()) + ([pool.Bg, pool.Bu] if gate_up else []):
            b.normal_(0, 0.01)
        pool.scale.fill_(2.0)
        return pool

    def place(gen, B, start):
        for b in range(B):
            gen.sampler.set_row(b, SamplingParams(), 1000 + b, 1 << 12, [b + 1])
        gen.pos.fill_(start)
        gen.book.pos = [start] * B
        gen.book.max_new = [1 << 12] * B
        gen.book.generated = [0] * B

    pages_per_seq = CONTEXT // PAGE_KEYS

    def allocator(B):
        num_pages = 2 * B * pages_per_seq
        alloc = PageAllocator(num_pages, PAGE_KEYS, B, pages_per_seq, dev, free_order=np.random.default_rng(B).permutation(num_pages).tolist())
        for i in range(pages_per_seq):
            for b in range(B):
                alloc.reserve(b, (i + 1) * PAGE_KEYS - 1)
        return alloc

    def fill_caches(decs):
        for dp in decs:
            dp.attention.k_pool.normal_(0, 0.8)
            dp.attention.v_pool.normal_(0, 0.8)

    # ---- the new launch alone against the composition it replaces ----
    R, K, N = RANK, HIDDEN, FFN
    for B in BATCHES:
        Bg, Bu = (torch.empty(ADAPTERS, R, N, dtype=torch.float16, device=dev).normal_(0, 0.01) for _ in range(2))
        Bblock = torch.zeros(ADAPTERS, 2 * R, 2 * N, dtype=torch.float16, device=dev)
        Bblock[:, :R, 0::2], Bblock[:, R:, 1::2] = Bg, Bu
        scale = torch.full((ADAPTERS,), 2.0, dtype=torch.float32, device=dev)
        t = torch.randn(B, 2 * R, device=dev)
        y, y0 = torch.randn(B, 2 * N, device=dev).half(), None
        y0 = y.clone()
        c, u = torch.empty(B, N, dtype=torch.float16, device=dev), torch.randn(B, N, device=dev).half()
        ra = torch.full((B,), -1, dtype=torch.int32, device=dev)

        def new(n=LAUNCHES):
            for _ in range(n):
                expand_silu_mul(t, Bg, Bu, scale, ra, y, c)

        def composition(n=LAUNCHES):
            for _ in range(n):
                expand_add(t, Bblock, scale, ra, y)
                capi.check(capi.lib().tce_silu_mul_half(c.data_ptr(), u.data_ptr(), c.numel(), _stream()))
        graphs = {}
        for name, fn in (("expand_silu_mul", new), ("expand_add + silu_mul", composition)):
            fn(2)
            torch.cuda.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                fn()
        for rep in range(REPEATS):
            for form in WORDS:
                ra.copy_(torch.tensor(words(form, B), dtype=torch.int32))
                for name, graph in graphs.items():  # the forms alternate

                    def replay(n):
                        for _ in range(n):
                            graph.replay()
                    y.copy_(y0)  # (the composition accumulates into y: keep it finite)
                    c.normal_(0, 1)
                    replay(2)
                    y.copy_(y0)
                    us = timed(replay, 10) * 1e3 / LAUNCHES
                    emit({"what": "gate/up expand alone (graph of %d)" % LAUNCHES, "form": "launch", "kernel": name, "R": R, "N": N, "lora": form, "batch": B, "repeat": rep,
                          "us_per_launch": round(us, 2)})
        del graphs, Bblock

    # ---- the graph replay: the three-target pool against the gate_up=True pool ----
    for B in BATCHES:
        alloc = allocator(B)
        pools = {"pool3": filled_pool(False), "pool4": filled_pool(True)}
        gens = {}
        for name, pool in pools.items():
            decs = [PagedBatchedDecoder(b, alloc, lora=pool.layer(i)) for i, b in enumerate(blocks)]
            fill_caches(decs)
            gens[name] = BatchedGenerator(decs, final_gamma, lm_head, table, max_new=1 << 12, graph=True, lora=pool)
        start = CONTEXT - (TOKENS + WARMUP) - 4  # the timed tokens end just below CONTEXT keys
        for rep in range(REPEATS):
            for form in WORDS:
                for name, gen in gens.items():  # the forms alternate
                    place(gen, B, start)
                    pools[name].row_adapter.copy_(torch.tensor(words(form, B), dtype=torch.int32))
                    gen.run(WARMUP)
                    ms = timed(gen.run, TOKENS)
                    emit({"what": "BatchedGenerator.run (graph), one replay = one token", "form": "replay", "pool": name, "lora": form, "batch": B, "keys": CONTEXT, "repeat": rep,
                          "ms_per_token": round(ms, 4), "launches_per_token": gen.launches_per_token})
        del gens, pools, alloc
        torch.cuda.empty_cache()

    # ---- one speculative replay, T = 4, with and without a pool ----
    B, T = SPEC_B, SPEC_T
    alloc = allocator(B)
    pool = filled_pool(True, rows_per_seq=T)
    gens = {}
    for name, view in (("none", lambda i: None), ("pool4 rows", pool.layer)):
        decs = [SpeculativeDecoder(b, alloc, T, lora=view(i)) for i, b in enumerate(blocks)]
        fill_caches(decs)
        gens[name] = SpeculativeGenerator(decs, final_gamma, lm_head, table, max_new=1 << 12, graph=True, script=True, lora=pool if name != "none" else None)
    start = CONTEXT - (SPEC_STEPS + WARMUP) * T - 8
    for rep in range(REPEATS):
        for name, form in (("none", "none"), ("pool4 rows", "off"), ("pool4 rows", "own")):
            gen = gens[name]
            place(gen, B, start)
            gen.history.fill_(1)
            gen.script.fill_(5)  # every row t >= 1 is fed a (wrong) draft: all T rows of a slot are active, a step emits one token
            if form != "none":
                pool.row_adapter.copy_(torch.tensor(words(form, B, T), dtype=torch.int32))
            gen.run(WARMUP, record=False)
            ms = timed(lambda n: gen.run(n, record=False), SPEC_STEPS)
            emit({"what": "SpeculativeGenerator.run (graph), one replay = one step of T rows per slot (scripted wrong drafts: all T rows active, one token kept)", "form": "spec", "lora": form, "pool": name,
                  "batch": B, "rows_per_seq": T, "keys": CONTEXT, "repeat": rep, "ms_per_step": round(ms, 4), "launches_per_step": gen.launches_per_token})


if __name__ == "__main__":
    main()
