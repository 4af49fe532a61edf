#!/usr/bin/env python3
"""The e4m3 paged KV cache on the clock: fp16 pages against fp8 pages (tinychatengine_amd/paged_kv.py, kv_dtype="fp8_e4m3") in ONE process on Llama-3-8B's shapes
(32 query / 8 key-value heads; the layer step: 32 layers, hidden 4096, ffn 14336), page_keys = 64, page numbers dealt from a seeded shuffle of a pool twice the pages
in use.  The two forms alternate and every point is measured REPEATS times: the record shows each form's own repeat-to-repeat spread beside the difference.

    python scripts/fp8_kv_time.py [OUT.jsonl]             all three parts
    python scripts/fp8_kv_time.py --attention [OUT.jsonl] the attention launch alone (tce_attention_decode_step_paged_f16 / _fp8) at B = 8 and 16, 512 / 2048 / 8192 keys,
                                                          one graph of 20 launches over ROTATE layers' pools (so the cache comes from HBM, not from the memory-side cache)
    python scripts/fp8_kv_time.py --step [OUT.jsonl]      the 32-layer PagedBatchedDecoder step under one graph at the same points
    python scripts/fp8_kv_time.py --prefill [OUT.jsonl]   one paged-prefill point: a 512-row chunk on 7680 cached keys (tce_attention_prefill_paged_f16 / _fp8, both launches)
    python scripts/fp8_kv_time.py --accuracy [OUT.jsonl]  the worst per-head error of the fp8 step against the UNQUANTISED fp16 paged step on Gaussian inputs,
                                                          exponents 0, in units of max|out| of the head (reported, asserted nowhere: it depends on the data)
    python scripts/fp8_kv_time.py --memory [OUT.jsonl]    computed, not measured (no GPU): bytes per token and the README's 16-slot example in both formats

A point where fp8 is more than one round trip (1.55 us) slower than fp16 is marked "slower_than_one_round_trip": it deserves a
rocprofv3 --kernel-trace --stats run of its own and a sentence of cause in DESIGN.md.
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BATCHES = (8, 16)
CONTEXTS = (512, 2048, 8192)
PAGE_KEYS = 64
POOL_FACTOR = 2
REPEATS = 3
ROTATE = 8  # pools the attention-alone graph walks through
ROUND_TRIP_US = 1.55
LAYERS, HIDDEN, HEADS, KV_HEADS, FFN, HD = 32, 4096, 32, 8, 14336, 128
PREFILL_POS, PREFILL_M = 7680, 512
FORMS = ("fp16", "fp8_e4m3")


def memory_record():
    import numpy as np
    slots, max_keys = 16, 8192
    lengths = np.clip(np.random.default_rng(8192).lognormal(np.log(400.0), 1.2, slots).astype(np.int64), 1, max_keys)  # (scripts/paged_decode_time.py's example)
    pages = int(sum((int(n) + PAGE_KEYS - 1) // PAGE_KEYS for n in lengths))
    rec = {"what": "memory held, computed", "slots": slots, "page_keys": PAGE_KEYS, "layers": LAYERS, "tokens": int(lengths.sum()), "live_pages": pages}
    for form, elem in (("fp16", 2), ("fp8_e4m3", 1)):
        per_token = KV_HEADS * HD * 2 * LAYERS * elem
        rec[form] = {"bytes_per_token_all_layers": per_token, "bytes_in_live_pages": pages * PAGE_KEYS * per_token}
    rec["ratio"] = rec["fp8_e4m3"]["bytes_per_token_all_layers"] / rec["fp16"]["bytes_per_token_all_layers"]
    return rec


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    out_path = args[0] if args else None
    parts = [f[2:] for f in flags] or ["memory", "attention", "step", "prefill", "accuracy"]
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec) + "\n")

    if "memory" in parts:
        emit(memory_record())
    if parts != ["memory"]:
        measure([p for p in parts if p != "memory"], emit)
    if out_path:
        with open(out_path, "w") as f:
            f.writelines(lines)


def measure(parts, emit):
    import numpy as np
    import torch
    from tinychatengine_amd import capi
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchDecodeAttention, PagedBatchedDecoder
    assert torch.cuda.is_available(), "a GPU measurement: no device, no number"
    capi.lib()
    dev = torch.device("cuda:0")
    ctx_max = max(CONTEXTS)
    ang = np.random.default_rng(0).uniform(0, 2 * np.pi, (ctx_max, HD // 2))
    cos = torch.from_numpy(np.concatenate([np.cos(ang), np.cos(ang)], axis=1).astype(np.float16)).to(dev)
    sin = torch.from_numpy(np.concatenate([np.sin(ang), np.sin(ang)], axis=1).astype(np.float16)).to(dev)

    def graph_of(fn):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        return g.replay

    def timed(run, reps):
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            run()
        b_.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b_) / reps

    def allocator(B, keys):
        pages_per_seq = keys // PAGE_KEYS
        num_pages = POOL_FACTOR * B * pages_per_seq
        alloc = PageAllocator(num_pages, PAGE_KEYS, B, pages_per_seq, dev, free_order=np.random.default_rng(B).permutation(num_pages).tolist())
        for i in range(pages_per_seq):  # slot by slot in turn: a sequence's pages are scattered over the pool and interleaved with the others'
            for b in range(B):
                alloc.reserve(b, (i + 1) * PAGE_KEYS - 1)
        return alloc

    from tinychatengine_amd.paged_kv import fp8_quantize_reference
    block = (np.random.default_rng(1).standard_normal(1 << 20) * 0.8).astype(np.float16)
    block8 = torch.from_numpy(fp8_quantize_reference(block, 0)).to(dev)  # a Gaussian block on the e4m3 grid (exponent 0), tiled over the fp8 pools

    def fill(att):
        """Gaussian cache contents, sigma 0.8: fp16 pools directly, fp8 pools by tiling a quantised Gaussian block."""
        for pool in (att.k_pool, att.v_pool):
            if att.fp8:
                flat = pool.view(-1)
                for o in range(0, flat.numel(), block8.numel()):
                    n = min(block8.numel(), flat.numel() - o)
                    flat[o:o + n].copy_(block8[:n])
            else:
                pool.normal_(0, 0.8)

    def compare(what, point, ms, unit_us):
        med = {f: sorted(ms[f])[len(ms[f]) // 2] for f in FORMS}
        diff_us = (med["fp8_e4m3"] - med["fp16"]) * 1e3 / unit_us
        emit({"what": what + ": fp8 against fp16", **point, "fp16_median_ms": round(med["fp16"], 5), "fp8_median_ms": round(med["fp8_e4m3"], 5),
              "time_ratio": round(med["fp8_e4m3"] / med["fp16"], 4), "difference_us_per_launch": round(diff_us, 3),
              "fp16_spread_ms": round(max(ms["fp16"]) - min(ms["fp16"]), 5), "slower_than_one_round_trip": diff_us > ROUND_TRIP_US})

    if "attention" in parts:
        for B in BATCHES:
            for ctx in CONTEXTS:
                alloc = allocator(B, ctx)
                atts = {f: [PagedBatchDecodeAttention(alloc, HEADS, KV_HEADS, dev, cos, sin, kv_dtype=f) for _ in range(ROTATE)] for f in FORMS}
                qkv = (torch.randn(B, (HEADS + 2 * KV_HEADS) * HD, device=dev) * 0.9).half()
                out = torch.empty(B, HEADS * HD, dtype=torch.float16, device=dev)
                pos = torch.full((B,), ctx - 1, dtype=torch.int32, device=dev)
                runs = {}
                for f in FORMS:
                    for a in atts[f]:
                        fill(a)

                    def launches(layers=atts[f]):
                        for i in range(20):
                            layers[i % ROTATE].step(qkv, pos, ctx - 1, out=out)
                    runs[f] = graph_of(launches)
                ms = {f: [] for f in FORMS}
                for rep in range(REPEATS):
                    for f in FORMS:  # the forms alternate
                        t = timed(runs[f], 20) / 20
                        ms[f].append(t)
                        emit({"what": "attention launch alone", "form": f, "batch": B, "keys": ctx, "repeat": rep, "us_per_launch": round(t * 1e3, 3), "page_keys": PAGE_KEYS,
                              "cache_bytes_read": B * KV_HEADS * ctx * HD * 2 * (1 if f == "fp8_e4m3" else 2)})
                compare("attention launch alone", {"batch": B, "keys": ctx}, ms, 1.0)
                del runs, atts, alloc
                torch.cuda.empty_cache()

    if "step" in parts:
        from tinychatengine_amd.decoder_block import DecoderBlock
        blocks = [DecoderBlock(HIDDEN, HEADS, FFN, ctx_max, dev, cos, sin, seed=100 + i, kv_heads=KV_HEADS) for i in range(LAYERS)]
        for B in BATCHES:
            for ctx in CONTEXTS:
                alloc = allocator(B, ctx)
                h0 = torch.randn(B, HIDDEN, device=dev).to(torch.float16)
                h = h0.clone()
                pos = torch.full((B,), ctx - 1, dtype=torch.int32, device=dev)
                ms = {f: [] for f in FORMS}
                runs = {}
                for f in FORMS:
                    decs = [PagedBatchedDecoder(b, alloc, kv_dtype=f) for b in blocks]
                    for d in decs:
                        fill(d.attention)

                    def step(decs=decs):
                        h.copy_(h0)
                        for d in decs:
                            d.step(h, pos, ctx - 1)
                    runs[f] = graph_of(step)
                for rep in range(REPEATS):
                    for f in FORMS:  # the forms alternate
                        t = timed(runs[f], 30)
                        ms[f].append(t)
                        emit({"what": "PagedBatchedDecoder.step", "form": f, "batch": B, "keys": ctx, "repeat": rep, "ms_per_step": round(t, 4),
                              "tokens_per_s": round(B * 1e3 / t, 1), "layers": LAYERS, "page_keys": PAGE_KEYS, "lm_head": False})
                compare("PagedBatchedDecoder.step", {"batch": B, "keys": ctx}, ms, float(LAYERS))
                del runs, decs, alloc
                torch.cuda.empty_cache()
        del blocks
        torch.cuda.empty_cache()

    if "prefill" in parts:
        keys = PREFILL_POS + PREFILL_M
        alloc = allocator(1, keys)
        atts = {f: PagedBatchDecodeAttention(alloc, HEADS, KV_HEADS, dev, cos, sin, kv_dtype=f) for f in FORMS}
        qkv = (torch.randn(PREFILL_M, (HEADS + 2 * KV_HEADS) * HD, device=dev) * 0.9).half()
        out = torch.empty(PREFILL_M, HEADS * HD, dtype=torch.float16, device=dev)
        seg = [(0, PREFILL_POS, PREFILL_M)]
        ms = {f: [] for f in FORMS}
        for f in FORMS:
            fill(atts[f])
        for rep in range(REPEATS):
            for f in FORMS:
                t = timed(lambda: atts[f].prefill(seg, qkv, out=out), 20)
                ms[f].append(t)
                emit({"what": "paged prefill chunk", "form": f, "cached_keys": PREFILL_POS, "rows": PREFILL_M, "repeat": rep, "us_per_call": round(t * 1e3, 2),
                      "describe": capi.describe_prefill_paged(HEADS, KV_HEADS, True, seg)})
        compare("paged prefill chunk", {"cached_keys": PREFILL_POS, "rows": PREFILL_M}, ms, 1.0)

    if "accuracy" in parts:
        B, ctx = 8, 2048
        alloc = allocator(B, ctx)
        a16 = PagedBatchDecodeAttention(alloc, HEADS, KV_HEADS, dev, cos, sin)
        a8 = PagedBatchDecodeAttention(alloc, HEADS, KV_HEADS, dev, cos, sin, kv_dtype="fp8_e4m3")
        a16.k_pool.normal_(0, 0.8)
        a16.v_pool.normal_(0, 0.8)
        a8.k_pool.copy_(torch.from_numpy(fp8_quantize_reference(a16.k_pool, 0)))  # (exponents 0)
        a8.v_pool.copy_(torch.from_numpy(fp8_quantize_reference(a16.v_pool, 0)))
        qkv = (torch.randn(B, (HEADS + 2 * KV_HEADS) * HD, device=dev) * 0.9).half()
        for keys in (64, 512, 2048):
            pos = torch.full((B,), keys - 1, dtype=torch.int32, device=dev)
            o16 = a16.step(qkv, pos, ctx - 1).float().view(B, HEADS, HD)
            o8 = a8.step(qkv, pos, ctx - 1).float().view(B, HEADS, HD)
            torch.cuda.synchronize()
            rel = ((o8 - o16).abs().amax(dim=2) / o16.abs().amax(dim=2))
            emit({"what": "fp8 step against the unquantised fp16 paged step", "batch": B, "keys": keys, "inputs": "Gaussian, sigma 0.8 (cache) / 0.9 (q, k, v rows)",
                  "k_scale_log2": 0, "v_scale_log2": 0, "worst_head_error_over_head_max": round(float(rel.max()), 5), "median_head_error_over_head_max": round(float(rel.median()), 5)})


if __name__ == "__main__":
    main()
