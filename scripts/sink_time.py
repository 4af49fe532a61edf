#!/usr/bin/env python3
"""Attention sinks on the clock (tinychatengine_amd/paged_kv.py, window=W, sinks=S): the sink step and prefill against the windowed ones in ONE process, the attention
launch alone, on Llama-3-8B's head shapes (32 query / 8 key-value heads), fp16 pages, page_keys = 64, page numbers dealt from a seeded shuffle.  After
scripts/window_time.py: the forms alternate and every point is measured REPEATS times, device events around 200 launches (one graph of 20 launches over ROTATE layers'
pools, replayed 10 times).

    python scripts/sink_time.py [OUT.jsonl]            both parts
    python scripts/sink_time.py --step [OUT.jsonl]     W = 4096, S = 4 at position 32767, B = 1 / 4 / 16: the sink step against the windowed step
    python scripts/sink_time.py --prefill [OUT.jsonl]  a chunk of 512 rows on 8192 cached keys, W = 4096: S = 4 against the windowed prefill

EXPECTATION (written before the first run): the step is within noise of the windowed one -- it adds one group of four keys to one wave of one chunk slot, two 16-byte
loads of cos / sin row S + W - 1 to the prologue batch, one rotation of q, and one table word (lane 62) to a request that is made anyway; the cut is for S4 + W + 3 =
4103 keys against 4099, the same nine chunk slots.  "Within noise" is judged against the windowed step's own spread over its repeats: the records carry both, and
`within_noise` is |difference of the medians| <= max(the two spreads, 2 % of the windowed median).  The prefill chunk: every block binds, so each walks one more key
tile (the sink pass) on top of ~72 (4096 / 64 + the diagonal) and re-reads its raw q rows once: expected + 1 .. 2 %.

A compile and a CPU rehearsal of this script are not a measurement: it refuses to run without a device.
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BATCHES = (1, 4, 16)
PAGE_KEYS = 64
REPEATS = 3
ROTATE = 2          # pools the graph walks through (a layer's pair of pools is 2 GiB at 32768 keys and B = 16)
LAUNCHES, REPLAYS = 20, 10
HEADS, KV_HEADS, HD = 32, 8, 128
W, S, POS = 4096, 4, 32767
PREFILL_POS, PREFILL_M = 8192, 512


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    parts = [a[2:] for a in sys.argv[1:] if a.startswith("--")] or ["step", "prefill"]
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec) + "\n")

    measure(parts, emit)
    if args:
        with open(args[0], "w") as f:
            f.writelines(lines)


def measure(parts, emit):
    import numpy as np
    import torch
    from tinychatengine_amd import capi
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchDecodeAttention
    assert torch.cuda.is_available(), "a GPU measurement: no device, no number"
    capi.lib()
    dev = torch.device("cuda:0")
    ang = np.random.default_rng(0).uniform(0, 2 * np.pi, (POS + 1, HD // 2))
    cos = torch.from_numpy(np.concatenate([np.cos(ang), np.cos(ang)], axis=1).astype(np.float16)).to(dev)
    sin = torch.from_numpy(np.concatenate([np.sin(ang), np.sin(ang)], axis=1).astype(np.float16)).to(dev)

    def timed(run, reps):
        for _ in range(3):
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
        num_pages = B * pages_per_seq + 8
        alloc = PageAllocator(num_pages, PAGE_KEYS, B, pages_per_seq, dev, free_order=np.random.default_rng(B).permutation(num_pages).tolist())
        for b in range(B):
            alloc.reserve(b, keys - 1)
        return alloc

    def layers(alloc, sinks, n):
        atts = [PagedBatchDecodeAttention(alloc, HEADS, KV_HEADS, dev, cos, sin, window=W, sinks=sinks) for _ in range(n)]
        for a in atts:
            a.k_pool.normal_(0, 0.8)
            a.v_pool.normal_(0, 0.8)
        return atts

    def step_graph(atts, B):
        qkv = (torch.randn(B, (HEADS + 2 * KV_HEADS) * HD, device=dev) * 0.9).half()
        out = torch.empty(B, HEADS * HD, dtype=torch.float16, device=dev)
        pos = torch.full((B,), POS, dtype=torch.int32, device=dev)

        def launches():
            for i in range(LAUNCHES):
                atts[i % len(atts)].step(qkv, pos, POS, out=out)
        launches()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            launches()

        def replay():
            g.replay()
        replay.keep, replay.out = launches, out
        return replay

    def verdict(med, spread, base, new):
        diff = med[new] - med[base]
        noise = max(spread[base], spread[new], 0.02 * med[base])
        return {"difference": round(diff, 3), "relative": round(diff / med[base], 4), "noise": round(noise, 3), "within_noise": abs(diff) <= noise}

    if "step" in parts:
        for B in BATCHES:
            alloc = allocator(B, POS + 1)
            runs = {"window_step": step_graph(layers(alloc, None, ROTATE), B), "sink_step": step_graph(layers(alloc, S, ROTATE), B)}
            us = {f: [] for f in runs}
            for rep in range(REPEATS):
                for f, run in runs.items():
                    run.out.zero_()
                    t = timed(run, REPLAYS) / LAUNCHES * 1e3
                    assert bool(torch.count_nonzero(run.out[-1]) > 0), f"{f}: the last row came out zero: its position word was not an active one"
                    us[f].append(t)
                    emit({"what": "W = 4096, S = 4 at position 32767", "form": f, "batch": B, "repeat": rep, "us_per_launch": round(t, 3), "launches": LAUNCHES * REPLAYS})
            med, spread = {f: sorted(v)[len(v) // 2] for f, v in us.items()}, {f: max(v) - min(v) for f, v in us.items()}
            emit({"what": "W = 4096, S = 4 at position 32767: medians", "batch": B, **{f + "_us": round(v, 3) for f, v in med.items()},
                  **{f + "_spread_us": round(v, 3) for f, v in spread.items()}, **verdict(med, spread, "window_step", "sink_step"),
                  "describe_sink": capi.describe_attention_paged_sink(B, HEADS, KV_HEADS, POS, PAGE_KEYS, W, S),
                  "describe_window": capi.describe_attention_paged_window(B, HEADS, KV_HEADS, POS, PAGE_KEYS, W)})
            del runs, alloc
            torch.cuda.empty_cache()

    if "prefill" in parts:
        keys = PREFILL_POS + PREFILL_M
        alloc = allocator(1, (keys + PAGE_KEYS - 1) // PAGE_KEYS * PAGE_KEYS)
        atts = {"prefill_window": layers(alloc, None, 1)[0], "prefill_sink": layers(alloc, S, 1)[0]}
        qkv = (torch.randn(PREFILL_M, (HEADS + 2 * KV_HEADS) * HD, device=dev) * 0.9).half()
        out = torch.empty(PREFILL_M, HEADS * HD, dtype=torch.float16, device=dev)
        seg = [(0, PREFILL_POS, PREFILL_M)]
        us = {f: [] for f in atts}
        for rep in range(REPEATS):
            for f, a in atts.items():
                t = timed(lambda a=a: a.prefill(seg, qkv, out=out), 200) * 1e3
                us[f].append(t)
                emit({"what": "paged prefill chunk", "form": f, "cached_keys": PREFILL_POS, "rows": PREFILL_M, "repeat": rep, "us_per_call": round(t, 2), "calls": 200})
        med, spread = {f: sorted(v)[len(v) // 2] for f, v in us.items()}, {f: max(v) - min(v) for f, v in us.items()}
        emit({"what": "paged prefill chunk: medians", "cached_keys": PREFILL_POS, "rows": PREFILL_M, "window": W, "sinks": S, **{f + "_us": round(v, 2) for f, v in med.items()},
              **{f + "_spread_us": round(v, 2) for f, v in spread.items()}, **verdict(med, spread, "prefill_window", "prefill_sink")})


if __name__ == "__main__":
    main()
