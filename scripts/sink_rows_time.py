#!/usr/bin/env python3
"""The multi-row attention launch with sinks on the clock (tinychatengine_amd/speculative.py: PagedRowsDecodeAttention with window=W, sinks=S): ONE rows-sink launch of T
rows per sequence against (i) the T single sink launches it replaces and (ii) the rows-window launch at the same positions, in ONE process on Llama-3-8B's head
shapes (32 query / 8 key-value heads), fp16 pages, page_keys = 64, page numbers dealt from a seeded shuffle.  W = 4096, S = 4; T = 2, 4, 8; B = 1, 4, 16.

    rows_sink         T rows at positions 32768 - T .. 32767, window 4096, sinks 4, on the pool a sink run leaves (the pages between the sinks' and the window given back)
    single_sink_x_T   T launches of the one-row sink step at those positions, one after the other, on the same pool
    rows_window       the rows-window launch at the same positions on the same pool: what the sinks cost on the multi-row step

The forms alternate and every point is measured REPEATS times, device events around 200 units (one graph of 20 units over ROTATE layers' pools, replayed 10 times; a
unit is one launch, or the T single launches).

    python scripts/sink_rows_time.py [OUT.jsonl]          (profiles/sink_rows/sink_rows_time.jsonl)

A compile and a CPU rehearsal of this script are not a measurement: it refuses to run without a device.
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BATCHES = (1, 4, 16)
ROWS = (2, 4, 8)
PAGE_KEYS = 64
REPEATS = 3
ROTATE = 4
UNITS, REPLAYS = 20, 10
HEADS, KV_HEADS, HD = 32, 8, 128
W, S, KEYS = 4096, 4, 32768


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec) + "\n")

    measure(emit)
    if args:
        with open(args[0], "w") as f:
            f.writelines(lines)


def measure(emit):
    import numpy as np
    import torch
    from tinychatengine_amd import capi
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchDecodeAttention
    from tinychatengine_amd.speculative import PagedRowsDecodeAttention
    assert torch.cuda.is_available(), "a GPU measurement: no device, no number"
    capi.lib()
    dev = torch.device("cuda:0")
    ang = np.random.default_rng(0).uniform(0, 2 * np.pi, (KEYS, HD // 2))
    cos = torch.from_numpy(np.concatenate([np.cos(ang), np.cos(ang)], axis=1).astype(np.float16)).to(dev)
    sin = torch.from_numpy(np.concatenate([np.sin(ang), np.sin(ang)], axis=1).astype(np.float16)).to(dev)

    def graph_of(fn, out):
        """A replay of fn's launches; the returned callable keeps fn -- and every buffer the captured launches use -- alive."""
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()

        def replay():
            g.replay()
        replay.keep, replay.out = fn, out
        return replay

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

    def recycled_allocator(B):
        """Table rows of KEYS keys over a pool that holds little more than the sinks' page and the window per slot: every slot walks to its last key page by page and
        gives the pages between its first and the window back as it goes -- a generator's pool after a long run on sink layers."""
        num_pages = B * (W // PAGE_KEYS + 3) + 8
        alloc = PageAllocator(num_pages, PAGE_KEYS, B, KEYS // PAGE_KEYS, dev, free_order=np.random.default_rng(B).permutation(num_pages).tolist())
        for last in range(PAGE_KEYS - 1, KEYS, PAGE_KEYS):
            for b in range(B):
                alloc.release_behind(b, last - W + 1, keep_pages=1)
                alloc.reserve(b, last)
        alloc.check_invariants()
        assert all(len(alloc.kept[b]) == 1 and alloc.holds(b, 0, S) for b in range(B))
        return alloc

    def randomise(atts):
        for a in atts:
            a.k_pool.normal_(0, 0.8)
            a.v_pool.normal_(0, 0.8)
        return atts

    def rows_graph(atts, B, T, first_pos, bound):
        qkv = (torch.randn(B * T, (HEADS + 2 * KV_HEADS) * HD, device=dev) * 0.9).half()
        out = torch.empty(B * T, HEADS * HD, dtype=torch.float16, device=dev)
        pos = (first_pos + torch.arange(T, dtype=torch.int32, device=dev)).repeat(B).contiguous()
        assert atts[0].table_violations(pos, bound) == 0

        def launches():
            for i in range(UNITS):
                atts[i % len(atts)].step(qkv, pos, bound, out=out)
        return graph_of(launches, out)

    def singles_graph(atts, B, T, first_pos, bound):
        qkv = [(torch.randn(B, (HEADS + 2 * KV_HEADS) * HD, device=dev) * 0.9).half() for _ in range(T)]
        out = torch.empty(B, HEADS * HD, dtype=torch.float16, device=dev)
        pos = [torch.full((B,), first_pos + t, dtype=torch.int32, device=dev) for t in range(T)]

        def launches():
            for i in range(UNITS):
                for t in range(T):
                    atts[i % len(atts)].step(qkv[t], pos[t], bound, out=out)
        return graph_of(launches, out)

    for B in BATCHES:
        alloc = recycled_allocator(B)
        singles = randomise([PagedBatchDecodeAttention(alloc, HEADS, KV_HEADS, dev, cos, sin, window=W, sinks=S) for _ in range(ROTATE)])
        for T in ROWS:
            rows_s = randomise([PagedRowsDecodeAttention(alloc, HEADS, KV_HEADS, dev, cos, sin, rows_per_seq=T, window=W, sinks=S) for _ in range(ROTATE)])
            rows_w = randomise([PagedRowsDecodeAttention(alloc, HEADS, KV_HEADS, dev, cos, sin, rows_per_seq=T, window=W) for _ in range(ROTATE)])
            runs = {"rows_sink": rows_graph(rows_s, B, T, KEYS - T, KEYS - 1),
                    "single_sink_x_T": singles_graph(singles, B, T, KEYS - T, KEYS - 1),
                    "rows_window": rows_graph(rows_w, B, T, KEYS - T, KEYS - 1)}
            us = {f: [] for f in runs}
            for rep in range(REPEATS):
                for f, run in runs.items():
                    run.out.zero_()
                    t = timed(run, REPLAYS) / UNITS * 1e3
                    assert bool(torch.count_nonzero(run.out[-1]) > 0), f"{f}: the last row came out zero: its position word was not an active one"
                    us[f].append(t)
                    emit({"what": "rows-sink attention launch", "form": f, "batch": B, "rows_per_seq": T, "window": W, "sinks": S, "repeat": rep, "us_per_unit": round(t, 3),
                          "units": UNITS * REPLAYS})
            med = {f: sorted(v)[len(v) // 2] for f, v in us.items()}
            emit({"what": "rows-sink attention launch: medians", "batch": B, "rows_per_seq": T, "window": W, "sinks": S, **{f + "_us": round(v, 3) for f, v in med.items()},
                  "spread_us": {f: round(max(v) - min(v), 3) for f, v in us.items()},
                  "rows_sink_over_singles": round(med["rows_sink"] / med["single_sink_x_T"], 3),
                  "rows_sink_over_rows_window": round(med["rows_sink"] / med["rows_window"], 3),
                  "describe_sink": capi.describe_attention_paged_sink(B, HEADS, KV_HEADS, KEYS - 1, PAGE_KEYS, W, S),
                  "describe_window": capi.describe_attention_paged_window(B, HEADS, KV_HEADS, KEYS - 1, PAGE_KEYS, W)})
            del runs, rows_s, rows_w
            torch.cuda.empty_cache()
        del singles, alloc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
