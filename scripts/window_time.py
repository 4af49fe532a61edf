#!/usr/bin/env python3
"""Sliding-window attention on the clock (tinychatengine_amd/paged_kv.py, window=W): the windowed paged step and prefill against the unwindowed ones in ONE process on
Llama-3-8B's head shapes (32 query / 8 key-value heads), fp16 pages, page_keys = 64, page numbers dealt from a seeded shuffle.  B = 1, 4 and 16; the forms alternate and
every point is measured REPEATS times, device events around 200 launches (one graph of 20 launches over ROTATE layers' pools, replayed 10 times).

    python scripts/window_time.py [OUT.jsonl]                 all three parts
    python scripts/window_time.py --never-binding [OUT.jsonl] W = 2^30 against the existing step at 512 and 2048 keys: what the table-word request behind the position
                                                              word costs (the design predicts one dependent round trip, 1.55 us: DESIGN.md 3.4)
    python scripts/window_time.py --far [OUT.jsonl]           W = 4096 at position 32767 against the existing step at position 4095 and at position 32767: the windowed
                                                              launch should sit near the former and far from the latter.  Twice: on the pool the unwindowed step needs
                                                              (every page of 32768 keys held) and on the pool a windowed run leaves (the pages behind the window given
                                                              back: as many pages as the step at 4095 holds)
    python scripts/window_time.py --prefill [OUT.jsonl]       a chunk of 512 rows on 8192 cached keys, W = 4096 and no window

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
ROTATE = 4          # pools the graph walks through (2 at 32768 keys: a layer's pair of pools is 2 GiB there at B = 16)
LAUNCHES, REPLAYS = 20, 10
ROUND_TRIP_US = 1.55
HEADS, KV_HEADS, HD = 32, 8, 128
NEVER = 1 << 30
FAR_W, FAR_POS = 4096, 32767
PREFILL_POS, PREFILL_M, PREFILL_W = 8192, 512, 4096


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    parts = [a[2:] for a in sys.argv[1:] if a.startswith("--")] or ["never-binding", "far", "prefill"]
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
    ang = np.random.default_rng(0).uniform(0, 2 * np.pi, (FAR_POS + 1, HD // 2))
    cos = torch.from_numpy(np.concatenate([np.cos(ang), np.cos(ang)], axis=1).astype(np.float16)).to(dev)
    sin = torch.from_numpy(np.concatenate([np.sin(ang), np.sin(ang)], axis=1).astype(np.float16)).to(dev)

    def graph_of(fn, out):
        """A replay of fn's launches.  The returned callable keeps fn -- and with it every buffer the captured launches read and write -- alive, and checks once per
        timing that the rows were active (an overwritten position word would make the launch an empty one, and a fast one)."""
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

    def allocator(B, keys):
        pages_per_seq = keys // PAGE_KEYS
        num_pages = B * pages_per_seq + 8
        alloc = PageAllocator(num_pages, PAGE_KEYS, B, pages_per_seq, dev, free_order=np.random.default_rng(B).permutation(num_pages).tolist())
        for b in range(B):
            alloc.reserve(b, keys - 1)
        return alloc

    def recycled_allocator(B, keys, window):
        """Table rows of `keys` keys over a pool that holds little more than the window per slot: every slot walks to its last key page by page and gives the pages
        behind the window back as it goes (PageAllocator.release_behind) -- what a generator's pool looks like after a long windowed run."""
        num_pages = B * (window // PAGE_KEYS + 2) + 8
        alloc = PageAllocator(num_pages, PAGE_KEYS, B, keys // PAGE_KEYS, dev, free_order=np.random.default_rng(B).permutation(num_pages).tolist())
        for last in range(PAGE_KEYS - 1, keys, PAGE_KEYS):
            for b in range(B):
                alloc.release_behind(b, last - window + 1)
                alloc.reserve(b, last)
        alloc.check_invariants()
        return alloc

    def layers(alloc, window, n):
        atts = [PagedBatchDecodeAttention(alloc, HEADS, KV_HEADS, dev, cos, sin, window=window) for _ in range(n)]
        for a in atts:
            a.k_pool.normal_(0, 0.8)
            a.v_pool.normal_(0, 0.8)
        return atts

    def step_graph(atts, B, pos_value, bound):
        qkv = (torch.randn(B, (HEADS + 2 * KV_HEADS) * HD, device=dev) * 0.9).half()
        out = torch.empty(B, HEADS * HD, dtype=torch.float16, device=dev)
        pos = torch.full((B,), pos_value, dtype=torch.int32, device=dev)

        def launches():
            for i in range(LAUNCHES):
                atts[i % len(atts)].step(qkv, pos, bound, out=out)
        return graph_of(launches, out)

    def race(what, point, runs):
        """runs: {form: replay}.  REPEATS rounds, the forms alternating; one record per (form, repeat) and the medians."""
        us = {f: [] for f in runs}
        for rep in range(REPEATS):
            for f, run in runs.items():
                run.out.zero_()
                t = timed(run, REPLAYS) / LAUNCHES * 1e3
                assert bool(torch.count_nonzero(run.out[-1]) > 0), f"{f}: the last row came out zero: its position word was not an active one"
                us[f].append(t)
                emit({"what": what, "form": f, **point, "repeat": rep, "us_per_launch": round(t, 3), "launches": LAUNCHES * REPLAYS})
        return {f: sorted(v)[len(v) // 2] for f, v in us.items()}, {f: max(v) - min(v) for f, v in us.items()}

    if "never-binding" in parts:
        for B in BATCHES:
            for keys in (512, 2048):
                alloc = allocator(B, keys)
                runs = {"step": step_graph(layers(alloc, None, ROTATE), B, keys - 1, keys - 1), "window_never_binding": step_graph(layers(alloc, NEVER, ROTATE), B, keys - 1, keys - 1)}
                med, spread = race("never-binding window against the existing step", {"batch": B, "keys": keys}, runs)
                diff = med["window_never_binding"] - med["step"]
                emit({"what": "never-binding window against the existing step: difference", "batch": B, "keys": keys, "step_median_us": round(med["step"], 3),
                      "window_median_us": round(med["window_never_binding"], 3), "difference_us": round(diff, 3), "step_spread_us": round(spread["step"], 3),
                      "predicted_us": ROUND_TRIP_US, "more_than_predicted": diff > ROUND_TRIP_US,
                      "describe": capi.describe_attention_paged_window(B, HEADS, KV_HEADS, keys - 1, PAGE_KEYS, NEVER)})
                del runs, alloc
                torch.cuda.empty_cache()

    if "far" in parts:
        for B in BATCHES:
            near_alloc, far_alloc = allocator(B, FAR_W), allocator(B, FAR_POS + 1)
            runs = {"step_at_4095": step_graph(layers(near_alloc, None, ROTATE), B, FAR_W - 1, FAR_W - 1),
                    "step_at_32767": step_graph(layers(far_alloc, None, 2), B, FAR_POS, FAR_POS),
                    "window_4096_at_32767": step_graph(layers(far_alloc, FAR_W, 2), B, FAR_POS, FAR_POS),
                    # the same launch on the pool a windowed run really leaves: as many pages as the step at 4095 holds, ROTATE layers
                    "window_4096_at_32767_recycled_pool": step_graph(layers(recycled_allocator(B, FAR_POS + 1, FAR_W), FAR_W, ROTATE), B, FAR_POS, FAR_POS)}
            med, spread = race("W = 4096 at position 32767", {"batch": B}, runs)
            emit({"what": "W = 4096 at position 32767: medians", "batch": B, **{f + "_us": round(v, 3) for f, v in med.items()},
                  "window_over_step_at_4095": round(med["window_4096_at_32767"] / med["step_at_4095"], 3),
                  "window_recycled_pool_over_step_at_4095": round(med["window_4096_at_32767_recycled_pool"] / med["step_at_4095"], 3),
                  "step_at_32767_over_window": round(med["step_at_32767"] / med["window_4096_at_32767"], 3),
                  "describe_window": capi.describe_attention_paged_window(B, HEADS, KV_HEADS, FAR_POS, PAGE_KEYS, FAR_W),
                  "describe_step_at_32767": capi.describe_attention_paged(B, HEADS, KV_HEADS, FAR_POS, PAGE_KEYS)})
            del runs, near_alloc, far_alloc
            torch.cuda.empty_cache()

    if "prefill" in parts:
        keys = PREFILL_POS + PREFILL_M
        alloc = allocator(1, (keys + PAGE_KEYS - 1) // PAGE_KEYS * PAGE_KEYS)
        atts = {"prefill": layers(alloc, None, 1)[0], "prefill_window_4096": layers(alloc, PREFILL_W, 1)[0]}
        qkv = (torch.randn(PREFILL_M, (HEADS + 2 * KV_HEADS) * HD, device=dev) * 0.9).half()
        out = torch.empty(PREFILL_M, HEADS * HD, dtype=torch.float16, device=dev)
        seg = [(0, PREFILL_POS, PREFILL_M)]
        us = {f: [] for f in atts}
        for rep in range(REPEATS):
            for f, a in atts.items():
                t = timed(lambda a=a: a.prefill(seg, qkv, out=out), 200) * 1e3
                us[f].append(t)
                emit({"what": "paged prefill chunk", "form": f, "cached_keys": PREFILL_POS, "rows": PREFILL_M, "repeat": rep, "us_per_call": round(t, 2), "calls": 200})
        med = {f: sorted(v)[len(v) // 2] for f, v in us.items()}
        emit({"what": "paged prefill chunk: medians", "cached_keys": PREFILL_POS, "rows": PREFILL_M, "window": PREFILL_W, **{f + "_us": round(v, 2) for f, v in med.items()},
              "window_over_full": round(med["prefill_window_4096"] / med["prefill"], 3), "describe": capi.describe_prefill_paged(HEADS, KV_HEADS, True, seg)})


if __name__ == "__main__":
    main()
