#!/usr/bin/env python3
"""The paged KV cache on the clock: BatchedDecoder (contiguous caches) against PagedBatchedDecoder (tinychatengine_amd/paged_kv.py) in ONE process on
Llama-3-8B's shapes (32 layers, hidden 4096, 32 query / 8 key-value heads, ffn 14336), B in {1, 8, 16}, 512 and 2048 keys, page_keys = 64.  Page numbers are
dealt from a seeded shuffle of a pool four times the pages in use, slot by slot in turn, so a sequence's pages lie all over the pool.  The two forms alternate and
every configuration is repeated REPEATS times: the record shows the contiguous form's own repeat-to-repeat spread beside the difference between the forms.

    python scripts/paged_decode_time.py [OUT.jsonl]          one graph per (form, B, context), device events over 50 replays after 5 warm-up replays, per repeat
    python scripts/paged_decode_time.py --eager [OUT.jsonl]  the same launches without graphs, 10 steps per repeat: the driver for
                                                             rocprofv3 --kernel-trace --stats (a run of its own)
    python scripts/paged_decode_time.py --summarize DIR [OUT.jsonl]
                                                             the two attention kernels' times from that run's kernel trace -- told apart by the kernel's last
                                                             template argument (PAGED) --, per grid (B = grid y) and per repeat, and the round-trip budget
    python scripts/paged_decode_time.py --memory [OUT.jsonl] computed, not measured (no GPU): the bytes each form holds for 16 slots, max_keys = 8192 and seeded lengths

The budget: the paged launch may cost one dependent L2-hit round trip more than the contiguous launch -- a fifth of the contiguous launch's
median at B = 1 and 512 keys in the same run (the step is a chain of five) -- on top of the contiguous form's own spread between repeats at that point.
"""
import csv
import glob
import json
import os
import sys
from collections import defaultdict

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BATCHES = (1, 8, 16)
CONTEXTS = (512, 2048)
PAGE_KEYS = 64
POOL_FACTOR = 4
REPEATS = 3
LAYERS, HIDDEN, HEADS, KV_HEADS, FFN = 32, 4096, 32, 8, 14336
WORKGROUPS_X = {128: 512, 256: 2048}  # query heads x chunk slots of the fitted cut -> the context it was cut for (4 chunks at 512 keys, 8 at 2048)


def memory_record():
    """16 slots, max_keys = 8192, lengths from a seeded log-normal (median 400 tokens, a few long ones): what each form holds, all 32 layers."""
    import numpy as np
    slots, max_keys = 16, 8192
    lengths = np.clip(np.random.default_rng(8192).lognormal(np.log(400.0), 1.2, slots).astype(np.int64), 1, max_keys)
    key_bytes = KV_HEADS * 128 * 2 * 2 * LAYERS  # K and V, fp16, every layer
    pages = int(sum((int(n) + PAGE_KEYS - 1) // PAGE_KEYS for n in lengths))
    return {"what": "memory held, computed", "slots": slots, "max_keys": max_keys, "page_keys": PAGE_KEYS, "layers": LAYERS, "lengths": [int(n) for n in lengths],
            "tokens": int(lengths.sum()), "bytes_per_key_all_layers": key_bytes, "contiguous_bytes_reserved": slots * max_keys * key_bytes,
            "paged_live_pages": pages, "paged_bytes_in_live_pages": pages * PAGE_KEYS * key_bytes,
            "ratio": round(slots * max_keys / (pages * PAGE_KEYS), 2)}


def summarize(root):
    rows = []
    for path in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    acc = defaultdict(list)
    for r in rows:
        name = r.get("Kernel_Name", "").replace(" ", "")
        if "attn_decode_fast_kernel" not in name:
            continue
        form = "paged" if "true,true>" in name else "contiguous" if "true,false>" in name or name.endswith("true>") else None
        if form is None:  # a single-sequence form
            continue
        key = (int(r["Grid_Size_X"]) // 256, int(r.get("Grid_Size_Y") or 1), form)
        acc[key].append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0))
    med = lambda v: sorted(v)[len(v) // 2]
    out, table = [], {}
    for (wgs_x, gy, form), ts in sorted(acc.items()):
        ts.sort()
        n = len(ts) // REPEATS
        reps = [med([t for _, t in ts[i * n:(i + 1) * n]]) for i in range(REPEATS)] if n else []  # the run alternates the forms: consecutive thirds are the repeats
        all_t = [t for _, t in ts]
        rec = {"kernel": form, "workgroups_x": wgs_x, "keys": WORKGROUPS_X.get(wgs_x), "batch": gy, "dispatches": len(ts), "median_us": round(med(all_t), 2),
               "min_us": round(min(all_t), 2), "repeat_medians_us": [round(x, 2) for x in reps]}
        table[(wgs_x, gy, form)] = rec
        out.append(rec)
    base = table.get((128, 1, "contiguous"))
    if base:
        trip = base["median_us"] / 5.0
        spread = max(base["repeat_medians_us"]) - min(base["repeat_medians_us"]) if base["repeat_medians_us"] else 0.0
        for (wgs_x, gy, form), rec in sorted(table.items()):
            if form != "paged" or (wgs_x, gy, "contiguous") not in table:
                continue
            c = table[(wgs_x, gy, "contiguous")]
            budget = c["median_us"] + trip + spread
            out.append({"what": "round-trip budget", "keys": rec["keys"], "batch": gy, "contiguous_median_us": c["median_us"], "paged_median_us": rec["median_us"],
                        "difference_us": round(rec["median_us"] - c["median_us"], 2), "one_round_trip_us": round(trip, 2), "contiguous_spread_at_b1_512_us": round(spread, 2),
                        "budget_us": round(budget, 2), "within_budget": rec["median_us"] <= budget})
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--summarize" in sys.argv or "--memory" in sys.argv:
        res = summarize(args[0]) if "--summarize" in sys.argv else [memory_record()]
        out = args[1] if "--summarize" in sys.argv and len(args) > 1 else args[0] if "--memory" in sys.argv and args else None
        for r in res:
            print(json.dumps(r))
        if out:
            with open(out, "w") as f:
                f.write("".join(json.dumps(r) + "\n" for r in res))
        return
    eager = "--eager" in sys.argv
    out_path = args[0] if args else None
    import numpy as np
    import torch
    from tinychatengine_amd import capi
    from tinychatengine_amd.batch_decode import BatchedDecoder
    from tinychatengine_amd.decoder_block import DecoderBlock
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchedDecoder
    assert torch.cuda.is_available(), "a GPU measurement: no device, no number"
    capi.lib()
    dev = torch.device("cuda:0")
    hd, ctx_max = 128, max(CONTEXTS)
    ang = np.random.default_rng(0).uniform(0, 2 * np.pi, (ctx_max, hd // 2))
    cos = torch.from_numpy(np.concatenate([np.cos(ang), np.cos(ang)], axis=1).astype(np.float16)).to(dev)
    sin = torch.from_numpy(np.concatenate([np.sin(ang), np.sin(ang)], axis=1).astype(np.float16)).to(dev)
    blocks = [DecoderBlock(HIDDEN, HEADS, FFN, ctx_max, dev, cos, sin, seed=100 + i, kv_heads=KV_HEADS) for i in range(LAYERS)]
    reps = 10 if eager else 50
    lines = []

    def emit(rec):
        rec.update({"layers": LAYERS, "hidden": HIDDEN, "heads": HEADS, "kv_heads": KV_HEADS, "ffn": FFN, "lm_head": False, "mode": "eager" if eager else "graph"})
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec) + "\n")

    def prepare(fn):
        """fn (eager: every dispatch of a configuration then belongs to one of its repeats), or a graph of it after one eager call."""
        if eager:
            return fn
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        return g.replay

    def timed(run):
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

    emit(memory_record())
    for B in BATCHES:
        cont = [BatchedDecoder(b, B) for b in blocks]
        pages_per_seq = ctx_max // PAGE_KEYS
        num_pages = POOL_FACTOR * B * pages_per_seq
        alloc = PageAllocator(num_pages, PAGE_KEYS, B, pages_per_seq, dev, free_order=np.random.default_rng(B).permutation(num_pages).tolist())
        for i in range(pages_per_seq):  # slot by slot in turn: a sequence's pages are scattered over the pool and interleaved with the others'
            for b in range(B):
                alloc.reserve(b, (i + 1) * PAGE_KEYS - 1)
        paged = [PagedBatchedDecoder(b, alloc) for b in blocks]
        for dc, dp in zip(cont, paged):
            dc.attention.k_cache.normal_(0, 0.8)
            dc.attention.v_cache.normal_(0, 0.8)
            dp.attention.k_pool.normal_(0, 0.8)
            dp.attention.v_pool.normal_(0, 0.8)
        h0 = torch.randn(B, HIDDEN, device=dev).to(torch.float16)
        h = h0.clone()
        pos = torch.zeros(B, dtype=torch.int32, device=dev)
        assert paged[0].attention.table_violations(torch.full((B,), ctx_max - 1, dtype=torch.int32, device=dev), ctx_max - 1) == 0
        for ctx in CONTEXTS:
            pos.fill_(ctx - 1)

            def step_of(decs):
                def step():
                    h.copy_(h0)
                    for d in decs:
                        d.step(h, pos, ctx - 1)
                return step
            runs = {"contiguous": prepare(step_of(cont)), "paged": prepare(step_of(paged))}
            for rep in range(REPEATS):
                for form in ("contiguous", "paged"):  # the forms alternate
                    ms = timed(runs[form])
                    emit({"what": "BatchedDecoder.step" if form == "contiguous" else "PagedBatchedDecoder.step", "form": form, "batch": B, "keys": ctx, "repeat": rep,
                          "ms_per_step": round(ms, 4), "tokens_per_s": round(B * 1e3 / ms, 1), "page_keys": PAGE_KEYS if form == "paged" else None,
                          "pool_pages": num_pages if form == "paged" else None, "pages_in_use": alloc.pages_in_use() if form == "paged" else None,
                          "launches_per_step": LAYERS * (BatchedDecoder.LAUNCHES if cont[0]._up is None else BatchedDecoder.LAUNCHES + 2)})
            del runs
        del cont, paged, alloc
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            f.writelines(lines)


if __name__ == "__main__":
    main()
