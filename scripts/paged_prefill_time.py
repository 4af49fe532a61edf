#!/usr/bin/env python3
"""The paged prefill on the clock (tce_attention_prefill_paged_f16, tinychatengine_amd/paged_kv.py), Llama-3-8B's attention shape (32 query / 8 key-value heads),
page_keys = 64, page numbers dealt from a seeded shuffle of a pool four times the pages in use.  Both forms run in ONE process, alternating, every point repeated
REPEATS times: the record shows the contiguous form's own repeat-to-repeat spread beside the difference between the forms.

    python scripts/paged_prefill_time.py [OUT.jsonl]          graphs of CALLS calls, device events over REPLAYS replays after 2 warm-up replays, per repeat
    python scripts/paged_prefill_time.py --eager [OUT.jsonl]  the same calls without graphs, 6 per repeat: the driver for rocprofv3 --kernel-trace --stats (a run of
                                                              its own, nothing else traced)
    python scripts/paged_prefill_time.py --summarize DIR [OUT.jsonl]
                                                              the attention kernels' times from that run's kernel trace (attn_prefill_kernel / attn_prefill_paged_kernel), per
                                                              grid
    python scripts/paged_prefill_time.py --memory [OUT.jsonl] D, computed (no GPU): the staging bytes no longer allocated

  A  the attention call (prepare + attention launches): DecodeAttention.prefill on a contiguous cache against PagedBatchDecodeAttention.prefill, (pos, m) in POINTS
  B  admission of a chunk, attention part of one layer: gather pos keys -> tce_attention_prefill_f16 -> scatter m rows (what PagedBatchedDecoder.prefill did before
     the paged prefill; all three remain callable) against the one paged call.  Condition: paged <= sequence + the sequence's spread, at every point.
  C  ragged admission, one whole Llama-3-8B layer: 8 prompts of 64 rows, and 4 of 30, as one prefill_many against that many prefill calls.  Condition: one call is
     not slower.
"""
import csv
import glob
import json
import os
import sys
from collections import defaultdict

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

POINTS = ((0, 512), (0, 2048), (1536, 512), (7680, 512))
RAGGED = ((8, 64), (4, 30))
PAGE_KEYS, POOL_FACTOR, REPEATS, CALLS, REPLAYS = 64, 4, 3, 10, 10
HIDDEN, HEADS, KV_HEADS, FFN, MAX_KEYS = 4096, 32, 8, 14336, 8192


def memory_records():
    out = []
    for max_keys in (2048, 8192):
        per_layer = 2 * KV_HEADS * max_keys * 128 * 2
        out.append({"what": "D staging cache no longer allocated, computed", "max_keys": max_keys, "kv_heads": KV_HEADS, "bytes_per_layer": per_layer, "layers": 32,
                    "bytes_per_model": 32 * per_layer})
    return out


def summarize(root):
    rows = []
    for path in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    acc = defaultdict(list)
    for r in rows:
        name = r.get("Kernel_Name", "").replace(" ", "")
        for tag in ("attn_prefill_paged_kernel", "attn_prefill_kernel", "attn_prefill_prepare_kernel", "kv_pages_copy_kernel"):
            if tag in name:
                acc[(name[name.index(tag):].split("(")[0], int(r["Grid_Size_X"]), int(r.get("Grid_Size_Y") or 1))].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
                break
    med = lambda v: sorted(v)[len(v) // 2]
    return [{"what": "kernel time, rocprofv3 --kernel-trace", "kernel": k, "grid_x_threads": gx, "grid_y_threads": gy, "dispatches": len(ts), "median_us": round(med(ts), 2),
             "min_us": round(min(ts), 2), "max_us": round(max(ts), 2)} for (k, gx, gy), ts in sorted(acc.items())]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--summarize" in sys.argv or "--memory" in sys.argv:
        res = summarize(args[0]) if "--summarize" in sys.argv else memory_records()
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
    from tinychatengine_amd.attention_ops import DecodeAttention
    from tinychatengine_amd.decoder_block import DecoderBlock
    from tinychatengine_amd.paged_kv import PageAllocator, PagedBatchDecodeAttention, PagedBatchedDecoder
    assert torch.cuda.is_available(), "a GPU measurement: no device, no number"
    capi.lib()
    dev = torch.device("cuda:0")
    ang = np.random.default_rng(0).uniform(0, 2 * np.pi, (MAX_KEYS, 64))
    cos = torch.from_numpy(np.concatenate([np.cos(ang), np.cos(ang)], axis=1).astype(np.float16)).to(dev)
    sin = torch.from_numpy(np.concatenate([np.sin(ang), np.sin(ang)], axis=1).astype(np.float16)).to(dev)
    calls, replays = (1, 6) if eager else (CALLS, REPLAYS)
    lines = []

    def emit(rec):
        rec.update({"heads": HEADS, "kv_heads": KV_HEADS, "page_keys": PAGE_KEYS, "mode": "eager" if eager else "graph", "where": "one MI355X, one session"})
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec) + "\n")

    def prepare(fn):
        fn()
        torch.cuda.synchronize()
        if eager:
            return fn
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(calls):
                fn()
        return g.replay

    def timed(run):
        """microseconds per call"""
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(replays):
            run()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / (replays * calls)

    def compare(what, label, runs, extra):
        """runs: {"contiguous" | "sequence" | "separate": fn, "paged": fn}; the forms alternate, REPEATS times"""
        base = [k for k in runs if k != "paged"][0]
        ready = {k: prepare(f) for k, f in runs.items()}
        t = {k: [] for k in runs}
        for _ in range(REPEATS):
            for k in runs:
                t[k].append(timed(ready[k]))
        med = lambda v: sorted(v)[len(v) // 2]
        spread = max(t[base]) - min(t[base])
        rec = {"what": what, "unit": label, **extra, f"{base}_us": [round(x, 2) for x in t[base]], "paged_us": [round(x, 2) for x in t["paged"]],
               f"{base}_median_us": round(med(t[base]), 2), "paged_median_us": round(med(t["paged"]), 2), f"{base}_spread_us": round(spread, 2),
               "difference_us": round(med(t["paged"]) - med(t[base]), 2), "paged_not_slower_beyond_spread": med(t["paged"]) <= med(t[base]) + spread}
        emit(rec)

    for r in memory_records():
        emit(r)

    # ---- A and B: the attention part ----
    stride = MAX_KEYS // PAGE_KEYS
    num_pages = POOL_FACTOR * stride
    alloc = PageAllocator(num_pages, PAGE_KEYS, 1, stride, dev, free_order=np.random.default_rng(1).permutation(num_pages).tolist())
    alloc.reserve(0, MAX_KEYS - 1)
    P = PagedBatchDecodeAttention(alloc, HEADS, KV_HEADS, dev, cos, sin)
    att = DecodeAttention(HEADS, 128, MAX_KEYS, dev, cos, sin, kv_heads=KV_HEADS)
    staging = P.staging()
    for t_ in (P.k_pool, P.v_pool, att.k_cache, att.v_cache):
        t_.normal_(0, 0.8)
    for pos, m in POINTS:
        qkv = (torch.randn(m, (HEADS + 2 * KV_HEADS) * 128, device=dev) * 0.9).half()
        out_c, out_p = torch.empty(m, HEADS * 128, dtype=torch.float16, device=dev), torch.empty(m, HEADS * 128, dtype=torch.float16, device=dev)
        d = capi.describe_prefill_paged(HEADS, KV_HEADS, True, [(0, pos, m)])
        extra = {"pos": pos, "m": m, "form": d["form"], "pair": d["pair"], "blocks": d["blocks"]}
        compare("A attention call (prepare + attention launches)", "call", {"contiguous": lambda: att.prefill(qkv, pos, out=out_c), "paged": lambda: P.prefill([(0, pos, m)], qkv, out=out_p)}, extra)

        def sequence():
            if pos > 0:
                P.gather_into(0, staging, 0, pos)
            staging.prefill(qkv, pos, out=out_c)
            P.admit(0, staging, pos, m)
        compare("B admission of a chunk, attention part of one layer", "call", {"sequence": sequence, "paged": lambda: P.prefill([(0, pos, m)], qkv, out=out_p)},
                {**extra, "sequence": "gather pos keys -> tce_attention_prefill_f16 -> scatter m rows"})
    del P, att, staging, alloc
    torch.cuda.empty_cache()

    # ---- C: ragged admission, one whole layer ----
    block = DecoderBlock(HIDDEN, HEADS, FFN, 2048, dev, cos[:2048].contiguous(), sin[:2048].contiguous(), seed=100, kv_heads=KV_HEADS)
    for n, m in RAGGED:
        stride = 2048 // PAGE_KEYS
        num_pages = POOL_FACTOR * n * stride
        alloc = PageAllocator(num_pages, PAGE_KEYS, n, stride, dev, free_order=np.random.default_rng(n).permutation(num_pages).tolist())
        dec = PagedBatchedDecoder(block, alloc)
        xs = [(torch.randn(m, HIDDEN, device=dev)).half() for _ in range(n)]
        work = [x.clone() for x in xs]

        def reset():
            for w, x in zip(work, xs):
                w.copy_(x)

        def separate():
            reset()
            for s, w in enumerate(work):
                dec.prefill(s, w, 0)

        def together():
            reset()
            dec.prefill_many([(s, w, 0) for s, w in enumerate(work)])
        compare("C ragged admission, one whole layer (linears included)", "layer", {"separate": separate, "paged": together},
                {"prompts": n, "rows_each": m, "separate": f"{n} PagedBatchedDecoder.prefill calls", "paged": "one prefill_many"})
        del dec, alloc
    if out_path:
        with open(out_path, "w") as f:
            f.writelines(lines)


if __name__ == "__main__":
    main()
