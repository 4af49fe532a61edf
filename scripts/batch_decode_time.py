#!/usr/bin/env python3
"""Batched decode on Llama-3-8B's true shapes (32 layers, hidden 4096, 32 query / 8 key-value heads, ffn 14336): one step of B sequences through the 32
decoder layers (tinychatengine_amd/batch_decode.py: 7 launches per layer) against the single-sequence DecoderBlock.step token (5 launches per layer) in
the same process.  Synthetic weights as bench.py's whole_token_leg; KV caches distinct per layer and slot (they stream from HBM).  lm_head is left out of
both.

    python scripts/batch_decode_time.py [OUT.jsonl]          one graph per (B, context), device events over 50 replays after 5 warm-up replays
    python scripts/batch_decode_time.py --eager [OUT.jsonl]  the same launches without graphs, 10 steps per configuration: the driver for
                                                             rocprofv3 --kernel-trace --stats (a run of its own)
    python scripts/batch_decode_time.py --summarize DIR      the attention kernels' times from that run's kernel trace, per grid (B = grid y)
"""
import csv
import glob
import json
import os
import sys
from collections import defaultdict

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BATCHES = (1, 2, 4, 8, 16)
CONTEXTS = (512, 2048)
LAYERS, HIDDEN, HEADS, KV_HEADS, FFN = 32, 4096, 32, 8, 14336


def summarize(root):
    rows = []
    for path in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    acc = defaultdict(list)
    for r in rows:
        name = r.get("Kernel_Name", "")
        if "attn_decode_fast_kernel" not in name:
            continue
        form = "batch" if "true>" in name.replace(" ", "") else "single"
        key = (form, int(r["Grid_Size_X"]) // 256, int(r.get("Grid_Size_Y") or 1))
        acc[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    out = []
    for (form, wgs_x, gy), ts in sorted(acc.items()):
        ts.sort()
        out.append({"kernel": form, "workgroups_x": wgs_x, "batch": gy, "dispatches": len(ts), "median_us": round(ts[len(ts) // 2], 2), "min_us": round(ts[0], 2)})
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--summarize" in sys.argv:
        res = summarize(args[0])
        for r in res:
            print(json.dumps(r))
        if len(args) > 1:
            with open(args[1], "w") as f:
                f.write("".join(json.dumps(r) + "\n" for r in res))
        return
    eager = "--eager" in sys.argv
    out_path = args[0] if args else None
    import numpy as np
    import torch
    from tinychatengine_amd import capi
    from tinychatengine_amd.batch_decode import BatchedDecoder
    from tinychatengine_amd.decoder_block import DecoderBlock
    assert torch.cuda.is_available(), "a GPU measurement: no device, no number"
    capi.lib()
    dev = torch.device("cuda:0")
    hd, ctx_max = 128, max(CONTEXTS)
    ang = np.random.default_rng(0).uniform(0, 2 * np.pi, (ctx_max, hd // 2))
    cos = torch.from_numpy(np.concatenate([np.cos(ang), np.cos(ang)], axis=1).astype(np.float16)).to(dev)
    sin = torch.from_numpy(np.concatenate([np.sin(ang), np.sin(ang)], axis=1).astype(np.float16)).to(dev)
    blocks = [DecoderBlock(HIDDEN, HEADS, FFN, ctx_max, dev, cos, sin, seed=100 + i, kv_heads=KV_HEADS) for i in range(LAYERS)]
    for b in blocks:
        b.attention.k_cache.normal_(0, 0.8)
        b.attention.v_cache.normal_(0, 0.8)
    reps = 10 if eager else 50
    lines = []

    def emit(rec):
        rec.update({"layers": LAYERS, "hidden": HIDDEN, "heads": HEADS, "kv_heads": KV_HEADS, "ffn": FFN, "lm_head": False, "mode": "eager" if eager else "graph"})
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec) + "\n")

    def timed(fn):
        """ms per call: a graph of fn replayed `reps` times after 5 warm-up replays (eager: fn itself)."""
        fn()
        torch.cuda.synchronize()
        run = fn
        if not eager:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
            run = g.replay
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

    # the yardstick: the single-sequence token (DecoderBlock.step, position on the device)
    hid0 = torch.randn(1, HIDDEN, device=dev).to(torch.float16)
    hid = hid0.clone()
    pos1 = torch.zeros(1, dtype=torch.int32, device=dev)
    for ctx in CONTEXTS:
        pos1.fill_(ctx - 1)

        def token():
            hid.copy_(hid0)
            for b in blocks:
                b.step(hid, ctx - 1, pos_device=pos1)
        ms = timed(token)
        emit({"what": "single-sequence DecoderBlock.step", "batch": 1, "keys": ctx, "ms_per_step": round(ms, 4), "tokens_per_s": round(1e3 / ms, 1),
              "launches_per_step": LAYERS * DecoderBlock.LAUNCHES})
    for B in BATCHES:
        decs = [BatchedDecoder(b, B) for b in blocks]
        for d in decs:
            d.attention.k_cache.normal_(0, 0.8)
            d.attention.v_cache.normal_(0, 0.8)
        h0 = torch.randn(B, HIDDEN, device=dev).to(torch.float16)
        h = h0.clone()
        pos = torch.zeros(B, dtype=torch.int32, device=dev)
        for ctx in CONTEXTS:
            pos.fill_(ctx - 1)

            def step():
                h.copy_(h0)
                for d in decs:
                    d.step(h, pos, ctx - 1)
            ms = timed(step)
            emit({"what": "BatchedDecoder.step", "batch": B, "keys": ctx, "ms_per_step": round(ms, 4), "tokens_per_s": round(B * 1e3 / ms, 1),
                  "launches_per_step": LAYERS * (BatchedDecoder.LAUNCHES if decs[0]._up is None else BatchedDecoder.LAUNCHES + 2),
                  "gate_up": "pairs" if decs[0]._up is None else "gate, up, silu_mul"})
        del decs
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            f.writelines(lines)


if __name__ == "__main__":
    main()
