#!/usr/bin/env python3
"""The segmented tiled expands on the clock at prompt sizes, in ONE process: Llama-3-8B's shapes at r = 16 at rows 256, 512 and 2048, under the two sets of words of
scripts/lora_tiled_time.py (`one`: every row on adapter 0; `eight`: 8 equal admissions, admission i on adapter i), with its clock (graph_us: REPS captured copies,
device events around the replays, the forms alternating REPEATS times, medians and spreads).

    gate_up    hidden 4096 -> 2 x ffn 14336, A [32][4096], Bg / Bu [16][14336]; shrink + expand:
        pair     tce_lora_shrink_f16 + tce_lora_expand_silu_mul_f16: what a gate_up=True pool runs at every row count without segmented=True
        tiled    tce_lora_shrink_tiled_f16 + tce_lora_expand_silu_mul_tiled_f16
    qkv        4096 -> 6144 (32 query heads over 8 key / value heads) at R 48, B block-structured as pack_adapter leaves it; the EXPAND alone, on the same partial sums:
        tiled      tce_lora_expand_add_tiled_f16
        segmented  tce_lora_expand_add_segmented_tiled_f16, bounds 0 / 4096 / 5120 / 6144

Before the clock: gate_up -- the largest |pair - tiled| (another summation order: last-bit differences are expected); qkv -- are the two results the same bits.
`gate_up_tiled_from` at the end: the smallest measured row count from which the tiled gate/up is faster than the pair at EVERY larger measured point, both sets of
words, by more than both spreads; None if there is no such point.  No speed was promised for either form: the numbers are what they are.

    python scripts/lora_tiled_seg_time.py [OUT.jsonl]        (default profiles/lora_tiled_seg/lora_tiled_seg_time.jsonl)
"""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

HIDDEN, FFN, Q, KV, RANK = 4096, 14336, 4096, 1024, 16
ROWS = (256, 512, 2048)
ADAPTERS = 8


def main():
    import torch
    from lora_tiled_time import REPEATS, REPLAYS, WINDOW_US, eager_us, graph_us
    from tinychatengine_amd import lora
    assert torch.cuda.is_available(), "no GPU: nothing is measured (there is no fallback)"
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "lora_tiled_seg", "lora_tiled_seg_time.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    dev, recs = torch.device("cuda:0"), []
    gen = torch.Generator(device=dev).manual_seed(6)
    rnd = lambda *shape, std=1.0: torch.empty(shape, device=dev).normal_(0, std, generator=gen).half()
    scale = torch.ones(ADAPTERS, device=dev)
    Agu, Bg, Bu = rnd(ADAPTERS, 2 * RANK, HIDDEN, std=HIDDEN ** -0.5), rnd(ADAPTERS, RANK, FFN, std=0.01), rnd(ADAPTERS, RANK, FFN, std=0.01)
    N, seg = Q + 2 * KV, (0, Q, Q + KV, Q + 2 * KV)
    Aq, Bq = rnd(ADAPTERS, 3 * RANK, HIDDEN, std=HIDDEN ** -0.5), torch.zeros(ADAPTERS, 3 * RANK, N, dtype=torch.float16, device=dev)
    for s in range(3):
        Bq[:, s * RANK:(s + 1) * RANK, seg[s]:seg[s + 1]] = rnd(ADAPTERS, RANK, seg[s + 1] - seg[s], std=0.01)
    with open(out_path, "w") as f:
        for rows in ROWS:
            x, y, c0 = rnd(rows, HIDDEN), rnd(rows, 2 * FFN), rnd(rows, N)
            t, pg, pq = torch.empty(rows, 2 * RANK, dtype=torch.float32, device=dev), lora.tiled_workspace(rows, HIDDEN, 2 * RANK, dev), lora.tiled_workspace(rows, HIDDEN, 3 * RANK, dev)
            act = {k: torch.empty(rows, FFN, dtype=torch.float16, device=dev) for k in ("pair", "tiled")}
            c = {k: c0.clone() for k in ("tiled", "segmented")}
            for setting in ("one", "eight"):
                words = torch.zeros(rows, dtype=torch.int32, device=dev) if setting == "one" else (torch.arange(rows, device=dev) // (rows // ADAPTERS)).int()
                lora.shrink_tiled(x, Aq, words, pq)

                def gu_pair():
                    lora.shrink(x, Agu, words, t)
                    lora.expand_silu_mul(t, Bg, Bu, scale, words, y, act["pair"])

                def gu_tiled():
                    lora.shrink_tiled(x, Agu, words, pg)
                    lora.expand_silu_mul_tiled(pg, Bg, Bu, scale, words, y, act["tiled"], HIDDEN)

                targets = {"gate_up": {"pair": gu_pair, "tiled": gu_tiled},
                           "qkv_expand": {"tiled": lambda: lora.expand_add_tiled(pq, Bq, scale, words, c["tiled"], HIDDEN),
                                          "segmented": lambda: lora.expand_add_segmented_tiled(pq, Bq, scale, words, c["segmented"], HIDDEN, seg)}}
                for target, forms in targets.items():
                    for v in c.values():
                        v.copy_(c0)
                    for fn in forms.values():
                        fn()
                    torch.cuda.synchronize()
                    check = ({"max_abs_pair_minus_tiled": float((act["pair"].float() - act["tiled"].float()).abs().max())} if target == "gate_up" else
                             {"segmented_bits_equal_tiled": bool(torch.equal(c["tiled"].view(torch.int16), c["segmented"].view(torch.int16)))})
                    reps = {n: int(min(200, max(2, WINDOW_US / max(eager_us(torch, fn), 1.0)))) for n, fn in forms.items()}
                    times = {n: [] for n in forms}
                    for _ in range(REPEATS):  # the forms alternate
                        for n, fn in forms.items():
                            for v in c.values():
                                v.copy_(c0)  # (the expands accumulate: every window starts from the same C)
                            times[n].append(graph_us(torch, fn, reps[n]))
                    rec = {"target": target, "rows": rows, "words": setting, "reps": reps, "replays": REPLAYS, "repeats": REPEATS,
                           "us": {n: round(statistics.median(v), 2) for n, v in times.items()}, "spread_us": {n: round(max(v) - min(v), 2) for n, v in times.items()}, **check}
                    recs.append(rec)
                    f.write(json.dumps(rec) + "\n")
                    f.flush()
                    print(json.dumps(rec), flush=True)
        gu = [r for r in recs if r["target"] == "gate_up"]
        won = {rows: all(r["us"]["pair"] - r["us"]["tiled"] > r["spread_us"]["pair"] + r["spread_us"]["tiled"] for r in gu if r["rows"] == rows) for rows in ROWS}
        frm = None
        for rows in reversed(ROWS):
            if not won[rows]:
                break
            frm = rows
        f.write(json.dumps({"gate_up_tiled_from": frm, "gate_up_tiled_faster_at_both_words_by_more_than_the_spreads": won}) + "\n")
        print({"gate_up_tiled_from": frm}, flush=True)


if __name__ == "__main__":
    main()
