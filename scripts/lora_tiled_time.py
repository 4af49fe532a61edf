#!/usr/bin/env python3
"""The two forms of the adapted linear's LoRA launches on the clock at prompt sizes, in ONE process: Llama-3-8B's shapes at r = 16 -- qkv 4096 -> 6144 at R 48,
o 4096 -> 4096 and down 14336 -> 4096 at R 16 -- at rows 16, 64, 128, 256, 512 and 2048, under two sets of words:

    one      every row on adapter 0 (a prompt, or a prefill_many of prompts on one adapter)
    eight    8 equal admissions, admission i on adapter i (rows / 8 contiguous rows each)

    pair     tce_lora_shrink_f16 + tce_lora_expand_add_f16 (lora.shrink / lora.expand_add): today's launches
    tiled    tce_lora_shrink_tiled_f16 + tce_lora_expand_add_tiled_f16
    base     tce_w4a16_forward of the target's base linear at M = rows: the yardstick the adapter's cost stands beside (the words do not reach it)

REPS copies of a form captured in one graph (sized to a window of about WINDOW_US from a first eager measurement), device events around REPLAYS replays, warmed;
the forms alternate, REPEATS times; medians and spreads (max - min over the repeats) are written.  Before the clock: both forms on the same operands, the largest
|difference| of their fp16 results (another summation order: last-bit differences are expected, anything larger is not).

`tiled_from` at the end: the smallest measured row count from which the tiled pair is faster than today's at EVERY larger measured point -- every target, both sets of
words -- by more than both spreads; None if there is no such point.  LoraPool's default stays None either way.

EXPECTATION (written down before the first run, to be confirmed or refuted by the numbers):
  * today's pair serves 4 rows per read of its piece of the adapter with one fmaf per element, so its time grows linearly in rows from the first row block on; the
    tiled pair serves 32 rows per read on matrix instructions and should grow about 8 times more slowly until the C rows' traffic (rows * N * 4 bytes) takes over;
  * at 16 rows the tiled shrink is ONE row tile x S(K) workgroups (4 for K = 4096) against R / 4 x 4 workgroups of today's, and the tiled pair carries the partial
    sums' round trip: the tiled pair is expected to lose or tie at 16 rows and to win from 64 or 128 rows on, by several times at 512 and 2048;
  * `eight` costs today's pair nothing extra (a block of 4 rows never straddles two admissions at these sizes) and the tiled pair a second pass only in tiles that
    straddle two admissions (rows / 8 < 32: at 16, 64 and 128 rows every tile holds 2 .. 8 adapters): its advantage should be smaller there and the same from 256 on;
  * the tiled pair's time at 512 rows should be of the order of the base linear's (27 us for q/k/v), not a multiple of it.

    python scripts/lora_tiled_time.py [OUT.jsonl]        (default profiles/lora_tiled/lora_tiled_time.jsonl)
"""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

TARGET_SHAPES = {"qkv": (48, 4096, 6144), "o": (16, 4096, 4096), "down": (16, 14336, 4096)}  # target: (R, K, N)
ROWS = (16, 64, 128, 256, 512, 2048)
ADAPTERS = 8
REPLAYS, WARMUP, REPEATS = 5, 2, 3
WINDOW_US = 5000.0  # a timed window (one replay) is REPS copies sized to about this long, 2 <= REPS <= 200


def graph_us(torch, fn, reps):
    """median microseconds of one fn() among `reps` captured copies, over REPLAYS replays"""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn()
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(reps):
                fn()
    for _ in range(WARMUP):
        g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPLAYS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / reps)
    return statistics.median(out)


def eager_us(torch, fn):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0


def main():
    import torch
    from tinychatengine_amd import capi, lora
    from tinychatengine_amd.linear import Linear_half_int4, _stream
    assert torch.cuda.is_available(), "no GPU: nothing is measured (there is no fallback)"
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "lora_tiled", "lora_tiled_time.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    dev, recs = torch.device("cuda:0"), []
    gen = torch.Generator(device=dev).manual_seed(5)
    rnd = lambda *shape, std=1.0: torch.empty(shape, device=dev).normal_(0, std, generator=gen).half()
    with open(out_path, "w") as f:
        for target, (R, K, N) in TARGET_SHAPES.items():
            A, B, scale = rnd(ADAPTERS, R, K, std=K ** -0.5), rnd(ADAPTERS, R, N, std=0.01), torch.ones(ADAPTERS, device=dev)
            base = Linear_half_int4.from_float(rnd(N, K, std=K ** -0.5).float()).prepack()
            for rows in ROWS:
                x, c0 = rnd(rows, K), rnd(rows, N)
                t, part, out = torch.empty(rows, R, dtype=torch.float32, device=dev), lora.tiled_workspace(rows, K, R, dev), torch.empty_like(c0)
                for setting in ("one", "eight"):
                    words = torch.zeros(rows, dtype=torch.int32, device=dev) if setting == "one" else (torch.arange(rows, device=dev) // (rows // ADAPTERS)).int()
                    c_pair, c_tiled = c0.clone(), c0.clone()

                    def pair():
                        lora.shrink(x, A, words, t)
                        lora.expand_add(t, B, scale, words, c_pair)

                    def tiled():
                        lora.shrink_tiled(x, A, words, part)
                        lora.expand_add_tiled(part, B, scale, words, c_tiled, K)

                    pair()
                    tiled()
                    torch.cuda.synchronize()
                    diff = float((c_pair.float() - c_tiled.float()).abs().max())
                    moved = float((c_pair.float() - c0.float()).abs().max())
                    forms = {"pair": pair, "tiled": tiled, "base": lambda: capi.check(capi.w4a16_forward(base.desc(x, out), _stream()))}
                    reps = {n: int(min(200, max(2, WINDOW_US / max(eager_us(torch, fn), 1.0)))) for n, fn in forms.items()}
                    times = {n: [] for n in forms}
                    for _ in range(REPEATS):  # the forms alternate
                        for n, fn in forms.items():
                            c_pair.copy_(c0)  # (the expands accumulate: every window starts from the same C)
                            c_tiled.copy_(c0)
                            times[n].append(graph_us(torch, fn, reps[n]))
                    rec = {"target": target, "R": R, "K": K, "N": N, "rows": rows, "words": setting, "slices": lora.tiled_slices(K), "reps": reps, "replays": REPLAYS,
                           "repeats": REPEATS, "us": {n: round(statistics.median(v), 2) for n, v in times.items()},
                           "spread_us": {n: round(max(v) - min(v), 2) for n, v in times.items()}, "max_abs_pair_minus_tiled": diff, "max_abs_delta": moved}
                    recs.append(rec)
                    f.write(json.dumps(rec) + "\n")
                    f.flush()
                    print(json.dumps(rec), flush=True)
        won = {rows: all(r["us"]["pair"] - r["us"]["tiled"] > r["spread_us"]["pair"] + r["spread_us"]["tiled"] for r in recs if r["rows"] == rows) for rows in ROWS}
        frm = None
        for rows in reversed(ROWS):
            if not won[rows]:
                break
            frm = rows
        f.write(json.dumps({"tiled_from": frm, "tiled_faster_at_every_target_and_words_by_more_than_the_spreads": won}) + "\n")
        print({"tiled_from": frm}, flush=True)


if __name__ == "__main__":
    main()
