#!/usr/bin/env python3
"""The FP8 linears on the clock, in ONE process: 4096 x 4096, 11008 x 4096 (gate / up) and 4096 x 11008 (down) at M = 1, 4, 16, 64, 512, 2048.

    skinny / tiled   tce_w8a8_fp8_forward_f16 with the form bit set (the skinny form up to M = 16) on already quantised rows
    quantise         tce_fp8_quantize_rows_f16 alone, M rows of K
    w4a16            the parent's yardstick: tce_w4a16_forward on a prepacked Linear_half_int4 of the same shape

REPS copies captured in one graph, device events around REPLAYS replays, warmed; the forms alternate, REPEATS times; medians and spreads (max - min over the repeats).
Derived per point: the skinny / tiled form's share of 8 TB/s on N K weight bytes, and TFLOP/s (2 M N K).  `tiled_from` at the end: the smallest measured M from which
the tiled form is faster than the skinny one at every larger measured M on every shape by more than both spreads (17 -- past the skinny form's last row count -- when
there is none): fp8_linear.hip's kTiledFromM is set from it.

    python scripts/fp8_linear_time.py [OUT.jsonl]        (default profiles/fp8_linear/fp8_linear_time.jsonl)
"""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [(4096, 4096), (11008, 4096), (4096, 11008)]  # (N, K)
ROWS = [1, 4, 16, 64, 512, 2048]
REPLAYS, WARMUP, REPEATS = 5, 2, 3
WINDOW_US = 10000.0  # a timed window (one replay) is REPS copies sized to about this long from a first eager measurement, 2 <= REPS <= 200


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
    from tinychatengine_amd import capi, quantize
    from tinychatengine_amd.linear import Linear_half_fp8, Linear_half_int4, _stream
    assert torch.cuda.is_available(), "no GPU: nothing is measured (there is no fallback)"
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "fp8_linear", "fp8_linear_time.jsonl")
    dev, recs = torch.device("cuda:0"), []
    gen = torch.Generator(device=dev).manual_seed(5)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        for N, K in SHAPES:
            wq = torch.randint(0, 127, (N, K), dtype=torch.uint8, device=dev, generator=gen)  # finite, positive bytes
            fp8 = Linear_half_fp8(wq, torch.full((N,), 2.0 ** -10, dtype=torch.float32, device=dev))
            w4 = Linear_half_int4(*quantize.quantize_q4_6(torch.empty(N, K, device=dev).normal_(0, 0.02, generator=gen))).prepack()
            for M in ROWS:
                x = torch.empty(M, K, device=dev).normal_(0, 1, generator=gen).half()
                xq, sx = fp8.quantize_rows(x)
                y8, y4 = torch.empty(M, N, dtype=torch.float16, device=dev), torch.empty(M, N, dtype=torch.float16, device=dev)
                forms = {"tiled": lambda: fp8.forward_quantized(xq, sx, y8, capi.TCE_FP8_FORM_TILED), "quantise": lambda: fp8.quantize_rows(x),
                         "w4a16": lambda: capi.check(capi.w4a16_forward(w4.desc(x, y4), _stream()))}
                if M <= 16:
                    forms["skinny"] = lambda: fp8.forward_quantized(xq, sx, y8, capi.TCE_FP8_FORM_SKINNY)
                reps = {n: int(min(200, max(2, WINDOW_US / max(eager_us(torch, fn), 1.0)))) for n, fn in forms.items()}
                times = {n: [] for n in forms}
                for _ in range(REPEATS):  # the forms alternate
                    for n, fn in forms.items():
                        times[n].append(graph_us(torch, fn, reps[n]))
                us = {n: statistics.median(v) for n, v in times.items()}
                rec = {"N": N, "K": K, "M": M, "reps": reps, "replays": REPLAYS, "repeats": REPEATS, "us": {n: round(v, 2) for n, v in us.items()},
                       "spread_us": {n: round(max(v) - min(v), 2) for n, v in times.items()},
                       "share_of_8TBps_on_NK_bytes": {n: round(N * K / (us[n] * 1e-6) / 8e12, 4) for n in ("skinny", "tiled") if n in us},
                       "tflops": {n: round(2.0 * M * N * K / (us[n] * 1e-6) / 1e12, 2) for n in ("skinny", "tiled", "w4a16") if n in us}}
                recs.append(rec)
                f.write(json.dumps(rec) + "\n")
                f.flush()
                print(json.dumps(rec), flush=True)
        wins = {M: all(r["us"]["skinny"] - r["us"]["tiled"] > r["spread_us"]["skinny"] + r["spread_us"]["tiled"] for r in recs if r["M"] == M) for M in ROWS if M <= 16}
        frm = 17
        for M in sorted(wins, reverse=True):
            if not wins[M]:
                break
            frm = M
        f.write(json.dumps({"tiled_from": frm, "tiled_faster_on_every_shape_by_more_than_the_spreads": wins}) + "\n")
        print({"tiled_from": frm}, flush=True)


if __name__ == "__main__":
    main()
