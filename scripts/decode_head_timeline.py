#!/usr/bin/env python3
"""The time budget of a decode launch (profiles/decode_head/): the stamped form of the int8 decode kernel (lab build, debug mode 7704) on the five
launch shapes of the Llama-3-8B token -- q/k/v grouped, o_proj, gate+up grouped, down_proj, lm_head -- issued in token order with the weights rotating over the layers.

    python -m tinychatengine_amd.build --lab
    TCE_LIB_PATH=tinychatengine_amd/lib/libtce_hip_lab.so python scripts/decode_head_timeline.py [--layers 8] [--reps 12] [--label new] >> timeline.jsonl

Wave 0 of every workgroup reads the 100 MHz clock at wave entry, behind its last weight request, with x staged, with the contraction done and behind the store, and
the shader clock at the first two (csrc/w4a16_gemv_i8.hip, I8Stamps).  Per shape, over every workgroup of the launches of the timed repetitions: the median / p10 / p90
of each interval from wave entry (ns; the clock's step is 10 ns), the head in shader cycles, and the launch's span (first entry to last store).
The launches are issued one by one (no graph): the idle time between them is not what is measured here."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from tinychatengine_amd import capi
from tinychatengine_amd.decode import SHAPES, DecodeLinears

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=8)
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--label", default="")
args = ap.parse_args()

L = capi.lib()
dev = torch.device("cuda:0")
dl = DecodeLinears(SHAPES["llama3-8b"], device=dev, prepack=True, layers=args.layers)
launches = dl.token_launches()
names = ["qkv grouped", "o_proj", "gate+up grouped", "down_proj"] * args.layers + ["lm_head"]
SLOTS = 16384  # workgroups per launch at most (lm_head: 8016)
buf = torch.zeros((len(launches), SLOTS, 8), dtype=torch.int64, device=dev)
stream = torch.cuda.current_stream().cuda_stream
rows = {n: [] for n in dict.fromkeys(names)}
spans = {n: [] for n in rows}
for rep in range(args.warmup + args.reps):
    buf.zero_()
    torch.cuda.synchronize()
    for i, group in enumerate(launches):
        capi.check(L.tce_w4a16_set_debug_buffer(C.c_void_p(buf[i].data_ptr())))
        capi.check(L.tce_w4a16_set_debug_mode(7704))
        capi.check(capi.w4a16_forward_group(group, stream) if len(group) > 1 else capi.w4a16_forward(group[0], stream))
    torch.cuda.synchronize()
    if rep < args.warmup:
        continue
    t = buf.cpu().numpy()
    for i, n in enumerate(names):
        live = t[i][t[i][:, 0] != 0]
        assert len(live), f"launch {i} ({n}) wrote no stamps: is TCE_LIB_PATH the lab build?"
        rows[n].append(live)
        spans[n].append((live[:, 4].max() - live[:, 0].min()) * 10)
capi.check(L.tce_w4a16_set_debug_mode(7705))
capi.check(L.tce_w4a16_set_debug_buffer(None))


def q(a):
    return [round(float(np.percentile(a, p)), 1) for p in (10, 50, 90)]


for n, parts in rows.items():
    a = np.concatenate(parts)
    first = np.concatenate([p[p[:, 0] - p[:, 0].min() < 50] for p in parts])  # workgroups that entered within 0.5 us of the launch's first: the first generation's front
    rec = {"label": args.label, "launch": n, "workgroups_per_launch": len(parts[0]), "launches": len(parts), "ns_p10_p50_p90_from_wave_entry": {
        "requests_issued": q((a[:, 1] - a[:, 0]) * 10), "x_staged": q((a[:, 2] - a[:, 0]) * 10), "contraction_done": q((a[:, 3] - a[:, 0]) * 10), "stored": q((a[:, 4] - a[:, 0]) * 10)},
        "ns_p10_p50_p90_contraction_done_to_stored": q((a[:, 4] - a[:, 3]) * 10),  # the tail of the launch, per workgroup (profiles/decode_tail/)
        "head_shader_cycles_p10_p50_p90": q(a[:, 6] - a[:, 5]),
        "first_front_requests_issued_ns_p10_p50_p90": q((first[:, 1] - first[:, 0]) * 10), "first_front_head_shader_cycles_p10_p50_p90": q(first[:, 6] - first[:, 5]),
        "first_front_stored_ns_p10_p50_p90": q((first[:, 4] - first[:, 0]) * 10),
        "launch_span_ns_p10_p50_p90": q(np.array(spans[n]))}
    print(json.dumps(rec), flush=True)
