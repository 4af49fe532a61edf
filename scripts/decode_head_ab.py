#!/usr/bin/env python3
"""Same-session A/B of two builds of the library on the headline (plain `bench.py`: one Llama-3-8B decode token, graph replay), for a change that acts INSIDE the
stream-ordered launches (the decode kernels' flat / preloaded arguments, profiles/decode_head/):

    python scripts/decode_head_ab.py <parent build's libtce_hip.so> [--out DIR] [--pairs 3] [--steps 200] [--no-trace | --trace-only]

  1. parent / new / parent / new ... (`TCE_LIB_PATH=<parent>` against the in-tree build, as scripts/probes/ab_libs.sh alternates builds): every bench line -> DIR/bench_ab.jsonl,
     closed by a verdict row: the gain of the medians against three times the parent's own max - min over its repeats;
  2. `bench.py --dump-outputs` under both builds: the .npy files compared byte for byte (a row of bench_ab.jsonl); `bench.py --shapes-only` under both builds, untraced:
     the token's launch shapes on their own (a row per build);
  3. `rocprofv3 --kernel-trace --stats` around `bench.py --shapes-only` under both builds (kernel trace only: counters never share a run with tracing): the durations per
     (kernel, grid, workgroup) -> DIR/kernel_stats_{parent,new}.txt.

Every step that opens the GPU runs under its own `timeout -k 10`; the first step that fails, faults or runs out of time ends the script: nothing is started after it.
"""
import argparse
import csv
import filecmp
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
from collections import defaultdict

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu_step(what, cmd, limit, env=None, log=None):
    """one GPU step under its own time limit; any failure ends the script here"""
    full = ["timeout", "-k", "10", str(limit)] + cmd
    print(f"== {what}: {' '.join(cmd)}", flush=True)
    r = subprocess.run(full, cwd=REPO, env={**os.environ, **(env or {})}, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if log:
        with open(log, "w") as f:
            f.write(r.stdout)
    if r.returncode != 0:
        print(r.stdout[-4000:])
        print(f"!! {what}: exit status {r.returncode} -- stopping, nothing else is started", flush=True)
        sys.exit(r.returncode)
    return r.stdout


def bench_line(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    return json.loads(lines[-1])


def kernel_stats(trace_dir, dst, title):
    rows = []
    for f in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)):
        rows += [r for r in csv.DictReader(open(f)) if "tce::" in r.get("Kernel_Name", "")]
    by = defaultdict(list)
    for r in rows:
        name = r["Kernel_Name"]
        name = name[name.find("tce::"):].replace("tce::(anonymous namespace)::", "")
        name = name.split("(")[0][:72]
        by[(name, int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0), int(r.get("Workgroup_Size_X", r.get("Workgroup_Size", 0)) or 0))].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    with open(dst, "w") as f:
        f.write(f"# {title}: rocprofv3 --kernel-trace --stats around `bench.py --shapes-only`; kernel | grid threads x workgroup | n | duration us min / median / mean\n")
        for k, d in sorted(by.items(), key=lambda kv: -sum(kv[1])):
            d.sort()
            f.write(f"{k[0]} | {k[1]} x {k[2]} | n={len(d)} | {d[0] / 1e3:.2f} / {d[len(d) // 2] / 1e3:.2f} / {sum(d) / len(d) / 1e3:.2f}\n")
    return len(rows)


def traces(a, envs, tmp):
    for build in ("parent", "new"):
        d = os.path.join(tmp, "kt_" + build)
        gpu_step(f"kernel trace {build}", ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "kt", "--", sys.executable, "bench.py", "--shapes-only"], 600, envs[build],
                 log=os.path.join(tmp, f"kt_{build}.log"))
        n = kernel_stats(d, os.path.join(a.out, f"kernel_stats_{build}.txt"), build)
        print(f"   {n} dispatches", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "decode_head"))
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--no-trace", action="store_true", help="steps 1 and 2 only")
    ap.add_argument("--trace-only", action="store_true", help="step 3 only")
    a = ap.parse_args()
    parent = os.path.abspath(a.parent)
    assert os.path.exists(parent), parent
    os.makedirs(a.out, exist_ok=True)
    envs = {"parent": {"TCE_LIB_PATH": parent}, "new": {}}
    os.environ.pop("TCE_LIB_PATH", None)
    rows, series = [], {"parent": [], "new": []}
    if a.trace_only:
        tmp = tempfile.mkdtemp(prefix="decode_head_ab_")
        try:
            traces(a, envs, tmp)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        return
    for i in range(max(a.pairs, 3)):
        for build in ("parent", "new"):
            j = bench_line(gpu_step(f"bench {build} #{i + 1}", [sys.executable, "bench.py", "--steps", str(a.steps)], 600, envs[build]))
            series[build].append(j["value"])
            rows.append({"build": build, "repeat": i + 1, "value": j["value"], "unit": j.get("unit"), "ms_per_step": j.get("ms_per_step"), "steps": j.get("steps")})
            print(f"   {build}: {j['value']} {j.get('unit')}", flush=True)
    spread = max(series["parent"]) - min(series["parent"])
    gain = statistics.median(series["new"]) - statistics.median(series["parent"])
    rows.append({"verdict": "gain" if gain > 3 * spread else "within noise", "parent": series["parent"], "new": series["new"], "parent_max_minus_min": round(spread, 3),
                 "gain_of_medians": round(gain, 3), "gain_percent": round(100 * gain / statistics.median(series["parent"]), 3), "required": "gain_of_medians > 3 x parent_max_minus_min"})
    print(json.dumps(rows[-1]), flush=True)
    # outputs, byte for byte
    tmp = tempfile.mkdtemp(prefix="decode_head_ab_")
    try:
        for build in ("parent", "new"):
            gpu_step(f"dump outputs {build}", [sys.executable, "bench.py", "--steps", "20", "--dump-outputs", os.path.join(tmp, build)], 600, envs[build])
        names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(tmp, "parent", "*.npy")))
        names_new = sorted(os.path.basename(f) for f in glob.glob(os.path.join(tmp, "new", "*.npy")))
        differing = [n for n in names if n not in names_new or not filecmp.cmp(os.path.join(tmp, "parent", n), os.path.join(tmp, "new", n), shallow=False)]
        rows.append({"dump_outputs": "byte-identical" if names and names == names_new and not differing else "DIFFERENT", "files": len(names), "differing": differing})
        print(json.dumps(rows[-1]), flush=True)
        # the token's launch shapes on their own (`roofline.shapes` of the full bench line: graph-replayed, weights rotating over the layers), untraced
        for build in ("parent", "new"):
            out = gpu_step(f"launch shapes {build}", [sys.executable, "bench.py", "--shapes-only"], 600, envs[build])
            shapes = bench_line(out)["decode_launch_shapes"]["linears"]
            rows.append({"build": build, "launch_shapes": [{"name": r.get("name"), "launch": r.get("launch"), "us": r.get("us"), "frac_of_8TBs": r.get("frac_of_8TBs")} for r in shapes]})
            print(json.dumps(rows[-1]), flush=True)
        with open(os.path.join(a.out, "bench_ab.jsonl"), "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in rows))
        if differing or not names or names != names_new:
            sys.exit(1)
        if not a.no_trace:
            traces(a, envs, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
