#!/usr/bin/env python3
"""bench.py -- decode tokens/s of the W4A16 hot path (the linears of one decode token) on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload baseline-named|llama3-8b|llama2-13b] [--dump-outputs DIR] [--full]

A "step" is one decode token: every W4A16 linear of every transformer block + lm_head (M = 1), issued through the
C ABI of libtce_hip.so as ONE hipGraph replay (tinychatengine_amd.capi.Plan); weights are synthetic N(0, 0.02^2)
quantized with the reference's q4_6 recipe, all layers distinct (3.4 GB for the default workload, so a token streams
from HBM, not from the 256 MB Infinity Cache) and resident in HBM before the timed region.  N > 1: one process per
GPU (torch.distributed, backend nccl == RCCL), every linear column-sharded N-way, one all-gather per transformer block.

Prints ONE JSON line (rank 0): metric/value/unit/ms_per_step per the driver contract.  A plain run does only that: set up, warm up,
time the K steps, write the outputs (--dump-outputs), print the line.  --full adds everything else the benchmark measures:
  "roofline":     the dominant kernel (the grouped gate+up GEMV launch), algorithmic bytes / HIP-event time, vs 8 TB/s
  "cpu_baseline": the reference's own CPU path (oracle/_ref, built by oracle/Makefile) timed on this host, and the parity check
  "other_configs" & co.: the other workloads, precisions and sizes (--no-extras / --no-cpu-baseline drop parts of it).
Only the cpu_baseline leg touches oracle/; the measured path never does.

--dump-outputs DIR: after the timed steps, every output buffer of the token as the last step left it (the last block's q/k/v, o, gate,
up, down and the logits) as DIR/<name>.npy in float32.  Weights and activations are seeded, so the same arguments give the same inputs.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s is the measured streaming ceiling


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200, help="timed steps (decode tokens)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true", help="besides the headline: the roofline leg, the other workloads / precisions / sizes, the adapter path, "
                                                         "the CPU baseline and the parity check (a plain run times the headline only)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="write the outputs of the last timed step as DIR/<name>.npy (float32)")
    ap.add_argument("--workload", default="llama3-8b", choices=["baseline-named", "llama3-8b", "llama2-13b", "tiny"],
                    help="the model whose decode token is the headline `value`.  Default: the model the metric names (Llama-3-8B's true shapes, llm/include/model.h:83); "
                         "the shape set BASELINE.json's configs[1] spells (4096x4096, 4096x11008: Llama-2-7B widths) is timed beside it and reported under `baseline_named_shapes` "
                         "and, launch by launch, under `roofline.shapes`")
    ap.add_argument("--no-prepack", action="store_true", help="decode on the q4_6 arrays with the fp16-unpack GEMV kernels (rounds 1-3) instead of the int8-contraction "
                                                               "kernel on the packed copies (round 4): A/B runs")
    ap.add_argument("--layers", type=int, default=None, help="override the number of transformer blocks (debug only)")
    ap.add_argument("--ungrouped", action="store_true", help="one launch per linear, as the reference issues them")
    ap.add_argument("--gathers-per-block", type=int, default=0, choices=[0, 1, 4], help="N > 1: 0 (default) = time both the north-star definition (1) and the dependency-faithful form (4)")
    ap.add_argument("--gather", default="all", choices=["all", "peer", "rccl"],
                    help="N > 1: how the ranks' output slices are joined -- peer: tce_allgather_f16 (one peer-write kernel per exchange over xGMI, csrc/comm.hip); rccl: torch.distributed "
                         "all_gather_into_tensor; all (default): both are timed in the same run (config.gather_variants), the headline is the faster one-gather-per-block variant")
    ap.add_argument("--no-projection", action="store_true", help="N = 1: skip other_configs.projected_scaling (this GPU timing one rank's N/P-row shards for P = 2, 4, 8)")
    ap.add_argument("--issue", default="graph", choices=["auto", "graph", "token"],
                    help="N = 1: graph = one hipGraph of 129 launches per token (stream order); token = ONE persistent kernel per token, the linears' data "
                         "flow ordered by tagged output words (TCE_PLAN_TAGGED); auto = both are verified against each other and timed, the faster one is the step")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--roofline-only", action="store_true", help="run only the dominant-kernel loop (for rocprofv3)")
    ap.add_argument("--roofline-launches", type=int, default=256)
    ap.add_argument("--roofline-eager", action="store_true", help="roofline leg without graph capture (for rocprofv3 PMC passes)")
    ap.add_argument("--shapes-only", action="store_true", help="run only the per-launch-shape legs (every launch shape of the token + the attention step) and print them: the "
                    "command scripts/profile_r3.sh traces with rocprofv3 (graph-replayed; with --roofline-eager issued eagerly for the PMC passes)")
    ap.add_argument("--no-extras", action="store_true", help="skip the short prefill-GEMM / W8A8 legs (BASELINE configs 3 and 4) reported under \"other_configs\"")
    ap.add_argument("--force-dist", action="store_true", help="run the N>1 code path (RCCL init, gathers, graph capture) even with one rank")
    ap.add_argument("--no-graph", action="store_true", help="N > 1: issue the token eagerly instead of capturing GEMVs + gathers into one graph")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="torch.distributed backend (gloo + TCE_BENCH_SINGLE_DEVICE=1: exercise the multi-rank orchestration on one GPU)")
    ap.add_argument("--selftest-emit", default="", help=argparse.SUPPRESS)
    ap.add_argument("--cpu-worker", default="", choices=["", "avx", "avx_cold", "ref", "parity"], help=argparse.SUPPRESS)
    ap.add_argument("--threads", type=int, default=8, help=argparse.SUPPRESS)
    ap.add_argument("--parity-dir", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


LINE_BUDGET = 6000  # bytes; the driver keeps the last 8 KB of stdout+stderr (BENCH_r04: a 21.7 KB line came back as parsed = null)


def _r(x, n=3):
    return round(x, n) if isinstance(x, float) else x


def compact_line(full: dict, details_file: str | None = None, budget: int = LINE_BUDGET) -> dict:
    """The ONE line the driver reads, from the full record (which goes to `details_file`): the contract keys as they are, every table as rows of
    numbers, no prose.  Blocks are dropped lowest priority first until the line fits `budget` bytes -- the contract keys, `roofline` and
    `cpu_baseline` are never dropped.  (Report shape of the reference: one number per section, llm/include/profiler.h:38-47.)"""
    out = {k: full[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data") if k in full}
    cfg = full.get("config", {})
    c = {k: cfg[k] for k in ("workload", "parallelism", "issue", "algorithmic_bytes_per_token") if k in cfg}
    for k in ("workload", "parallelism", "issue"):
        if isinstance(c.get(k), str) and len(c[k]) > 200:
            c[k] = c[k][:197] + "..."
    gv = cfg.get("gather_variants")
    if isinstance(gv, dict):
        c["gather_variants"] = {("peer" if k.startswith("peer") else "rccl" if k.startswith("RCCL") else k[:8]) + ("_4" if ", 4 gather" in k else "_1" if ", 1 gather" in k else "") + ("x1" if "one launch per block" in k else "f" if "inside the block" in k else ""):
                                (v.get("tokens_per_s", "rejected") if isinstance(v, dict) else v) for k, v in gv.items()}
    for k in ("ranks", "rccl_ranks", "gather_path"):
        if k in cfg:
            c[k] = cfg[k]
    out["config"] = c
    if "whole_token" in full:
        w = full["whole_token"]
        out["whole_token"] = {k: w[k] for k in ("achieved_GBs_per_gpu", "frac_of_8TBs", "launches_per_token", "event_ms_per_token") if k in w}
    roof = full.get("roofline")
    if isinstance(roof, dict):
        rr = {k: roof[k] for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_launch", "avg_launch_us", "launches_timed", "launch_us_p10_p50_p90",
                                   "measured_streaming_read_GBs", "error") if k in roof}
        if isinstance(roof.get("kernel"), str):
            rr["kernel"] = roof["kernel"][:120]
        if isinstance(roof.get("shapes"), list):
            rr["shapes_cols"] = ["workload", "name", "launch", "us", "frac_of_8TBs"]
            rr["shapes"] = [[r.get("workload", ""), r.get("name", ""), r.get("launch", "").replace(" (lm_head)", ""), r.get("us"), r.get("frac_of_8TBs")] for r in roof["shapes"]]
        out["roofline"] = rr
    optional = []  # (priority, key, value): lower priority number = dropped later

    def opt(prio, key, val):
        if val is not None:
            optional.append((prio, key, val))

    cpu = full.get("cpu_baseline")
    if isinstance(cpu, dict):
        cc = {k: cpu[k] for k in ("value", "unit", "cores", "kind", "cpu_model", "nproc", "error") if k in cpu}
        if isinstance(cpu.get("sample"), str):
            cc["sample"] = cpu["sample"][:160]
        out["cpu_baseline"] = cc
        if "value_weights_from_dram" in cpu:
            cc["value_weights_from_dram"] = cpu["value_weights_from_dram"]
    par = full.get("parity")
    if isinstance(par, dict):
        opt(0, "parity", {k: par[k] for k in ("worst_err_over_tol", "max_share_passing_only_through_the_floor", "max_share_failing_with_floor_rms_over_256", "error") if k in par}
            | ({"linears_checked": len(par["rows"])} if isinstance(par.get("rows"), list) else {}))
    rn = full.get("cpu_baseline_ref_naive")
    if isinstance(rn, dict):
        opt(1, "cpu_baseline_ref_naive", {"value": rn.get("value"), "unit": rn.get("unit"), "cores": rn.get("cores"), "kind": rn.get("kind"), "sample": str(rn.get("sample", ""))[:90]})
    ap_ = full.get("adapter_path")
    if isinstance(ap_, dict):
        a = ap_.get("adapter") if isinstance(ap_.get("adapter"), dict) else {}
        c_ = {"model": ap_.get("model"), "keys": ap_.get("keys"), **{k: a.get(k) for k in ("tokens_per_s", "ms_per_token_wall", "ms_per_token_events", "host_us_per_call", "launches_per_token")}}
        for leg in ("capi_eager", "capi_graph"):
            if isinstance(ap_.get(leg), dict):
                c_[leg + "_tokens_per_s"] = ap_[leg].get("tokens_per_s")
                c_[leg + "_host_us_per_call"] = ap_[leg].get("host_us_per_call")
        for k in ("adapter_over_graph", "adapter_first_token_ms", "error"):
            if k in ap_:
                c_[k] = ap_[k] if k != "error" else str(ap_[k])[:160]
        opt(0, "adapter_path", c_)
    for key in ("baseline_named_shapes", "llama3_8b_true_shapes"):
        sec = full.get(key)
        if isinstance(sec, dict):
            s = {k: sec[k] for k in ("tokens_per_s", "ms_per_token", "frac_of_8TBs", "error") if k in sec}
            dwa = sec.get("decode_with_attention")
            if isinstance(dwa, dict):
                for ctx in ("context_512", "context_2048"):
                    if isinstance(dwa.get(ctx), dict):
                        s["with_attention_" + ctx[8:] + "_keys_tokens_per_s"] = dwa[ctx].get("tokens_per_s")
            opt(2, key, s)
    oc = full.get("other_configs") if isinstance(full.get("other_configs"), dict) else {}
    dwa = oc.get("decode_with_attention")
    if isinstance(dwa, dict):
        d = {"launches_per_token": dwa.get("launches_per_token")}
        for ctx in ("context_512", "context_2048"):
            if isinstance(dwa.get(ctx), dict):
                d[ctx] = {k: dwa[ctx].get(k) for k in ("tokens_per_s", "ms_per_token", "frac_of_8TBs")}
        pf = dwa.get("prefill")
        if isinstance(pf, dict):
            for k in ("prompt_512_rows", "prompt_2048_rows"):
                if isinstance(pf.get(k), dict):
                    d[k] = {"ms": pf[k].get("ms"), "TFLOPs": pf[k].get("TFLOPs_linears_plus_causal_attention")}
        if "error" in dwa:
            d["error"] = str(dwa["error"])[:120]
        opt(3, "decode_with_attention", d)
    gemm_rows = []
    for m in (512, 2048, 4096):
        rows = oc.get(f"w4a16_prefill_gemm_M{m}")
        if isinstance(rows, list):
            for r in rows:
                if isinstance(r, dict) and "TFLOPs" in r:
                    us = (r.get("prepacked") or {}).get("us")
                    gemm_rows.append([r.get("M"), r.get("N"), r.get("K"), us, r.get("TFLOPs"), r.get("frac_of_2500_TFLOPs")])
    if gemm_rows:
        opt(4, "w4a16_prefill_gemm", {"cols": ["M", "N", "K", "us", "TFLOPs", "frac_of_2500"], "rows": gemm_rows})
    w8 = full.get("w8a8_opt125m_shapes")
    if isinstance(w8, dict) and isinstance(w8.get("launches"), list):
        opt(5, "w8a8_opt125m_shapes", {"cols": ["batch", "M", "N", "K", "us", "TOPs", "frac_of_5000"],
                                        "rows": [[r.get("batch", 1), r.get("M"), r.get("N"), r.get("K"), r.get("us"), r.get("TOPs"), r.get("frac_of_5000_TOPs")] for r in w8["launches"]]})
    zp = oc.get("gate_up_random_zero_points")
    if isinstance(zp, dict):
        opt(6, "gate_up_random_zero_points", {k: zp.get(k) for k in ("us", "frac_of_8TBs", "us_zero_point_8") if k in zp})
    ps = oc.get("projected_scaling")
    if isinstance(ps, dict) and isinstance(ps.get("models"), dict):
        pr = {}
        for name, m in ps["models"].items():
            pr[name.split(" ")[0]] = {p: (v.get("tokens_per_s") or v.get("projected_tokens_per_s_1_gather_per_block_peer_write")) for p, v in m.items() if isinstance(v, dict)}
        opt(8, "projected_scaling_NOT_MEASURED", pr)
    sec13 = full.get("llama2_13b")
    if isinstance(sec13, dict):
        opt(2, "llama2_13b", {k: sec13[k] for k in ("tokens_per_s", "ms_per_token", "frac_of_8TBs", "gather", "error") if k in sec13})
    if details_file:
        out["details_file"] = details_file
    for _, key, val in sorted(optional, key=lambda t: t[0]):
        trial = dict(out, **{key: val})
        if len(json.dumps(trial, separators=(",", ":"))) <= budget:
            out = trial
        else:
            out.setdefault("dropped_for_size", []).append(key)
    return out


def dump_line(d: dict) -> str:
    return json.dumps(d, separators=(",", ":"))


# ----------------------------------------------------------------------------------------------------------------
def other_configs_leg(torch, dev):
    """BASELINE.json configs 3 and 4, measured live next to the headline metric (they are parity-test cases, not the bench
    line, but their rates belong beside it): W4A16 prefill GEMM at M = 512 on the three Llama linear shapes (TFLOP/s against
    the 2.5 PFLOP/s dense fp16 MFMA peak) and the W8A8 int8 GEMM on the OPT-125M shapes.  hipGraph of back-to-back launches
    rotating over distinct weights, HIP events around the replays; a few seconds in total."""
    import ctypes as C
    from tinychatengine_amd import capi
    from tinychatengine_amd.linear import Linear_half_int4
    L = capi.lib()

    def time_graph(fn, launches, reps=int(os.environ.get("TCE_BENCH_GEMM_REPS", "8"))):
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            sp = C.c_void_p(s.cuda_stream)
            with torch.cuda.graph(g, stream=s):
                for i in range(launches):
                    fn(i, sp)
        for _ in range(8):  # burn-in: the first replays after allocating fresh weights run ~10 % slow
            g.replay()
        torch.cuda.synchronize()
        samples = []
        for _ in range(3):  # (round 5: three samples of `reps` replays, the median -- one sample of 3 x 16 launches moved by +-5 % from run to run)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            samples.append(e0.elapsed_time(e1) * 1e3 / (reps * launches))
        return sorted(samples)[1]

    out = {"w4a16_prefill_gemm_M512": [], "w4a16_prefill_gemm_M2048": [], "w4a16_prefill_gemm_M4096": [], "w8a8_opt125m": []}
    scratch = torch.zeros(int(L.tce_w4a16_gemm_scratch_bytes()), dtype=torch.uint8, device=dev)  # lets the pre-packed GEMM split K across workgroups
    gen = torch.Generator(device=dev).manual_seed(1)
    for (N, K) in ((4096, 4096), (11008, 4096), (4096, 11008)):
        nsets = max(2, int(3e8 // (N * K // 2)))  # > 256 MiB of distinct weights: they come from HBM
        zw = (K // 128 + 7) // 8
        sets = []
        for _ in range(nsets):
            qw = torch.randint(-2**31, 2**31 - 1, (N, K // 8), dtype=torch.int32, device=dev, generator=gen)
            sc = (torch.rand((N, zw * 8), device=dev, generator=gen) * 0.01 + 0.001).to(torch.float16)
            zp = torch.full((N, zw), -2004318072, dtype=torch.int32, device=dev)  # 0x88888888
            sets.append((qw, sc, zp))
        # the q4_mfma copies (tce_w4a16_prepack: load-time, once per tensor) that let tce_w4a16_forward choose the 128-row MFMA kernel
        need = int(L.tce_w4a16_prepack_bytes(N, K, 128))
        packs = []
        for (q, s_, z) in sets:
            pk = torch.empty(need, dtype=torch.uint8, device=dev)
            d = capi.W4A16Desc(M=1, N=N, K=K, group_size=128, qweight=q.data_ptr(), scales=s_.data_ptr(), zeros=z.data_ptr())
            capi.check(L.tce_w4a16_prepack(C.byref(d), pk.data_ptr(), None))
            packs.append(pk)
        torch.cuda.synchronize()
        for M in (512, 2048, 4096):
            x = torch.randn(M, K, device=dev, generator=gen).to(torch.float16)
            y = torch.empty(M, N, dtype=torch.float16, device=dev)
            row = {"M": M, "N": N, "K": K}
            for name, with_pack in (("q4_6_only", False), ("prepacked", True)):
                # flags: what a host sets once per linear at load time -- the reference's quantizer writes zero point 8 everywhere (quantize_methods.py:436-440) and
                # tce_w4a16_check_zero_point_8 confirms it on the tensor (the C++ adapter does exactly this: adapter/matmul_operator_hip.cc); the wide GEMM forms
                # and the decode kernel's fast path read no zero points on such a linear
                ds = [capi.W4A16Desc(M=M, N=N, K=K, group_size=128, A=x.data_ptr(), qweight=q.data_ptr(), scales=s_.data_ptr(), zeros=z.data_ptr(), C=y.data_ptr(),
                                     prepacked=pk.data_ptr() if with_pack else None, scratch=scratch.data_ptr() if with_pack else None,
                                     flags=capi.TCE_W4_ZERO_POINT_IS_8 if int(L.tce_w4a16_check_zero_point_8(z.data_ptr(), z.numel())) == 1 else 0)
                      for (q, s_, z), pk in zip(sets, packs)]
                us = time_graph(lambda i, sp: capi.check(L.tce_w4a16_forward(C.byref(ds[i % len(ds)]), sp)), 16)
                buf = C.create_string_buffer(256)
                L.tce_w4a16_describe_dispatch(C.byref(ds[0]), buf, 256)
                row[name] = {"us": round(us, 1), "TFLOPs": round(2.0 * M * N * K / us / 1e6, 1), "dispatch": buf.value.decode()}
            best = max(row["q4_6_only"]["TFLOPs"], row["prepacked"]["TFLOPs"])
            row["TFLOPs"] = row["prepacked"]["TFLOPs"]  # what a caller that prepacked at load time gets
            row["frac_of_2500_TFLOPs"] = round(row["TFLOPs"] / 2500.0, 3)
            row["best_of_both_TFLOPs"] = best
            out[f"w4a16_prefill_gemm_M{M}"].append(row)
        del packs
        del sets
    # BASELINE config 4: the OPT-125M linears at M = 512 / 108 / 1 (the reference's test shapes: test_ops.cc:177-345) ...
    for (M, N, K) in ((512, 768, 768), (512, 3072, 768), (512, 768, 3072), (108, 768, 768), (108, 3072, 768), (108, 768, 3072), (1, 768, 768), (1, 3072, 768), (1, 768, 3072)):
        a = torch.randint(-128, 128, (M, K), dtype=torch.int8, device=dev)
        b = torch.randint(-128, 128, (N, K), dtype=torch.int8, device=dev)
        bias = torch.randint(-128, 128, (N,), dtype=torch.int8, device=dev)
        o = torch.empty((M, N), dtype=torch.int8, device=dev)
        d = capi.W8A8Desc(M=M, N=N, K=K, batch=1, A=a.data_ptr(), B=b.data_ptr(), bias=bias.data_ptr(), C=o.data_ptr(), alpha=0.0005, beta=0.02,
                          q_min=-128, q_max=127, bias_kind=capi.TCE_BIAS_INT8, out_kind=capi.TCE_OUT_INT8)
        # (round 5: through the size-prefixed descriptor with a scratch area -- few tiles with a long k chain, 512 / 108 x 768 x 3072, have their k-steps cut across workgroups)
        v2 = capi.W8A8DescV2(struct_size=C.sizeof(capi.W8A8DescV2), reserved0=0, desc=d, scratch=capi.w8a8_scratch(dev).data_ptr())
        us = time_graph(lambda i, sp: capi.check(L.tce_w8a8_matmul_v2(C.byref(v2), sp)), 64)
        us_plain = time_graph(lambda i, sp: capi.check(L.tce_w8a8_matmul(C.byref(d), sp)), 64)
        out["w8a8_opt125m"].append({"M": M, "N": N, "K": K, "us": round(us, 2), "TOPs": round(2.0 * M * N * K / us / 1e6, 1), "us_without_scratch": round(us_plain, 2)})
    # ... and its two attention BMMs as one batched launch each: b = 12, (512, 512, 64) fp32 out and (512, 64, 512) int8 out (test_ops.cc:380-410, 444-473)
    for (b_, M, N, K, fp32) in ((12, 512, 512, 64, True), (12, 512, 64, 512, False)):
        a = torch.randint(-128, 128, (b_, M, K), dtype=torch.int8, device=dev)
        w = torch.randint(-128, 128, (b_, N, K), dtype=torch.int8, device=dev)
        o = torch.empty((b_, M, N), dtype=torch.float32 if fp32 else torch.int8, device=dev)
        d = capi.W8A8Desc(M=M, N=N, K=K, batch=b_, A=a.data_ptr(), B=w.data_ptr(), C=o.data_ptr(), strideA=M * K, strideB=N * K, strideC=M * N, alpha=0.0013,
                          q_min=-128, q_max=127, bias_kind=capi.TCE_BIAS_NONE, out_kind=capi.TCE_OUT_FP32 if fp32 else capi.TCE_OUT_INT8)
        us = time_graph(lambda i, sp: capi.check(L.tce_w8a8_matmul(C.byref(d), sp)), 64)
        out["w8a8_opt125m"].append({"batch": b_, "M": M, "N": N, "K": K, "out": "fp32" if fp32 else "int8", "us": round(us, 2), "TOPs": round(2.0 * b_ * M * N * K / us / 1e6, 1)})
    # ... and the same operator at the larger OPT widths' prefill shapes (OPT-6.7B q / fc1 / fc2 at 512 and 2048 rows: the 128-row int8 tiles), weight
    # copies rotating through more than the memory-side cache (HBM-resident weights, as in the model)
    out["w8a8_opt6p7b_prefill"] = []
    for (M, N, K) in ((512, 4096, 4096), (512, 16384, 4096), (512, 4096, 16384), (2048, 4096, 4096), (2048, 16384, 4096), (2048, 4096, 16384)):
        a = torch.randint(-128, 128, (M, K), dtype=torch.int8, device=dev)
        ncopies = max(2, int(3.2e8 // (N * K)) + 1)  # (round 4: the copies together exceed the 256 MiB memory-side cache -- an OPT-6.7B layer's weights come from HBM; two copies, 134 MB, did not)
        bs = [torch.randint(-128, 128, (N, K), dtype=torch.int8, device=dev) for _ in range(ncopies)]
        bias = torch.randint(-128, 128, (N,), dtype=torch.int8, device=dev)
        o = torch.empty((M, N), dtype=torch.int8, device=dev)
        ds = [capi.W8A8Desc(M=M, N=N, K=K, batch=1, A=a.data_ptr(), B=b.data_ptr(), bias=bias.data_ptr(), C=o.data_ptr(), alpha=0.0005, beta=0.02,
                            q_min=-128, q_max=127, bias_kind=capi.TCE_BIAS_INT8, out_kind=capi.TCE_OUT_INT8) for b in bs]
        us = time_graph(lambda i, sp: capi.check(L.tce_w8a8_matmul(C.byref(ds[i % ncopies]), sp)), max(16, ncopies))
        out["w8a8_opt6p7b_prefill"].append({"M": M, "N": N, "K": K, "weight_copies": ncopies, "us": round(us, 2), "TOPs": round(2.0 * M * N * K / us / 1e6, 1), "frac_of_5000_TOPs": round(2.0 * M * N * K / us / 1e6 / 5000.0, 3)})
        del bs, ds
    torch.cuda.empty_cache()
    return out


# ----------------------------------------------------------------------------------------------------------------
def roofline_leg(dl, torch, launches: int, eager: bool = False, which: int = 2, quick: bool = False, knobs=None, groups=None):
    """The dominant kernel in isolation: the grouped gate+up GEMV launch (2*ffn rows x hidden), `launches` back-to-back
    launches on one stream, rotating over the layers' distinct weights (ring >> Infinity Cache), HIP events on that
    stream around the whole sequence.  achieved = algorithmic bytes per launch / average launch duration."""
    from tinychatengine_amd import capi
    st = torch.cuda.current_stream().cuda_stream
    if groups is None:
        groups = [dl.block_launches(li)[which] for li in range(dl.n_layers)]
    d0 = groups[0]
    formula_bytes = sum(capi.algorithmic_bytes(dl.m, d.N, d.K, d.group_size) for d in d0)
    # SURVEY 8d's formula counts the packed zero points (N*K/(2G) bytes); with TCE_W4_ZERO_POINT_IS_8 (what the reference quantizer
    # always writes) the kernel never reads them, so they do not belong in the numerator of ITS bandwidth
    zeros_bytes = sum(d.N * d.K // (2 * d.group_size) for d in d0 if d.flags & capi.TCE_W4_ZERO_POINT_IS_8)
    bytes_per_launch = formula_bytes - zeros_bytes
    arrs = [(capi.W4A16Desc * len(g))(*g) for g in groups]
    L = capi.lib()
    import ctypes as C
    stp = C.c_void_p(st)
    if knobs and any(knobs):  # the headline step is a TCE_PLAN_TUNED plan: the launch is measured the way that plan issues it (tce_plan_launch_geometry's encoding)
        rows, wn, wk, dcode = knobs
        if rows:
            capi.set_gemv_config(rows, wn, wk, dcode % 100)
        capi.check(L.tce_w4a16_set_debug_mode(41 if (dcode // 100) % 10 else 40))
        capi.check(L.tce_w4a16_set_debug_mode(10 + dcode // 1000))
    try:
        return _roofline_leg_body(dl, torch, launches, eager, quick, capi, L, C, st, stp, groups, d0, arrs, formula_bytes, bytes_per_launch, zeros_bytes, knobs)
    finally:
        if knobs and any(knobs):
            capi.set_gemv_config()
            L.tce_w4a16_set_debug_mode(40)
            L.tce_w4a16_set_debug_mode(10)


def _roofline_leg_body(dl, torch, launches, eager, quick, capi, L, C, st, stp, groups, d0, arrs, formula_bytes, bytes_per_launch, zeros_bytes, knobs):
    for i in range(min(32, launches)):
        capi.check(L.tce_w4a16_forward_group(arrs[i % len(arrs)], len(d0), stp))
    torch.cuda.synchronize()
    if eager:  # profiling runs: per-kernel durations come from rocprofv3, the event time below is host-bound
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(launches):
            capi.check(L.tce_w4a16_forward_group(arrs[i % len(arrs)], len(d0), stp))
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / launches
        return {"bound": "hbm", "achieved": round(bytes_per_launch / us / 1e3, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "avg_launch_us": round(us, 3), "timing": "eager launches (host-bound; use the rocprofv3 kernel durations)",
                "algorithmic_bytes_per_launch": bytes_per_launch}
    # captured into a graph so the host launch rate (~3-4 us per call) does not bound a ~8 us kernel
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        sp = C.c_void_p(s.cuda_stream)
        with torch.cuda.graph(g, stream=s):
            for i in range(launches):
                capi.check(L.tce_w4a16_forward_group(arrs[i % len(arrs)], len(d0), sp))
    for _ in range(8):  # burn-in, as in the other legs: the first replays after the device sat idle for the host-side set-up run up to 8 % slow
        g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 10
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / (reps * launches)
    gbs = bytes_per_launch / us / 1e3
    if quick:  # the per-shape table: rate only
        return {"launch": "+".join(str(d.N) for d in d0) + f" x {d0[0].K}", "us": round(us, 2), "GBs": round(gbs, 1), "frac_of_8TBs": round(gbs / HBM_PEAK_GBS, 3),
                "bytes": bytes_per_launch, "kernel": capi.describe_dispatch(d0[0])}
    # spread: the same graph replayed 15 more times, each replay timed on its own (median and p10 / p90)
    per = []
    for _ in range(15):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); g.replay(); b.record(); torch.cuda.synchronize()
        per.append(a.elapsed_time(b) * 1e3 / launches)
    per.sort()
    # a measured ceiling beside the 8 TB/s spec: plain 16-byte loads over 1 GiB of the same weights (tce_prefetch), nothing else
    ceiling = None
    try:
        span = torch.empty(1 << 30, dtype=torch.uint8, device=torch.device("cuda", torch.cuda.current_device()))
        for _ in range(2):
            capi.check(L.tce_prefetch(C.c_void_p(span.data_ptr()), span.numel(), 0, stp))
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(4):
            capi.check(L.tce_prefetch(C.c_void_p(span.data_ptr()), span.numel(), 0, stp))
        b.record(); torch.cuda.synchronize()
        ceiling = round(4 * span.numel() / (a.elapsed_time(b) * 1e-3) / 1e9, 1)
        del span
    except Exception:  # noqa: BLE001
        ceiling = None
    return {
        "bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
        **_pmc_traffic(bytes_per_launch),
        "kernel": f"{'w4a16_gemv_i8_kernel (int8 contraction on the packed copy)' if capi.describe_dispatch(d0[0]).startswith('gemv-i8') else 'w4a16_gemv_kernel (fp16 unpack on q4_6)'}"
                  f", grouped gate+up launch, N={'+'.join(str(d.N) for d in d0)}, K={d0[0].K}, M={dl.m}",
        "dispatch": capi.describe_dispatch(d0[0]),
        "algorithmic_bytes_per_launch": bytes_per_launch, "survey_8d_formula_bytes_per_launch": formula_bytes,
        "bytes_note": "formula of SURVEY 8d minus the packed zero points the zero-point-8 kernel never reads" if zeros_bytes else "formula of SURVEY 8d",
        "avg_launch_us": round(us, 3), "launches_timed": reps * launches,
        "launch_us_p10_p50_p90": [round(per[1], 3), round(per[len(per) // 2], 3), round(per[-2], 3)],
        "measured_streaming_read_GBs": ceiling, "frac_of_measured_streaming_read": (round(gbs / ceiling, 4) if ceiling else None),
        "timing": "HIP events on the launch stream around graph-replayed back-to-back launches rotating over all layers' weights (includes inter-kernel gaps)",
        **({"issued_as": f"the headline plan's choice for this launch (TCE_PLAN_TUNED): rows, waves_n, waves_k, depth code = {list(knobs)}"} if knobs and any(knobs) else {}),
    }


def launch_shape_table(dl, torch, launches: int = 128):
    """us / GB/s / fraction of 8 TB/s of every launch shape of the token.  The four per-block launches are timed
    like the roofline leg (rotating over the layers' weights).  lm_head is ONE tensor (65-260 MB) that a back-to-back loop would serve
    from the 256 MB Infinity Cache, so each lm_head launch is followed by three gate+up launches of rotating layers (>= 270 MB of other
    weights) and their separately measured time is subtracted."""
    from tinychatengine_amd import capi
    import ctypes as C
    rows = [roofline_leg(dl, torch, launches, which=w, quick=True) for w in range(4)]
    for r, nm in zip(rows, ("qkv (one launch)", "o_proj", "gate+up (one launch)", "down_proj")):
        r["name"] = nm
    # the ffn x hidden projection ALONE (the shape BASELINE.json spells as 4096x11008 read row-major: one of gate / up without its sibling)
    rows.append(dict(roofline_leg(dl, torch, launches, quick=True, groups=[dl.block_launches(li)[2][:1] for li in range(dl.n_layers)]), name="gate_proj alone"))
    L = capi.lib()
    gu = [dl.block_launches(li)[2] for li in range(dl.n_layers)]
    arrs = [(capi.W4A16Desc * len(g))(*g) for g in gu]
    d = dl.lm_head.desc(dl.x, dl.logits)
    lm = (capi.W4A16Desc * 1)(d)
    n = 24
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        sp = C.c_void_p(s.cuda_stream)
        with torch.cuda.graph(g, stream=s):
            for i in range(n):
                capi.check(L.tce_w4a16_forward_group(lm, 1, sp))
                for j in range(3):
                    capi.check(L.tce_w4a16_forward_group(arrs[(3 * i + j) % len(arrs)], len(gu[0]), sp))
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / (5 * n) - 3 * rows[2]["us"]
    b = capi.algorithmic_bytes(dl.m, d.N, d.K, d.group_size) - (d.N * d.K // (2 * d.group_size) if d.flags & capi.TCE_W4_ZERO_POINT_IS_8 else 0)
    rows.append({"name": "lm_head", "launch": f"{d.N} x {d.K} (lm_head)", "kernel": capi.describe_dispatch(d), "us": round(us, 2), "GBs": round(b / us / 1e3, 1), "frac_of_8TBs": round(b / us / 1e3 / HBM_PEAK_GBS, 3),
                 "bytes": b, "timing": "interleaved with 3 gate+up launches (cache flush), their time subtracted"})
    return rows


def random_zero_points_leg(dl, torch, layers: int = 8, launches: int = 128):
    """The dominant launch with REAL (random) zero points: the same gate+up weights, the zero-point words replaced and re-packed, so the kernel reads them and runs
    its general-zero-point form (one more MFMA pair per unit for (8 - z) * sum x, csrc/w4a16_gemv_i8.hip; reference: gemv_cuda.cu:159-166 reads them too).
    Timed exactly like roofline.shapes' rows (a graph of back-to-back launches rotating over `layers` weight sets: 8 x 61 MB > the 256 MB cache)."""
    from tinychatengine_amd.linear import Linear_half_int4
    groups, keep = [], []
    g = torch.Generator(device=dl.device).manual_seed(77)
    for li in range(min(layers, dl.n_layers)):
        b = dl.blocks[li]
        pair = []
        for lin, out in ((b["gate"], dl.out_gate), (b["up"], dl.out_up)):
            z = torch.randint(-(1 << 31), (1 << 31) - 1, lin.zero_point.shape, dtype=torch.int64, device=dl.device, generator=g).to(torch.int32)
            l2 = Linear_half_int4(lin.weight, lin.scale, z, lin.group_size).prepack()
            assert not l2.zeros_are_8
            keep.append(l2)
            pair.append(l2.desc(dl.h2, out))
        groups.append(pair)
    torch.cuda.synchronize()
    r = roofline_leg(dl, torch, launches, quick=True, groups=groups)
    same = roofline_leg(dl, torch, launches, quick=True, groups=[dl.block_launches(li)[2] for li in range(len(groups))])
    zb = sum(d.N * d.K // (2 * d.group_size) for d in groups[0])
    return {"launch": r["launch"], "us": r["us"], "bytes_with_zero_points": r["bytes"], "GBs": r["GBs"], "frac_of_8TBs": r["frac_of_8TBs"], "kernel": r["kernel"],
            "us_zero_point_8": same["us"], "frac_zero_point_8": same["frac_of_8TBs"], "zero_point_bytes": zb, "weight_sets": len(groups)}


def shapes_only_leg(dl, torch, dev, shape, eager: bool):
    """Every launch shape of the token and the attention step on their own, for rocprofv3 (scripts/profile_r3.sh): graph-replayed exactly
    like `other_configs.decode_launch_shapes` of the bench line, or (eager) as plain launches for the PMC passes, which serialise kernels."""
    import ctypes as C
    import numpy as np
    from tinychatengine_amd import capi
    from tinychatengine_amd.attention_ops import DecodeAttention
    L = capi.lib()
    out = {"mode": "eager launches" if eager else "hipGraph replays (the bench line's method)"}
    if eager:
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rows = []
        for w in range(4):
            groups = [dl.block_launches(li)[w] for li in range(dl.n_layers)]
            arrs = [(capi.W4A16Desc * len(g))(*g) for g in groups]
            for i in range(96):
                capi.check(L.tce_w4a16_forward_group(arrs[i % len(arrs)], len(groups[0]), st))
            torch.cuda.synchronize()
            rows.append({"launch": "+".join(str(d.N) for d in groups[0]) + f" x {groups[0][0].K}", "eager_launches": 96})
        lm = (capi.W4A16Desc * 1)(dl.lm_head.desc(dl.x, dl.logits))
        gu = [dl.block_launches(li)[2] for li in range(dl.n_layers)]
        ga = [(capi.W4A16Desc * len(g))(*g) for g in gu]
        for i in range(12):
            capi.check(L.tce_w4a16_forward_group(lm, 1, st))
            for j in range(3):  # > 256 MB of other weights between two lm_head launches
                capi.check(L.tce_w4a16_forward_group(ga[(3 * i + j) % len(ga)], len(gu[0]), st))
        torch.cuda.synchronize()
        rows.append({"launch": f"{dl.lm_head.out_features} x {dl.lm_head.in_features} (lm_head)", "eager_launches": 12})
        out["linears"] = rows
    else:
        out["linears"] = launch_shape_table(dl, torch)
    # the attention step: multi-head (the baseline-named model) and 32 query heads over 8 key / value heads (Llama-3-8B), caches rotating through > 256 MB
    heads = shape.hidden // 128
    att_rows = []
    for (h, kvh) in ((heads, heads), (heads, max(1, heads // 4))):
        for ctx in (512, 2048):
            bytes_ = 2 * kvh * ctx * 128 * 2
            nsets = min(96, max(4, int(3.2e8 // bytes_) + 1))
            cos = torch.randn(ctx + 1, 128, device=dev).half()
            sin = torch.randn(ctx + 1, 128, device=dev).half()
            atts = [DecodeAttention(h, 128, ctx, dev, cos, sin, kv_heads=kvh) for _ in range(nsets)]
            for a_ in atts:
                a_.k_cache.normal_(0, 0.8)
                a_.v_cache.normal_(0, 0.8)
            qkv = torch.randn((h + 2 * kvh) * 128, device=dev).half()
            oo = torch.empty(h, 128, dtype=torch.float16, device=dev)
            n = max(32, nsets)

            def step(i):
                atts[i % nsets].step(qkv, ctx - 1, out=oo)
            if eager:
                for i in range(n):
                    step(i)
                torch.cuda.synchronize()
                us = None
            else:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    for i in range(n):
                        step(i)
                g.replay()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(3):
                    g.replay()
                e1.record()
                torch.cuda.synchronize()
                us = round(e0.elapsed_time(e1) * 1e3 / (3 * n), 2)
                del g
            att_rows.append({"launch": f"attention step {h} query / {kvh} kv heads, {ctx} keys", "us": us, "kv_cache_bytes": bytes_, "launches": n,
                             "GBs": None if us is None else round(bytes_ / us / 1e3, 1), "cut": capi.describe_attention_step(h, ctx, kvh)})
            del atts
    out["attention_step"] = att_rows
    return out


def opt_layer_leg(torch, dev, size="125M"):
    """BASELINE config 4 as a WORKLOAD, not four shapes: whole SmoothQuant OPT decoder stacks (llm/include/model.h: OPT-125M -- embed 768,
    12 heads, ffn 3072, 12 layers; OPT-1.3B -- 2048, 32, 8192, 24; OPT-6.7B -- 4096, 32, 16384, 32) on this library's launches (tinychatengine_amd/opt_layer.py;
    Int8OPTDecoderLayer.cc:24-59, Int8OPTAttention.cc:183-284): one decode token over a 512-key cache (5 launches per layer) and -- at 125M -- a 512-row
    prefill (12 launches per layer), every layer with its own weights, the stack captured in one hipGraph.  At 1.3B / 6.7B a layer's int8 weights are 50 / 201 MB
    (the stack far beyond the memory-side cache): `weight_stream_GBps` is the figure a roofline prices."""
    from tinychatengine_amd.opt_layer import Int8OPTDecoderLayer
    E, H, F, NL = {"125M": (768, 12, 3072, 12), "1.3B": (2048, 32, 8192, 24), "6.7B": (4096, 32, 16384, 32)}[size]
    out = {"model": f"OPT-{size} (embed {E}, {H} heads, ffn {F}, {NL} layers)", "weights": "synthetic int8"}
    for name, m, pos in (("decode_512_keys", 1, 511), ("prefill_512_rows", 512, 0)) if size == "125M" else (("decode_512_keys", 1, 511),):
        tgz = pos + m
        layers = [Int8OPTDecoderLayer(E, H, F, 512, m, dev, seed=7 + i) for i in range(NL)]
        hid = torch.randn(m, E, device=dev)
        hid0 = hid.clone()
        mask = torch.zeros((m, tgz), device=dev)
        if m > 1:
            mask.masked_fill_(torch.triu(torch.ones(m, tgz, dtype=torch.bool, device=dev), diagonal=pos + 1), torch.finfo(torch.float32).min)

        def token():
            hid.copy_(hid0)
            for l in layers:
                l.step(hid, pos, mask)
        token()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            token()
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 20
        a.record()
        for _ in range(reps):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1e3 / reps
        ops = layers[0].int8_ops(m, tgz)
        wbytes = 4 * E * E + 2 * E * F + 2 * H * tgz * (E // H)  # a layer's int8 weights + the cache rows a decode token reads
        out[name] = {"rows": m, "keys": tgz, "us_per_layer": round(us / NL, 2), "launches_per_layer": layers[0].launches(m), f"us_per_{NL}_layers": round(us, 1),
                     "int8_TOPs": round(ops * NL / us / 1e6, 2), "finite": bool(torch.isfinite(hid).all().item()),
                     **({f"tokens_per_s_{NL}_layers": round(1e6 / us, 1), "weight_MB_per_layer": round(wbytes / 1e6, 2), "weight_stream_GBps": round(wbytes * NL / us / 1e3, 1),
                         "frac_of_8TBps": round(wbytes * NL / us / 1e3 / 8000, 3)} if m == 1 else {f"prefill_tokens_per_s_{NL}_layers": round(m * 1e6 / us, 1)})}
        del g, layers
    torch.cuda.empty_cache()
    return out


def projected_scaling_leg(torch, dev, G, prepack=True):
    """"if only one GPU is visible, report P > 1 as not measurable here plus the measured per-shard kernel times at N/P shapes".
    This GPU plays rank 0 of P = 2, 4, 8: all of one token's linears at N/P rows (tce_w4a16_shard's row ranges; weights 1/P of the model, still
    more than the memory-side cache for the 7B-class sets at P <= 8) as one stream-ordered hipGraph -- the compute side of a sharded token,
    MEASURED.  The exchange side is NOT measurable on one GPU: the projection adds gathers x an ASSUMED cost per gather (stated) and is
    labelled as a projection; nothing here is a scaling measurement."""
    from tinychatengine_amd.decode import SHAPES, DecodeLinears
    st = torch.cuda.current_stream().cuda_stream
    assumed = {"peer_write_gather_us": 3.0, "rccl_gather_us": 12.0}
    out = {"label": "PROJECTION from one GPU: per-rank shard compute is measured, the gather cost is assumed",
           "assumed_gather_cost_us": dict(assumed, source="MI355X_MICROARCH.md price list, allgather row (8-32 KB all-to-all inside one device: 2.4-4.2 us; an xGMI hop is not in it); "
                                                          "RCCL: order of 10 us per small collective"),
           "models": {}}
    for key in ("baseline-named", "llama3-8b", "llama2-13b"):
        shape = SHAPES[key]
        rows = {}
        for P in (1, 2, 4, 8):
            try:
                dlp = DecodeLinears(shape, device=dev, group_size=G, rank=0, world=P, m=1, prepack=prepack)
                plan = dlp.make_plan()
                for _ in range(5):
                    plan.launch(st)
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(30):
                    plan.launch(st)
                b.record()
                torch.cuda.synchronize()
                ms = a.elapsed_time(b) / 30
                n1, n4 = shape.layers + 1, shape.layers * (3 + len(shape.qkv)) + 1  # exchanges per token: 1 per block + logits; qkv slices, o, gate, up, down per block + logits
                row = {"shard_compute_ms_per_token": round(ms, 4), "shard_weight_bytes": dlp.token_bytes(), "launches": plan.n_launches}
                if P > 1:
                    # the one-gather-per-block form: a rank's linears of a block are ONE launch (round 6, tce_w4a16_forward_independent) -- MEASURED here like the four-launch form
                    plan1 = dlp.make_plan(one_launch_per_block=True)
                    for _ in range(5):
                        plan1.launch(st)
                    torch.cuda.synchronize()
                    a.record()
                    for _ in range(30):
                        plan1.launch(st)
                    b.record()
                    torch.cuda.synchronize()
                    ms1 = a.elapsed_time(b) / 30
                    row["shard_compute_ms_per_token_one_launch_per_block"] = round(ms1, 4)
                    row["launches_one_launch_per_block"] = plan1.n_launches
                    del plan1
                    for gname, gus in assumed.items():
                        row[f"projected_tokens_per_s_1_gather_per_block_{gname[:-10]}"] = round(1e3 / (min(ms, ms1) + n1 * gus * 1e-3), 1)
                        row[f"projected_tokens_per_s_4_gathers_per_block_{gname[:-10]}"] = round(1e3 / (ms + n4 * gus * 1e-3), 1)
                else:
                    row["tokens_per_s"] = round(1e3 / ms, 1)
                rows[f"P={P}"] = row
                del plan, dlp
                torch.cuda.empty_cache()
            except Exception as e:  # noqa: BLE001
                rows[f"P={P}"] = {"error": f"{type(e).__name__}: {e}"}
        out["models"][shape.name] = rows
    return out


def whole_token_leg(torch, dev, shape, dl):
    """One decode token through 32 complete decoder layers on this library's calls (tinychatengine_amd/decoder_block.py): per layer
    [RMSNorm + q/k/v] [RoPE + KV append + attention, one launch] [o_proj + residual] [RMSNorm + gate/up + SiLU*mul] [down_proj + residual],
    then lm_head -- 161 launches where the reference issues ~650 -- captured in one graph per context length.  Synthetic weights and
    caches; the KV caches (2 x 32 x ctx x 128 halves per layer) are distinct per layer, so they stream from HBM like the weights."""
    import numpy as np
    from tinychatengine_amd import capi
    from tinychatengine_amd.decoder_block import DecoderBlock
    heads, hd, ctx_max = shape.hidden // 128, 128, 2048
    kv_heads = shape.qkv[1] // 128 if len(shape.qkv) == 3 else heads  # separate q / k / v widths: grouped-query attention (Llama-3-8B: 32 / 8, model.h:83)
    ang = np.random.default_rng(0).uniform(0, 2 * np.pi, (ctx_max, hd // 2))
    cos = torch.from_numpy(np.concatenate([np.cos(ang), np.cos(ang)], axis=1).astype(np.float16)).to(dev)
    sin = torch.from_numpy(np.concatenate([np.sin(ang), np.sin(ang)], axis=1).astype(np.float16)).to(dev)
    blocks = [DecoderBlock(shape.hidden, heads, shape.ffn, ctx_max, dev, cos, sin, seed=100 + i, kv_heads=kv_heads) for i in range(shape.layers)]
    for b in blocks:
        b.attention.k_cache.normal_(0, 0.8)
        b.attention.v_cache.normal_(0, 0.8)
    hid = torch.randn(1, shape.hidden, device=dev).to(torch.float16)
    hid0 = hid.clone()
    out = {"launches_per_token": shape.layers * DecoderBlock.LAUNCHES + 1, "layers": shape.layers, "query_heads": heads, "kv_heads": kv_heads,
           "note": "the position lives in a device word (tce_attention_decode_step_pos_f16): the captured token is replayable for growing contexts; timed at a fixed context"}
    pos_t = torch.zeros(1, dtype=torch.int32, device=dev)
    # round 4: the norms on the PRODUCER side (tce_w4a16_forward_residual_rmsnorm): q/k/v and gate/up are plain launches on rows the previous launch's residual
    # epilogue normalised; one tce_rmsnorm_half in front of the first layer, the final norm (gamma = 1) in front of lm_head from the last down_proj
    from tinychatengine_amd.linear import rmsnorm_half
    # (measured SLOWER, profiles/r4: 1.65 against 1.41 ms per token -- every producer launch pays the write-through acknowledgements and the last workgroup's serial pass,
    # +3.8 us each; kept behind TCE_BENCH_WHOLE_TOKEN_CHAINED=1 for the record.  The default token carries the norms as fused prologues of q/k/v and gate/up.)
    chained = all(b.qkv.packed is not None for b in blocks) and os.environ.get("TCE_BENCH_WHOLE_TOKEN_CHAINED", "") == "1"
    ws = torch.zeros(int(capi.lib().tce_w4a16_residual_rmsnorm_workspace_bytes()), dtype=torch.uint8, device=dev)
    xn = [torch.empty_like(hid), torch.empty_like(hid)]
    final_gamma = torch.ones(shape.hidden, device=dev)
    out["norms"] = ("on the producer side: o_proj / down_proj + residual + the next RMSNorm as one launch (tce_w4a16_forward_residual_rmsnorm), q/k/v and gate/up plain; "
                    "+ 1 tce_rmsnorm_half per token") if chained else "fused prologues in the q/k/v and gate/up launches"
    if chained:
        out["launches_per_token"] += 1
    for ctx in (512, 2048):
        pos = ctx - 1
        pos_t.fill_(pos)
        def token():
            hid.copy_(hid0)
            if not chained:
                for b in blocks:
                    b.step(hid, pos, pos_device=pos_t)
                capi.check(capi.w4a16_forward(dl.lm_head.desc(hid, dl.logits), torch.cuda.current_stream().cuda_stream))
                return
            rmsnorm_half(hid, blocks[0].gamma1, blocks[0].eps, out=xn[0])
            for i, b in enumerate(blocks):
                b.step_chained(hid, xn[i % 2], pos, blocks[i + 1].gamma1 if i + 1 < len(blocks) else final_gamma, xn[(i + 1) % 2], ws, pos_device=pos_t)
            capi.check(capi.w4a16_forward(dl.lm_head.desc(xn[len(blocks) % 2], dl.logits), torch.cuda.current_stream().cuda_stream))
        token()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            token()
        for _ in range(5):
            g.replay()
        torch.cuda.synchronize()
        a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(50):
            g.replay()
        b_.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b_) / 50
        kv = 2 * kv_heads * ctx * hd * 2 * shape.layers
        wb = sum(b.linear_bytes() for b in blocks)
        out[f"context_{ctx}"] = {"tokens_per_s": round(1e3 / ms, 1), "ms_per_token": round(ms, 4), "kv_cache_bytes_read": kv,
                                 "frac_of_8TBs": round((wb + kv) / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                 "finite": bool(torch.isfinite(hid.float()).all().item())}
        del g
    # the same layers for a PROMPT: m rows at once through DecoderBlock.prefill (RMSNorm, the MFMA GEMMs on pre-packed weights, the prefill attention:
    # 10 launches per layer), positions 0 .. m - 1; eager launches (a 512-row layer is ~0.3 ms of kernels)
    try:
        for b in blocks:
            b.prepare_prefill()
        pre = {"launches_per_layer": DecoderBlock.PREFILL_LAUNCHES}
        for m in (512, 2048):
            rows0 = torch.randn(m, shape.hidden, device=dev).to(torch.float16)
            rows = rows0.clone()

            def prompt():
                rows.copy_(rows0)
                for b in blocks:
                    b.prefill(rows, 0)
            prompt()
            torch.cuda.synchronize()
            a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            reps = 3
            a.record()
            for _ in range(reps):
                prompt()
            b_.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b_) / reps
            lin_flops = 2.0 * m * sum(l.out_features * l.in_features for b in blocks[:1] for l in (b.qkv, b.o, b.gate, b.up, b.down)) * shape.layers
            att_flops = 4.0 * heads * hd * (m * (m + 1) / 2) * shape.layers
            pre[f"prompt_{m}_rows"] = {"ms": round(ms, 3), "prompt_tokens_per_s": round(m * 1e3 / ms, 0), "ms_per_layer": round(ms / shape.layers, 4),
                                       "TFLOPs_linears_plus_causal_attention": round((lin_flops + att_flops) / (ms * 1e-3) / 1e12, 1),
                                       "finite": bool(torch.isfinite(rows.float()).all().item())}
            del rows, rows0
        out["prefill"] = pre
    except Exception as e:  # noqa: BLE001
        out["prefill"] = {"error": f"{type(e).__name__}: {e}"}
    del blocks
    torch.cuda.empty_cache()
    return out


def adapter_path_leg(workload: str, keys: int = 512):
    """The DROP-IN path on the clock: tinychatengine_amd/lib/adapter_bench (adapter/adapter_bench.cc, plain C++) issues whole decode tokens the way
    the reference's host does -- matmul::MatmulOperator::gemv_forward_cuda per linear through libtce_matmul_operator.so, null stream, eager, the reference's glue order
    (Int4llamaDecoderLayer.cu:73-115) -- 200 tokens after 20, wall-clock + HIP events + host time per call; beside it the same launch list through the C ABI directly
    (eager, and captured into one hipGraph).  Runs as its own process while this one is idle."""
    import subprocess
    exe = os.path.join(REPO, "tinychatengine_amd", "lib", "adapter_bench")
    model = {"llama3-8b": "llama3-8b", "baseline-named": "llama2-7b", "tiny": "tiny"}.get(workload)
    if model is None or not os.path.exists(exe):
        return {"error": f"no adapter_bench for workload {workload}" if model is None else f"{exe} not built (python -m tinychatengine_amd.build)"}
    r = subprocess.run([exe, "--model", model, "--tokens", "200", "--warmup", "20", "--keys", str(keys)], capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    if r.returncode != 0 or not lines:
        return {"error": f"adapter_bench rc {r.returncode}: {(r.stdout + r.stderr)[-300:]}"}
    d = json.loads(lines[-1])
    d["how"] = ("adapter/adapter_bench.cc: MatmulOperator::gemv_forward_cuda per linear (fused qkv, o, gate, up, down, lm_head), null stream, eager; glue = tce_rmsnorm_half / tce_add_half / "
                "tce_silu_mul_half + one attention-step launch; 11 launches per block; capi_* = the same launch list through the C ABI without the adapter")
    return d


def _pmc_traffic(bytes_per_launch):
    """HBM bytes per launch of the dominant kernel from the rocprofv3 --pmc FETCH_SIZE pass of this same roofline command
    (scripts/profile_r4.sh; corrected as the MI355X guide prescribes: KiB x 1024 x 2 on gfx950).  The counters cannot be
    collected from inside the timed process, so the figure comes from a committed profiles/*/traffic.json -- and is reported ONLY if
    that pass ran on this launch (same algorithmic bytes) of THIS kernel: the file carries the sha256 of the kernel's sources, and a
    source that has changed since (a change that could add traffic) makes the figure null until the profile script is re-run."""
    import glob
    import hashlib
    here = os.path.dirname(os.path.abspath(__file__))
    best = None
    for f in sorted(glob.glob(os.path.join(here, "profiles", "*", "traffic.json"))):
        try:
            t = json.load(open(f))
            if t.get("algorithmic_bytes_per_launch") != bytes_per_launch or not t.get("kernel_sources"):
                continue
            sha = hashlib.sha256(b"".join(open(os.path.join(here, "tinychatengine_amd", "csrc", s), "rb").read() for s in t["kernel_sources"])).hexdigest()
            if sha == t.get("kernel_sources_sha256"):
                best = (t, f)
        except Exception:  # noqa: BLE001
            continue
    if not best:
        return {"traffic": None, "traffic_source": "no committed rocprofv3 FETCH_SIZE pass matches this launch AND the current kernel sources (scripts/profile_r4.sh writes one)"}
    t, f = best
    return {"traffic": t["hbm_read_bytes_per_launch"],
            "traffic_source": f"rocprofv3 --pmc FETCH_SIZE (x1024x2), median of {t['dispatches']} dispatches of {t['kernel'][:60]}, {os.path.relpath(f, here)} (kernel sources unchanged since: sha256 match)"}


def cpu_baseline_worker(args):
    """Child process: time ONE flavour of the reference's CPU path (built from /root/reference into oracle/_ref) on a
    bounded sample -- one transformer block's linears + lm_head at full size -- and print one JSON line.  Runs in
    its own process because the reference's AVX path keeps a static thread pool sized by its first call
    (kernels/avx/matmul_avx_int8_int4.cc:340) and so that a crash in reference code cannot take the GPU number down."""
    import numpy as np
    from oracle import oracle as O
    from tinychatengine_amd.decode import SHAPES
    shape = SHAPES[args.workload]
    kind, threads = args.cpu_worker, args.threads
    if kind == "parity":
        return parity_worker(args)
    h, f = shape.hidden, shape.ffn
    block = [(n, h) for n in shape.qkv] + [(h, h), (f, h), (f, h), (h, f)]
    head = (shape.vocab, h)
    rng = np.random.default_rng(4321)
    t_block, t_head = 0.0, 0.0
    for (n, k) in block + [head]:
        codes = rng.integers(0, 16, (n, k), dtype=np.uint8)  # timing does not depend on the code values
        a = rng.standard_normal((1, k)).astype(np.float16).astype(np.float32)
        if kind in ("avx", "avx_cold"):
            d = (rng.random((n, k // 32), dtype=np.float32) * 0.01 + 0.001)
            packed = O.ReferenceAVX.pack_q4_3(codes)
            ref_avx = O.ReferenceAVX(num_thread=threads)
            if kind == "avx":  # ten repetitions on ONE copy: a linear's 8-30 MB of W4A8 weights stay in this host's L3
                call = ref_avx.make_timed_call(a, packed, d, 1, n, k)
            else:  # (round 6) the weights from DRAM, as the GPU leg's come from HBM: copies in rotation, > 768 MB between two uses of one
                ncopy = max(2, min(32, int(768e6 // packed.nbytes) + 1))
                calls = [ref_avx.make_timed_call(a, packed.copy(), d.copy(), 1, n, k) for _ in range(ncopy)]
                it = [0]

                def call(calls=calls, it=it):
                    calls[it[0] % len(calls)]()
                    it[0] += 1
            warm, reps = 3, 10
        else:
            ref = O.Reference()
            seq = (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)
            s32 = (rng.random((n, k // 128), dtype=np.float32) * 0.01 + 0.001)
            call = lambda: ref.naive_mat_mul_int4(a, seq, s32, 8.0, 1, n, k, 128)
            warm, reps = 1, 1
        for _ in range(warm):
            call()
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        dt = (time.perf_counter() - t0) / reps
        if (n, k) == head:
            t_head = dt
        else:
            t_block += dt
    print(json.dumps({"tokens_per_s": 1.0 / (t_block * shape.layers + t_head), "block_ms": t_block * 1e3, "lm_head_ms": t_head * 1e3}))


def parity_worker(args):
    """Child process (the CHECKER, not the thing measured): the outputs the GPU produced for full-size linears of the headline workload (written to a scratch directory by
    parity_leg) against the oracle's restatement of the reference arithmetic -- per linear the worst error over the tests' tolerance 1e-3 * max(|ref|, rms / 64), the share of
    outputs that pass only through the rms / 64 floor, and what a floor of rms / 256 would fail."""
    import numpy as np
    from oracle.oracle import Oracle
    orc = Oracle()
    rows = []
    for name in sorted(os.listdir(args.parity_dir)):
        if not name.endswith(".npz"):
            continue
        z = np.load(os.path.join(args.parity_dir, name))
        n, k = int(z["n"]), int(z["k"])
        ref = orc.w4a16_gemv_q4_6_mt(z["x"], z["qweight"].view(np.uint32), z["scales"], z["zeros"].view(np.uint32), 1, n, k, 128).astype(np.float64).ravel()
        got = z["y"].astype(np.float64).ravel()
        rms = float(np.sqrt(np.mean(ref * ref)))
        err = np.abs(got - ref)
        tol64, tol256 = 1e-3 * np.maximum(np.abs(ref), rms / 64.0), 1e-3 * np.maximum(np.abs(ref), rms / 256.0)
        rows.append({"linear": name[:-4], "N": n, "K": k, "worst_err_over_tol": round(float((err / tol64).max()), 3),
                     "share_passing_only_through_the_floor": round(float((err > 1e-3 * np.abs(ref)).mean()), 6),
                     "share_failing_with_floor_rms_over_256": round(float((err > tol256).mean()), 6),
                     "worst_err_over_tol_with_floor_rms_over_256": round(float((err / tol256).max()), 3),
                     "err_rms_over_ref_rms": float(f"{np.sqrt(np.mean(err * err)) / rms:.3e}")})
    print(json.dumps({"rows": rows}))


def parity_leg(dl, torch, workload: str):
    """Tolerance evidence in the driver's own record: block 0's linears and lm_head of the headline workload, FULL size, M = 1 -- computed by the
    product path here, checked by the oracle in a child process (the cpu_baseline leg's checker; nothing of oracle/ is imported into this process)."""
    import shutil
    import subprocess
    import tempfile
    import numpy as np
    d = tempfile.mkdtemp(prefix="tce_parity_")
    try:
        b = dl.blocks[0]
        gx = torch.Generator(device=dl.device).manual_seed(777)
        named = [(f"{i}_{nm}", l) for i, (nm, l) in enumerate([*[(f"qkv{j}", l) for j, l in enumerate(b["qkv"])], ("o", b["o"]), ("gate", b["gate"]), ("up", b["up"]), ("down", b["down"]),
                                                              ("lm_head", dl.lm_head)])]
        for nm, l in named:
            x = torch.empty((1, l.in_features), dtype=torch.float32, device=dl.device).normal_(0, 1, generator=gx).to(torch.float16)
            y = l.forward(x)
            torch.cuda.synchronize()
            np.savez(os.path.join(d, nm + ".npz"), n=l.out_features, k=l.in_features, x=x.cpu().numpy(), y=y.cpu().numpy(), qweight=l.weight.cpu().numpy(),
                     scales=l.scale.cpu().numpy(), zeros=l.zero_point.cpu().numpy())
        cmd = [sys.executable, os.path.abspath(__file__), "--cpu-worker", "parity", "--parity-dir", d, "--workload", workload]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
        if r.returncode != 0:
            return {"error": f"exit {r.returncode}: {r.stderr.strip()[-300:]}"}
        rows = json.loads(r.stdout.strip().splitlines()[-1])["rows"]
        return {"tolerance": "|gpu - oracle| <= 1e-3 * max(|oracle|, rms(oracle) / 64) per output (tests/conftest.py w4a16_close); every output of every listed linear checked",
                "worst_err_over_tol": max(x["worst_err_over_tol"] for x in rows), "max_share_passing_only_through_the_floor": max(x["share_passing_only_through_the_floor"] for x in rows),
                "max_share_failing_with_floor_rms_over_256": max(x["share_failing_with_floor_rms_over_256"] for x in rows), "rows": rows}
    except Exception as e:  # noqa: BLE001 -- evidence, never the reason a bench line is missing
        return {"error": f"{type(e).__name__}: {e}"}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def cpu_baseline_leg(workload: str, shape):
    """The reference's CPU path on this host (rank 0, N=1 only).  (i) kernels/avx W4A8 fast path -- what the reference
    runs on x86 (group 32; NOT the same arithmetic as the GPU W4A16 path) at 8 threads (the reference's default
    opt_params.num_thread, kernels/matmul.h:75) and at min(nproc, 64); (ii) kernels/ref-class naive_mat_mul_int4
    (the parity oracle's source; group 128; single-threaded code)."""
    import subprocess
    from oracle import oracle as O
    ncpu = os.cpu_count() or 1
    try:
        with open("/proc/cpuinfo") as fh:
            model = next((l.split(":", 1)[1].strip() for l in fh if l.startswith("model name")), "unknown")
    except OSError:
        model = "unknown"

    def run(kind, threads):
        cmd = [sys.executable, os.path.abspath(__file__), "--cpu-worker", kind, "--threads", str(threads), "--workload", workload]
        env = dict(os.environ, HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env)
        if r.returncode != 0:
            return {"error": f"exit {r.returncode}: {r.stderr.strip()[-200:]}"}
        return json.loads(r.stdout.strip().splitlines()[-1])

    res = {"cpu_model": model, "nproc": ncpu}
    sample = f"one transformer block's linears + lm_head at full size (M=1), scaled x{shape.layers} blocks"
    if O.have_ref_avx():
        best = None
        for th in sorted({8, min(ncpu, 64)}):
            r = run("avx", th)
            res[f"avx_{th}t"] = r
            if "tokens_per_s" in r and (best is None or r["tokens_per_s"] > best[1]):
                best = (th, r["tokens_per_s"])
        if best:
            cold = run("avx_cold", best[0])
            res[f"avx_cold_{best[0]}t"] = cold
            res["avx"] = {"value": round(best[1], 3), "unit": "tokens/s", "cores": best[0], "kind": "reference",
                          "sample": f"kernels/avx mat_mul_accelerator_int8_int4_fast_no_offset (W4A8, group 32, {best[0]} threads; best of 8 / {min(ncpu, 64)} threads), {sample}, 10 reps each ON ONE COPY of a linear's weights (8-30 MB: resident in this host's L3)",
                          **({"value_weights_from_dram": round(cold["tokens_per_s"], 3), "weights_from_dram": "the same call over copies in rotation (> 768 MB between two uses of a copy), as the GPU leg's weights come from HBM"} if "tokens_per_s" in cold else {})}
    if O.have_ref():
        r = run("ref", 1)
        res["ref_1t"] = r
        if "tokens_per_s" in r:
            res["ref"] = {"value": round(r["tokens_per_s"], 4), "unit": "tokens/s", "cores": 1, "kind": "reference",
                          "sample": f"kernels/matmul_int4.cc naive_mat_mul_int4 (generic branch, group 128, single-threaded code), {sample}"}
    return res


# ----------------------------------------------------------------------------------------------------------------
def dump_outputs(dl, dirname: str, rank: int = 0) -> None:
    """What the timed step computed, as its last replay left it: the output buffer of every linear (the last block's, the buffers are reused block
    after block) and the logits, as float32 .npy files (~0.7 MB for the default workload).  N > 1: rank 0's slices, plus the joined rows when the
    run gathers them."""
    import numpy as np
    import torch
    if rank != 0:
        return
    torch.cuda.synchronize()
    os.makedirs(dirname, exist_ok=True)
    bufs = {f"out_qkv{i}": t for i, t in enumerate(dl.out_qkv)}
    bufs.update(out_o=dl.out_o, out_gate=dl.out_gate, out_up=dl.out_up, out_down=dl.out_down, logits=dl.logits)
    if dl.world > 1 and hasattr(dl, "g_logits"):
        bufs.update({f"gathered_qkv{i}": t for i, t in enumerate(dl.g_qkv)})
        bufs.update(gathered_o=dl.g_o, gathered_gate=dl.g_gate, gathered_up=dl.g_up, gathered_down=dl.g_down, gathered_logits=dl.g_logits)
    for name, t in bufs.items():
        np.save(os.path.join(dirname, name + ".npy"), t.detach().float().cpu().numpy())


def main():
    args = parse_args()
    if args.cpu_worker:
        return cpu_baseline_worker(args)
    import faulthandler
    faulthandler.enable()
    import torch
    from tinychatengine_amd import capi
    from tinychatengine_amd.decode import SHAPES, DecodeLinears

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the N ranks ourselves (one process per GPU, rendezvous on 127.0.0.1) as a child job and exit
        # with its status -- rank 0's JSON line is this command's last line of stdout, exactly as under `python -m torch.distributed.run ... bench.py --gpus N`
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1", "--master-port", str(port),
               os.path.abspath(__file__), *sys.argv[1:]]
        print(f"[bench] --gpus {args.gpus} without WORLD_SIZE: starting the ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
        import subprocess
        sys.exit(subprocess.call(cmd))
    if args.selftest_emit:
        return selftest_emit(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the launcher started {world} ranks (WORLD_SIZE={world})")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    capi.lib()
    if os.environ.get("TCE_BENCH_SINGLE_DEVICE") == "1":  # debugging: every rank on GPU 0 (only meaningful with --backend gloo)
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1 or args.force_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)

    shape = SHAPES[args.workload]
    G = 128
    if args.force_dist:
        os.environ["TCE_FORCE_GATHER_BUFFERS"] = "1"
    prepack = not args.no_prepack  # load-time re-layout of every linear (tce_w4a16_prepack): the decode launches then run on the packed copies (csrc/w4a16_gemv_i8.hip)
    dl = DecodeLinears(shape, device=dev, group_size=G, rank=rank, world=world, m=1, layers=args.layers,
                       dataflow=(world == 1 and not args.ungrouped and shape.qkv[0] >= shape.hidden), prepack=prepack)
    want_peer = args.gather in ("all", "peer")
    peer_state = "not requested (--gather rccl)" if not want_peer else "single GPU"
    ranks_info = None
    if dist is not None:
        # who runs where: one row per rank -- device index, PCI address, name -- so that a scaling record shows N distinct devices
        try:
            pr = torch.cuda.get_device_properties(dev)
            mine = {"rank": rank, "device": dev.index, "pci_bus_id": "%04x:%02x:%02x" % (getattr(pr, "pci_domain_id", 0), getattr(pr, "pci_bus_id", 0), getattr(pr, "pci_device_id", 0)),
                    "name": pr.name}
        except Exception as e:  # noqa: BLE001
            mine = {"rank": rank, "device": getattr(dev, "index", None), "error": f"{type(e).__name__}: {e}"}
        ranks_info = [None] * world
        dist.all_gather_object(ranks_info, mine)
    if dist is not None and want_peer:
        # The peer-write gather needs every rank's window mapped into every other rank (hipIpc) and one exchange to come back right.
        # Every step is agreed on by ALL ranks (a rank that failed alone would leave the others waiting); otherwise: RCCL.
        def agree(ok: bool) -> bool:
            t = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            return bool(t.item())
        comm, handle, why = None, b"", ""
        try:
            n_max = max(*shape.qkv, shape.hidden, shape.ffn, shape.vocab)
            comm = capi.Comm(rank, world, n_max, slots=8)
            handle = comm.export()
        except Exception as e:  # noqa: BLE001
            why = f"window: {type(e).__name__}: {e}"
        got = [None] * world
        dist.all_gather_object(got, handle)
        ok = comm is not None and all(h for h in got)
        if ok:
            try:
                comm.connect(got)
            except Exception as e:  # noqa: BLE001
                ok, why = False, f"connect: {type(e).__name__}: {e}"
        if agree(ok):
            try:  # slot 7, a known pattern: rank r contributes r + 1
                part = dl.out_down.view(-1)
                part.fill_(float(rank + 1))
                comm.allgather(7, part.data_ptr(), dl.g_down.data_ptr(), dl.g_down.numel(), torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                want = torch.arange(1, world + 1, device=dev).repeat_interleave(part.numel()).to(torch.float16)
                ok = comm.status() == 0 and torch.equal(dl.g_down.view(-1), want)
                if not ok:
                    why = f"test exchange: status {comm.status()}"
            except Exception as e:  # noqa: BLE001
                ok, why = False, f"test exchange: {type(e).__name__}: {e}"
            ok = agree(ok)
        peer_state = "peer-write windows mapped on every rank, test exchange ok" if ok else ("not available: " + (why or "another rank failed to map a window or to exchange"))
        if ok:
            dl.comm = comm
        else:
            if why:
                print(f"[bench] rank {rank}: peer-write gather not available ({why}); using RCCL all-gathers", file=sys.stderr)
            elif rank == 0:
                print("[bench] peer-write gather not available on another rank; using RCCL all-gathers", file=sys.stderr)
            if args.gather == "peer":
                args.gather = "rccl"
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream

    if args.roofline_only:
        r = roofline_leg(dl, torch, args.roofline_launches, eager=args.roofline_eager)
        if rank == 0:
            print(json.dumps({"roofline": r}))
        return
    if args.shapes_only:
        r = shapes_only_leg(dl, torch, dev, shape, eager=args.roofline_eager)
        if rank == 0:
            print(json.dumps({"decode_launch_shapes": r}))
        return

    # ---- the step ----
    variants = None
    tuned_knobs = None
    if dist is None:
        plan = dl.make_plan(grouped=not args.ungrouped)
        step = lambda: plan.launch(stream)
        n_launches = plan.n_launches
        mode = "one hipGraph replay per token (129 launches in stream order)" if not args.ungrouped else "one hipGraph replay per token"
        if dl.dataflow and args.issue != "graph":
            try:  # the token-kernel variant never takes the bench line down with it: any failure leaves the stream-ordered graph as the step
                # the same launch list as ONE persistent kernel; what the two forms must agree on, bit for bit: every output of the token
                tplan = dl.make_plan(tagged=True)
                outs = [*dl.out_qkv, dl.out_o, dl.out_gate, dl.out_up, dl.out_down, dl.logits]
                why = None
                if not tplan.tagged:
                    why = "the library built the plan stream-ordered (tce_plan_is_chained = %d)" % tplan.kind
                else:
                    plan.launch(stream)
                    torch.cuda.synchronize()
                    want = [o.clone() for o in outs]
                    for rep in range(3):
                        for o in outs:
                            o.fill_(float("nan"))
                        tplan.launch(stream)
                        tplan.status()
                        if not all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(want, outs)):
                            why = f"outputs differ from the stream-ordered plan (replay {rep})"
                            break
                    if why is None and not torch.isfinite(dl.logits.float()).all():
                        why = "non-finite logits"
                if why is not None:
                    if args.issue == "token":
                        raise SystemExit(f"--issue token: {why}")
                    print(f"[bench] token kernel not used: {why}", file=sys.stderr)
                    variants = {"token kernel": {"rejected": why}}
                else:
                    def rate(fn, n):
                        for _ in range(10):
                            fn()
                        torch.cuda.synchronize()
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        for _ in range(n):
                            fn()
                        b.record()
                        torch.cuda.synchronize()
                        return a.elapsed_time(b) / n
                    tstep = lambda: tplan.launch(stream)
                    ms_g, ms_t = rate(step, max(50, args.steps // 2)), rate(tstep, max(50, args.steps // 2))
                    tplan.status()
                    variants = {"hipGraph of 129 launches (stream order)": {"ms_per_token": round(ms_g, 4), "tokens_per_s": round(1e3 / ms_g, 1)},
                                "token kernel (TCE_PLAN_TAGGED)": {"ms_per_token": round(ms_t, 4), "tokens_per_s": round(1e3 / ms_t, 1), "geometry": tplan.geometry(),
                                                                    "body": ("int8 contraction on the packed copies (csrc/w4a16_gemv_i8_token.hip, round 6: profiles/r6/i8_token_kernel.md)" if tplan.kind == 4
                                                                             else "fp16 unpack (csrc/w4a16_gemv_stream.hip, round 2)"),
                                                                    "verified": "all outputs of the token bit-identical to the stream-ordered plan, 3 replays"}}
                    if args.issue == "token" or ms_t < ms_g:
                        step = tstep
                        n_launches = 2
                        mode = ("one persistent kernel per token: the 129 launches walked by the same workgroups, the linears' data flow ordered by tagged "
                                "output words (TCE_PLAN_TAGGED) + a one-thread kernel that advances the tag")
                    try:  # round 3: the same data flow as ONE KERNEL PER LAUNCH on two alternating graph branches (TCE_PLAN_OVERLAPPED, csrc/w4a16_gemv_ovl.hip)
                        oplan = dl.make_plan(overlapped=True)
                        if not oplan.overlapped:
                            variants["overlapped launches (TCE_PLAN_OVERLAPPED)"] = {"rejected": f"built as kind {oplan.kind}"}
                        else:
                            bad = None
                            for rep in range(3):
                                for o in outs:
                                    o.fill_(float("nan"))
                                oplan.launch(stream)
                                oplan.status()
                                if not all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(want, outs)):
                                    bad = f"outputs differ from the stream-ordered plan (replay {rep})"
                                    break
                            if bad:
                                variants["overlapped launches (TCE_PLAN_OVERLAPPED)"] = {"rejected": bad}
                            else:
                                ms_o = rate(lambda: oplan.launch(stream), max(50, args.steps // 2))
                                oplan.status()
                                variants["overlapped launches (TCE_PLAN_OVERLAPPED)"] = {"ms_per_token": round(ms_o, 4), "tokens_per_s": round(1e3 / ms_o, 1),
                                                                                          "verified": "all outputs of the token bit-identical to the stream-ordered plan, 3 replays"}
                                if ms_o < min(ms_g, ms_t) and args.issue == "auto":
                                    step = lambda: oplan.launch(stream)
                                    n_launches = plan.n_launches + 1
                                    mode = "one kernel per launch on two alternating graph branches, the data flow ordered by tagged output words (TCE_PLAN_OVERLAPPED)"
                    except Exception as e:  # noqa: BLE001
                        variants["overlapped launches (TCE_PLAN_OVERLAPPED)"] = {"rejected": f"{type(e).__name__}: {e}"}
                        try:
                            capi.lib().tce_reset_last_error()
                            torch.cuda.synchronize()
                        except Exception:  # noqa: BLE001
                            pass
                    try:  # the stream-ordered graph with every launch's geometry timed on THIS device at plan creation (TCE_PLAN_TUNED): neighbouring
                        # geometries rank differently from box to box (profiles/r3/gemv_rows3_ab.jsonl)
                        uplan = dl.make_plan(tuned=True)
                        for o in outs:
                            o.fill_(float("nan"))
                        uplan.launch(stream)
                        torch.cuda.synchronize()
                        worst = max(float((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-6)) for a, b in zip(outs, want))
                        if not all(bool(torch.isfinite(o.float()).all()) for o in outs) or worst != 0.0:
                            variants["hipGraph, geometries timed on this device (TCE_PLAN_TUNED)"] = {"rejected": f"outputs differ from the untuned plan: worst |diff| / max = {worst:.2e}"}
                        else:
                            ustep = lambda: uplan.launch(stream)
                            n_ab = max(50, args.steps // 2)
                            ab = [(rate(step_g0, n_ab), rate(ustep, n_ab)) for step_g0 in (lambda: plan.launch(stream),) * 3]  # alternating: clocks drift within a process
                            ms_g2, ms_u = min(x for x, _ in ab), min(y for _, y in ab)
                            variants["hipGraph, geometries timed on this device (TCE_PLAN_TUNED)"] = {
                                "ms_per_token": round(ms_u, 4), "tokens_per_s": round(1e3 / ms_u, 1), "untuned_graph_in_the_same_alternation_ms": round(ms_g2, 4),
                                "verified": "all outputs of the token bit-identical to the untuned plan",
                                "chosen (rows, waves_n, waves_k, depth) for the first block's launches and lm_head; zeros: the dispatcher's rule kept": [list(g) for g in (uplan.launch_geometries()[:4] + uplan.launch_geometries()[-1:])]}
                            if ms_u < 0.995 * ms_g2 and ms_u < ms_t and args.issue == "auto" and n_launches == plan.n_launches:
                                tuned_knobs = uplan.launch_geometries()[2] if plan.n_launches > 2 else None  # the grouped gate+up launch of block 0
                                step = ustep
                                mode = "one hipGraph replay per token (129 launches in stream order, launch geometries timed on this device at plan creation: TCE_PLAN_TUNED)"
                    except Exception as e:  # noqa: BLE001
                        variants["hipGraph, geometries timed on this device (TCE_PLAN_TUNED)"] = {"rejected": f"{type(e).__name__}: {e}"}
                        try:
                            capi.lib().tce_reset_last_error()
                            torch.cuda.synchronize()
                        except Exception:  # noqa: BLE001
                            pass
            except SystemExit:
                raise
            except Exception as e:  # noqa: BLE001
                if args.issue == "token":
                    raise
                print(f"[bench] token kernel not used: {type(e).__name__}: {e}", file=sys.stderr)
                variants = {"token kernel": {"rejected": f"{type(e).__name__}: {e}"}}
                step = lambda: plan.launch(stream)
                n_launches = plan.n_launches
                try:
                    capi.lib().tce_reset_last_error()
                    torch.cuda.synchronize()
                except Exception:  # noqa: BLE001
                    pass
    else:
        n_launches = dl.n_layers * 4 + 1

        def build_dist_step(gpb, gather, dl=dl, block_launch="four"):
            """The distributed token (gpb gathers per block, joined by `gather`; block_launch "one": a rank's linears of a block as ONE launch, gpb = 1 only) as a
            callable + how it is issued."""
            graph = None
            try:  # capture GEMVs + RCCL all-gathers of one token into one graph; fall back to eager issue if capture fails
                if args.no_graph or (args.backend != "nccl" and gather != "peer"):
                    raise RuntimeError("graph capture not requested / not available with this backend")
                # the ranks meet before anything that exchanges data runs: a peer-write gather waits a bounded time (2 s) for the other ranks' slices and
                # then flags the communicator, and building the shards / capturing the graph takes the ranks seconds, not all the same number
                dist.barrier()
                torch.cuda.synchronize()
                for _ in range(3):
                    dl.run_token_distributed(gpb, gather=gather, block_launch=block_launch)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):  # the RCCL watchdog thread may call HIP APIs meanwhile
                    dl.run_token_distributed(gpb, gather=gather, block_launch=block_launch)
                step = graph.replay
                mode = f"one graph replay per token (GEMVs + {'peer-write' if gather == 'peer' else 'RCCL'} all-gathers captured)"
            except Exception as e:  # noqa: BLE001
                if rank == 0:
                    print(f"[bench] graph capture of the distributed token failed ({type(e).__name__}: {e}); issuing eagerly", file=sys.stderr)
                # a failed capture leaves hipErrorStreamCaptureInvalidated as the runtime's sticky last error, which the next
                # launch's error check would report as its own: drain it before issuing eagerly
                # torch.cuda.graph.__exit__ raises out of capture_end() before it restores the current stream: the dead capture
                # stream would stay current and every eager launch would fail on it
                torch.cuda.set_stream(torch.cuda.default_stream())
                capi.lib().tce_reset_last_error()
                torch.cuda.synchronize()
                step = lambda: dl.run_token_distributed(gpb, gather=gather, block_launch=block_launch)
                mode = "eager issue per token"
            return step, mode

    def fence():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def timed_run(step):
        fence()  # (N > 1: the ranks start their first replay together, see above)
        if os.environ.pop("TCE_BENCH_TEST_LATE_RANK", "") and rank == world - 1:
            time.sleep(1.0)  # test hook: this rank trails by more than the gather's wait bound once -> the RCCL repeat below is exercised
        for _ in range(args.warmup):
            step()
        fence()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(args.steps):
            step()
        e1.record()
        fence()
        wall = time.perf_counter() - t0
        if dist is not None:
            tw = torch.tensor([wall], dtype=torch.float64, device=dev)
            dist.all_reduce(tw, op=dist.ReduceOp.MAX)
            wall = float(tw.item())
        return wall, e0.elapsed_time(e1)

    def time_gather_variants(dl):
        """(gather_variants, runs) for one set of sharded linears: every way the ranks' slices can be joined, timed one after the other."""
        gathers = [g for g in (("peer", "rccl") if args.gather == "all" else (args.gather,)) if g != "peer" or getattr(dl, "comm", None) is not None]
        gpbs = (1, 4) if args.gathers_per_block == 0 else (args.gathers_per_block,)
        gather_variants, runs = {}, []
        for gpb, blk in [(g, b) for g in gpbs for b in ((("fused", "one", "four") if g == 1 else ("four",)))]:
            for gth in gathers:
                if blk == "fused" and gth != "peer":
                    continue
                name = f"{'peer-write kernel (tce_allgather_f16)' if gth == 'peer' else 'RCCL all_gather_into_tensor'}, {gpb} gather{'s' if gpb > 1 else ''} per block" + \
                       (", one launch per block (tce_w4a16_forward_independent)" if blk == "one" else "")
                if blk == "fused":
                    name = "peer-write exchange inside the block's one launch (tce_w4a16_forward_independent_gather), 1 gather per block"
                try:
                    step_v, mode_v = build_dist_step(gpb, gth, dl, blk)
                    wall_v, ev_v = timed_run(step_v)
                    ok = True
                    if gth == "peer":
                        # a peer-write gather that timed out (a rank trailing by more than the bound, a window that stopped being reachable) voids the
                        # timing; all ranks agree on that, the communicator is re-armed for the next variant
                        bad = torch.tensor([1 if dl.comm.status() != 0 else 0], dtype=torch.int32, device=dev)
                        dist.all_reduce(bad, op=dist.ReduceOp.MAX)
                        if int(bad.item()):
                            ok = False
                            dist.barrier()
                            torch.cuda.synchronize()
                            dl.comm.reset()
                            dist.barrier()
                    gather_variants[name] = ({"ms_per_token": round(wall_v * 1e3 / args.steps, 4), "tokens_per_s": round(args.steps / wall_v, 1), "issue": mode_v} if ok
                                             else {"rejected": "tce_comm_status != 0 on some rank: a peer-write gather timed out"})
                    if ok:
                        runs.append((gpb, gth, wall_v, ev_v, mode_v, name, blk))
                except Exception as e:  # noqa: BLE001 -- one variant never takes the others down with it
                    gather_variants[name] = {"rejected": f"{type(e).__name__}: {e}"}
                    try:
                        torch.cuda.set_stream(torch.cuda.default_stream())
                        capi.lib().tce_reset_last_error()
                        torch.cuda.synchronize()
                    except Exception:  # noqa: BLE001
                        pass
        return gather_variants, runs

    gather_variants = None
    llama13 = None
    if dist is None:
        wall, ev_ms_total = timed_run(step)
        if args.dump_outputs:
            dump_outputs(dl, args.dump_outputs)
    else:
        # Every way the ranks' slices can be joined, in ONE run (the first session on an 8-GPU node should not have to be repeated four
        # times): {peer-write kernel, RCCL} x {1 gather per block -- the north-star definition --, 4 -- the dependency-faithful form}.
        # The headline is the faster one-gather-per-block variant; all of them are under config.gather_variants.
        gather_variants, runs = time_gather_variants(dl)
        if not runs:
            raise SystemExit("no gather variant completed: " + json.dumps(gather_variants))
        one = [r for r in runs if r[0] == min(g for g, *_ in runs)]
        gpb_h, gth_h, wall, ev_ms_total, mode, name_h, blk_h = min(one, key=lambda r: r[2])
        args.gathers_per_block, args.gather = gpb_h, gth_h
        n_launches = dl.n_layers * (4 if blk_h == "four" else 1) + 1  # (the gather kernels / collectives are not counted; "fused": there are none but the logits')
        gather_variants["headline"] = name_h
        if args.dump_outputs:  # (every variant computes the same token; the last one timed left it in the buffers)
            dump_outputs(dl, args.dump_outputs, rank)
        # BASELINE config 5 (Llama-2-13B column-sharded 8 ways) beside the headline workload when the run has its eight ranks (VERDICT r4 item 7 ii): same
        # variants, same timing; never takes the headline down with it
        if world == 8 and args.workload != "llama2-13b" and args.full and not args.no_extras:
            try:
                dl13 = DecodeLinears(SHAPES["llama2-13b"], device=dev, group_size=G, rank=rank, world=world, m=1, prepack=prepack)
                if getattr(dl, "comm", None) is not None:
                    def exchange13(h):
                        got13 = [None] * world
                        dist.all_gather_object(got13, h)
                        return got13
                    dl13.attach_peer_comm(exchange13)
                gv13, runs13 = time_gather_variants(dl13)
                sh13 = SHAPES["llama2-13b"]
                bytes13 = sum(capi.algorithmic_bytes(1, n, k, G) for (n, k) in
                              ([(n, sh13.hidden) for n in sh13.qkv] + [(sh13.hidden, sh13.hidden), (sh13.ffn, sh13.hidden), (sh13.ffn, sh13.hidden), (sh13.hidden, sh13.ffn)]) * dl13.n_layers
                              + [(sh13.vocab, sh13.hidden)])
                one13 = [r for r in runs13 if r[0] == 1] or runs13
                best13 = min(one13, key=lambda r: r[2]) if one13 else None
                llama13 = {"workload": sh13.name, "gather_variants": gv13, "algorithmic_bytes_per_token": bytes13,
                           **({"tokens_per_s": round(args.steps / best13[2], 1), "ms_per_token": round(best13[2] * 1e3 / args.steps, 4), "headline": best13[5],
                               "gather": best13[5], "frac_of_8TBs": round(bytes13 * args.steps / best13[2] / (world * 8.0e12), 4)} if best13 else {})}
                del dl13
            except Exception as e:  # noqa: BLE001
                llama13 = {"error": f"{type(e).__name__}: {e}"}
    ms_per_step = wall * 1e3 / args.steps
    ev_ms_per_step = ev_ms_total / args.steps
    tok_s = args.steps / wall

    token_bytes_rank = dl.token_bytes()
    token_bytes_full = sum(capi.algorithmic_bytes(1, n, k, G) for (n, k) in
                           ([(n, shape.hidden) for n in shape.qkv] + [(shape.hidden, shape.hidden), (shape.ffn, shape.hidden),
                                                                       (shape.ffn, shape.hidden), (shape.hidden, shape.ffn)]) * dl.n_layers
                           + [(shape.vocab, shape.hidden)])
    # the dominant kernel in isolation (at N > 1: this rank's row shard of it; purely local, every rank runs it so the ranks
    # stay in step for the teardown)
    roof = None
    if args.full:
        try:
            roof = roofline_leg(dl, torch, args.roofline_launches, knobs=tuned_knobs)
            if world > 1:
                roof["kernel"] += f", rows sharded {world}-way (this rank's shard)"
        except Exception as e:  # noqa: BLE001 -- never takes the headline number down with it
            roof = None if world > 1 else {"error": f"{type(e).__name__}: {e}"}
    whole = {"achieved_GBs_per_gpu": round(token_bytes_rank / (ev_ms_per_step * 1e-3) / 1e9, 1),
             "frac_of_8TBs": round(token_bytes_rank / (ev_ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
             "algorithmic_bytes_per_token_per_gpu": token_bytes_rank, "launches_per_token": n_launches,
             "event_ms_per_token": round(ev_ms_per_step, 4)}

    extras = None
    secondary = None
    if rank == 0 and world == 1 and args.full and not args.no_extras:
        try:
            extras = other_configs_leg(torch, dev)
        except Exception as e:  # noqa: BLE001 -- never takes the headline number down with it
            extras = {"error": f"{type(e).__name__}: {e}"}
        for size, key in (("125M", "w8a8_opt125m_layer"), ("1.3B", "w8a8_opt1p3b_layer"), ("6.7B", "w8a8_opt6p7b_layer")):
            try:  # BASELINE config 4 as whole OPT decoder stacks (graph plans): us and launches per layer, the rate the int8 weights stream at
                extras[key] = opt_layer_leg(torch, dev, size)
            except Exception as e:  # noqa: BLE001
                extras[key] = {"error": f"{type(e).__name__}: {e}"}
        try:  # every launch shape of the token on its own: us, GB/s, fraction of 8 TB/s (same timing method as the roofline leg)
            extras["decode_launch_shapes"] = launch_shape_table(dl, torch)
        except Exception as e:  # noqa: BLE001
            extras["decode_launch_shapes"] = {"error": f"{type(e).__name__}: {e}"}
        try:  # the cost of real AWQ zero points on the dominant launch
            extras["gate_up_random_zero_points"] = random_zero_points_leg(dl, torch)
        except Exception as e:  # noqa: BLE001
            extras["gate_up_random_zero_points"] = {"error": f"{type(e).__name__}: {e}"}
        if args.workload in ("baseline-named", "llama3-8b") and not args.no_projection:
            try:  # SURVEY 8e on one GPU: per-rank shard compute at N/P rows, measured; the exchange side assumed and labelled
                extras["projected_scaling"] = projected_scaling_leg(torch, dev, G, prepack)
            except Exception as e:  # noqa: BLE001
                extras["projected_scaling"] = {"error": f"{type(e).__name__}: {e}"}
        if args.workload in ("baseline-named", "llama3-8b"):
            try:  # the callers either side of the path: a WHOLE decode token -- norms, RoPE, KV append, attention, residuals -- in 5 launches per layer
                extras["decode_with_attention"] = whole_token_leg(torch, dev, shape, dl)
            except Exception as e:  # noqa: BLE001
                extras["decode_with_attention"] = {"error": f"{type(e).__name__}: {e}"}
            # The other of the two shape sets this metric is read on: BASELINE.json names "Llama-3-8B" and spells Llama-2-7B widths (4096x4096, 4096x11008).
            # The headline `value` is the model the metric names; the spelled shapes are timed here, the same way, and reported at the top level.
            other_key = "baseline-named" if args.workload == "llama3-8b" else "llama3-8b"
            try:
                dl2 = DecodeLinears(SHAPES[other_key], device=dev, group_size=G, m=1, prepack=prepack,
                                    dataflow=(not args.ungrouped and SHAPES[other_key].qkv[0] >= SHAPES[other_key].hidden))
                plan2 = dl2.make_plan()
                for _ in range(5):
                    plan2.launch(stream)
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(50):
                    plan2.launch(stream)
                b.record()
                torch.cuda.synchronize()
                ms2 = a.elapsed_time(b) / 50
                secondary = {
                    "workload": SHAPES[other_key].name, "tokens_per_s": round(1e3 / ms2, 1), "ms_per_token": round(ms2, 4), "algorithmic_bytes_per_token": dl2.token_bytes(),
                    "frac_of_8TBs": round(dl2.token_bytes() / (ms2 * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "launches_per_token": plan2.n_launches,
                    "launch_shapes": launch_shape_table(dl2, torch, 96)}
                del plan2
                try:
                    secondary["decode_with_attention"] = whole_token_leg(torch, dev, SHAPES[other_key], dl2)
                except Exception as e:  # noqa: BLE001
                    secondary["decode_with_attention"] = {"error": f"{type(e).__name__}: {e}"}
                del dl2
                torch.cuda.empty_cache()
            except Exception as e:  # noqa: BLE001
                secondary = {"error": f"{type(e).__name__}: {e}"}

    adapter = None
    if rank == 0 and world == 1 and args.full and not args.no_extras and args.workload in ("baseline-named", "llama3-8b", "tiny"):
        torch.cuda.synchronize()
        try:
            adapter = adapter_path_leg(args.workload)
        except Exception as e:  # noqa: BLE001
            adapter = {"error": f"{type(e).__name__}: {e}"}

    cpu = None
    parity = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        try:
            cpu = cpu_baseline_leg(args.workload, shape)
        except Exception as e:  # noqa: BLE001 -- the baseline must never take the GPU number down with it
            cpu = {"error": f"{type(e).__name__}: {e}"}
        if prepack and not args.layers:
            parity = parity_leg(dl, torch, args.workload)

    if rank == 0:
        out = {
            "metric": "decode tokens/s (W4A16 linears of one token, M=1) + GEMV GB/s vs HBM roofline",
            "value": round(tok_s, 2), "unit": "tokens/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "int4 weights x fp16 activations, fp32 accumulate", "data": "synthetic",
            "config": {"workload": f"W4A16 decode GEMV M=1, {shape.name}: {dl.n_layers} blocks x [qkv {list(shape.qkv)}, o {shape.hidden}, gate/up {shape.ffn}, down] + lm_head {shape.vocab}, group 128",
                       "parallelism": (f"tp{world} column-sharded, {args.gathers_per_block} "
                                       + ("peer-write all-gather(s) (tce_allgather_f16)" if args.gather == "peer" else f"{'RCCL' if args.backend == 'nccl' else args.backend} all-gather(s)")
                                       + " per block") if world > 1 else "single GPU",
                       "issue": mode, **({"issue_variants": variants} if variants else {}), **({"gather_variants": gather_variants} if gather_variants else {}),
                       **({"ranks": ranks_info, "rccl_ranks": (dist.get_world_size() if args.backend == "nccl" else 0),
                           "gather_path": {"peer": peer_state, "rccl": f"torch.distributed backend {args.backend} ({'RCCL' if args.backend == 'nccl' else 'CPU stand-in'})",
                                           "headline": args.gather}} if dist is not None else {}),
                       "grouped_launches": not args.ungrouped,
                       "decode_kernel": ("int8 contraction on the packed copy of every linear (tce_w4a16_prepack at load time; csrc/w4a16_gemv_i8.hip)" if prepack
                                         else "fp16 unpack on the q4_6 arrays (csrc/w4a16_gemv.hip)"),
                       "activations": ("the linears feed each other as in the decoder (x -> qkv; o reads the q slice; o -> gate/up; gate -> down; down -> next block; "
                                       "last down -> lm_head); W ~ N(0, 1/K)") if dl.dataflow else "every linear reads its own fixed N(0,1) vector; W ~ N(0, 0.02^2)",
                       "algorithmic_bytes_per_token": token_bytes_full},
            "whole_token": whole,
        }
        if roof is not None:
            # every launch shape of the token inside the block the driver keeps: this workload's and -- the shapes BASELINE.json spells, on which the 0.70 bar is
            # quoted -- the baseline-named set's (4096 x 4096 = o_proj, 4096 x 11008 = down_proj / the gate projection alone)
            if extras is not None and isinstance(extras.get("decode_launch_shapes"), list) and isinstance(roof, dict) and "error" not in roof:
                keep = ("name", "launch", "kernel", "us", "GBs", "frac_of_8TBs", "bytes")
                shp = [dict({k: r[k] for k in keep if k in r}, workload=args.workload) for r in extras["decode_launch_shapes"]]
                if isinstance(secondary, dict) and isinstance(secondary.get("launch_shapes"), list):
                    other_key = "baseline-named" if args.workload == "llama3-8b" else "llama3-8b"
                    shp += [dict({k: r[k] for k in keep if k in r}, workload=other_key) for r in secondary["launch_shapes"]]
                roof["shapes"] = shp
                roof["shapes_timing"] = "as the dominant launch: hipGraph of back-to-back launches rotating over the 32 layers' weights, HIP events on the launch stream (rocprofv3 rows: profiles/r4/)"
            out["roofline"] = roof
        if secondary is not None:
            out["baseline_named_shapes" if args.workload == "llama3-8b" else "llama3_8b_true_shapes"] = secondary
        if extras is not None:
            # BASELINE config 4 (W8A8 on the OPT-125M shapes) inside the line the driver keeps: every launch with its time over the 1.55 us boundary between two
            # dependent launches (measured with a no-work kernel: DESIGN.md 3.0) -- these shapes are 5-11 us launches -- and its fraction of the dense int8 peak
            if isinstance(extras.get("w8a8_opt125m"), list):
                cfg4 = []
                for r in extras["w8a8_opt125m"]:
                    if "us" not in r: continue
                    ops = 2.0 * r.get("batch", 1) * r["M"] * r["N"] * r["K"]
                    over = max(r["us"] - 1.55, 0.05)
                    cfg4.append(dict(r, us_over_the_launch_boundary=round(over, 2), TOPs_over_the_boundary=round(ops / over / 1e6, 1), frac_of_5000_TOPs=round(ops / r["us"] / 1e6 / 5000.0, 4)))
                out["w8a8_opt125m_shapes"] = {"note": "tce_w8a8_matmul, bit-exact with kernels/ref/matmul_ref_int8.cc; graphs of 64 back-to-back launches on ONE weight set (L2-resident; the whole model is 94 MB: other_configs.w8a8_opt125m_layer walks per-layer weights), HIP events; boundary = 1.55 us per dependent launch",
                                              "launches": cfg4}
            out["other_configs"] = extras
        if llama13 is not None:
            out["llama2_13b"] = llama13  # BASELINE config 5, column-sharded over the run's eight ranks
        if adapter is not None:
            out["adapter_path"] = adapter
        if parity is not None:
            out["parity"] = parity
        if cpu is not None:
            main_cpu = cpu.get("avx") or cpu.get("ref")
            if main_cpu:
                out["cpu_baseline"] = dict(main_cpu, cpu_model=cpu.get("cpu_model"), nproc=cpu.get("nproc"))
                if "avx" in cpu and "ref" in cpu:
                    out["cpu_baseline_ref_naive"] = cpu["ref"]
            else:
                out["cpu_baseline"] = cpu
    emit_line(out if rank == 0 else None, rank, world, dist, torch)
    if dist is not None:
        dist.destroy_process_group()


def emit_line(out, rank, world, dist, torch=None):
    """Rank 0 writes the full record to a side file and prints its compact form as the LAST line of the job's stdout."""
    line = None
    if rank == 0:
        # the full record goes to a side file; the line the driver reads is its compact form, <= LINE_BUDGET bytes (tests/test_bench_contract.py)
        details = os.environ.get("TCE_BENCH_DETAILS") or os.path.join(REPO, "gpurun_out", f"bench_details_n{world}.json")
        try:
            os.makedirs(os.path.dirname(details), exist_ok=True)
            with open(details, "w") as f:
                json.dump(out, f, indent=1)
            details_rel = os.path.relpath(details, REPO)
        except OSError as e:
            print(f"[bench] could not write {details}: {e}", file=sys.stderr)
            details_rel = None
        line = dump_line(compact_line(out, details_rel))
        if len(line) > 8192:  # cannot happen with LINE_BUDGET < 8192 unless the mandatory blocks grew: fail loudly rather than print a line the driver cannot read
            raise SystemExit(f"bench line is {len(line)} bytes (> 8192)")
    # RCCL's banner sits in the C stdio buffer and would otherwise come out AFTER the JSON line at exit: every rank flushes
    # its C streams, the ranks meet, and only then rank 0 prints -- the JSON line is the last line of the job's stdout
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:  # noqa: BLE001
        pass
    sys.stdout.flush()
    if dist is not None:
        dist.barrier()
        if torch is not None and torch.cuda.is_available():
            torch.cuda.synchronize()
    if rank == 0:
        print(line, flush=True)


def selftest_emit(args):
    """`--selftest-emit FILE`: no GPU work -- push a stored FULL record (plus, for N > 1, a gather-variant block) through exactly the code that prints the
    bench line, under the same launch path (`--gpus N` re-exec, gloo rendezvous): tests/test_bench_contract.py checks the last stdout line and its size."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        dist.init_process_group("gloo", rank=rank, world_size=world)
    out = None
    if rank == 0:
        with open(args.selftest_emit) as f:
            out = json.loads(f.read().strip().splitlines()[-1])
        out["n_gpus"] = world
        if world > 1:
            names = [f"{g}, {n} gather{'s' if n > 1 else ''} per block" for n in (1, 4) for g in ("peer-write kernel (tce_allgather_f16)", "RCCL all_gather_into_tensor")]
            names = ["peer-write exchange inside the block's one launch (tce_w4a16_forward_independent_gather), 1 gather per block"] + \
                    [nm + ", one launch per block (tce_w4a16_forward_independent)" for nm in names[:2]] + names
            out["config"]["gather_variants"] = dict({nm: {"ms_per_token": 1.0, "tokens_per_s": 1000.0, "issue": "x" * 120} for nm in names}, headline=names[0])
            out["config"]["ranks"] = [{"rank": r, "device": r, "pci_bus_id": "0000:00:00.0"} for r in range(world)]
    print(f"[bench] rank {rank}: selftest noise on stdout before the line")
    emit_line(out, rank, world, dist)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
