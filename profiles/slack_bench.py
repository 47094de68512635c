"""svx_row_slack next to the svx_align_batch step whose level 0 it measures; one JSON line per leg:
    python profiles/slack_bench.py > profiles/slack_bench.jsonl
  entry   the benchmark's default step (bench.py: 1024 pairs of 4096 x 4096, K = 4, d = 1024, bf16, a = 5, W = 7, coarse to
          fine): per repetition one step with stage timing on (svx_set_profiling 1), its band_dp0 stage -- the forward band
          DP of level 0, the yardstick: the same serial chain with a min-and-argmin -- and one row_slack() call between HIP
          events (the C entry alone, into buffers allocated once).  5 repetitions, medians.  Also the post-processing
          scratch the call grew (svx_scratch_bytes after minus before) and the summary's totals.
  parts   the same call under `rocprofv3 --kernel-trace --stats`: the average device time of the backward sweep and of the
          slack kernel (a run of its own: tracing is not mixed with the timings above).
Each leg runs in a fresh child process under its own time limit."""
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "speech-vecalign_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

REPS = 5


def prepare(pairs, N):
    import numpy as np
    import torch
    import bench
    from synth import alignment_types
    from svx.vecalign import dp_utils
    dev = torch.device("cuda:0")
    K, d = 4, 1024
    docs = []
    for i in range(0, pairs, 16):
        docs += bench.synth_pairs_device(N, N, K, d, list(range(i, min(pairs, i + 16))), dev, torch.bfloat16)
    rngs = [np.random.RandomState(7 + i) for i in range(pairs)]
    return dp_utils.PreparedBatch(docs, alignment_types(K + 1), 0.2, 7, 300, 20000, 100, rngs=rngs, device=0)


def leg_entry(pairs, N):
    import ctypes
    import torch
    pb = prepare(pairs, N)
    ctx = pb.ctx
    pb.run()
    torch.cuda.synchronize()
    before = int(ctx.lib.svx_scratch_bytes(ctx.h))
    slack, summary = pb.row_slack()   # (warm: the scratch is allocated)
    torch.cuda.synchronize()
    scratch = int(ctx.lib.svx_scratch_bytes(ctx.h)) - before
    ptrs = pb._slack_ptrs
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms, dp0, step = [], [], []
    ctx.check(ctx.lib.svx_set_profiling(ctx.h, 1))
    try:
        for _ in range(REPS):
            pb.run()
            torch.cuda.synchronize()
            dp0.append(float(ctx.lib.svx_stage_ms(ctx.h, b"band_dp0")))
            step.append(float(ctx.lib.svx_stage_ms(ctx.h, b"total")))
            a.record()
            ctx.check(ctx.lib.svx_row_slack(ctx.h, ptrs, ctypes.c_void_p(summary.data_ptr()), pairs))
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
    finally:
        ctx.lib.svx_set_profiling(ctx.h, 0)
    s = summary.cpu().numpy()
    print(json.dumps({"leg": "entry", "pairs": pairs, "N": N, "M": N, "d": 1024, "storage": "bf16", "a": 5, "W": 7, "band": 14, "reps": REPS,
                      "row_slack_ms": statistics.median(ms), "row_slack_ms_all": ms,
                      "band_dp0_ms": statistics.median(dp0), "step_total_ms": statistics.median(step),
                      "row_slack_over_band_dp0": statistics.median(ms) / statistics.median(dp0),
                      "scratch_bytes": scratch, "rows": int(s[:, 0].sum()), "rows_slack_zero": int(s[:, 1].sum()),
                      "rows_slack_inf": int(s[:, 2].sum()), "failed_pairs": int((s[:, 0] < 0).sum())}), flush=True)


def leg_traced(pairs, N):
    """What the `parts` leg runs under the tracer: one step, then REPS calls."""
    import torch
    pb = prepare(pairs, N)
    pb.run()
    for _ in range(REPS):
        pb.row_slack()
    torch.cuda.synchronize()


def leg_parts(pairs, N):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--",
               sys.executable, os.path.abspath(__file__), "--one", "traced", str(pairs), str(N)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            print(json.dumps({"leg": "parts", "rc": r.returncode, "error": (r.stderr or r.stdout)[-400:]}), flush=True)
            return r.returncode
        out = {"leg": "parts", "pairs": pairs, "N": N, "calls": REPS}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for key, tag in (("k_bk_fast", "sweep"), ("k_bk_wide", "sweep"), ("k_path_slack", "slack"), ("k_sparse_dp_fast_batch", "forward_dp_all_levels")):
                    if key + "(" in row["Name"] or key + "<" in row["Name"]:
                        out[tag + "_kernel"] = key
                        out[tag + "_calls"] = out.get(tag + "_calls", 0) + int(row["Calls"])
                        out[tag + "_total_ms"] = out.get(tag + "_total_ms", 0.0) + float(row["TotalDurationNs"]) / 1e6
        for tag in ("sweep", "slack"):
            if tag + "_calls" in out:
                out[tag + "_ms_per_call"] = out[tag + "_total_ms"] / out[tag + "_calls"]
        print(json.dumps(out), flush=True)
    return 0


def main():
    if len(sys.argv) > 4 and sys.argv[1] == "--one":
        pairs, N = int(sys.argv[3]), int(sys.argv[4])
        return {"entry": leg_entry, "traced": leg_traced, "parts": leg_parts}[sys.argv[2]](pairs, N) or 0
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--N", type=int, default=4096)
    args = ap.parse_args()
    for name in ("entry", "parts"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, str(args.pairs), str(args.N)], capture_output=True,
                           text=True, timeout=420)
        if r.returncode != 0 or not r.stdout.strip():
            print(json.dumps({"leg": name, "rc": r.returncode, "error": r.stderr[-400:]}), flush=True)
            return r.returncode or 1
        print(r.stdout.strip().splitlines()[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
