"""svx_row_alternatives next to the svx_align_batch step whose level 0 it measures; one JSON line per leg:
    python profiles/alt_bench.py > profiles/alt_bench.jsonl
  entry   the shape of slack_bench.py (1024 pairs of 4096 x 4096, K = 4, d = 1024, bf16, a = 5, W = 7, coarse to fine).  From
          one process, per repetition: one step with stage timing on, then between HIP events one svx_row_slack call, one
          svx_row_alternatives(16, +inf) call and one svx_row_alternatives(16, penalty / 4) call (the C entries alone, into
          buffers allocated once; penalty = the median level-0 deletion penalty of the batch).  5 repetitions, medians.  Also
          the post-processing scratch the call grew and the summaries' totals.
  parts   the (16, +inf) call under `rocprofv3 --kernel-trace --stats`: the average device time of the backward sweep and of
          k_row_alt (a run of its own: tracing is not mixed with the timings above).
  dist    how long detours are: tests/golden/example_trim and around_ref.block_deletion_pair(seed=0) (-a 5, RandomState(11),
          coarse to fine), K = 256 for the distribution of n_detour and K = 16 for the share of status 1.
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

from slack_bench import prepare   # noqa: E402  (the batch of slack_bench.py; this directory is on the path of a script run from it)

REPS = 5
K = 16


def leg_entry(pairs, N):
    import ctypes
    import numpy as np
    import torch
    pb = prepare(pairs, N)
    ctx = pb.ctx
    pb.run()
    torch.cuda.synchronize()
    pen = float(np.median(pb.raw_results()[3][:, 0]))
    slack, s_summary = pb.row_slack()   # (warm: the scratch is allocated)
    torch.cuda.synchronize()
    before = int(ctx.lib.svx_scratch_bytes(ctx.h))
    alt = pb.row_alternatives(K)
    torch.cuda.synchronize()
    scratch = int(ctx.lib.svx_scratch_bytes(ctx.h))
    ca, summary = pb._alt_keep[0], alt['summary']
    sums = {}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    ms = {"row_slack": [], "alt_inf": [], "alt_quarter": [], "step": []}
    vp = ctypes.c_void_p
    ctx.check(ctx.lib.svx_set_profiling(ctx.h, 1))
    try:
        for _ in range(REPS):
            pb.run()
            torch.cuda.synchronize()
            ms["step"].append(float(ctx.lib.svx_stage_ms(ctx.h, b"total")))
            ev[0].record()
            ctx.check(ctx.lib.svx_row_slack(ctx.h, pb._slack_ptrs, vp(s_summary.data_ptr()), pairs))
            ev[1].record()
            ctx.check(ctx.lib.svx_row_alternatives(ctx.h, ca, K, float("inf"), vp(summary.data_ptr()), pairs))
            ev[2].record()
            torch.cuda.synchronize()
            sums["inf"] = summary.cpu().numpy().copy()
            ev[3].record()
            ctx.check(ctx.lib.svx_row_alternatives(ctx.h, ca, K, pen / 4, vp(summary.data_ptr()), pairs))
            ev[4].record()
            torch.cuda.synchronize()
            sums["quarter"] = summary.cpu().numpy().copy()
            for name, i in (("row_slack", 0), ("alt_inf", 1), ("alt_quarter", 3)):
                ms[name].append(ev[i].elapsed_time(ev[i + 1]))
    finally:
        ctx.lib.svx_set_profiling(ctx.h, 0)
    out = {"leg": "entry", "pairs": pairs, "N": N, "M": N, "d": 1024, "storage": "bf16", "a": 5, "W": 7, "band": 14, "reps": REPS,
           "max_detour": K, "penalty_median": pen, "step_total_ms": statistics.median(ms["step"]),
           "row_slack_ms": statistics.median(ms["row_slack"]), "row_alternatives_inf_ms": statistics.median(ms["alt_inf"]),
           "row_alternatives_quarter_penalty_ms": statistics.median(ms["alt_quarter"]), "ms_all": ms,
           "scratch_bytes_after": scratch, "scratch_bytes_grown_over_row_slack": scratch - before}
    for tag, s in sums.items():
        out["summary_" + tag] = {"rows": int(s[:, 0].sum()), "with_edge": int(s[:, 1].sum()), "detours_written": int(s[:, 2].sum()),
                                 "too_long": int(s[:, 3].sum()), "failed_pairs": int((s[:, 0] < 0).sum())}
    print(json.dumps(out), flush=True)


def leg_traced(pairs, N):
    """What the `parts` leg runs under the tracer: one step, then REPS calls."""
    import torch
    pb = prepare(pairs, N)
    pb.run()
    for _ in range(REPS):
        pb.row_alternatives(K)
    torch.cuda.synchronize()


def leg_parts(pairs, N):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--",
               sys.executable, os.path.abspath(__file__), "--one", "traced", str(pairs), str(N)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            print(json.dumps({"leg": "parts", "rc": r.returncode, "error": (r.stderr or r.stdout)[-400:]}), flush=True)
            return r.returncode
        out = {"leg": "parts", "pairs": pairs, "N": N, "calls": REPS, "max_detour": K}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for key, tag in (("k_bk_fast", "sweep"), ("k_bk_wide", "sweep"), ("k_row_alt", "alt")):
                    if key + "(" in row["Name"] or key + "<" in row["Name"]:
                        out[tag + "_kernel"] = key
                        out[tag + "_calls"] = out.get(tag + "_calls", 0) + int(row["Calls"])
                        out[tag + "_total_ms"] = out.get(tag + "_total_ms", 0.0) + float(row["TotalDurationNs"]) / 1e6
        for tag in ("sweep", "alt"):
            if tag + "_calls" in out:
                out[tag + "_ms_per_call"] = out[tag + "_total_ms"] / out[tag + "_calls"]
        print(json.dumps(out), flush=True)
    return 0


def leg_dist(pairs, N):
    import numpy as np
    import torch
    from around_ref import block_deletion_pair
    from synth import alignment_types
    from svx.vecalign import dp_utils
    from svx.vecalign.vecalign import load_document, resolve_search_params
    trim = os.path.join(ROOT, "tests", "golden", "example_trim")
    types, src_k, tgt_k, W = resolve_search_params(6, None, 5)
    docs = []
    for lang, k, side in (("en", src_k, "src"), ("de", tgt_k, "tgt")):
        _, v = load_document(os.path.join(trim, f"segments_{lang}.txt"),
                             [os.path.join(trim, f"cat_segs_{lang}.txt"), os.path.join(trim, f"embeds_{lang}.f16")], False, True, k,
                             os.path.join(trim, f"ignore_{side}.txt"), True)
        docs.append(v)
    v0, v1, _ = block_deletion_pair(seed=0)
    jobs = (("example_trim", tuple(docs), types, W, 0),
            ("block_deletion_pair(seed=0)", (torch.from_numpy(v0).cuda(), torch.from_numpy(v1).cuda()), alignment_types(5), 7, 11))
    for name, pair, ty, w, seed in jobs:
        pb = dp_utils.PreparedBatch([pair], ty, 0.2, w, 300, 20000, 100, rngs=[np.random.RandomState(seed)])
        pb.run()
        out = {"leg": "dist", "input": name}
        for k in (256, K):
            alt = pb.row_alternatives(k)
            torch.cuda.synchronize()
            n = int(alt['summary'][0, 0])
            span = alt['span'][:n].cpu().numpy()
            nd = np.sort(span[span[:, 3] == 0, 2])
            if k == 256:
                sl = alt['slack'][:n].cpu().numpy()
                out.update(rows=n, penalty=float(pb.raw_results()[3][0, 0]), with_edge=int(alt['summary'][0, 1]),
                           n_detour_quartiles=[int(nd[int(q * (len(nd) - 1))]) for q in (0, 0.25, 0.5, 0.75, 1)] if len(nd) else None,
                           n_detour_mean=float(nd.mean()) if len(nd) else None,
                           n_detour_histogram={str(v): int(c) for v, c in zip(*np.unique(nd, return_counts=True))},
                           span_rows_replaced_median=float(np.median((span[:, 1] - span[:, 0])[span[:, 3] == 0])) if len(nd) else None,
                           slack_median=float(np.median(sl)), status_counts_K256=np.bincount(span[:, 3], minlength=4).tolist())
            else:
                out["status_counts_K16"] = np.bincount(span[:, 3], minlength=4).tolist()
                out["share_too_long_K16"] = float((span[:, 3] == 1).mean())
        print(json.dumps(out), flush=True)
    return 0


def main():
    if len(sys.argv) > 4 and sys.argv[1] == "--one":
        pairs, N = int(sys.argv[3]), int(sys.argv[4])
        return {"entry": leg_entry, "traced": leg_traced, "parts": leg_parts, "dist": leg_dist}[sys.argv[2]](pairs, N) or 0
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--legs", default="entry,parts,dist")
    args = ap.parse_args()
    for name in args.legs.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, str(args.pairs), str(args.N)], capture_output=True,
                           text=True, timeout=420)
        if r.returncode != 0 or not r.stdout.strip():
            print(json.dumps({"leg": name, "rc": r.returncode, "error": r.stderr[-400:]}), flush=True)
            return r.returncode or 1
        for ln in r.stdout.strip().splitlines():
            if ln.startswith("{"):
                print(ln, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
