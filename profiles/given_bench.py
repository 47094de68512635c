"""svx_score_alignments on the batch's own result ("own"), next to the svx_align_batch step of the same batch; one JSON
line per leg:
    python profiles/given_bench.py > profiles/given_bench.jsonl
  batch   the benchmark's default step (bench.py: 1024 pairs of 4096 x 4096, K = 4, d = 1024, bf16, a = 5, W = 7, coarse to
          fine, pipeline on): milliseconds per step, and milliseconds of one score_alignments("own") call over all pairs
          (HIP events around 20 calls behind a finished step).
  long    one pair of 32768 x 32768, same settings.
Per leg also: entry_ms, the C entry alone (20 svx_score_alignments calls into the same buffers between HIP events: the
binding's output fills and uploads are not in it), the priced rows, the HBM bytes they stand for (two candidate rows per
priced row) and bytes / entry_ms; and, since the call must not wait for the device, the host's wall clock per call while
it queues two calls behind a step that is still running, with the time the device then needs to drain.
Each leg runs in a fresh child process."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "speech-vecalign_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def leg(name, pairs, N):
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
    pb = dp_utils.PreparedBatch(docs, alignment_types(K + 1), 0.2, 7, 300, 20000, 100, rngs=rngs, device=0)
    ctx = pb.ctx
    ctx.set_pipeline(True)
    pb.run()
    pb.flush()
    torch.cuda.synchronize()
    steps = 3
    t0 = time.perf_counter()
    for _ in range(steps):
        pb.run()
    pb.flush()
    torch.cuda.synchronize()
    step_ms = 1e3 * (time.perf_counter() - t0) / steps
    own = ["own"] * pairs
    got = pb.score_alignments(own)          # (warm: the scratch is allocated)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls = 20
    keep = []
    a.record()
    t0 = time.perf_counter()
    for _ in range(calls):
        keep.append(pb.score_alignments(own))
    host_ms = 1e3 * (time.perf_counter() - t0) / calls
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / calls
    # the C entry alone, into the buffers of the warm-up call (the binding's output fills and row upload are not in it)
    cg = got.cgiven
    a.record()
    for _ in range(calls):
        ctx.check(ctx.lib.svx_score_alignments(ctx.h, cg, pairs))
    b.record()
    torch.cuda.synchronize()
    entry_ms = a.elapsed_time(b) / calls
    # behind a step that is still running: the host must get its calls queued without waiting for the device.  Two calls,
    # the CLI's pattern: the post-processing scratch has two pinned descriptor buffers taken in turn, so a third call
    # would wait for the first one's upload (svxl_scratch_begin)
    pb.run()
    t0 = time.perf_counter()
    for _ in range(2):
        ctx.check(ctx.lib.svx_score_alignments(ctx.h, cg, pairs))
    behind_ms = 1e3 * (time.perf_counter() - t0) / 2
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    drain_ms = 1e3 * (time.perf_counter() - t1)
    rep = got.report.cpu().numpy()
    ctx.set_pipeline(False)
    priced = int(rep[:, 1].sum())
    nbytes = priced * 2 * d * 2
    print(json.dumps({"leg": name, "pairs": pairs, "N": N, "M": N, "d": d, "storage": "bf16", "step_ms": step_ms, "score_own_ms": ms,
                      "score_own_host_ms_per_call": host_ms, "entry_ms": entry_ms, "share_of_step": entry_ms / step_ms,
                      "host_ms_per_call_behind_a_running_step": behind_ms, "device_drain_ms_after_those_calls": drain_ms,
                      "rows": int(rep[:, 0].sum()), "priced_rows": priced, "row_bytes": nbytes, "GB_per_s": nbytes / (entry_ms * 1e-3) / 1e9,
                      "complete_pairs": int((rep[:, 7] == 1).sum()), "outside_nodes": int(rep[:, 6].sum())}), flush=True)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        return leg("batch", int(sys.argv[3]), 4096) if sys.argv[2] == "batch" else leg("long", 1, 32768)
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    args = ap.parse_args()
    for name in ("batch", "long"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, str(args.pairs)], capture_output=True, text=True, timeout=420)
        if r.returncode != 0 or not r.stdout.strip():
            print(json.dumps({"leg": name, "rc": r.returncode, "error": r.stderr[-400:]}), flush=True)
            return r.returncode or 1
        print(r.stdout.strip().splitlines()[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
