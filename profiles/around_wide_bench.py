"""Wide bands around a prior (SVX_SEARCH_AROUND_WIDE) against the two searches a caller had before, on one shape:
32768 x 32768, K = 4, d = 1024, bf16, a = 5, one and eight pairs per call, inputs resident in HBM, pipeline off.
    python profiles/around_wide_bench.py [--commit TEXT] > profiles/around_wide_bench.jsonl
Legs (each in a fresh child process, one JSON line each, for 1 and for 8 pairs):
  around_wide_time   a time prior of 100-segment windows (svx_time_prior, made inside the timed loop) at its covering
                     width (svx_prior_width: 101, a band of 202 cells): the tile sweep around the prior's path
  straight_2048      Sakoe-Chiba band of 2048 cells around the straight line (the tile sweep)
  coarse_to_fine     the reference's recursion, W = 7
The synthetic target is a noisy copy of the source (no drift), so all three searches can find the same alignment; what
is compared is the cost of the search region.  Per leg: ms per pair (wall clock over the timed steps), the `tiles` stage
timer of one profiled call, svx_scratch_bytes, and how many alignment spans are identical to the coarse-to-fine result
of the same pairs (spans_total = spans of this leg)."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "speech-vecalign_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

N, K, D, A, WARMUP, STEPS = 32768, 4, 1024, 5, 2, 10
LEGS = ("around_wide_time", "straight_2048", "coarse_to_fine")
WINDOW = 100


def one(leg, pairs):
    import numpy as np
    import torch
    from synth import alignment_types, make_pair_device
    from svx import _lib
    from svx.vecalign import dp_utils
    dev = torch.device("cuda:0")
    ctx = _lib.context(0)
    ctx.set_pipeline(False)
    types = alignment_types(A)
    docs = [make_pair_device(N, N, K, D, 300 + i, dev, torch.bfloat16) for i in range(pairs)]
    rngs = lambda s: [np.random.RandomState(s + i) for i in range(pairs)]
    extra = {}

    def make(which):
        if which == "coarse_to_fine":
            pb = dp_utils.PreparedBatch(docs, types, 0.2, 7, 300, 20000, 100, rngs=rngs(1000), device=0)
            return pb, pb.run, 7
        if which == "straight_2048":
            pb = dp_utils.PreparedBatch(docs, types, 0.2, 1024, 300, 20000, 100, rngs=rngs(1000), device=0, search="straight")
            return pb, pb.run, 1024
        starts = 16000 * np.arange(N, dtype=np.int64)
        fr = np.stack([starts, starts + 12000], axis=1)
        probe = dp_utils.PreparedBatch(docs[:1], types, 0.2, 3, 300, 20000, 100, rngs=rngs(1000)[:1], device=0, search="around_wide",
                                       priors=[None], frames=[(fr, fr)])
        probe.time_prior(WINDOW * 16000, 0)
        W = int(probe.prior_width()[0])       # the covering width of this prior: every pair has the same timestamps
        pb = dp_utils.PreparedBatch(docs, types, 0.2, W, 300, 20000, 100, rngs=rngs(1000), device=0, search="around_wide",
                                    priors=[None] * pairs, frames=[(fr, fr)] * pairs)

        def step():
            pb.time_prior(WINDOW * 16000, 0)
            pb.run()
        return pb, step, W

    pb, step, W = make(leg)
    for _ in range(WARMUP):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    res = pb.results()
    scratch = int(ctx.lib.svx_scratch_bytes(ctx.h))
    ctx.check(ctx.lib.svx_set_profiling(ctx.h, 1))
    step()
    ctx.sync()
    tiles_ms = float(ctx.lib.svx_stage_ms(ctx.h, b"tiles"))
    total_ms = float(ctx.lib.svx_stage_ms(ctx.h, b"total"))
    ctx.check(ctx.lib.svx_set_profiling(ctx.h, 0))
    if leg == "coarse_to_fine":
        ref = res
    else:
        del pb
        ref_pb, ref_step, _ = make("coarse_to_fine")
        ref_step()
        ref = ref_pb.results()
    spans = lambda r: {(tuple(x), tuple(y)) for x, y in r[0]}
    same = sum(len(spans(a) & spans(b)) for a, b in zip(res, ref))
    out = {"leg": leg, "N": N, "M": N, "K": K, "d": D, "dtype": "bf16", "a": A, "width_over2": W, "band_cells": 2 * W,
           "pairs_per_call": pairs, "steps": STEPS, "ms_per_pair": 1e3 * el / STEPS / pairs, "tiles_stage_ms": tiles_ms,
           "total_stage_ms": total_ms, "svx_scratch_bytes": scratch, "spans_total": sum(len(r[0]) for r in res),
           "spans_identical_to_coarse_to_fine": same, "lib": os.path.basename(_lib.LIB_PATH)}
    out.update(extra)
    print(json.dumps(out), flush=True)


def main():
    if len(sys.argv) > 3 and sys.argv[1] == "--one":
        return one(sys.argv[2], int(sys.argv[3]))
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None)
    ap.add_argument("--pairs", default="1,8")
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    for pairs in [int(v) for v in args.pairs.split(",")]:
        for leg in LEGS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", leg, str(pairs)], capture_output=True, text=True, timeout=280)
            if r.returncode != 0 or not r.stdout.strip():
                print(json.dumps({"leg": leg, "pairs_per_call": pairs, "rc": r.returncode, "error": r.stderr[-400:]}), flush=True)
                return r.returncode or 1
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            rec["commit"] = commit   # None outside a git checkout
            print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
