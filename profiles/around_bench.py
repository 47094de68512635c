"""Band search around a prior alignment (svx_align_around) against the two searches it sits between, on one shape:
4096 x 4096, K = 4, d = 1024, bf16, a = 5, W = 7, 64 pairs per call, inputs resident in HBM, pipeline off.
    python profiles/around_bench.py [--parent-lib PATH] [--commit TEXT] > profiles/around_bench.jsonl
Legs (each in a fresh child process, one JSON line each):
  coarse_to_fine   the reference's recursion (pyramid + deeper levels + level 0)
  straight         band around the straight line (no pyramid; only right when both documents advance at the same rate)
  around_pass11    around the output of a coarse-to-fine pass with the (1,1) type only, read on the device; the first pass
                   is made once, outside the timed loop (ms_first_pass states its cost)
  around_time      around a time prior (svx_time_prior, windows of 64 segments); the prior is made inside the timed loop
--parent-lib: a libsvx.so built from the parent commit; the two existing legs are then timed on it as well (SVX_LIB).
--commit: what to record as the commit the numbers were taken at (default: git's HEAD, when there is a checkout)."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "speech-vecalign_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

N, K, D, A, W, PAIRS, WARMUP, STEPS = 4096, 4, 1024, 5, 7, 64, 3, 10
LEGS = ("coarse_to_fine", "straight", "around_pass11", "around_time")


def one(leg):
    import numpy as np
    import torch
    from synth import alignment_types, make_pair_device
    from svx import _lib
    from svx.vecalign import dp_utils
    dev = torch.device("cuda:0")
    if os.environ.get("AROUND_BENCH_PARENT"):   # the parent's library has no entry points for the new mode
        for name in ("svx_align_around", "svx_time_prior"):
            _lib._SIGS.pop(name, None)
    _lib.context(0).set_pipeline(False)
    types = alignment_types(A)
    docs = [make_pair_device(N, N, K, D, 300 + i, dev, torch.bfloat16) for i in range(PAIRS)]
    rngs = lambda s: [np.random.RandomState(s + i) for i in range(PAIRS)]
    extra = {}
    if leg in ("coarse_to_fine", "straight"):
        pb = dp_utils.PreparedBatch(docs, types, 0.2, W, 300, 20000, 100, rngs=rngs(1000), device=0, search=leg)
        step = pb.run
    elif leg == "around_pass11":
        first = dp_utils.PreparedBatch(docs, [(1, 1)], 0.2, W, 300, 20000, 100, rngs=rngs(2000), device=0)
        first.run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first.run()
        torch.cuda.synchronize()
        extra["ms_first_pass"] = 1e3 * (time.perf_counter() - t0)
        pb = dp_utils.PreparedBatch(docs, types, 0.2, W, 300, 20000, 100, rngs=rngs(1000), device=0, search="around", priors=first)
        step = pb.run
    else:
        starts = 16000 * np.arange(N, dtype=np.int64)
        fr = np.stack([starts, starts + 12000], axis=1)
        pb = dp_utils.PreparedBatch(docs, types, 0.2, W, 300, 20000, 100, rngs=rngs(1000), device=0, search="around",
                                    priors=[None] * PAIRS, frames=[(fr, fr)] * PAIRS)

        def step():
            pb.time_prior(64 * 16000, 0)
            pb.run()
    for _ in range(WARMUP):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    res = pb.results()
    cover = all([x for al in r[0] for x in al[0]] == list(range(N)) and [y for al in r[0] for y in al[1]] == list(range(N)) for r in res)
    one_one = sum(1 for r in res for x, y in r[0] if len(x) == 1 and len(y) == 1 and x == y) / float(PAIRS * N)
    out = {"leg": leg, "N": N, "M": N, "K": K, "d": D, "dtype": "bf16", "a": A, "W": W, "pairs_per_call": PAIRS, "steps": STEPS,
           "ms_per_step": 1e3 * el / STEPS, "pairs_per_s": STEPS * PAIRS / el, "alignments_cover_both_documents": cover,
           "true_1to1_fraction": one_one, "lib": os.path.basename(_lib.LIB_PATH)}
    out.update(extra)
    print(json.dumps(out), flush=True)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        return one(sys.argv[2])
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    parent = args.parent_lib
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    runs = [(leg, None) for leg in LEGS] + ([(leg, parent) for leg in LEGS[:2]] if parent else [])
    for leg, lib in runs:
        env = dict(os.environ)
        if lib:
            env["SVX_LIB"] = os.path.abspath(lib)
            env["AROUND_BENCH_PARENT"] = "1"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", leg], capture_output=True, text=True, timeout=280, env=env)
        if r.returncode != 0 or not r.stdout.strip():
            print(json.dumps({"leg": leg, "rc": r.returncode, "error": r.stderr[-400:]}), flush=True)
            return r.returncode or 1
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        rec["build"] = "parent commit" if lib else "this change"
        rec["commit"] = commit   # None outside a git checkout
        print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
