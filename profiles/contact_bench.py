"""Band contact and band doubling (svx_band_contact, svx_align_widen) on two shapes, one JSON line per leg:
    python profiles/contact_bench.py > profiles/contact_bench.jsonl
  contact   the benchmark's default step (bench.py: 1024 pairs of 4096 x 4096, K = 4, d = 1024, bf16, a = 5, W = 7, coarse to
            fine, pipeline on): milliseconds per step, and milliseconds of one svx_band_contact call over the 1024 pairs
            (HIP events around 20 calls behind a finished step).
  widen     one pair, 4096 source segments, the target a noisy copy without source segments 1500..2499 (3096 segments):
            svx_align_widen from a 14-cell straight band (up to 8 doublings) against ONE straight search at the width the
            doubling ended with.  Wall clock of the call, rounds, true pairs found.
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


def contact(pairs):
    import numpy as np
    import torch
    import bench
    from synth import alignment_types
    from svx.vecalign import dp_utils
    dev = torch.device("cuda:0")
    N, K, d = 4096, 4, 1024
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
    rows = pb.band_contact()          # (warm: the scratch is allocated)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls = 20
    a.record()
    for _ in range(calls):
        rows = pb.band_contact()
    b.record()
    torch.cuda.synchronize()
    r = rows.cpu().numpy()
    ctx.set_pipeline(False)
    print(json.dumps({"leg": "contact", "pairs": pairs, "N": N, "M": N, "step_ms": step_ms, "band_contact_ms": a.elapsed_time(b) / calls,
                      "touching_pairs": int((r[:, 0] > 0).sum()), "min_clearance": int(r[:, 2].min()), "nodes_mean": float(r[:, 3].mean())}), flush=True)


def widen():
    import numpy as np
    import torch
    from around_ref import block_deletion_pair, true_pairs_found
    from synth import alignment_types
    from svx.vecalign import dp_utils
    v0, v1, src = block_deletion_pair(N=4096, lo=1500, hi=2500, K=4, d=1024, seed=0)
    docs = [(torch.from_numpy(v0).cuda().bfloat16(), torch.from_numpy(v1).cuda().bfloat16())]
    types = alignment_types(5)

    def timed(fn):
        fn()                          # (warm: arenas and scratch allocated)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out
    pb = dp_utils.PreparedBatch(docs, types, 0.2, 7, 300, 20000, 100, rngs=[np.random.RandomState(11)], device=0, search="straight")
    pb.ctx.set_pipeline(False)
    ms_w, report = timed(lambda: pb.run_widen(max_rounds=8))
    found_w = true_pairs_found(pb.results()[0][0], src)
    W = int(report[0, 1])
    direct = dp_utils.PreparedBatch(docs, types, 0.2, W, 300, 20000, 100, rngs=[np.random.RandomState(11)], device=0, search="straight")
    ms_d, _ = timed(direct.run)
    same = direct.results()[0][0] == pb.results()[0][0]
    c = direct.band_contact().cpu().numpy()[0]
    print(json.dumps({"leg": "widen", "N": 4096, "M": int(v1.shape[1]), "report": report[0].tolist(), "widen_ms": ms_w, "true_pairs_widen": found_w,
                      "direct_width_over2": W, "direct_ms": ms_d, "true_pairs_direct": true_pairs_found(direct.results()[0][0], src),
                      "direct_touch": int(c[0]), "same_spans": bool(same), "true_pairs": int(len(src))}), flush=True)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        return contact(int(sys.argv[3]) if len(sys.argv) > 3 else 1024) if sys.argv[2] == "contact" else widen()
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    args = ap.parse_args()
    for leg in ("contact", "widen"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", leg, str(args.pairs)], capture_output=True, text=True, timeout=420)
        if r.returncode != 0 or not r.stdout.strip():
            print(json.dumps({"leg": leg, "rc": r.returncode, "error": r.stderr[-400:]}), flush=True)
            return r.returncode or 1
        print(r.stdout.strip().splitlines()[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
