"""Row slack in wide bands: the time of PreparedBatch.row_slack_wide() (svx_row_slack_wide: node table, backward tile sweep with
the fused cut minimum, slack kernel) next to the forward "tiles" stage of the same run, which is the yardstick -- the
forward sweep is what the aligner itself pays for the band.

    python profiles/slack_wide_bench.py [--workloads c4x1,c4x8,dense16] [--reps 5] [--out profiles/slack_wide_bench.jsonl]

Workloads (bench.py's data, synth_pairs_device): c4xP = 32768 x 32768, band 2048, bf16, d = 1024, -a 5, P pairs;
denseP = 4096 x 4096, every cell, P pairs.  Per workload one JSON line: medians over --reps of the two stage times
(profiling mode 1: HIP events around the stage, the call waits for them), their ratio, the post-processing scratch the call
added, and the phase split of one more call under SVX_TILE_PROF=1 (100 MHz ticks summed over the persistent workgroups,
read off the library's stderr line)."""
import argparse
import json
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "speech-vecalign_amd"))
sys.path.insert(0, ROOT)


def phase_split(call):
    """Run `call` with SVX_TILE_PROF=1 and parse the library's '[svx backward tile sweep ...] p0(name)=ms ...' line."""
    os.environ["SVX_TILE_PROF"] = "1"
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        try:
            call()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
            os.environ.pop("SVX_TILE_PROF", None)
        f.seek(0)
        text = f.read().decode(errors="replace")
    line = [ln for ln in text.splitlines() if "backward tile sweep" in ln]
    return {m.group(1): float(m.group(2)) for m in re.finditer(r"p\d\(([^)]*)\)=([0-9.]+)", line[-1])} if line else {}


def run(name, reps):
    import torch
    from bench import alignment_types, synth_pairs_device
    from svx.vecalign import dp_utils
    dev = torch.device("cuda", 0)
    m = re.fullmatch(r"(c4x|dense)(\d+)", name)
    P = int(m.group(2))
    if m.group(1) == "c4x":
        N = M = 32768
        W = 1024
    else:
        N = M = 4096
        W = N + 1
    K, d = 4, 1024
    docs = []
    for i in range(0, P, 4):
        docs += synth_pairs_device(N, M, K, d, [300 + j for j in range(i, min(P, i + 4))], dev, torch.bfloat16)
    rngs = [np.random.RandomState(np.random.SeedSequence([4242, 0, i]).generate_state(4)) for i in range(P)]
    pb = dp_utils.PreparedBatch(docs, alignment_types(K + 1), 0.2, W, 300, 20000, 100, rngs=rngs, device=0, search="straight")
    ctx, lib = pb.ctx, pb.ctx.lib
    ctx.set_pipeline(False)
    pb.run()
    before = int(lib.svx_scratch_bytes(ctx.h))
    pb.row_slack_wide()
    torch.cuda.synchronize()
    added = int(lib.svx_scratch_bytes(ctx.h)) - before
    lib.svx_set_profiling(ctx.h, 1)
    fwd, bwd = [], []
    for _ in range(reps):
        pb.run()
        fwd.append(lib.svx_stage_ms(ctx.h, b"tiles"))
        sl, summ = pb.row_slack_wide()
        bwd.append(lib.svx_stage_ms(ctx.h, b"tiles_bwd"))
    lib.svx_set_profiling(ctx.h, 0)
    split = phase_split(lambda: (pb.row_slack_wide(), torch.cuda.synchronize()))
    sl, summ = sl.cpu().numpy(), summ.cpu().numpy()
    f, b = float(np.median(fwd)), float(np.median(bwd))
    return dict(workload=name, n=N, m=M, band=2 * W, pairs=P, d=d, dtype="bf16", alignment_max_size=K + 1, reps=reps,
                tiles_ms=f, tiles_bwd_ms=b, ratio=b / f, tiles_ms_all=fwd, tiles_bwd_ms_all=bwd, scratch_added_bytes=added,
                phase_ms_summed_over_workgroups=split, summary_pair0=summ[0].tolist(),
                slack_median_pair0=float(np.median(sl[:summ[0][0]])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c4x1,c4x8,dense16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slack_wide_bench.jsonl"))
    args = ap.parse_args()
    with open(args.out, "w") as out:
        for name in args.workloads.split(","):
            rec = run(name, args.reps)
            out.write(json.dumps(rec) + "\n")
            out.flush()
            print(json.dumps(rec))


if __name__ == "__main__":
    main()
