"""Straight search (Sakoe-Chiba band / dense mode) with larger type sets: the general tile shape against the -a 5
shape the benchmark's c4 and dense legs run.  Every configuration runs in a fresh child process (fresh context, so
svx_scratch_bytes is that configuration's own arena) and prints one JSON line.
    python profiles/straight_types_bench.py > profiles/straight_types_bench.jsonl
Configurations: C4 (32768^2, d = 1024, bf16, band 2048) with -a 5 / 6 / 10 at 1 and 8 pairs per call; dense 4096^2
with -a 5 / 10 at 16 pairs per call; --many_to_one 50 on 8192 x 2048 (band 512), one pair; and the SVX_TILE_PROF
phase split of the C4 -a 5 and -a 10 sweeps, with
the type groups and re-stream factor of -a 7, -a 10, -a 16 and --many_to_one 50."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "speech-vecalign_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CONFIGS = [
    # name, N, M, a (or None), many_to_one (or None), W, pairs, steps, warmup, tile phase split
    ("c4_a5_1pair", 32768, 32768, 5, None, 1024, 1, 3, 1, False),
    ("c4_a6_1pair", 32768, 32768, 6, None, 1024, 1, 3, 1, False),
    ("c4_a10_1pair", 32768, 32768, 10, None, 1024, 1, 3, 1, False),
    ("c4_a5_8pairs", 32768, 32768, 5, None, 1024, 8, 2, 1, False),
    ("c4_a6_8pairs", 32768, 32768, 6, None, 1024, 8, 2, 1, False),
    ("c4_a10_8pairs", 32768, 32768, 10, None, 1024, 8, 2, 1, False),
    ("dense_a5_16pairs", 4096, 4096, 5, None, 4097, 16, 2, 1, False),
    ("dense_a10_16pairs", 4096, 4096, 10, None, 4097, 16, 2, 1, False),
    ("m2o50_8192x2048_band512", 8192, 2048, None, 50, 256, 1, 3, 1, False),
    ("c4_a5_1pair_phases", 32768, 32768, 5, None, 1024, 1, 1, 1, True),
    ("c4_a10_1pair_phases", 32768, 32768, 10, None, 1024, 1, 1, 1, True),
    # (the phase line of the general shape also states its type groups and re-stream factor)
    ("plan_a7", 2048, 2048, 7, None, 1024, 1, 1, 1, True),
    ("plan_a16", 2048, 2048, 16, None, 1024, 1, 1, 1, True),
    ("plan_m2o50", 4096, 1024, None, 50, 256, 1, 1, 1, True),
]


def one(name):
    import numpy as np
    import torch
    from synth import alignment_types, make_pair_device
    from svx import _lib
    from svx.vecalign import dp_utils
    from svx.vecalign.vecalign import resolve_search_params
    c = next(c for c in CONFIGS if c[0] == name)
    _, N, M, a, m2o, W, P, steps, warmup, phases = c
    if a is not None:
        types, kx, ky = alignment_types(a), a - 1, a - 1
    else:
        types, kx, ky, _ = resolve_search_params(10, m2o, 5)
    d, dev = 1024 if a is not None else 256, torch.device("cuda:0")
    _lib.context(0).set_pipeline(False)
    docs = []
    for i in range(P):
        v0, v1 = make_pair_device(N, M, max(kx, ky), d, 300 + i, dev, torch.bfloat16)
        docs.append((v0[:kx].contiguous(), v1[:ky].contiguous()))
    rngs = [np.random.RandomState(1000 + i) for i in range(P)]
    pb = dp_utils.PreparedBatch(docs, types, 0.2, W, 300, 20000, 100, rngs=rngs, device=0, search="straight")
    ctx, lib = pb.ctx, pb.ctx.lib
    for _ in range(warmup):
        pb.run()
    torch.cuda.synchronize()
    if phases:
        os.environ["SVX_TILE_PROF"] = "1"   # (k_band_tiles* sum their phase ticks; printed on stderr)
    else:
        lib.svx_set_profiling(ctx.h, 2)
    t0 = time.perf_counter()
    for _ in range(steps):
        pb.run()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    out = {"name": name, "N": N, "M": M, "d": d, "dtype": "bf16", "types": len(types), "band": 2 * W, "pairs_per_call": P,
           "steps": steps, "ms_per_pair": 1e3 * el / (steps * P), "pairs_per_s": steps * P / el,
           "scratch_bytes": int(lib.svx_scratch_bytes(ctx.h))}
    if not phases:
        out["stage_ms_per_call"] = {k: lib.svx_stage_ms(ctx.h, k.encode()) / steps for k in ("tiles", "traceback0", "total")}
        lib.svx_set_profiling(ctx.h, 0)
        res = pb.results()
        out["alignments_cover_both_documents"] = all(
            [x for al in r[0] for x in al[0]] == list(range(N)) and [y for al in r[0] for y in al[1]] == list(range(M)) for r in res)
    print(json.dumps(out), flush=True)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        return one(sys.argv[2])
    only = sys.argv[1:]
    for c in CONFIGS:
        if only and c[0] not in only:
            continue
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", c[0]], capture_output=True, text=True, timeout=300)
        line = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else json.dumps({"name": c[0], "error": r.stderr[-400:]})
        if r.returncode == 0 and c[9]:
            rec = json.loads(line)
            rec["tile_phases"] = [ln for ln in r.stderr.splitlines() if ln.startswith("[svx tile sweep")]
            line = json.dumps(rec)
        print(line, flush=True)
        if r.returncode != 0:
            print(json.dumps({"name": c[0], "rc": r.returncode}), flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
