"""Timing of svx_alignment_rows against the four launches it replaces -- not the headline bench (bench.py), not a test.
python profiles/align_rows_bench.py [--pairs 64] [--n 4096] [--k 4] [--d 1024] [--dtype bf16] [--warmup 5] [--reps 30]

After one svx_align_batch over the batch, for the same kept rows (non-deletions with a score up to the median):
  fused   svx_alignment_rows: flag + count, scan, gather (raw copies and unit rows of both sides, each row read once)
  split   what had to be done without it: the alignments read back, an index built on the host and uploaded, then
          svx_gather_rows per side and svx_unit_rows per side.  `split_ms` times the four launches alone, index already
          on the device; `split_host_ms` is the wall time of the read-back, the index and its upload.
HIP events around every repetition, the two ways taking turns, median over the repetitions.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("speech-vecalign_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))


def timed(fns, warmup, reps, torch):
    """Median / min / max milliseconds of every function, the functions taking turns repetition by repetition."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for fn, out in zip(fns, ms):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
    return [(float(np.median(m)), float(np.min(m)), float(np.max(m))) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--dtype", choices=["bf16", "f16", "f32"], default="bf16")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import torch
    from svx import _lib
    from svx.vecalign import dp_utils
    from synth import alignment_types, make_pair_device
    tdt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[a.dtype]
    code = {"bf16": _lib.SVX_BF16, "f16": _lib.SVX_F16, "f32": _lib.SVX_F32}[a.dtype]
    e = 4 if a.dtype == "f32" else 2
    dev = torch.device("cuda", 0)
    # one tensor per side, so that the split way can gather with ONE launch per side (row = ((pair * K + layer) * n + i))
    big = [torch.empty((a.pairs, a.k, a.n, a.d), dtype=tdt, device=dev) for _ in range(2)]
    for i in range(a.pairs):
        v0, v1 = make_pair_device(a.n, a.n, a.k, a.d, 1000 + i, dev, tdt)
        big[0][i], big[1][i] = v0, v1
    docs = [(big[0][i], big[1][i]) for i in range(a.pairs)]
    pb = dp_utils.PreparedBatch(docs, alignment_types(a.k + 1), 0.2, 7, 300, 20000, 100,
                                rngs=[np.random.RandomState(i) for i in range(a.pairs)], device=0)
    ctx = pb.ctx
    assert pb.vecs[0][0].data_ptr() == big[0][0].data_ptr()
    pb.run()
    info, align, scores, _, offs = pb.raw_results()
    live = np.concatenate([scores[offs[i]:offs[i] + info[i, 0]][(align[offs[i]:offs[i] + info[i, 0], 1] > 0) & (align[offs[i]:offs[i] + info[i, 0], 3] > 0)]
                           for i in range(a.pairs)])
    T = float(np.median(live))

    # ---- fused
    rows = pb.alignment_rows(T, "fp16")
    kept = pb.rows_count()
    cap = int(rows[0].shape[0])
    x_rows, y_rows, x_unit, y_unit, src, count = rows
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def fused():
        ctx.check(ctx.lib.svx_alignment_rows(ctx.h, code, a.d, pb.cpairs, a.pairs, T, cap, P(x_rows), P(y_rows), P(x_unit), P(y_unit),
                                             _lib.SVX_F16, P(src), P(count)))

    # ---- split: host round trip once (wall time), then the four launches
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h_info, h_align, h_scores = pb.info.cpu().numpy(), pb.align.cpu().numpy(), pb.scores.cpu().numpy()
    ix, iy = [], []
    for i in range(a.pairs):
        r = h_align[offs[i]:offs[i] + h_info[i, 0]]
        s = h_scores[offs[i]:offs[i] + h_info[i, 0]]
        r = r[(r[:, 1] > 0) & (r[:, 3] > 0) & (s <= T)]
        ix.append((i * a.k + r[:, 1] - 1) * a.n + r[:, 0] + r[:, 1] - 1)
        iy.append((i * a.k + r[:, 3] - 1) * a.n + r[:, 2] + r[:, 3] - 1)
    ix = torch.from_numpy(np.concatenate(ix).astype(np.int32)).to(dev)
    iy = torch.from_numpy(np.concatenate(iy).astype(np.int32)).to(dev)
    torch.cuda.synchronize()
    host_ms = (time.perf_counter() - t0) * 1e3
    assert ix.shape[0] == kept
    gx, gy = torch.empty((kept, a.d), dtype=tdt, device=dev), torch.empty((kept, a.d), dtype=tdt, device=dev)
    ux, uy = torch.empty((kept, a.d), dtype=torch.float16, device=dev), torch.empty((kept, a.d), dtype=torch.float16, device=dev)
    n_table = a.pairs * a.k * a.n

    def split():
        for table, idx, g, u in ((big[0], ix, gx, ux), (big[1], iy, gy, uy)):
            ctx.check(ctx.lib.svx_gather_rows(ctx.h, P(table), n_table, a.d, code, P(idx), kept, P(g)))
            ctx.check(ctx.lib.svx_unit_rows(ctx.h, P(g), code, kept, a.d, P(u), _lib.SVX_F16))
    fused_ms, split_ms = timed([fused, split], a.warmup, a.reps, torch)
    same = bool(torch.equal(gx.view(torch.int16), x_rows[:kept].view(torch.int16)) and torch.equal(uy.view(torch.int16), y_unit[:kept].view(torch.int16)))
    fused_bytes = kept * 2 * (2 * e + 2) * a.d             # per side and row: read e d, write e d + 2 d
    split_bytes = kept * 2 * (3 * e + 2) * a.d             # gather: read + write e d; unit: read e d, write 2 d
    print(json.dumps({"op": "svx_alignment_rows", "pairs": a.pairs, "n": a.n, "k": a.k, "d": a.d, "dtype": a.dtype, "kept": kept,
                      "alignments": int(info[:, 0].sum()), "warmup": a.warmup, "reps": a.reps,
                      "fused_ms": round(fused_ms[0], 4), "fused_min_max_ms": [round(fused_ms[1], 4), round(fused_ms[2], 4)],
                      "fused_bytes": fused_bytes, "fused_gbs": round(fused_bytes / fused_ms[0] / 1e6, 1),
                      "split_ms": round(split_ms[0], 4), "split_min_max_ms": [round(split_ms[1], 4), round(split_ms[2], 4)],
                      "split_bytes": split_bytes, "split_gbs": round(split_bytes / split_ms[0] / 1e6, 1),
                      "split_host_ms": round(host_ms, 3), "same_bits": same}))


if __name__ == "__main__":
    main()
