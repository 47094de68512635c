"""Timing of svx_concat_rows against svx_alignment_rows on the same batch -- not the headline bench (bench.py), not a test.
python profiles/concat_rows_bench.py [--pairs 64] [--n 4096] [--k 4] [--d 1024] [--dtype bf16] [--warmup 5] [--reps 30]

After one svx_align_batch over the batch, base rows = non-deletions with a score up to the median:
  rows    svx_alignment_rows: flag + count, scan, gather                                                  (three launches)
  cat1    svx_concat_rows, max_num_align = 1, no duration filter, frames = NULL: the same rows            (seven launches)
  cat3    svx_concat_rows, max_num_align = 3, max_sil 1.0, max_dur 20.0 on both sides, min_frames 16000, over made-up
          timestamps (concat_rows_ref.frames_for: segments of 0.3 .. 4 s, one gap in seven over max_sil)
HIP events around every repetition, the three taking turns, median over the repetitions.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("speech-vecalign_amd", "tests", "oracle", "profiles"):
    sys.path.insert(0, os.path.join(ROOT, p))


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
    from align_rows_bench import timed
    from concat_rows_ref import frames_for
    from svx import _lib
    from svx.vecalign import dp_utils
    from synth import alignment_types, make_pair_device
    tdt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[a.dtype]
    code = {"bf16": _lib.SVX_BF16, "f16": _lib.SVX_F16, "f32": _lib.SVX_F32}[a.dtype]
    e = 4 if a.dtype == "f32" else 2
    dev = torch.device("cuda", 0)
    docs = [make_pair_device(a.n, a.n, a.k, a.d, 1000 + i, dev, tdt) for i in range(a.pairs)]
    frames = [(frames_for(np.random.RandomState([i, 0]), a.n), frames_for(np.random.RandomState([i, 1]), a.n)) for i in range(a.pairs)]
    pb = dp_utils.PreparedBatch(docs, alignment_types(a.k + 1), 0.2, 7, 300, 20000, 100,
                                rngs=[np.random.RandomState(i) for i in range(a.pairs)], device=0, frames=frames)
    ctx = pb.ctx
    pb.run()
    info, align, scores, _, offs = pb.raw_results()
    live = np.concatenate([scores[offs[i]:offs[i] + info[i, 0]][(align[offs[i]:offs[i] + info[i, 0], 1] > 0) & (align[offs[i]:offs[i] + info[i, 0], 3] > 0)]
                           for i in range(a.pairs)])
    T = float(np.median(live))
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    old = pb.alignment_rows(T, "fp16")
    kept = pb.rows_count()
    cap1 = int(old[0].shape[0])
    cat = pb.concat_rows(dict(max_score=T, max_num_align=3, max_sil=1.0, max_dur=20.0, both_sides=True, min_frames=16000), "fp16")
    fit3, wide3 = (int(v) for v in cat[5].cpu())
    cap3 = int(cat[0].shape[0])
    one = tuple(None if t is None else torch.empty_like(t[:cap1]) for t in cat[:4]) + (torch.empty((cap1, 8), dtype=torch.int32, device=dev), torch.empty_like(cat[5]))

    def prm(num, min_frames):
        c = _lib.ConcatParams()
        c.max_score, c.max_num_align, c.sample_rate, c.max_sil, c.max_dur, c.both_sides, c.min_frames = T, num, 16000, 1.0, 20.0, 1, min_frames
        return c
    p1, p3 = prm(1, 0), prm(3, 16000)

    def rows():
        ctx.check(ctx.lib.svx_alignment_rows(ctx.h, code, a.d, pb.cpairs, a.pairs, T, cap1, P(old[0]), P(old[1]), P(old[2]), P(old[3]),
                                             _lib.SVX_F16, P(old[4]), P(old[5])))

    def cat1():
        ctx.check(ctx.lib.svx_concat_rows(ctx.h, code, a.d, pb.cpairs, None, a.pairs, ctypes.byref(p1), cap1, P(one[0]), P(one[1]), P(one[2]), P(one[3]),
                                          _lib.SVX_F16, P(one[4]), P(one[5])))

    def cat3():
        ctx.check(ctx.lib.svx_concat_rows(ctx.h, code, a.d, pb.cpairs, pb.cframes, a.pairs, ctypes.byref(p3), cap3, P(cat[0]), P(cat[1]), P(cat[2]), P(cat[3]),
                                          _lib.SVX_F16, P(cat[4]), P(cat[5])))
    rows_ms, cat1_ms, cat3_ms = timed([rows, cat1, cat3], a.warmup, a.reps, torch)
    fit1 = int(one[5][0])
    same = bool(fit1 == kept and torch.equal(one[0][:kept].view(torch.int16), old[0][:kept].view(torch.int16))
                and torch.equal(one[3][:kept].view(torch.int16), old[3][:kept].view(torch.int16))
                and torch.equal(one[4][:kept, :2], old[4][:kept]))
    per_row = 2 * (2 * e + 2) * a.d                         # per side and row: read e d, write e d + 2 d
    print(json.dumps({"op": "svx_concat_rows", "pairs": a.pairs, "n": a.n, "k": a.k, "d": a.d, "dtype": a.dtype, "base_rows": kept,
                      "alignments": int(info[:, 0].sum()), "warmup": a.warmup, "reps": a.reps,
                      "rows_ms": round(rows_ms[0], 4), "rows_min_max_ms": [round(rows_ms[1], 4), round(rows_ms[2], 4)],
                      "cat1_ms": round(cat1_ms[0], 4), "cat1_min_max_ms": [round(cat1_ms[1], 4), round(cat1_ms[2], 4)],
                      "cat1_over_rows": round(cat1_ms[0] / rows_ms[0], 3), "cat1_same_bits": same,
                      "cat3_ms": round(cat3_ms[0], 4), "cat3_min_max_ms": [round(cat3_ms[1], 4), round(cat3_ms[2], 4)],
                      "cat3_fit": fit3, "cat3_wide": wide3, "cat3_rows_per_s": round(fit3 / cat3_ms[0] * 1e3),
                      "cat3_gbs": round(fit3 * per_row / cat3_ms[0] / 1e6, 1), "rows_gbs": round(kept * per_row / rows_ms[0] / 1e6, 1)}))


if __name__ == "__main__":
    main()
