"""Timing of margin-based mining (svx/postprocess/mine.py) beside the two searches it follows -- not the headline bench (bench.py).

python profiles/mine_bench.py [--n 131072] [--db 131072] [--d 1024] [--k 16] [--margin ratio] [--reps 7] [--out FILE]

One process, random rows.  After a warm-up of every step at full size, `reps` repetitions of: the two searches (x in y,
y in x), the new kernels (two svx_knn_list_means and two svx_margin_candidates), each group between one pair of HIP events,
and the retrieval step of "max" (stable sort on the device, copy to the host, svx_mine_greedy) by the host clock around
a device synchronise.  One JSON line: the median and the min..max of each figure, the new kernels' share of the search
time, and their bytes (n k (4 + 8) in, n (4 + 8 + 4) out and n k gathered floats per direction; n 4 k in, n 4 out per
list mean) over their time."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "speech-vecalign_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--db", type=int, default=131072)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--margin", default="ratio")
    ap.add_argument("--storage", default="fp16")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from svx.postprocess import mine
    from svx.postprocess.flat_index import FlatIndex
    g = torch.Generator(device="cuda").manual_seed(0)
    idx_x, idx_y = FlatIndex(a.d, a.storage), FlatIndex(a.d, a.storage)
    idx_x.add(torch.randn(a.n, a.d, device="cuda", generator=g))
    idx_y.add(torch.randn(a.db, a.d, device="cuda", generator=g))
    idx_x.ctx.use_current_stream()
    x, y, k = idx_x.rows, idx_y.rows, a.k

    def timed(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        return out, ev[0].elapsed_time(ev[1])

    def searches():
        return idx_y.search(x, k) + idx_x.search(y, k)

    def kernels(lists):
        sims_xy, ids_xy, sims_yx, ids_yx = lists
        mean_x, mean_y = mine.list_means(sims_xy), mine.list_means(sims_yx)
        fwd = mine.candidate_scores(sims_xy, ids_xy, mean_x, mean_y, a.margin)
        bwd = mine.candidate_scores(sims_yx, ids_yx, mean_y, mean_x, a.margin)
        return fwd[0], fwd[1], bwd[0], bwd[1]

    def retrieval(best):
        t0 = time.perf_counter()
        res = mine.select_pairs(*best, retrieval="max")
        torch.cuda.synchronize()
        return res, (time.perf_counter() - t0) * 1e3

    ms = {"search_x2": [], "mine_kernels": [], "host_sort_greedy": []}
    for rep in range(a.reps + 1):   # (repetition 0 is the warm-up)
        lists, t_search = timed(searches)
        best, t_kern = timed(lambda: kernels(lists))
        res, t_host = retrieval(best)
        if rep:
            ms["search_x2"].append(t_search)
            ms["mine_kernels"].append(t_kern)
            ms["host_sort_greedy"].append(t_host)
    nbytes = 0
    for rows in (a.n, a.db):
        nbytes += rows * k * 4 + rows * 4                                # list mean
        nbytes += rows * k * (4 + 8) + rows * k * 4 + rows * 4 + rows * (8 + 4)    # candidates: lists, gathered means, own mean, best
    rec = {"op": "mine: 2 x search, 2 x list_means + 2 x margin_candidates, max retrieval", "n": a.n, "db": a.db, "d": a.d, "k": k,
           "margin": a.margin, "storage": a.storage, "reps": a.reps, "pairs": int(res[0].shape[0]),
           "checksum": float(best[1].double().sum().item() + best[3].double().sum().item())}
    for name, v in ms.items():
        rec[name] = {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    rec["mine_kernels_over_search"] = round(rec["mine_kernels"]["ms_median"] / rec["search_x2"]["ms_median"], 5)
    rec["mine_kernels_bytes"] = nbytes
    rec["mine_kernels_gbps"] = round(nbytes / (rec["mine_kernels"]["ms_median"] * 1e-3) / 1e9, 1)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
