"""Timing of the grouped search (svx_knn_search_groups) against the loop of per-group svx_knn_search calls it replaces, and of
the local-mining CLI end to end -- not the headline bench (bench.py).

python profiles/group_search_bench.py [--case many|big|cli|all] [--reps 9] [--k 16] [--d 1024] [--storage fp16] [--out FILE]

  many   1024 groups of 1148 x 1035 rows (the example document pair), both directions: the case the grouped search exists for
  big    4 groups of 16384 x 16384 rows, both directions: launch overhead is negligible, both paths run the same sweep
  cli    python -m svx.postprocess.mine_local on the three-pair tree of tests/test_gpu_group_search.py (example_full,
         example_trim, a 10-row document) repeated --cli-copies times: pairs per second, files to files (wall clock)

Per search case three paths are timed in turn within every repetition, each between one pair of HIP events on the current
stream (the loops are host-bound: the events then span the host's time):
  grouped      two FlatIndex.search_groups calls (one per direction)
  loop_cabi    per group and direction one svx_knn_search call straight through the C ABI into preallocated outputs, with
               id_base = db_off[g]: the launches alone
  loop_index   per group and direction an index object over the group's rows and FlatIndex.search: what a caller had to
               write before (two output allocations per call; ids without the group's base)
One JSON line per case: median (min .. max) of every path over the repetitions, the ratios to `grouped`, the loop's per-call
overhead (loop - grouped) / calls, and checksums (the double sum of the similarities and the sum of the ids) which must agree
between `grouped` and `loop_cabi`."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "speech-vecalign_amd"))

CASES = {"many": (1024, 1148, 1035), "big": (4, 16384, 16384)}


def unit_rows(idx_cls, n, d, storage, gen):
    """n random unit rows in the storage type, made 65536 rows at a time."""
    import torch
    idx = idx_cls(d, storage)
    for lo in range(0, n, 65536):
        idx.add(torch.randn(min(65536, n - lo), d, device="cuda", generator=gen))
    return idx


def search_case(a, name):
    import numpy as np
    import torch
    from svx import _lib
    from svx.postprocess.flat_index import FlatIndex
    groups, nx, ny = CASES[name]
    k, d = a.k, a.d
    gen = torch.Generator(device="cuda").manual_seed(0)
    ix, iy = unit_rows(FlatIndex, groups * nx, d, a.storage, gen), unit_rows(FlatIndex, groups * ny, d, a.storage, gen)
    x, y = ix.rows, iy.rows
    x_off, y_off = np.arange(groups + 1, dtype=np.int64) * nx, np.arange(groups + 1, dtype=np.int64) * ny
    ctx = ix.ctx
    ctx.use_current_stream()
    lib, code = ctx.lib, ix.code
    pre = [(torch.empty((r.shape[0], k), dtype=torch.float32, device="cuda"), torch.empty((r.shape[0], k), dtype=torch.int64, device="cuda"))
           for r in (x, y)]
    esz = x.element_size()

    def grouped():
        return [iy.search_groups(x, k, x_off, y_off), ix.search_groups(y, k, y_off, x_off)]

    def loop_cabi():
        for (q, qo), (db, do), (S, I) in (((x, x_off), (y, y_off), pre[0]), ((y, y_off), (x, x_off), pre[1])):
            qp, dp, sp, ip = q.data_ptr(), db.data_ptr(), S.data_ptr(), I.data_ptr()
            for g in range(groups):
                qs, ds = int(qo[g]), int(do[g])
                rc = lib.svx_knn_search(ctx.h, ctypes.c_void_p(qp + qs * d * esz), code, int(qo[g + 1]) - qs, ctypes.c_void_p(dp + ds * d * esz),
                                        code, int(do[g + 1]) - ds, d, k, ds, ctypes.c_void_p(sp + qs * k * 4), ctypes.c_void_p(ip + qs * k * 8), 1)
                if rc:
                    ctx.check(rc)
        return pre

    def loop_index():
        out = []
        for (q, qo), (db, do) in (((x, x_off), (y, y_off)), ((y, y_off), (x, x_off))):
            out.append([FlatIndex.over(db[int(do[g]):int(do[g + 1])]).search(q[int(qo[g]):int(qo[g + 1])], k) for g in range(groups)])
        return out

    def checksum(res):
        return [float(sum(s.double().sum().item() for s, _ in res)), int(sum(i.sum().item() for _, i in res))]

    paths = (("grouped", grouped), ("loop_cabi", loop_cabi), ("loop_index", loop_index))
    sums = {}
    for pname, fn in paths:   # warm-up at full size, and the checksums
        res = fn()
        torch.cuda.synchronize()
        if pname != "loop_index":
            sums[pname] = checksum(res)
        del res
    ms = {pname: [] for pname, _ in paths}
    for _ in range(a.reps):
        for pname, fn in paths:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            res = fn()
            ev[1].record()
            torch.cuda.synchronize()
            ms[pname].append(ev[0].elapsed_time(ev[1]))
            del res
    calls = 2 * groups
    rec = {"op": "svx_knn_search_groups vs a loop of svx_knn_search", "case": name, "groups": groups, "rows": [nx, ny], "d": d, "k": k,
           "storage": a.storage, "reps": a.reps, "loop_calls": calls, "checksums": sums, "checksums_equal": sums["grouped"] == sums["loop_cabi"]}
    for pname in ms:
        v = ms[pname]
        rec[pname] = {"ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)}
    g = rec["grouped"]["ms_median"]
    rec["tflops_grouped"] = round(2.0 * 2 * groups * nx * ny * d / (g * 1e-3) / 1e12, 1)
    for pname in ("loop_cabi", "loop_index"):
        rec[pname + "_over_grouped"] = round(rec[pname]["ms_median"] / g, 3)
        rec[pname + "_overhead_us_per_call"] = round((rec[pname]["ms_median"] - g) * 1e3 / calls, 2)
    rec["grouped_within_loop_spread"] = g <= rec["loop_cabi"]["ms_median"] + (rec["loop_cabi"]["ms_max"] - rec["loop_cabi"]["ms_min"])
    return rec


def cli_case(a):
    import numpy as np
    from svx.postprocess import mine_local
    gd = os.path.join(ROOT, "tests", "golden")
    with tempfile.TemporaryDirectory() as tmp:
        for lang in ("en", "de"):
            os.makedirs(os.path.join(tmp, "cat", lang))
            os.makedirs(os.path.join(tmp, "emb", lang))
        meta, rows = [], 0
        for c in range(a.cli_copies):
            for name, folder, cut in (("full", "example_full", None), ("trim", "example_trim", None), ("tiny", "example_full", 10)):
                stem = "%s%03d" % (name, c)
                for lang in ("en", "de"):
                    emb, cat = os.path.join(gd, folder, "embeds_%s.f16" % lang), os.path.join(gd, folder, "cat_segs_%s.txt" % lang)
                    e_out, c_out = os.path.join(tmp, "emb", lang, "%s_%s.embed" % (stem, lang)), os.path.join(tmp, "cat", lang, "%s_%s.txt" % (stem, lang))
                    if cut is None:   # the golden files under another name
                        os.symlink(emb, e_out)
                        os.symlink(cat, c_out)
                        rows += os.path.getsize(emb) // 2048
                    else:
                        np.fromfile(emb, dtype=np.float16).reshape(-1, 1024)[:cut].tofile(e_out)
                        with open(cat) as f, open(c_out, "w") as o:
                            o.writelines(f.readlines()[:cut])
                        rows += cut
                meta.append("/audio/%s_en.wav\t/audio/%s_de.wav" % (stem, stem))
        with open(os.path.join(tmp, "meta.tsv"), "w") as f:
            f.write("\n".join(meta) + "\n")
        secs, stats = [], {}
        for r in range(a.cli_runs + 1):   # the first run warms up (context, kernels, page cache)
            t0 = time.perf_counter()
            mine_local.main([os.path.join(tmp, "meta.tsv"), os.path.join(tmp, "out%d" % r), "--src_lang", "en", "--tgt_lang", "de", "--concat_dir",
                             os.path.join(tmp, "cat"), "--embed_dir", os.path.join(tmp, "emb"), "--fp16_embed", "--k", str(a.k)], stats=stats)
            if r:
                secs.append(time.perf_counter() - t0)
    med = statistics.median(secs)
    return {"op": "python -m svx.postprocess.mine_local, files to files", "pairs": len(meta), "rows": rows, "k": a.k, "runs": a.cli_runs,
            "mined": stats["mined"], "small": stats["small"], "lines": stats["lines"], "s_median": round(med, 3), "s_min": round(min(secs), 3),
            "s_max": round(max(secs), 3), "pairs_per_s": round(len(meta) / med, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["many", "big", "cli", "all"], default="all")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--storage", default="fp16")
    ap.add_argument("--cli-copies", type=int, default=100)
    ap.add_argument("--cli-runs", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.reps < 9:
        ap.error("--reps: at least 9")
    lines = []
    for name in (("many", "big", "cli") if a.case == "all" else (a.case,)):
        rec = cli_case(a) if name == "cli" else search_case(a, name)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
