"""Timing of the id-returning search (svx_knn_search) beside svx_knn_mean_sim -- not the headline bench (bench.py).

python profiles/search_bench.py --parent-lib PATH [--n 131072] [--db 131072] [--d 1024] [--ks 16,64] [--rounds 3] [--reps 3] [--out FILE]

PATH is a libsvx.so built from the parent commit (profiles/build_variant.sh shows how A/B builds are selected with SVX_LIB).
Every round starts four fresh processes in turn -- mean_sim on the parent library, then mean_sim, search and one continued
merge_search sweep on this tree's library -- so the two builds alternate within one run; a process times every k after a warm-up, `reps`
times each, one pair of HIP events per repetition.  Per k one JSON line: the median and the min..max of each figure over
all rounds and repetitions, the ratio search / parent mean_sim, and TFLOP/s (2 n N d flops) against the dense fp16 MFMA peak
as the kernel's share of peak."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "speech-vecalign_amd"))
PEAK = 2500.0


def worker(a):
    import torch
    from svx import _lib
    from svx.postprocess.flat_index import FlatIndex
    if a.worker == "mean_sim" and os.environ.get("SVX_LIB"):
        _lib._SIGS.pop("svx_knn_search", None)   # a build of the parent commit does not export it
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(a.n, a.d, device="cuda", generator=g)
    idx = FlatIndex(a.d, a.storage)
    idx.add(torch.randn(a.db, a.d, device="cuda", generator=g))
    idx.ctx.use_current_stream()
    res = {}
    for k in a.ks:
        if a.worker == "mean_sim":
            run = lambda: idx.mean_sim(q, k)
        elif a.worker == "search":
            run = lambda: idx.search(q, k)[0]
        else:   # a continued sweep (first = 0: ties compared by id) over the same rows under new ids
            state = idx.merge_search(q, k)
            run = lambda: idx.merge_search(q, k, state, id_base=a.db)[0]
        out = run()   # warm-up at full size
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            out = run()
            ev[1].record()
            torch.cuda.synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        res[str(k)] = {"ms": ms, "checksum": float(out.double().sum().item())}
    print("RESULT " + json.dumps(res), flush=True)


def child(a, op, lib):
    env = dict(os.environ)
    if lib:
        env["SVX_LIB"] = os.path.abspath(lib)
    else:
        env.pop("SVX_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", op, "--n", str(a.n), "--db", str(a.db), "--d", str(a.d),
           "--ks", ",".join(map(str, a.ks)), "--reps", str(a.reps), "--storage", a.storage]
    out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=a.child_timeout).stdout
    line = [t for t in out.splitlines() if t.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--db", type=int, default=131072)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--ks", type=lambda s: [int(v) for v in s.split(",")], default=[16, 64])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--storage", default="fp16")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out")
    ap.add_argument("--worker", choices=["mean_sim", "search", "merge_search"])
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        ap.error("--parent-lib: a libsvx.so built from the parent commit")
    figures = (("mean_sim_parent", "mean_sim", a.parent_lib), ("mean_sim_change", "mean_sim", None), ("search_change", "search", None),
               ("merge_search_continued", "merge_search", None))
    ms = {name: {k: [] for k in a.ks} for name, _, _ in figures}
    sums = {name: {} for name, _, _ in figures}
    for r in range(a.rounds):
        for name, op, lib in figures:
            res = child(a, op, lib)
            for k in a.ks:
                ms[name][k] += res[str(k)]["ms"]
                sums[name][k] = res[str(k)]["checksum"]
            print("round %d %s: %s" % (r, name, {k: [round(v, 2) for v in res[str(k)]["ms"]] for k in a.ks}), flush=True)
    lines = []
    for k in a.ks:
        rec = {"op": "svx_knn_search vs svx_knn_mean_sim", "n": a.n, "db": a.db, "d": a.d, "k": k, "storage": a.storage,
               "rounds": a.rounds, "reps": a.reps, "mfma_peak_tflops": PEAK}
        for name in ms:
            v = ms[name][k]
            med = statistics.median(v)
            tf = 2.0 * a.n * a.db * a.d / (med * 1e-3) / 1e12
            rec[name] = {"ms_median": round(med, 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3), "tflops": round(tf, 1),
                         "share_of_peak": round(tf / PEAK, 4), "checksum": sums[name][k]}
        rec["mean_sim_change_over_parent"] = round(rec["mean_sim_change"]["ms_median"] / rec["mean_sim_parent"]["ms_median"], 4)
        rec["search_over_parent_mean_sim"] = round(rec["search_change"]["ms_median"] / rec["mean_sim_parent"]["ms_median"], 4)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
