"""Randomised parity sweep of straight search with the type sets of the general tile shape (not collected by pytest;
a 24-case slice runs in tests/test_gpu_straight_types_sweep.py):
    python tests/fuzz_straight_types.py --cases 500 --seed 0
Every case draws -a 7..16 or --many_to_one 9..100, a band of 33 cells up to the dense mode, the storage type,
deletions and zero rows, aligns a batch of pairs with SVX_SEARCH_STRAIGHT and compares each pair with the oracle's
make_sparse_costs / sparse_dp / sparse_traceback on the same straight path: identical spans, scores within 1e-4.
Exact ties (zero rows with equal norms: several alignments of the same total cost) and penalty knife-edges are
counted separately, by the rules of tests/fuzz_gpu_vs_oracle.py."""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "speech-vecalign_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def draw_types(rs):
    """-> (types, x layers, y layers, label)"""
    from synth import alignment_types
    from svx.vecalign.vecalign import resolve_search_params
    if rs.rand() < 0.5:
        a = int(rs.randint(7, 17))
        return alignment_types(a), a - 1, a - 1, "-a %d" % a
    m = int(rs.randint(9, 101))
    types, sk, tk, _ = resolve_search_params(10, m, 5)
    return types, sk, tk, "--many_to_one %d" % m


def run(cases, seed, batch=3, max_size=260, verbose=True):
    """-> (mismatches, exact ties, penalty knife-edges)"""
    import torch
    import oracle
    from fuzz_gpu_vs_oracle import PEN_TOL, knife_edge, straight_oracle
    from synth import make_pair, round_bf16
    from svx.vecalign import dp_utils
    rs = np.random.RandomState(seed)
    t0 = time.time()
    done = bad = ties = edges = 0
    while done < cases:
        types, kx, ky, label = draw_types(rs)
        W = int(rs.choice([rs.randint(33, 70), rs.randint(70, 160), max_size + 1]))
        sample = int(rs.choice([5000, 20000]))
        nsamp = int(rs.choice([7, 100]))
        frac = 0.2
        d = int(rs.choice([32, 64, 96]))
        store = str(rs.choice(["f32", "bf16", "f16"]))
        nb = min(batch, cases - done)
        hosts, devs = [], []
        for i in range(nb):
            n, m = int(rs.randint(1, max_size)), int(rs.randint(1, max_size))
            v0, v1 = make_pair(n, m, max(kx, ky), d, int(rs.randint(1 << 30)), deletions=int(rs.randint(0, 6)) if min(n, m) > 12 else 0,
                               zero_rows=int(rs.randint(0, 3)))
            v0, v1 = np.ascontiguousarray(v0[:kx]), np.ascontiguousarray(v1[:ky])
            if store == "bf16":
                v0, v1 = round_bf16(v0), round_bf16(v1)
                devs.append((torch.from_numpy(v0).cuda().bfloat16(), torch.from_numpy(v1).cuda().bfloat16()))
            elif store == "f16":
                v0, v1 = v0.astype(np.float16).astype(np.float32), v1.astype(np.float16).astype(np.float32)
                devs.append((torch.from_numpy(v0).cuda().half(), torch.from_numpy(v1).cuda().half()))
            else:
                devs.append((torch.from_numpy(v0).cuda(), torch.from_numpy(v1).cuda()))
            hosts.append((v0, v1))
        seeds = [int(rs.randint(1 << 30)) for _ in range(nb)]
        pb = dp_utils.PreparedBatch(devs, types, frac, W, 1 << 30, sample, nsamp, rngs=[np.random.RandomState(s) for s in seeds],
                                    search="straight")
        pb.run()
        res = pb.results()
        for i in range(nb):
            ref = straight_oracle(oracle, hosts[i][0], hosts[i][1], types, W, frac, sample, nsamp, seeds[i])
            al, sc = res[i][0], np.asarray(res[i][1])
            ok = al == ref[0] and (len(sc) == 0 or np.abs(sc - ref[1]).max() < 1e-4)
            why = ""
            if not ok:
                pen = ref[2]

                def objective(alg, scores, p):
                    return sum(c * len(x) * len(y) if (x and y) else p * (len(x) + len(y)) for (x, y), c in zip(alg, scores))
                cover = [v for x, _ in al for v in x] == list(range(hosts[i][0].shape[1])) and \
                    [v for _, y in al for v in y] == list(range(hosts[i][1].shape[1]))
                if cover and abs(objective(al, sc, pen) - objective(ref[0], ref[1], pen)) < 2e-6 * max(len(al), len(ref[0])):
                    ties += 1
                    ok = True
                    why = "exact tie"
                elif cover and abs(float(res[i][2][0]) - float(pen)) > PEN_TOL:
                    gpen = float(res[i][2][0])
                    good, why = knife_edge(oracle, [gpen], [float(pen)], lambda dd: pb.level_stack(i, 0)['knob_scores'], lambda dd: ref[3], frac)
                    if good:
                        ref2 = straight_oracle(oracle, hosts[i][0], hosts[i][1], types, W, frac, sample, nsamp, seeds[i], pen_override=gpen)
                        same = al == ref2[0] and (len(sc) == 0 or np.abs(sc - ref2[1]).max() < 1e-4)
                        tie2 = abs(objective(al, sc, gpen) - objective(ref2[0], ref2[1], gpen)) < 2e-6 * max(len(al), len(ref2[0]))
                        good = same or tie2
                    if good:
                        edges += 1
                        ok = True
            if not ok:
                bad += 1
            if verbose and (not ok or why):
                print(f"case {done + i}: {label} W={W} {store} d={d} n={hosts[i][0].shape[1]} m={hosts[i][1].shape[1]}: "
                      f"{'MISMATCH' if not ok else why}", flush=True)
        done += nb
        if verbose and done % 60 < nb:
            print(f"{done} cases, {bad} mismatches, {ties} exact ties, {edges} penalty knife-edges, {time.time() - t0:.0f} s", flush=True)
    if verbose:
        print(f"fuzz straight types: {done} cases, {bad} mismatches, {ties} exact ties, {edges} penalty knife-edges, "
              f"{time.time() - t0:.0f} s", flush=True)
    return bad, ties, edges


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=500)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-size", type=int, default=260)
    a = ap.parse_args()
    nbad, _, _ = run(a.cases, a.seed, max_size=a.max_size)
    sys.exit(1 if nbad else 0)
