"""Randomised parity sweep (not collected by pytest; run by hand on the GPU box):
    python tests/fuzz_gpu_vs_oracle.py --cases 300 --seed 0
Every case draws document sizes, overlap layers, alignment types, band width, pyramid threshold, storage type,
deletions and zero rows, aligns the pair with the HIP pipeline and with the CPU oracle on the same inputs and the
same random stream, and requires identical alignment spans and scores within 1e-4.  Cases run in batches so that
ragged batches are exercised too.

Exact ties: zero rows (PAD / ignored candidates) with equal norms give several alignments the same total cost in
exact arithmetic; the reference itself picks among them by fp64 rounding noise, which no implementation with a
different (equally valid) summation order of the fp32 dot products can reproduce.  Such cases are reported as
"tie" when the two objectives -- evaluated with the oracle's deletion penalty -- agree to 2e-6 per alignment, and
do not count as mismatches.

Percentile knife-edges: with very few sampled scores (n*m below costs_sample_size on tiny documents) a step of the
empirical cdf can coincide with a knot of the percentile map (2/56 == 1/28); which side np.searchsorted falls on is
then decided by the last bit of the scores, and the deletion penalty jumps by a whole inter-sample gap.  The same
happens whenever sample_size * k / 28 is a whole number (500 samples at percentile 0.5: cdf == 0.5 after exactly 250
samples): the histogram's bin width is max(scores) / 1000, and a one-ulp change of the largest score -- the size of
the difference between two summation orders of an fp32 dot product -- moves the rounded cdf across the knot.
A case is counted as a "penalty knife-edge" only when that explanation is CONSTRUCTIVELY verified (knife_edge()):
  (1) at every level whose penalty differs by more than 5e-5, the GPU's own sampled scores (svx_debug_level ->
      knob_scores) are within 2e-6 of the oracle's sampled scores, sample by sample, and numpy's DeletionKnob
      (the oracle's del_penalty_from_scores) applied to the GPU's scores returns the GPU's penalty bit for bit --
      so the penalty kernel and the sample gather are right and the jump is the reference's own discontinuity;
  (2) the oracle re-run with the GPU's penalties injected (same random stream) gives the GPU's spans, and scores
      within 1e-4 (or an exact tie by objective) -- so everything downstream of the estimate is right too.
Anything else with differing penalties is a MISMATCH.

--search straight runs the same comparison for SVX_SEARCH_STRAIGHT (narrow bands, the tile sweep, and bands that
cover the whole lattice) against make_sparse_costs / sparse_dp / sparse_traceback on the straight path."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "speech-vecalign_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


PEN_TOL, KS_TOL = 5e-5, 2e-6


def knife_edge(oracle, gpu_pens, ref_pens, gpu_scores_of, ref_scores_of, frac):
    """Condition (1) of the module docstring for every level whose penalties differ.  gpu_scores_of(depth) /
    ref_scores_of(depth) -> float32 sampled scores.  -> (ok, text)"""
    notes = []
    for depth, (gp, rp) in enumerate(zip(gpu_pens, ref_pens)):
        if abs(float(gp) - float(rp)) <= PEN_TOL:
            continue
        gs, rsc = np.asarray(gpu_scores_of(depth), np.float32), np.asarray(ref_scores_of(depth), np.float32)
        if gs.shape != rsc.shape:
            return False, "level %d: %d sampled scores on the GPU, %d in the oracle" % (depth, gs.size, rsc.size)
        worst = float(np.abs(gs.astype(np.float64) - rsc.astype(np.float64)).max())
        if not worst <= KS_TOL:
            return False, "level %d: sampled scores differ by %.3g" % (depth, worst)
        want = oracle.del_penalty_from_scores(gs, 0, max(gs), frac)
        if float(want) != float(gp):
            return False, "level %d: DeletionKnob(GPU scores) = %.17g, GPU penalty = %.17g" % (depth, float(want), float(gp))
        notes.append("level %d: scores within %.1e, DeletionKnob(GPU scores) == GPU penalty" % (depth, worst))
    return True, "; ".join(notes)


DIMS, STRAIGHT_DIMS, STORES = (32, 64, 256), (32, 64, 96, 256), ("f32", "bf16", "f16")


def store_round(v, store):
    from synth import round_bf16
    if store == "bf16":
        return round_bf16(v)
    if store == "f16":
        return v.astype(np.float16).astype(np.float32)
    return v


def to_devs(hosts, store):
    import torch
    cast = {"bf16": lambda t: t.bfloat16(), "f16": lambda t: t.half(), "f32": lambda t: t}[str(store)]
    return [(cast(torch.from_numpy(a).cuda()), cast(torch.from_numpy(b).cuda())) for a, b in hosts]


def draw_batches(cases, seed, batch=8, max_size=900, dims=DIMS, stores=STORES, zero_rows=3, k4_weight=0.0):
    """The sweep's cases, one configuration per batch (types / W / thresholds are batch-wide parameters), sizes vary
    inside it.  Yields (config dict, [(v0, v1) storage-rounded float32], [per-pair RandomState seeds]).  The defaults
    consume the RandomState exactly as the sweep always did (test_randomised_sweep_small: 160 cases, seed 11).
    zero_rows: most zero rows per document; k4_weight: share of batches forced to K = 4 / -a 5 (the benchmark's)."""
    from synth import alignment_types, make_pair
    rs = np.random.RandomState(seed)
    done = 0
    while done < cases:
        K = int(rs.randint(1, 6))
        amax = int(rs.randint(2, K + 2))
        if k4_weight and rs.rand() < k4_weight:
            K, amax = 4, 5
        types = alignment_types(amax)
        W = int(rs.randint(3, 12))
        max_full = int(rs.choice([40, 100, 300]))
        sample = int(rs.choice([500, 5000, 20000]))
        nsamp = int(rs.choice([0, 7, 100]))
        frac = float(rs.choice([0.05, 0.2, 0.5]))
        d = int(rs.choice(list(dims)))
        store = rs.choice(list(stores))
        nb = min(batch, cases - done)
        hosts = []
        for i in range(nb):
            n, m = int(rs.randint(1, max_size)), int(rs.randint(1, max_size))
            if rs.rand() < 0.15:
                n, m = int(rs.randint(1, 12)), int(rs.randint(1, 12))
            v0, v1 = make_pair(n, m, K, d, int(rs.randint(1 << 30)), deletions=int(rs.randint(0, 6)) if min(n, m) > 12 else 0,
                               zero_rows=int(rs.randint(0, zero_rows + 1)))
            hosts.append((store_round(v0, store), store_round(v1, store)))
        seeds = [int(rs.randint(1 << 30)) for _ in range(nb)]
        yield dict(K=K, amax=amax, types=types, W=W, max_full=max_full, sample=sample, nsamp=nsamp, frac=frac, d=d, store=str(store)), hosts, seeds
        done += nb


def _oracle_job(args):
    """One oracle.vecalign call in a worker process (never touches the GPU); only what the sweep reads comes back."""
    import oracle
    v0, v1, types, frac, W, max_full, sample, nsamp, seed = args
    try:
        ref = oracle.vecalign(v0, v1, types, frac, W, max_full, sample, nsamp, rng=np.random.RandomState(seed))
    except Exception as e:
        return e
    return {dd: {k: ref[dd][k] for k in ('final_alignments', 'alignment_scores', 'del_penalty', 'knob_scores') if k in ref[dd]}
            for dd in ref}


def oracle_pool(workers):
    """Pool for the oracle side of a sweep (spawn: the workers must not inherit an initialised HIP runtime)."""
    import multiprocessing
    return multiprocessing.get_context("spawn").Pool(min(int(workers), 16)) if workers else None


def run_sweep(cases, seed, batch=8, verbose=True, max_size=900, dims=DIMS, stores=STORES, zero_rows=3, k4_weight=0.0, workers=0):
    """-> (mismatches, exact ties, penalty knife-edges).  workers > 0: the oracle's calls of a batch run in that many
    processes (d = 1024 documents take seconds each)."""
    import oracle
    from svx.vecalign import dp_utils
    t0 = time.time()
    done = bad = ties = edges = 0
    pool = oracle_pool(workers)
    for cfg, hosts, seeds in draw_batches(cases, seed, batch, max_size, dims, stores, zero_rows, k4_weight):
        K, amax, types, W, max_full, sample = cfg['K'], cfg['amax'], cfg['types'], cfg['W'], cfg['max_full'], cfg['sample']
        nsamp, frac, d, store = cfg['nsamp'], cfg['frac'], cfg['d'], cfg['store']
        nb = len(hosts)
        devs = to_devs(hosts, store)
        refs = pool.map_async(_oracle_job, [(hosts[i][0], hosts[i][1], types, frac, W, max_full, sample, nsamp, seeds[i])
                                            for i in range(nb)]) if pool else None
        pb = None
        try:
            pb = dp_utils.PreparedBatch(devs, types, frac, W, max_full, sample, nsamp, rngs=[np.random.RandomState(s) for s in seeds])
            pb.run()
            res = pb.results()
        except Exception as e:  # an error must be an error on both sides
            res = e
        if pool:
            refs = refs.get()
        for i in range(nb):
            if pool:
                ref = refs[i]
            else:
                try:
                    ref = oracle.vecalign(hosts[i][0].copy(), hosts[i][1].copy(), types, frac, W, max_full, sample, nsamp,
                                          rng=np.random.RandomState(seeds[i]))
                except Exception as e:
                    ref = e
            ok = False
            if isinstance(res, Exception) or isinstance(ref, Exception):
                ok = isinstance(res, Exception) and isinstance(ref, Exception)
            else:
                al, sc = res[i][0], res[i][1]
                ok = al == ref[0]['final_alignments'] and (len(sc) == 0 or np.abs(np.asarray(sc) - ref[0]['alignment_scores']).max() < 1e-4)
            if not ok and not isinstance(res, Exception) and not isinstance(ref, Exception):
                al, sc, pens = res[i]
                ra, rsc = ref[0]['final_alignments'], ref[0]['alignment_scores']
                pen = ref[0]['del_penalty']

                def objective(alg, scores):
                    return sum(c * len(x) * len(y) if (x and y) else pen * (len(x) + len(y)) for (x, y), c in zip(alg, scores))
                cover = [v for x, _ in al for v in x] == list(range(hosts[i][0].shape[1])) and \
                    [v for _, y in al for v in y] == list(range(hosts[i][1].shape[1]))
                if cover and abs(objective(al, sc) - objective(ra, rsc)) < 2e-6 * max(len(al), len(ra)):
                    ties += 1
                    ok = True
                elif cover and max(abs(float(g) - float(ref[dd]['del_penalty'])) for g, dd in zip(pens, sorted(ref))) > PEN_TOL:
                    rpens = [float(ref[dd]['del_penalty']) for dd in sorted(ref)]
                    good, why = knife_edge(oracle, pens, rpens, lambda dd: pb.level_stack(i, dd)['knob_scores'],
                                           lambda dd: ref[dd]['knob_scores'], frac)
                    if good:  # (2): the oracle with the GPU's penalties, same random stream
                        ref2 = oracle.vecalign(hosts[i][0].copy(), hosts[i][1].copy(), types, frac, W, max_full, sample, nsamp,
                                               rng=np.random.RandomState(seeds[i]), del_penalties={dd: float(g) for dd, g in enumerate(pens)})
                        pen2 = ref2[0]['del_penalty']
                        ra2, rs2 = ref2[0]['final_alignments'], ref2[0]['alignment_scores']
                        obj2 = lambda alg, scores: sum(c * len(x) * len(y) if (x and y) else pen2 * (len(x) + len(y)) for (x, y), c in zip(alg, scores))
                        same = al == ra2 and (len(sc) == 0 or np.abs(np.asarray(sc) - rs2).max() < 1e-4)
                        tie2 = abs(obj2(al, sc) - obj2(ra2, rs2)) < 2e-6 * max(len(al), len(ra2))
                        good = same or tie2
                        why += "; oracle with the GPU's penalties: " + ("same spans and scores" if same else ("exact tie" if tie2 else "DIFFERENT RESULT"))
                    if good:
                        edges += 1
                        ok = True
                    print("penalty knife-edge" if good else "penalty differs, NOT a knife-edge:",
                          dict(n=hosts[i][0].shape[1], m=hosts[i][1].shape[1], sample=sample, frac=frac, store=str(store)),
                          [float(g) for g in pens], rpens, "|", why, flush=True)
            if not ok:
                bad += 1
                print("MISMATCH", dict(K=K, amax=amax, W=W, max_full=max_full, sample=sample, nsamp=nsamp, frac=frac, d=d, store=str(store),
                                       n=hosts[i][0].shape[1], m=hosts[i][1].shape[1], seed=seeds[i]),
                      repr(res)[:200] if isinstance(res, Exception) else "", repr(ref)[:200] if isinstance(ref, Exception) else "", flush=True)
                if not isinstance(res, Exception) and not isinstance(ref, Exception):
                    print("  gpu", res[i][0], [round(float(v), 7) for v in res[i][1]], [float(v) for v in res[i][2]])
                    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
                    np.savez(os.path.join(ROOT, "gpurun_out", "fuzz_case_%d.npz" % seeds[i]), v0=hosts[i][0], v1=hosts[i][1])
                    print("  ref", ref[0]['final_alignments'], [round(float(v), 7) for v in ref[0]['alignment_scores']],
                          [float(ref[dd]['del_penalty']) for dd in sorted(ref)], flush=True)
        done += nb
        if verbose and (done // nb) % 10 == 0:
            print(f"{done} cases, {bad} mismatches, {ties} exact ties, {edges} penalty knife-edges, {time.time() - t0:.0f} s", flush=True)
    if pool:
        pool.terminate()
        pool.join()
    print(f"fuzz: {done} cases, {bad} mismatches, {ties} exact ties, {edges} penalty knife-edges, {time.time() - t0:.0f} s")
    return bad, ties, edges


def straight_oracle(orc, v0, v1, types, W, frac, sample, nsamp, seed, pen_override=None):
    """make_sparse_costs + sparse_dp + sparse_traceback on the straight path with depth-0 norms and penalty.
    -> (alignments, scores, estimated penalty, sampled scores); pen_override replaces the estimate in the DP."""
    N, M = v0.shape[1], v1.shape[1]
    a, b = v0.copy(), v1.copy()
    orc.make_norm1(a)
    orc.make_norm1(b)
    rs = np.random.RandomState(seed)
    n0, n1 = orc.compute_norms(a, b, nsamp, rs), orc.compute_norms(b, a, nsamp, rs)
    pen, ks = orc.make_del_penalty(a[0], b[0], n0[0], n1[0], sample, frac, rs)
    path = orc.search_path([(list(range(N)), list(range(M)))], False, N, M)
    f, bo = orc.make_sparse_costs(a, b, n0, n1, path, types, W)
    al, sc = orc.sparse_traceback(*orc.sparse_dp(f, bo, types, pen if pen_override is None else pen_override, N, M), N, M)
    return al, sc, pen, ks


def run_straight_sweep(cases, seed, batch=6, verbose=True, max_size=500, dims=STRAIGHT_DIMS, stores=STORES, zero_rows=2):
    """SVX_SEARCH_STRAIGHT (band around the straight diagonal; wide bands run the tile sweep, bands that cover the
    lattice are the dense mode) against the oracle on the same straight path.  -> (mismatches, exact ties)"""
    import torch
    import oracle
    from synth import alignment_types, make_pair, round_bf16
    from svx.vecalign import dp_utils
    rs = np.random.RandomState(seed)
    t0 = time.time()
    done = bad = ties = errs = edges = 0
    nbatch = 0
    while done < cases:
        K = int(rs.randint(1, 6))
        amax = int(rs.randint(2, K + 2))
        types = alignment_types(amax)
        W = int(rs.choice([rs.randint(3, 33), rs.randint(33, 70), rs.randint(70, 160), max_size + 1]))
        sample = int(rs.choice([500, 5000, 20000]))
        nsamp = int(rs.choice([7, 100]))
        frac = float(rs.choice([0.05, 0.2, 0.5]))
        d = int(rs.choice(list(dims)))
        store = rs.choice(list(stores))
        nb = min(batch, cases - done)
        hosts, devs = [], []
        for i in range(nb):
            n, m = int(rs.randint(1, max_size)), int(rs.randint(1, max_size))
            if rs.rand() < 0.1:
                n, m = int(rs.randint(1, 12)), int(rs.randint(1, 12))
            v0, v1 = make_pair(n, m, K, d, int(rs.randint(1 << 30)), deletions=int(rs.randint(0, 6)) if min(n, m) > 12 else 0,
                               zero_rows=int(rs.randint(0, zero_rows + 1)))
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
        pb = None
        try:
            pb = dp_utils.PreparedBatch(devs, types, frac, W, 1 << 30, sample, nsamp, rngs=[np.random.RandomState(s) for s in seeds],
                                        search="straight")
            pb.run()
            res = pb.results()
        except Exception as e:
            res = e
        for i in range(nb):
            try:
                ref = straight_oracle(oracle, hosts[i][0], hosts[i][1], types, W, frac, sample, nsamp, seeds[i])
            except Exception as e:
                ref = e
            if isinstance(res, Exception) or isinstance(ref, Exception):
                ok = isinstance(res, Exception) and isinstance(ref, Exception)
                errs += 1
                if errs <= 3:
                    print("both sides raised:" if ok else "one side raised:", repr(res)[:160], "|", repr(ref)[:160], flush=True)
            else:
                al, sc = res[i][0], np.asarray(res[i][1])
                ok = al == ref[0] and (len(sc) == 0 or np.abs(sc - ref[1]).max() < 1e-4)
                if not ok:
                    pen = ref[2]

                    def objective(alg, scores):
                        return sum(c * len(x) * len(y) if (x and y) else pen * (len(x) + len(y)) for (x, y), c in zip(alg, scores))
                    cover = [v for x, _ in al for v in x] == list(range(hosts[i][0].shape[1])) and \
                        [v for _, y in al for v in y] == list(range(hosts[i][1].shape[1]))
                    if cover and abs(objective(al, sc) - objective(ref[0], ref[1])) < 2e-6 * max(len(al), len(ref[0])):
                        ties += 1
                        ok = True
                    elif cover and abs(float(res[i][2][0]) - float(pen)) > PEN_TOL:
                        gpen = float(res[i][2][0])
                        good, why = knife_edge(oracle, [gpen], [float(pen)], lambda dd: pb.level_stack(i, 0)['knob_scores'], lambda dd: ref[3], frac)
                        if good:
                            ref2 = straight_oracle(oracle, hosts[i][0], hosts[i][1], types, W, frac, sample, nsamp, seeds[i], pen_override=gpen)
                            obj2 = lambda alg, scores: sum(c * len(x) * len(y) if (x and y) else gpen * (len(x) + len(y)) for (x, y), c in zip(alg, scores))
                            same = al == ref2[0] and (len(sc) == 0 or np.abs(sc - ref2[1]).max() < 1e-4)
                            tie2 = abs(obj2(al, sc) - obj2(ref2[0], ref2[1])) < 2e-6 * max(len(al), len(ref2[0]))
                            good = same or tie2
                            why += "; oracle with the GPU's penalty: " + ("same spans and scores" if same else ("exact tie" if tie2 else "DIFFERENT RESULT"))
                        if good:
                            edges += 1
                            ok = True
                        print("penalty knife-edge" if good else "penalty differs, NOT a knife-edge:",
                              dict(n=hosts[i][0].shape[1], m=hosts[i][1].shape[1], sample=sample, frac=frac, store=str(store)),
                              gpen, float(pen), "|", why, flush=True)
            if not ok:
                bad += 1
                print("MISMATCH straight", dict(K=K, amax=amax, W=W, sample=sample, nsamp=nsamp, frac=frac, d=d, store=str(store),
                                                n=hosts[i][0].shape[1], m=hosts[i][1].shape[1], seed=seeds[i]),
                      repr(res)[:200] if isinstance(res, Exception) else "", repr(ref)[:200] if isinstance(ref, Exception) else "", flush=True)
                if not isinstance(res, Exception) and not isinstance(ref, Exception):
                    ga, ra = res[i][0], ref[0]
                    k = next((j for j in range(min(len(ga), len(ra))) if ga[j] != ra[j]), min(len(ga), len(ra)))
                    print("  first difference at alignment", k, "gpu", ga[max(0, k - 2):k + 4], "ref", ra[max(0, k - 2):k + 4])
                    print("  gpu scores", [round(float(v), 6) for v in res[i][1][max(0, k - 2):k + 4]], "ref", [round(float(v), 6) for v in ref[1][max(0, k - 2):k + 4]],
                          "pen gpu", [float(v) for v in res[i][2]], "ref", float(ref[2]), flush=True)
                    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
                    np.savez(os.path.join(ROOT, "gpurun_out", "fuzz_straight_%d.npz" % seeds[i]), v0=hosts[i][0], v1=hosts[i][1])
        done += nb
        nbatch += 1
        if verbose and nbatch % 10 == 0:
            print(f"{done} cases, {bad} mismatches, {ties} exact ties, {edges} penalty knife-edges, {errs} raised, {time.time() - t0:.0f} s", flush=True)
    print(f"fuzz straight: {done} cases, {bad} mismatches, {ties} exact ties, {edges} penalty knife-edges, {errs} raised on both sides, {time.time() - t0:.0f} s")
    return bad, ties


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--search", default="ref", choices=["ref", "straight"], help="ref: coarse-to-fine; straight: the straight band")
    ap.add_argument("--cases", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--max_size", type=int, default=900, help="documents have 1 .. max_size-1 segments")
    ap.add_argument("--pipeline", action="store_true", help="run the device side with the software pipeline on (svx_set_pipeline)")
    ap.add_argument("--dims", default="", help="embedding widths to draw from, e.g. 512,1024 (default: the small widths)")
    ap.add_argument("--stores", default="", help="storage types to draw from, e.g. bf16,f16")
    ap.add_argument("--zero_rows", type=int, default=-1, help="most zero rows per document (default: 3, straight: 2)")
    ap.add_argument("--k4_weight", type=float, default=0.0, help="share of batches forced to K = 4 / -a 5")
    ap.add_argument("--workers", type=int, default=0, help="processes for the oracle side (coarse-to-fine sweep)")
    a = ap.parse_args()
    kw = {}
    if a.dims:
        kw["dims"] = tuple(int(v) for v in a.dims.split(","))
    if a.stores:
        kw["stores"] = tuple(a.stores.split(","))
    if a.zero_rows >= 0:
        kw["zero_rows"] = a.zero_rows
    if a.pipeline:
        from svx import _lib
        _lib.context().set_pipeline(True)
    if a.search == "straight":
        bad, _ = run_straight_sweep(a.cases, a.seed, min(a.batch, 6), max_size=a.max_size, **kw)
        sys.exit(1 if bad else 0)
    bad, _, _ = run_sweep(a.cases, a.seed, a.batch, max_size=a.max_size, k4_weight=a.k4_weight, workers=a.workers, **kw)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
