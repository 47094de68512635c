"""Stage-by-stage comparison of the fused HIP pipeline (PreparedBatch.level_stack) with the oracle's stack and with
the float64 restatement (stage_ref.py).  Shared by test_gpu_stage_matrix.py, test_gpu_chunk_edges.py,
test_gpu_band_generations.py and test_gpu_example_stages.py; TEST INFRASTRUCTURE.

The rule for every continuous stage (n0, n1, the levels' normalised layer 0, finite band costs, dense costs, sampled
scores): with E_gpu = max |gpu - f64| and E_orc = max |oracle - f64| on the same cells,

        E_gpu <= max(2 * E_orc, 4 * 2^-24 * max |f64|).

The oracle sums its fp32 dot products sequentially; matrix-core and tree summation have a smaller error bound, so an
honest kernel is no further from the truth than the oracle, and the factor 2 lets an equally valid order land on the
other side of the truth.  The floor covers widths where the chain error vanishes and only the final fp32 roundings of
the two sides differ.  Neither number is fitted to what the kernels produce.

The CPU side (oracle + float64 chain) of a pair runs in a pool of processes that never touch the GPU (spawn)."""
import multiprocessing
import os

import numpy as np

from fuzz_gpu_vs_oracle import store_round as round_store, to_devs

U = 2.0 ** -24
FRAC, MAX_FULL, SAMPLE, NSAMP = 0.2, 300, 20000, 100
SCORE_TOL, PEN_TOL, FLIP_CAP = 1e-4, 5e-5, 1e-3
CONTINUOUS = ('n0', 'n1', 'v0_layer0', 'v1_layer0', 'a_b_costs', 'costs_1to1', 'knob_scores')


def host_pair(job):
    """The storage-rounded float32 embeddings of a job: synthetic (make_pair) unless the job carries arrays."""
    if 'v0' in job:
        return job['v0'], job['v1']
    from synth import make_pair
    v0, v1 = make_pair(job['n'], job['m'], max(job['k0'], job['k1']), job['d'], job['data_seed'], common=job.get('common', 0.0),
                       zero_rows=job.get('zero_rows', 0), deletions=job.get('deletions', 0))
    return (round_store(np.ascontiguousarray(v0[:job['k0']]), job['store']),
            round_store(np.ascontiguousarray(v1[:job['k1']]), job['store']))


def cpu_reference(job):
    """One pair on the CPU: the oracle's stack and the float64 chain on the oracle's discrete choices.
    -> (oracle stack without the embeddings (levels >= 1 keep layer 0), float64 stages)"""
    import oracle
    import stage_ref
    v0, v1 = host_pair(job)
    p = job['params']
    ref = oracle.vecalign(v0.copy(), v1.copy(), job['types'], p['frac'], job['W'], p['max_full'], p['sample'], p['nsamp'],
                          rng=np.random.RandomState(job['seed']))
    draws = stage_ref.replay_draws(oracle, job['seed'], v0.shape[1], v1.shape[1], v0.shape[0], v1.shape[0],
                                   p['max_full'], p['sample'], p['nsamp'])
    f64 = stage_ref.stack(v0, v1, job['types'], job['W'], draws, ref)
    out_ref, out_f64 = {}, {}
    for depth in ref:
        st = dict(ref[depth])
        a, b = st.pop('v0'), st.pop('v1')
        if depth >= 1:
            st['v0_layer0'], st['v1_layer0'] = a[0].copy(), b[0].copy()
        out_ref[depth] = st
        g = dict(f64[depth])
        a, b = g.pop('v0'), g.pop('v1')
        if depth >= 1:
            g['v0_layer0'], g['v1_layer0'] = a[0].copy(), b[0].copy()
        out_f64[depth] = g
    return out_ref, out_f64


class RefPool:
    """cpu_reference() for the pairs of many cases, a few cases ahead of the consumer (the results are large)."""

    def __init__(self, workers=12, ahead=3):
        self.pool = multiprocessing.get_context("spawn").Pool(min(workers, 16))
        self.ahead, self.order, self.pending = ahead, [], {}

    def plan(self, keyed_jobs):
        """keyed_jobs: [(key, [job, ...])] in the order they will be asked for."""
        self.order = list(keyed_jobs)

    def _submit(self, key, jobs):
        if key not in self.pending:
            self.pending[key] = [self.pool.apply_async(cpu_reference, (j,)) for j in jobs]

    def get(self, key, jobs):
        self._submit(key, jobs)
        keys = [k for k, _ in self.order]
        if key in keys:
            at = keys.index(key)
            for k, js in self.order[at + 1:at + 1 + self.ahead]:
                self._submit(k, js)
        return [r.get() for r in self.pending.pop(key)]

    def close(self):
        self.pool.terminate()
        self.pool.join()


def run_gpu(jobs, search="coarse_to_fine"):
    """One svx_align_batch call over the jobs' pairs -> (PreparedBatch, results, per-pair list of level stacks)."""
    from svx.vecalign import dp_utils
    hosts = [host_pair(j) for j in jobs]
    j0 = jobs[0]
    p = j0['params']
    devs = to_devs(hosts, j0['store'])
    pb = dp_utils.PreparedBatch(devs, j0['types'], p['frac'], j0['W'], p['max_full'], p['sample'], p['nsamp'],
                                rngs=[np.random.RandomState(j['seed']) for j in jobs], search=search)
    pb.run()
    res = pb.results()
    stacks = [[pb.level_stack(i, depth) for depth in range(pb.levels[i])] for i in range(len(jobs))]
    return pb, res, stacks


def stage_error(gpu, orc, f64):
    """-> (E_gpu, E_orc, bound, n) over the cells that are finite in the float64 stage."""
    f64 = np.asarray(f64, np.float64)
    fin = np.isfinite(f64)
    t = f64[fin]
    if t.size == 0:
        return 0.0, 0.0, 0.0, 0
    e_gpu = float(np.abs(np.asarray(gpu, np.float64)[fin] - t).max())
    e_orc = float(np.abs(np.asarray(orc, np.float64)[fin] - t).max())
    return e_gpu, e_orc, max(2.0 * e_orc, 4.0 * U * float(np.abs(t).max())), int(t.size)


def check_continuous(got, ref, f64, label, records=None, stages=CONTINUOUS):
    """The rule of the module docstring for every continuous stage of every depth.  -> list of failure texts.
    records (optional list) receives one dict per (stage, depth)."""
    fails = []
    for depth in sorted(ref):
        for name in stages:
            if name not in f64[depth]:
                continue
            if got[depth].get(name) is None:
                fails.append("%s depth %d: the GPU stack has no %s" % (label, depth, name))
                continue
            g, o, t = got[depth][name], ref[depth][name], f64[depth][name]
            if g.shape != t.shape or o.shape != t.shape:
                fails.append("%s depth %d %s: shapes gpu %s oracle %s f64 %s" % (label, depth, name, g.shape, o.shape, t.shape))
                continue
            if not np.array_equal(np.isfinite(g), np.isfinite(t)):
                fails.append("%s depth %d %s: finite pattern differs from the oracle's" % (label, depth, name))
                continue
            e_gpu, e_orc, bound, n = stage_error(g, o, t)
            if records is not None:
                records.append(dict(stage=name, depth=depth, E_gpu=e_gpu, E_orc=e_orc, bound=bound, size=n))
            if not e_gpu <= bound:
                fails.append("%s depth %d %s: E_gpu %.3e > max(2 E_orc = %.3e, floor 4 * 2^-24 max|f64| = %.3e) over %d values"
                             % (label, depth, name, e_gpu, 2 * e_orc, 4 * U * float(np.abs(t[np.isfinite(t)]).max()), n))
    return fails


def check_discrete(orc, got, res, ref, label, spans=True, frac=FRAC):
    """Discrete results exact against the oracle; the DP kernels exact on the GPU's own costs; float64 sums as
    test_full_stack_vs_oracle.  -> list of failure texts.  A case whose oracle penalties sit on a step of the
    percentile map (off_knife_edge) is reported as a fault of the case, whatever the GPU made of it."""
    fails = ["%s depth %d: the case is on a percentile knife-edge of the oracle itself (penalty %.9g, shifted scores %.9g): "
             "pick another seed" % ((label,) + e) for e in off_knife_edge(ref, frac)]

    def need(cond, depth, what):
        if not cond:
            fails.append("%s depth %d: %s" % (label, depth, what))
    top = max(ref)
    assert len(got) == len(ref), "%s: %d levels on the GPU, %d in the oracle" % (label, len(got), len(ref))
    for depth in sorted(ref):
        g, r = got[depth], ref[depth]
        need(abs(g['del_penalty'] - r['del_penalty']) <= PEN_TOL, depth,
             "del_penalty %.9g vs the oracle's %.9g" % (g['del_penalty'], r['del_penalty']))
        if 'searchpath' in r:
            need(g['searchpath'] == [tuple(p) for p in r['searchpath']], depth, "searchpath differs")
            need(np.array_equal(g['b_offset'], r['b_offset']), depth, "b_offset differs")
            need(np.array_equal(g['new_b_offset'], r['new_b_offset']), depth, "new_b_offset differs")
            a, b = g['a_b_costs'], r['a_b_costs']
            if a.shape != b.shape or not np.array_equal(np.isinf(a), np.isinf(b)):
                need(False, depth, "inf pattern of a_b_costs differs")
                continue
            # the DP on the GPU's own costs: bit for bit what the oracle's sparse_dp makes of them
            csum, xp, yp, bout = orc.sparse_dp(a, g['b_offset'], r['alignment_types'], g['del_penalty'], r['size0'], r['size1'])
            need(np.array_equal(g['a_b_xp'], xp) and np.array_equal(g['a_b_yp'], yp), depth, "a_b_xp / a_b_yp differ from sparse_dp(GPU costs)")
            need(np.array_equal(g['new_b_offset'], bout), depth, "new_b_offset differs from sparse_dp(GPU costs)")
            need(np.array_equal(g['a_b_csum'], csum), depth, "a_b_csum differs from sparse_dp(GPU costs)")
            # against the oracle's own back-pointers (costs differ in the last digits): off-path flips are capped
            for k in ('a_b_xp', 'a_b_yp'):
                share = float((g[k] != r[k]).mean())
                need(share <= FLIP_CAP, depth, "%s differs from the oracle's at a share of %.2e" % (k, share))
            fin = np.isfinite(r['a_b_csum'])
            need(np.array_equal(np.isfinite(g['a_b_csum']), fin), depth, "finite pattern of a_b_csum differs")
            if fin.any() and np.array_equal(np.isfinite(g['a_b_csum']), fin):
                err = float(np.abs(g['a_b_csum'][fin] - r['a_b_csum'][fin]).max())
                need(err <= 1e-4 * (1 + r['a_b_csum'][fin].max()), depth, "a_b_csum off by %.3e" % err)
        if spans or depth >= 1:
            need(g.get('alignments') == r['final_alignments' if depth == 0 else 'alignments'], depth, "alignments differ")
        if depth == top and 'costs_1to1' in r:
            need(g.get('costs_1to1') is not None, depth, "no costs_1to1")
            if g.get('costs_1to1') is not None:
                _, tb = orc.dense_dp(g['costs_1to1'], g['del_penalty'])
                need(np.array_equal(g['x_y_tb'], tb), depth, "x_y_tb differs from dense_dp(GPU costs)")
                share = float((g['x_y_tb'] != r['x_y_tb']).mean())
                need(share <= FLIP_CAP, depth, "x_y_tb differs from the oracle's at a share of %.2e" % share)
                need(orc.dense_traceback(g['x_y_tb']) == r['alignments'], depth, "dense traceback differs")
    if spans:
        al, sc, pens = res
        need(al == ref[0]['final_alignments'], 0, "final spans differ")
        if al == ref[0]['final_alignments'] and len(sc):
            err = float(np.abs(np.asarray(sc) - ref[0]['alignment_scores']).max())
            need(err <= SCORE_TOL, 0, "final scores off by %.3e" % err)
        rp = np.array([ref[d]['del_penalty'] for d in sorted(ref)])
        need(len(pens) == len(rp) and float(np.abs(np.asarray(pens) - rp).max()) <= PEN_TOL, 0, "penalties differ")
    return fails


def off_knife_edge(ref, frac, shift=2e-6):
    """Is the ORACLE's deletion penalty of every level stable under a shift of its sampled scores by +-2e-6 (the size of
    a legitimate difference between two summation orders)?  The percentile map is a step function of the scores
    (fuzz_gpu_vs_oracle.py, "percentile knife-edges"); inputs for which the reference itself sits on a step cannot
    tell a right kernel from a wrong one, so cases are chosen off it.  -> list of (depth, penalty, shifted penalty)"""
    import oracle
    out = []
    for depth in sorted(ref):
        ks = np.asarray(ref[depth]['knob_scores'], np.float32)
        for sh in (-shift, shift):
            moved = (ks + np.float32(sh)).astype(np.float32)
            pen = float(oracle.del_penalty_from_scores(moved, 0, max(moved), frac))
            if abs(pen - float(ref[depth]['del_penalty'])) > PEN_TOL:
                out.append((depth, float(ref[depth]['del_penalty']), pen))
    return out


def params(**kw):
    p = dict(frac=FRAC, max_full=MAX_FULL, sample=SAMPLE, nsamp=NSAMP)
    p.update(kw)
    return p


def pool_workers():
    return max(1, min(12, (os.cpu_count() or 2) - 1))
