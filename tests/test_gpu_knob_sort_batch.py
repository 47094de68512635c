"""The sample sort inside svx_align_batch (k_knob_sort, one workgroup per (pair, level)), through PreparedBatch.

Two batches, each ONE svx_align_batch call:

  "staged"  d = 64, K = 4: (700, 650) with two refined levels, (300, 280) with L = 0 and (2500, 40) -- every (pair, level)
            stages its scatter in LDS;
  "mixed"   d = 32, K = 1: the same three sizes and (19500, 64), whose level 0 (19 500 source rows, 20 000 samples) is
            past the staging LDS and takes the direct scatter in the same launch, beside staged ones.

The sort only permutes the samples; what depends on it are the sampled scores (k_knob_scores writes each to
kscore[sample id]) and the deletion penalty made of them.  Per level: knob_scores against the float64 chain of
stage_ref.py by the rule of stage_check.check_continuous, del_penalty against the oracle within stage_check.PEN_TOL; the
final alignments equal the oracle's; raw_results() is bit-identical with the software pipeline off and on and on a
second run of the same batch.

test_inputs_are_sound_on_the_cpu (no GPU) checks the inputs on the oracle's side: the level counts named above, which
levels stage, and that no oracle penalty sits on a step of the percentile map (stage_check.off_knife_edge)."""
import numpy as np
import pytest

import stage_check as sc
from synth import alignment_types

SIZES = ((700, 650), (300, 280), (2500, 40))
LONG = (19500, 64)
# name: (storage, d, K, types, W, sizes)
BATCHES = {
    "staged": ("bf16", 64, 4, alignment_types(5), 7, SIZES),
    "mixed": ("f32", 32, 1, alignment_types(2), 3, SIZES + (LONG,)),
}
LEVELS = {(700, 650): 3, (300, 280): 1, (2500, 40): 2, LONG: 3}   # pyramid levels (L + 1) at max_size_full_dp = 300


def jobs_of(name):
    store, d, k, types, W, sizes = BATCHES[name]
    base = 7000 * (sorted(BATCHES).index(name) + 1)
    return [dict(n=n, m=m, k0=k, k1=k, d=d, store=store, types=types, W=W, params=sc.params(), data_seed=base + i,
                 seed=base + 500 + i) for i, (n, m) in enumerate(sizes)]


@pytest.fixture(scope="module")
def refs():
    """(oracle stack, float64 stages) per pair of each batch, computed once."""
    return {name: [sc.cpu_reference(j) for j in jobs_of(name)] for name in BATCHES}


def takes_staged_way(n, kn):
    from svx import _lib
    return (n + 1 + kn) * 4 <= _lib.SVX_KNOB_SORT_STAGE_LDS


def test_inputs_are_sound_on_the_cpu(refs):
    import stage_ref
    for name in BATCHES:
        direct = []
        for job, (ref, f64) in zip(jobs_of(name), refs[name]):
            size = (job['n'], job['m'])
            assert len(ref) == LEVELS[size], "%s %s: %d levels" % (name, size, len(ref))
            assert not sc.off_knife_edge(ref, sc.FRAC), "%s %s sits on a percentile knife-edge: pick another seed" % (name, size)
            for depth, (n, m) in enumerate(stage_ref.level_sizes(size[0], size[1], sc.MAX_FULL)):
                kn = min(n * m, sc.SAMPLE)
                assert len(ref[depth]['knob_scores']) == kn
                if not takes_staged_way(n, kn):
                    direct.append((size, depth))
        assert direct == ([(LONG, 0)] if name == "mixed" else []), direct


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BATCHES))
def test_sorted_scores_and_alignments(orc, refs, name):
    jobs = jobs_of(name)
    _, res, stacks = sc.run_gpu(jobs)
    fails = []
    for i, (ref, f64) in enumerate(refs[name]):
        label = "%s pair %d (%d x %d)" % (name, i, jobs[i]['n'], jobs[i]['m'])
        assert len(stacks[i]) == len(ref), label
        fails += sc.check_continuous(stacks[i], ref, f64, label, stages=('knob_scores',))
        for depth in sorted(ref):
            g, r = stacks[i][depth]['del_penalty'], ref[depth]['del_penalty']
            if not abs(g - r) <= sc.PEN_TOL:
                fails.append("%s depth %d: del_penalty %.9g vs the oracle's %.9g" % (label, depth, g, r))
        al, scores, _ = res[i]
        if al != ref[0]['final_alignments']:
            fails.append("%s: final alignments differ from the oracle's" % label)
        elif len(scores) and float(np.abs(np.asarray(scores) - ref[0]['alignment_scores']).max()) > sc.SCORE_TOL:
            fails.append("%s: final scores differ from the oracle's" % label)
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BATCHES))
def test_raw_results_do_not_depend_on_the_sort_order(name):
    """The order inside one source row changes from run to run and with what runs beside the sort; no output bit does."""
    from svx import _lib
    from svx.vecalign import dp_utils
    from fuzz_gpu_vs_oracle import to_devs
    jobs = jobs_of(name)
    j0, p = jobs[0], jobs[0]['params']
    devs = to_devs([sc.host_pair(j) for j in jobs], j0['store'])
    ctx = _lib.context()
    was = ctx.pipeline

    def run_once():
        pb = dp_utils.PreparedBatch(devs, j0['types'], p['frac'], j0['W'], p['max_full'], p['sample'], p['nsamp'],
                                    rngs=[np.random.RandomState(j['seed']) for j in jobs])
        outs = []
        for _ in range(2):
            pb.run()
            if ctx.pipeline:
                pb.flush()
            outs.append([a.copy() for a in pb.raw_results()])
        return outs
    try:
        ctx.set_pipeline(False)
        plain = run_once()
        ctx.set_pipeline(True)
        piped = run_once()
    finally:
        ctx.set_pipeline(was)
    for other, what in ((plain[1], "second run"), (piped[0], "pipeline on"), (piped[1], "pipeline on, second run")):
        assert len(other) == len(plain[0])
        for a, b in zip(plain[0], other):
            assert np.array_equal(a, b), what
