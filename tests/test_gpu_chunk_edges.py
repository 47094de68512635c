"""Chunk edges of the band-cost kernels.  A search path is cut into chunks of lim + 1 points, lim = rows - min(2 W, 16)
(svxl_band_costs2_batch); a chunk reads a halo of rows around its points.  One batch per kernel generation holds
CONSECUTIVE document lengths n = n0 .. n0 + 2 (lim + 1), m = n - 3, so that the level-0 path length (~ n + m) walks
over several chunk boundaries; levels >= 1 always run the 64-row shape with type (1, 1), and n0 is chosen so that the
level-1 path length (~ n / 2 + m / 2) crosses one of its boundaries (a multiple of 64 - min(2 W, 16) + 1) inside the run too.
Small d keeps the oracle cheap; the chunking does not depend on d.

Level-0 and level-1 band costs by the rule of stage_check (no further from float64 than twice the oracle's own
distance, floor 4 * 2^-24 max|f64|); every discrete result, spans and scores against the oracle."""
import numpy as np
import pytest

import stage_check as sc
from synth import alignment_types

# name: storage, d, K, types, W, rows of the level-0 kernel shape, base of the pairs' RandomState seeds (chosen on the
# CPU such that the oracle is off the percentile knife-edge for every pair: the first test below)
CONFIGS = {
    "v3_bf16_256": ("bf16", 256, 4, alignment_types(5), 7, 32, 9000),      # k_band_costs3 NK 8: lim 18
    "v2_nslot8_f32_64": ("f32", 64, 4, alignment_types(5), 7, 32, 10000),   # k_band_costs2 {32, 8, 5, 3}: lim 18
    "v2_rows64_f32_64": ("f32", 64, 1, alignment_types(2), 3, 64, 9000),   # k_band_costs2 {64, 2, 1, 4} at every level: lim 58
}
N0, MAX_FULL, SAMPLE = 200, 80, 2000   # three levels over the whole run: 200 x 197 -> 100 x 98 -> 50 x 49 ... 318 x 315 -> 159 x 157 -> 79 x 78


def jobs_of(name):
    store, d, K, types, W, rows, seed0 = CONFIGS[name]
    lim = rows - min(2 * W, 16)
    return lim, [dict(n=n, m=n - 3, k0=K, k1=K, d=d, store=store, types=types, W=W, params=sc.params(max_full=MAX_FULL, sample=SAMPLE),
                      data_seed=7000 + n, seed=seed0 + n, common=1.4 if n % 2 else 0.0)
                 for n in range(N0, N0 + 2 * (lim + 1) + 1)]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_chunk_edge_inputs_are_off_the_knife_edge(name):
    """CPU: the oracle's own deletion penalties do not sit on a step of the percentile map for any pair of the run
    (stage_check.off_knife_edge), so `penalties within 5e-5` in the GPU test is a condition on the kernels.  SAMPLE is
    below the smallest level's n * m, so no level enumerates all pairs (n * m * k / 28 is whole for many sizes)."""
    _, jobs = jobs_of(name)
    pool = sc.RefPool(sc.pool_workers())
    try:
        refs = pool.get(name, jobs)
    finally:
        pool.close()
    edges = [(j['n'], sc.off_knife_edge(ref, j['params']['frac'])) for j, (ref, _) in zip(jobs, refs)]
    assert not [e for e in edges if e[1]], [e for e in edges if e[1]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_chunk_edge_sweep(orc, name):
    lim, jobs = jobs_of(name)
    W = jobs[0]['W']
    lim1 = 64 - min(2 * W, 16)
    pool = sc.RefPool(sc.pool_workers())
    try:
        _, res, stacks = sc.run_gpu(jobs)
        refs = pool.get(name, jobs)
    finally:
        pool.close()
    # the run does walk over chunk boundaries at both levels
    a0 = [len(ref[0]['searchpath']) for ref, _ in refs]
    a1 = [len(ref[1]['searchpath']) for ref, _ in refs]
    assert max(a0) // (lim + 1) - min(a0) // (lim + 1) >= 2, (min(a0), max(a0), lim)
    assert max(a1) // (lim1 + 1) > min(a1) // (lim1 + 1), (min(a1), max(a1), lim1)
    fails = []
    for i, (ref, f64) in enumerate(refs):
        assert len(ref) == 3
        label = "%s %d x %d" % (name, jobs[i]['n'], jobs[i]['m'])
        fails += sc.check_continuous(stacks[i], ref, f64, label, stages=('a_b_costs',))
        fails += sc.check_discrete(orc, stacks[i], res[i], ref, label)
    assert not fails, "\n".join(fails[:40])
