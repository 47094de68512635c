"""The randomised GPU-vs-oracle sweep (fuzz_gpu_vs_oracle.py) at the widths users run: a 24-case slice with
d in {512, 1024}, documents up to 2500 segments, K = 4 / -a 5 in at least half the batches, no zero rows.

Without zero rows the data are continuous, so exact ties cannot occur; and SEED is chosen such that the ORACLE ALONE is
not on a percentile knife-edge in any case (the CPU test below verifies the choice on every run): for every case and
level, DeletionKnob of the oracle's sampled scores shifted by +-2e-6 (the sweep's KS_TOL, the size of a legitimate
difference between two summation orders) stays within 5e-5 of the unshifted penalty.  So `ties + edges <= 1` in the GPU
test is a condition on the kernels, not a measurement."""
import numpy as np
import pytest

import fuzz_gpu_vs_oracle as fz

SEED = 10
WIDE = dict(batch=8, max_size=2500, dims=(512, 1024), zero_rows=0, k4_weight=0.5)
CASES = 24


def test_wide_slice_is_off_the_knife_edge(orc):
    import os
    pool = fz.oracle_pool(max(1, min(8, (os.cpu_count() or 2) - 1)))
    try:
        k4 = batches = 0
        pending = []
        for cfg, hosts, seeds in fz.draw_batches(CASES, SEED, **WIDE):
            batches += 1
            k4 += cfg['K'] == 4 and cfg['amax'] == 5
            assert cfg['d'] in (512, 1024)
            args = [(a, b, cfg['types'], cfg['frac'], cfg['W'], cfg['max_full'], cfg['sample'], cfg['nsamp'], s)
                    for (a, b), s in zip(hosts, seeds)]
            pending.append((cfg, [h[0].shape[1:] + h[1].shape[1:2] for h in hosts], pool.map_async(fz._oracle_job, args)))
        assert 2 * k4 >= batches, "K = 4 / -a 5 in %d of %d batches" % (k4, batches)
        for cfg, shapes, refs in pending:
            for shape, ref in zip(shapes, refs.get()):
                assert not isinstance(ref, Exception), (shape, ref)
                for depth in sorted(ref):
                    ks = np.asarray(ref[depth]['knob_scores'], np.float32)
                    for shift in (-2e-6, 2e-6):
                        moved = (ks + np.float32(shift)).astype(np.float32)
                        pen = orc.del_penalty_from_scores(moved, 0, max(moved), cfg['frac'])
                        assert abs(float(pen) - float(ref[depth]['del_penalty'])) <= fz.PEN_TOL, \
                            ("knife-edge in the oracle itself", shape, depth, float(pen), float(ref[depth]['del_penalty']))
    finally:
        pool.terminate()
        pool.join()


@pytest.mark.gpu
def test_randomised_sweep_wide():
    bad, ties, edges = fz.run_sweep(CASES, SEED, verbose=False, workers=12, **WIDE)
    assert bad == 0
    assert ties + edges <= 1
