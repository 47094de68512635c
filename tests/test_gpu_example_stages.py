"""The shipped en-de pair (tests/golden/example_full: real fp16 SONAR embeddings, d = 1024, 5 layers, -a 6: 15 types,
band 16, the reference's default parameters, seed 0) stage by stage: the only anisotropic REAL data in the tree, which
test_example_full.py checks through the command line for final spans and scores only.  Same assertions as
test_gpu_stage_matrix: discrete results exact against the oracle, the DP exact on the GPU's own costs, every continuous
stage no further from float64 than twice the oracle's own distance (stage_check)."""
import numpy as np
import pytest

import stage_check as sc
from test_example_full import load_side

pytestmark = pytest.mark.gpu


def test_example_full_stage_by_stage(orc):
    from svx.vecalign.vecalign import make_alignment_types
    v0, v1 = load_side("en", "src"), load_side("de", "tgt")
    assert v0.shape == (5, 237, 1024) and v1.shape == (5, 217, 1024)
    assert np.array_equal(v0, sc.round_store(v0, "f16")) and np.array_equal(v1, sc.round_store(v1, "f16"))   # fp16 payloads
    job = dict(v0=v0, v1=v1, store="f16", types=make_alignment_types(6), W=8, seed=0,
               params=sc.params(frac=0.2, max_full=300, sample=20000, nsamp=100))
    ref, f64 = sc.cpu_reference(job)
    assert len(ref) == 1 and 'costs_1to1' in f64[0] and 'a_b_costs' in f64[0]
    _, res, stacks = sc.run_gpu([job])
    fails = sc.check_continuous(stacks[0], ref, f64, "example_full") + sc.check_discrete(orc, stacks[0], res[0], ref, "example_full")
    assert not fails, "\n".join(fails)
