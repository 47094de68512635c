"""The kept-for-A/B band-cost kernels and the pipeline switch on the benchmark-shaped case (d = 1024, bf16, 4 layers,
10 types, band 14; three ragged pairs; both data kinds of test_gpu_stage_matrix).  SVX_BAND_V (2: the general kernel
k_band_costs2 at level 0 too, 3: k_band_costs3 there) and SVX_BAND_ASMLOAD are read at every launch, so the environment
switches them inside one process.  Every variant passes the float64 rule of stage_check on a_b_costs at every level, every discrete result
equals the oracle's, and so all variants give identical final spans.  bench comparisons of future kernel work rest on
these kernels."""
import numpy as np
import pytest

import stage_check as sc
from test_gpu_stage_matrix import jobs_of

pytestmark = pytest.mark.gpu

VARIANTS = (
    ("default", {}, None),
    ("SVX_BAND_V=2", {"SVX_BAND_V": "2"}, None),
    ("SVX_BAND_V=3", {"SVX_BAND_V": "3"}, None),
    ("SVX_BAND_ASMLOAD=0", {"SVX_BAND_ASMLOAD": "0"}, None),
    ("SVX_BAND_ASMLOAD=1", {"SVX_BAND_ASMLOAD": "1"}, None),
    ("pipeline on", {}, True),
    ("pipeline off", {}, False),
)
KNOBS = ("SVX_BAND_V", "SVX_BAND_ASMLOAD")


@pytest.mark.parametrize("kind", ["iid", "aniso"])
def test_band_generations_agree(orc, monkeypatch, kind):
    from svx import _lib
    jobs = jobs_of("bench_bf16_1024", kind)
    pool = sc.RefPool(3)
    try:
        refs = pool.get(kind, jobs)
    finally:
        pool.close()
    ctx = _lib.context()
    was = ctx.pipeline
    fails, spans = [], {}
    try:
        for name, env, pipe in VARIANTS:
            for k in KNOBS:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            if pipe is not None:
                ctx.set_pipeline(pipe)
            _, res, stacks = sc.run_gpu(jobs)
            ctx.sync()
            if pipe is not None:
                ctx.set_pipeline(was)
            spans[name] = [r[0] for r in res]
            for i, (ref, f64) in enumerate(refs):
                label = "%s [%s] pair %d" % (kind, name, i)
                fails += sc.check_continuous(stacks[i], ref, f64, label, stages=('a_b_costs',))
                fails += sc.check_discrete(orc, stacks[i], res[i], ref, label)
    finally:
        ctx.set_pipeline(was)
    assert not fails, "\n".join(fails[:40])
    assert all(s == spans["default"] for s in spans.values())
