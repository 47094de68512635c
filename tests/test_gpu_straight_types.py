"""Straight search (Sakoe-Chiba band and dense mode) with type sets beyond the two LDS-resident tile shapes: the
general tile shape of csrc/svx_tiles.hip (cost planes per group of types through global scratch, halo of the largest
x / y step, int32 back-pointers for steps above 15).  Every case has a band wider than 64 cells, so it runs on the
tile sweep.  Against the oracle's straight path (make_sparse_costs + sparse_dp + sparse_traceback on search_path
over the whole documents): identical spans, scores within 1e-4."""
import numpy as np
import pytest

from dp_ref import many_to_one_types, straight_oracle   # (shared with test_gpu_dp_ties.py)
from synth import alignment_types, make_pair, round_bf16

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-4


def storage(v, dt):
    if dt == "bf16":
        return round_bf16(v)
    if dt == "f16":
        return v.astype(np.float16).astype(np.float32)
    return v


def to_dev(v, dt):
    import torch
    tdt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[dt]
    return torch.from_numpy(v).cuda().to(tdt)


def run_case(orc, v0, v1, types, W, dt, seed):
    from svx.vecalign import dp_utils
    al_o, sc_o = straight_oracle(orc, v0, v1, types, W, seed)
    np.random.seed(seed)
    al_g, sc_g = dp_utils.align_band(to_dev(v0, dt), to_dev(v1, dt), types, 0.2, W, 20000, 100)
    assert al_g == al_o
    assert np.abs(np.asarray(sc_g) - np.asarray(sc_o)).max() < SCORE_TOL
    return al_g


CASES = [
    # name, N, M, K0, K1, d, dtype, a or None, many_to_one or None, W, deletions, zero rows
    ("a7_bf16_band", 500, 480, 6, 6, 1024, "bf16", 7, None, 40, 15, 0),      # 21 types on 6 + 6 layers
    ("a10_f32_band", 300, 290, 9, 9, 64, "f32", 10, None, 48, 9, 0),         # 45 types, steps of 9 (> the old halo)
    ("a10_f32_dense", 260, 250, 9, 9, 64, "f32", 10, None, 400, 9, 0),
    ("a16_f16_dense", 120, 118, 15, 15, 64, "f16", 16, None, 200, 4, 0),     # 120 types on 15 + 15 layers, packed
    ("m2o20_band", 330, 90, 20, 1, 64, "f32", None, 20, 60, 0, 0),          # int32 back-pointers, steps < 32
    ("m2o20_dense", 330, 90, 20, 1, 64, "bf16", None, 20, 400, 0, 0),
    ("m2o50_dense", 420, 130, 50, 1, 64, "f32", None, 50, 500, 0, 0),       # steps longer than a tile side
    ("a10_steep", 97, 1000, 9, 9, 64, "f32", 10, None, 45, 0, 0),            # steep straight path
    ("a8_zero_rows", 400, 380, 7, 7, 96, "bf16", 8, None, 33, 12, 30),       # exact ties, tail slab (d = 96)
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_straight_general_shape_vs_oracle(orc, case):
    name, N, M, K0, K1, d, dt, a, m2o, W, dels, zero = case
    types = alignment_types(a) if a is not None else many_to_one_types(m2o)
    v0, v1 = make_pair(N, M, max(K0, K1), d, 600 + N, deletions=dels, zero_rows=zero)
    v0, v1 = storage(np.ascontiguousarray(v0[:K0]), dt), storage(np.ascontiguousarray(v1[:K1]), dt)
    al = run_case(orc, v0, v1, types, W, dt, 41)
    if m2o is not None:
        assert max(len(x) for x, _ in al) > 1  # many-to-one steps are taken


def test_straight_general_shape_batch_equals_single(orc):
    """Several pairs of different sizes with -a 10 in one call (a call has one band width for all its pairs): each pair
    equals its own single-pair run and the oracle."""
    from svx.vecalign import dp_utils
    types = alignment_types(10)
    sizes = [(210, 200), (330, 310), (120, 260), (270, 270)]
    pairs, want = [], []
    for k, (N, M) in enumerate(sizes):
        v0, v1 = make_pair(N, M, 9, 64, 900 + k, deletions=5)
        pairs.append((v0, v1))
    W = 60
    for k, (v0, v1) in enumerate(pairs):
        want.append(straight_oracle(orc, v0, v1, types, W, 100 + k))
    rngs = [np.random.RandomState(100 + k) for k in range(len(pairs))]
    res = dp_utils.align_band_batch([(to_dev(v0, "f32"), to_dev(v1, "f32")) for v0, v1 in pairs], types, 0.2, W, 20000, 100, rngs=rngs)
    for k, (v0, v1) in enumerate(pairs):
        al_o, sc_o = want[k]
        assert res[k][0] == al_o
        assert np.abs(np.asarray(res[k][1]) - np.asarray(sc_o)).max() < SCORE_TOL
        one = dp_utils.align_band_batch([(to_dev(v0, "f32"), to_dev(v1, "f32"))], types, 0.2, W, 20000, 100,
                                        rngs=[np.random.RandomState(100 + k)])
        assert one[0][0] == res[k][0]
        assert np.array_equal(np.asarray(one[0][1]), np.asarray(res[k][1]))
