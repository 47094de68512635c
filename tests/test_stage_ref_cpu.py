"""stage_ref.py (the float64 restatement the GPU stage tests measure against) pinned to the oracle, on the CPU.

Bounds are derived, not measured (u = 2^-24, rows have norm <= 1):
  * fp32 dot product of d terms in ANY summation order, products rounded: |dot_f32 - dot| <= d u |a| |b|.
  * make_norm1 in fp32: squares (u), sum of d squares in any order (<= d u relative), sqrt (halves it, + u),
    + 1e-5 (u), divide (u): every element within (d / 2 + 4) u relative, so each row within eps_0 = (d / 2 + 4) u in L2.
  * downsample from rows that are eps_l off: pair sum 2 eps_l + 2 u; the column mean over h rows, summed
    sequentially, adds its own rounding <= 2 h u (as a vector) and carries <= 2 eps_l + 2 u; the difference t adds
    3 u; normalising a vector that is e off moves it by <= 2 e / |t|, plus make_norm1's own (d / 2 + 4) u:
        eps_{l+1} = 2 (4 eps_l + (2 h + 7) u) / min_row |t|  +  (d / 2 + 4) u.
  * the oracle's dot product of ITS rows against the exact dot product of the float64 rows:
        delta = d u (1 + e)^2 + 2 e + e^2,   e = the oracle rows' distance from the float64 rows (asserted <= eps_l).
  * norms = 1 - mean of S dots (BLAS + numpy mean, any order):  delta_n = delta + (S + 2) u.
  * cost = m (1 - dot) / (1e-6 + n0 + n1), evaluated in double and rounded once (score_path: one more fp32 add):
        |dc| <= (m delta + |c| (delta_n0 + delta_n1)) / (min den - delta_n0 - delta_n1) + two ulps of c.
delta stays below 2e-4 in every case (asserted), so a slip in a formula of stage_ref (a multiplier, a layer, an index:
>= 1e-3) cannot pass.  The 1e-6 of the dense / sparse denominators is below the oracle's own rounding error and is
not separable by any fp32 comparison; it is restated from the source."""
import numpy as np
import pytest

import stage_ref
from synth import alignment_types, make_pair
from stage_check import round_store

U = 2.0 ** -24

CASES = {
    # name: n, m, k0, k1, d, store, max_full, amax, W, sample
    "d8_f32": (157, 131, 3, 2, 8, "f32", 40, 4, 4, 2000),      # coarsest level 39 x 32 < sample: full enumeration
    "d64_bf16": (301, 275, 4, 2, 64, "bf16", 100, 5, 7, 500),
    "d1024_f16": (211, 189, 2, 3, 1024, "f16", 60, 4, 6, 500),
}


def build(name):
    n, m, k0, k1, d, store, max_full, amax, W, sample = CASES[name]
    v0, v1 = make_pair(n, m, max(k0, k1), d, 77, common=1.4 if d == 1024 else 0.0)
    v0, v1 = np.ascontiguousarray(v0[:k0]), np.ascontiguousarray(v1[:k1])
    v0[k0 - 1, 17, :] = 0.0   # one zero row (PAD candidate) per side
    v1[0, 23, :] = 0.0
    types = [(x, y) for x, y in alignment_types(amax) if x <= k0 and y <= k1]
    return round_store(v0, store), round_store(v1, store), types, W, max_full, sample


def row_err(a, b):
    return float(np.sqrt(((a.astype(np.float64) - b) ** 2).sum(axis=-1)).max())


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_stages_within_derived_bounds_of_float64(orc, name):
    v0, v1, types, W, max_full, sample = build(name)
    d, nsamp, seed = v0.shape[2], 100, 123
    ref = orc.vecalign(v0.copy(), v1.copy(), types, 0.2, W, max_full, sample, nsamp, rng=np.random.RandomState(seed))
    draws = stage_ref.replay_draws(orc, seed, v0.shape[1], v1.shape[1], v0.shape[0], v1.shape[0], max_full, sample, nsamp)
    assert sorted(draws) == sorted(ref) and len(ref) == 3
    f64 = stage_ref.stack(v0, v1, types, W, draws, ref)
    eps = (d / 2 + 4) * U
    for depth in sorted(ref):
        r, t, dr = ref[depth], f64[depth], draws[depth]
        # the replayed draws are the ones the oracle consumed: bit for bit through the oracle's own functions
        assert np.array_equal(orc.compute_norms(r['v0'], r['v1'], nsamp, stage_ref.Replay(dr['idx0'])), r['n0'])
        assert np.array_equal(orc.compute_norms(r['v1'], r['v0'], nsamp, stage_ref.Replay(dr['idx1'])), r['n1'])
        ks = np.empty(len(dr['knob_x']), np.float32)
        orc.score_path(dr['knob_x'], dr['knob_y'], r['n0'][0], r['n1'][0], r['v0'][0], r['v1'][0], ks)
        assert np.array_equal(ks, r['knob_scores'])
        if depth == 2:
            assert len(ks) == r['size0'] * r['size1'] or len(ks) == sample
        # vectors
        if depth >= 1:
            worst = 0.0
            for side in ('v0', 'v1'):
                prev = f64[depth - 1][side]
                h = prev.shape[1] // 2
                s = prev[:, 0:2 * h:2] + prev[:, 1:2 * h:2]
                tt = s - s.mean(axis=1, keepdims=True)
                tau = float(np.sqrt((tt * tt).sum(-1)).min())
                worst = max(worst, 2 * (4 * eps + (2 * h + 7) * U) / tau + (d / 2 + 4) * U)
            eps = worst
        e = max(row_err(r['v0'], t['v0']), row_err(r['v1'], t['v1']))
        assert e <= eps, (depth, e, eps)
        if depth == 0:   # zero rows stay zero on both sides
            assert not t['v0'][v0.shape[0] - 1, 17].any() and not r['v0'][v0.shape[0] - 1, 17].any()
        delta = d * U * (1 + e) ** 2 + 2 * e + e * e
        assert delta < 2e-4, (depth, delta)   # far below what a formula slip would cost
        # norms
        dn = {}
        for key, other in (('n0', 'v1'), ('n1', 'v0')):
            S = sum(len(i) for i in dr['idx0' if key == 'n0' else 'idx1'])
            dn[key] = delta + (S + 2) * U
            err = float(np.abs(r[key] - t[key]).max())
            assert err <= dn[key], (depth, key, err, dn[key])
        den_min = float(t['n0'].min() + t['n1'].min()) - dn['n0'] - dn['n1']
        assert den_min > 0.1

        def cost_bound(c, mult):
            c = np.abs(c)
            return (mult * delta + c * (dn['n0'] + dn['n1'])) / den_min + 4 * U * c

        err = np.abs(r['knob_scores'] - t['knob_scores'])
        assert (err <= cost_bound(t['knob_scores'], 2.0)).all(), (depth, "knob_scores", float(err.max()))
        if 'costs_1to1' in r:
            assert depth == 2
            err = np.abs(r['costs_1to1'] - t['costs_1to1'])
            assert (err <= cost_bound(t['costs_1to1'], 2.0)).all(), (depth, "costs_1to1", float(err.max()))
        if 'a_b_costs' in r:
            a, b = r['a_b_costs'], t['a_b_costs']
            assert a.shape == b.shape and np.array_equal(np.isinf(a), np.isinf(b)) and np.isfinite(b).any()
            for ti, (xo, yo) in enumerate(r['alignment_types']):
                fin = np.isfinite(b[ti])
                err = np.abs(a[ti][fin] - b[ti][fin])
                assert (err <= cost_bound(b[ti][fin], 2.0 * xo * yo)).all(), (depth, "a_b_costs", (xo, yo), float(err.max()))
        else:
            assert depth == 2


def test_norm1_and_downsample_edges():
    """Zero rows, odd lengths, and the float32 rounding of make_norm1's epsilon."""
    v = np.zeros((2, 5, 4))
    v[0, 1] = [3, 0, 4, 0]
    n = stage_ref.norm1(v)
    assert not n[1].any() and not n[0, 0].any()
    assert abs(np.sqrt((n[0, 1] ** 2).sum()) - 5 / (5 + float(np.float32(1e-5)))) < 1e-15
    rng = np.random.default_rng(0)
    v = rng.standard_normal((2, 7, 6))
    h = stage_ref.downsample(v)
    assert h.shape == (2, 3, 6)
    assert np.allclose(h, stage_ref.downsample(v[:, :6]), rtol=0, atol=0)   # the odd last row is dropped
    assert stage_ref.norms(v, v, None).shape == (2, 7) and (stage_ref.norms(v, v, None) == 1).all()


def test_make_pair_common_component():
    """common=0 leaves make_pair's arrays as they were; common=1.4 gives a mean cosine of 1.96 / 2.96 ~ 0.66 between
    unrelated rows and keeps zero rows zero."""
    a0, a1 = make_pair(120, 100, 3, 256, 9, zero_rows=2)
    b0, b1 = make_pair(120, 100, 3, 256, 9, zero_rows=2, common=0.0)
    assert np.array_equal(a0, b0) and np.array_equal(a1, b1)
    c0, c1 = make_pair(120, 100, 3, 256, 9, zero_rows=2, common=1.4)
    assert np.array_equal((a0 == 0).all(-1), (c0 == 0).all(-1)) and np.array_equal((a1 == 0).all(-1), (c1 == 0).all(-1))
    x = stage_ref.norm1(c0[0][10:60])
    y = stage_ref.norm1(c1[0][60:100])
    assert 0.6 < float((x @ y.T).mean()) < 0.72


@pytest.mark.parametrize("kind", ["iid", "aniso"])
def test_backpointer_flip_room(orc, kind):
    """test_gpu_stage_matrix caps the share of back-pointers that differ from the oracle's own at 1e-3 per array (nodes
    off the optimal path may flip when costs differ in the last digits).  That is a condition on the kernels only if
    the inputs leave room for it: here the oracle's DP runs on its own costs moved by +-E_orc (its distance from the
    float64 costs, random sign per cell), for the smallest pair of the benchmark-shaped case, and the flips that
    alone causes must stay below a quarter of the cap."""
    import stage_check as sc
    import test_gpu_stage_matrix as m
    job = m.jobs_of("bench_bf16_1024", kind)[0]
    ref, f64 = sc.cpu_reference(job)
    rng = np.random.default_rng(5)
    for depth in sorted(ref):
        r = ref[depth]
        if 'a_b_costs' in r:
            c = r['a_b_costs']
            e_orc = sc.stage_error(c, c, f64[depth]['a_b_costs'])[1]
            moved = (c + (e_orc * rng.choice([-1.0, 1.0], size=c.shape)).astype(np.float32)).astype(np.float32)
            _, xp, yp, _ = orc.sparse_dp(moved, r['b_offset'], r['alignment_types'], r['del_penalty'], r['size0'], r['size1'])
            for got, want in ((xp, r['a_b_xp']), (yp, r['a_b_yp'])):
                assert float((got != want).mean()) <= sc.FLIP_CAP / 4, (depth, float((got != want).mean()))
        if 'costs_1to1' in r:
            c = r['costs_1to1']
            e_orc = sc.stage_error(c, c, f64[depth]['costs_1to1'])[1]
            moved = (c + (e_orc * rng.choice([-1.0, 1.0], size=c.shape)).astype(np.float32)).astype(np.float32)
            _, tb = orc.dense_dp(moved, r['del_penalty'])
            assert float((tb != r['x_y_tb']).mean()) <= sc.FLIP_CAP / 4, (depth, float((tb != r['x_y_tb']).mean()))
