"""float64 restatement of every continuous stage of vecalign() (numpy only; TEST INFRASTRUCTURE).

The oracle (oracle/svx_oracle.c, oracle/oracle.py) restates the reference with the reference's own fp32 arithmetic
and summation order, so it carries the reference's rounding error: at d = 1024 its costs are up to a few 1e-6 away
from the exact value of the formula.  This module evaluates the same formulas in float64, which at these sizes is
exact for the purpose (d * 2^-53 ~ 1e-13), so that "GPU vs oracle" can be stated as "the GPU is no further from the
truth than the reference is" (tests/stage_check.py).

Every function takes the DISCRETE choices of a run (sampled indices, search path, band offsets) as arguments, so that
it is evaluated on exactly the cells the GPU and the oracle computed.  Inputs are the storage-rounded embeddings
(what the GPU reads) as float64.  Formulas: dp_core.pyx / dp_utils.py of the reference as restated in
oracle/svx_oracle.c (cited per function).  tests/test_stage_ref_cpu.py pins this module to the oracle.
"""
import math

import numpy as np

EPS_NORM = float(np.float32(1e-5))   # make_norm1 adds the python float 1e-5 to a float32: the add happens in float32


def norm1(v):
    """make_norm1 (dp_utils.py:32-40): v / (|v| + 1e-5) along the last axis; zero rows stay zero."""
    v = np.asarray(v, np.float64)
    return v / (np.sqrt((v * v).sum(axis=-1, keepdims=True)) + EPS_NORM)


def downsample(v):
    """downsample_vectors (dp_utils.py:362-378) on [K, n, d]: sums of row pairs (an odd last row is dropped), minus
    the per-layer mean row, then norm1."""
    v = np.asarray(v, np.float64)
    h = v.shape[1] // 2
    s = v[:, 0:2 * h:2, :] + v[:, 1:2 * h:2, :]
    return norm1(s - s.mean(axis=1, keepdims=True))


def norms(v_self, v_other, sampled_indices):
    """compute_norms (dp_utils.py:326-359): 1 - mean cosine with the sampled rows of the other side.
    sampled_indices: one index array per overlap layer of v_other (oracle.sample_norm_indices), or None when the
    reference draws nothing (num_samps_for_norm == 0 or an empty other side) and the norms are all one."""
    v_self = np.asarray(v_self, np.float64)
    if sampled_indices is None:
        return np.ones(v_self.shape[:2])
    samp = np.concatenate([np.asarray(v_other, np.float64)[k, idx, :] for k, idx in enumerate(sampled_indices)], axis=0)
    return 1.0 - np.matmul(v_self, samp.T).mean(axis=2)


def dense_costs(v0, v1, n0, n1, offset0=0, offset1=0):
    """make_dense_costs (dp_core.pyx:36-77): (offset0 + 1) (offset1 + 1) 2 (1 - <a, b>) / (1e-6 + n0 + n1) on the
    overlap layers offset0 of v0 / n0 and offset1 of v1 / n1 (the defaults: layer 0, factor 1)."""
    v0, v1 = np.asarray(v0, np.float64), np.asarray(v1, np.float64)
    dots = np.matmul(v0[offset0], v1[offset1].T)
    c = 2.0 * (1.0 - dots) / ((1e-6 + np.asarray(n0, np.float64)[offset0][:, None]) + np.asarray(n1, np.float64)[offset1][None, :])
    return c * float((offset0 + 1) * (offset1 + 1))


def score_path(xs, ys, n0, n1, v0, v1):
    """score_path (dp_core.pyx:143-161) on layer-0 arrays n0 [n], n1 [m], v0 [n, d], v1 [m, d]: no epsilon in the
    denominator."""
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    v0, v1 = np.asarray(v0, np.float64), np.asarray(v1, np.float64)
    dots = np.einsum("id,id->i", v0[xs], v1[ys])
    return 2.0 * (1.0 - dots) / (np.asarray(n0, np.float64)[xs] + np.asarray(n1, np.float64)[ys])


def band_costs(v0, v1, n0, n1, searchpath, b_offset, types, W, rows_per_block=256):
    """make_sparse_costs (dp_core.pyx:165-267) -> [T][A][B], B = 2 W.  Row aa = x + y of a path point (x, y) holds
    the cells yy = b_offset[aa] + b, xx = aa - yy; cells outside the documents are inf, like the oracle's.
    cost = 2 xo yo (1 - <v0[xo-1][xx], v1[yo-1][yy]>) / (1e-6 + n0[xo-1][xx] + n1[yo-1][yy])."""
    v0, v1 = np.asarray(v0, np.float64), np.asarray(v1, np.float64)
    n0, n1 = np.asarray(n0, np.float64), np.asarray(n1, np.float64)
    path = np.asarray(searchpath, np.int64).reshape(-1, 2)
    boff = np.asarray(b_offset, np.int64)
    A, B, T = path.shape[0], 2 * int(W), len(types)
    xsize, ysize = v0.shape[1], v1.shape[1]
    out = np.full((T, A, B), np.inf)
    aa_all = path[:, 0] + path[:, 1]
    for lo in range(0, A, rows_per_block):
        aa = aa_all[lo:lo + rows_per_block]
        yy = boff[aa][:, None] + np.arange(B)[None, :]
        xx = aa[:, None] - yy
        ok = (xx >= 0) & (xx < xsize) & (yy >= 0) & (yy < ysize)
        xv, yv = xx[ok], yy[ok]
        for t, (xo, yo) in enumerate(types):
            dots = np.einsum("id,id->i", v0[xo - 1][xv], v1[yo - 1][yv])
            c = (2.0 * xo * yo) * (1.0 - dots) / ((1e-6 + n0[xo - 1][xv]) + n1[yo - 1][yv])
            blk = out[t, :, :]
            rows = np.broadcast_to(aa[:, None], ok.shape)[ok]
            cols = np.broadcast_to(np.arange(B)[None, :], ok.shape)[ok]
            blk[rows, cols] = c
    return out


class Replay:
    """Stands in for a RandomState: hands out recorded choice() results in order."""

    def __init__(self, draws):
        self.draws = list(draws)

    def choice(self, a, size=None, replace=True):
        out = self.draws.pop(0)
        assert len(out) == size and (len(out) == 0 or (out.min() >= 0 and out.max() < a))
        return out


def level_sizes(n, m, max_size_full_dp):
    """Document sizes per depth (dp_utils.py:402-410)."""
    out = [(n, m)]
    while out[-1][0] * out[-1][1] > max_size_full_dp ** 2:
        out.append((out[-1][0] // 2, out[-1][1] // 2))
    return out


def replay_draws(oracle, seed, n, m, k0, k1, max_size_full_dp, costs_sample_size, num_samps_for_norm):
    """The index draws of oracle.vecalign for a pair of these sizes from RandomState(seed), in the order the stream
    is consumed: per depth the draws for n0 (rows of v1), then for n1 (rows of v0); then per depth the knob's x, y.
    -> {depth: {'idx0': [K1 arrays] | None, 'idx1': [K0 arrays] | None, 'knob_x', 'knob_y' (None when the
    reference samples nothing)}}"""
    rng = np.random.RandomState(seed)
    sizes = level_sizes(n, m, max_size_full_dp)
    out = {}
    for depth, (s0, s1) in enumerate(sizes):
        st = out[depth] = {}
        st['idx0'] = oracle.sample_norm_indices(s1, k1, num_samps_for_norm, rng) \
            if s1 and math.ceil(num_samps_for_norm / k1) else None
        st['idx1'] = oracle.sample_norm_indices(s0, k0, num_samps_for_norm, rng) \
            if s0 and math.ceil(num_samps_for_norm / k0) else None
    for depth, (s0, s1) in enumerate(sizes):
        if s0 > 0 and s1 > 0 and costs_sample_size > 0:
            out[depth]['knob_x'], out[depth]['knob_y'] = oracle.sample_knob_indices(s0, s1, costs_sample_size, rng)
        else:
            out[depth]['knob_x'] = out[depth]['knob_y'] = None
    return out


def stack(v0, v1, types, W, draws, discrete_from):
    """vecalign()'s continuous stages chained in float64 END TO END: level l+1's vectors come from the float64
    level l.  v0 / v1: storage-rounded embeddings [K, n, d]; draws: replay_draws(); discrete_from: the oracle's stack
    (only 'searchpath' and 'b_offset' of the refined levels are read).
    -> {depth: {'v0', 'v1', 'n0', 'n1', 'knob_scores'?, 'costs_1to1'? (coarsest), 'a_b_costs'? (refined)}}"""
    W = max(int(W), 3)
    depths = sorted(draws)
    out = {0: {'v0': norm1(v0), 'v1': norm1(v1)}}
    for depth in depths[1:]:
        out[depth] = {'v0': downsample(out[depth - 1]['v0']), 'v1': downsample(out[depth - 1]['v1'])}
    for depth in depths:
        st, dr = out[depth], draws[depth]
        st['n0'] = norms(st['v0'], st['v1'], dr['idx0'])
        st['n1'] = norms(st['v1'], st['v0'], dr['idx1'])
        if dr['knob_x'] is not None:
            st['knob_scores'] = score_path(dr['knob_x'], dr['knob_y'], st['n0'][0], st['n1'][0], st['v0'][0], st['v1'][0])
    top = out[depths[-1]]
    top['costs_1to1'] = dense_costs(top['v0'], top['v1'], top['n0'], top['n1'])
    for depth in ([0] if len(depths) == 1 else depths[:-1]):
        st, disc = out[depth], discrete_from[depth]
        st['a_b_costs'] = band_costs(st['v0'], st['v1'], st['n0'], st['n1'], disc['searchpath'], disc['b_offset'],
                                     types if depth == 0 else [(1, 1)], W)
    return out
