"""The DP kernels' tie rule, bit for bit.  The reference lets the first strictly smaller candidate win -- the alignment
types in list order, then the (0,1) deletion, then the (1,0) deletion -- and every DP kernel here rebuilds that rule
from parts (lane groups merged by (total, key), deletions folded in afterwards, half-waves and DPP merges in the tile
sweep).  On the two input families of dp_ref.py the costs are the same bits on the GPU and in the oracle, so nothing is
excused and no tolerance is used: every sum, every back-pointer, every span and every score below is compared with
np.array_equal / ==.  test_dp_ties_cpu.py shows, without a GPU, that these inputs are decided by ties often enough
and that each case would change under the opposite rule.

Kernel coverage of the per-op cases (csrc/svx_dp.hip; restated in dp_ref.dpf_groups / dpf_tpl):
    dpf_groups(T, B): G = 4 if B <= 16 else 2 if B <= 32 else 1, halved while T < G
    dpf_tpl(T, B):    t = ceil(T / G); TPLT = t if t <= 4 else 6 if t <= 6 else 0
B = 14 with T = 4, 6, 10, 15, 21, 28 -> k_sparse_dp_fast<1|2|3|4|6|0, 4>; B = 24 with T = 2, 3, 6, 8, 10, 15 -> <.., 2>;
B = 40 with T = 1, 2, 3, 4, 6, 10 -> <.., 1>; B = 96 -> k_sparse_dp<true>; B = 2000 with steps of 9 -> k_sparse_dp<false>.
The fused cases run the same 18 templates as k_sparse_dp_fast_batch (W = 7, 12, 20 -> G = 4, 2, 1), k_dense_stage_batch
and, in straight search with W >= 33, every shape of the tile sweep (csrc/svx_tiles.hip)."""
import multiprocessing

import numpy as np
import pytest

import dp_ref

pytestmark = pytest.mark.gpu


def differ(fails, label, what, got, want):
    """Bit-for-bit comparison of two arrays (inf pattern included) -> appends one line to `fails` when they differ."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        fails.append("%s: %s has shape %s, the oracle's %s" % (label, what, got.shape, want.shape))
    elif not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        fails.append("%s: %s differs from the oracle's at %d of %d entries, first at %s: %r vs %r"
                     % (label, what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


# ------------------------------------------------------------------------------------------ a. per-op sparse_dp
@pytest.mark.parametrize("case", dp_ref.P_SPARSE, ids=[c[0] for c in dp_ref.P_SPARSE])
def test_sparse_dp_ties_family_p(orc, case):
    from svx.vecalign import dp_core, dp_utils
    f, bo, types, pen, N, M = dp_ref.p_sparse_inputs(case)
    ro = orc.sparse_dp(f, bo, types, pen, N, M)
    rg = dp_core.sparse_dp(f, bo, types, pen, N, M)
    fails = []
    for what, g, o in zip(("csum", "xp", "yp", "b_offset_out"), rg, ro):
        differ(fails, case[0], what, g, o)
    assert not fails, "\n".join(fails)
    al_o, sc_o = orc.sparse_traceback(*ro, N, M)
    al_g, sc_g = dp_utils.sparse_traceback(*rg, N, M)
    assert al_g == al_o
    assert np.array_equal(np.asarray(sc_g), sc_o)


# ------------------------------------------------------------------------------------------ b. per-op dense_dp
@pytest.mark.parametrize("case", dp_ref.P_DENSE, ids=[c[0] for c in dp_ref.P_DENSE])
def test_dense_dp_ties_family_p(orc, case):
    from svx.vecalign import dp_core, dp_utils
    f, pen = dp_ref.p_dense_inputs(case)
    csum_o, bp_o = orc.dense_dp(f, pen)
    csum_g, bp_g = dp_core.dense_dp(f, pen)
    fails = []
    differ(fails, case[0], "csum", csum_g, csum_o)
    differ(fails, case[0], "bp", bp_g, bp_o)
    assert not fails, "\n".join(fails)
    assert dp_utils.dense_traceback(bp_g) == orc.dense_traceback(bp_o)


# ------------------------------------------------------------------------------------------ the oracle side of family Z
class RefFarm:
    """The oracle's results for every family Z case, computed once in processes that never touch the GPU (spawn) while
    the GPU tests above them run."""

    def __init__(self):
        self.pool = multiprocessing.get_context("spawn").Pool(8)
        self.jobs = {("fused", c[0]): self.pool.apply_async(dp_ref.z_fused_refs, (c[0],)) for c in dp_ref.Z_FUSED if not c[9]}
        for c in dp_ref.Z_STRAIGHT:
            self.jobs[("straight", c[0])] = self.pool.apply_async(dp_ref.z_straight_refs, (c[0], c[3] < 33))
        self.done = {}

    def get(self, kind, name):
        if (kind, name) not in self.done:
            self.done[(kind, name)] = self.jobs[(kind, name)].get()
        return self.done[(kind, name)]

    def close(self):
        self.pool.terminate()
        self.pool.join()


@pytest.fixture(scope="module")
def farm():
    f = RefFarm()
    yield f
    f.close()


def to_dev(v, store):
    import torch
    return torch.from_numpy(v).cuda().to({"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[store])


def compare_band_level(fails, label, g, r, lattice_only=False):
    """new_b_offset, csum and back-pointers of one refined level: every cell of the band, or with lattice_only the band
    cells that are nodes of the lattice, 0 <= x <= size0 and 0 <= y <= size1 (unreachable ones included)."""
    differ(fails, label, "new_b_offset", g['new_b_offset'], r['new_b_offset'])
    if g['new_b_offset'].shape != r['new_b_offset'].shape or g['a_b_csum'].shape != r['a_b_csum'].shape:
        fails.append("%s: node arrays have other shapes than the oracle's" % label)
        return
    keep = np.ones(r['a_b_csum'].shape, bool)
    if lattice_only:
        A2, B = keep.shape
        yy = np.arange(B)[None, :] + r['new_b_offset'][:, None]
        xx = np.arange(A2)[:, None] - yy
        keep = (0 <= xx) & (xx <= r['size0']) & (0 <= yy) & (yy <= r['size1'])
    for k in ('a_b_csum', 'a_b_xp', 'a_b_yp'):
        differ(fails, label, k + (" (lattice nodes)" if lattice_only else ""), np.where(keep, g[k], 0), np.where(keep, r[k], 0))


# ------------------------------------------------------------------------------------------ c. coarse-to-fine
@pytest.mark.parametrize("case", dp_ref.Z_FUSED, ids=[c[0] for c in dp_ref.Z_FUSED])
def test_fused_pipeline_ties_family_z(orc, farm, case):
    """Every stage of svx_align_batch on zero embeddings with caller-supplied dyadic normalisers, per level and each on
    its own line: knob_scores and del_penalty; a_b_costs (inf pattern included) and costs_1to1; then, with the GPU's
    penalties given to the oracle (so that a last-bit difference of a penalty can neither hide nor fake a DP finding),
    a_b_csum, a_b_xp, a_b_yp, new_b_offset, x_y_tb, the level's alignments and scores, final spans and scores."""
    from svx import _lib
    from svx.vecalign import dp_utils
    name, sizes, a, W, store, d, levels, max_full, seed, pipeline = case
    types = dp_ref.alignment_types(a)
    pairs = dp_ref.z_fused_pairs(case)
    refs = farm.get("fused", name.replace("_pipeline", ""))
    ctx = _lib.context()
    was = ctx.pipeline
    try:
        ctx.set_pipeline(pipeline)
        pb = dp_utils.PreparedBatch([(to_dev(p[0], store), to_dev(p[1], store)) for p in pairs], types, dp_ref.FRAC, W, max_full,
                                    dp_ref.SAMPLE, dp_ref.NSAMP, rngs=[np.random.RandomState(p[4]) for p in pairs],
                                    norms=[(p[2], p[3]) for p in pairs])
        pb.run()
        res = pb.results()
        stacks = [[pb.level_stack(i, depth) for depth in range(pb.levels[i])] for i in range(len(pairs))]
        ctx.sync()
    finally:
        ctx.set_pipeline(was)
    fails = []
    for i, (ref, got) in enumerate(zip(refs, stacks)):
        lab = "%s pair %d" % (name, i)
        assert len(got) == len(ref) >= 2, "%s: %d levels on the GPU, %d in the oracle" % (lab, len(got), len(ref))
        top = max(ref)
        pens = {}
        for depth in sorted(ref):
            g, r, dl = got[depth], ref[depth], "%s depth %d" % (lab, depth)
            differ(fails, dl, "knob_scores", g.get('knob_scores', np.zeros(0)), r['knob_scores'])
            if g['del_penalty'] != r['del_penalty']:
                fails.append("%s: del_penalty %r, the oracle's %r" % (dl, g['del_penalty'], r['del_penalty']))
                pens[depth] = g['del_penalty']
            if depth < top:
                differ(fails, dl, "a_b_costs", g['a_b_costs'], r['a_b_costs'])
                differ(fails, dl, "b_offset", g['b_offset'], r['b_offset'])
            else:
                differ(fails, dl, "costs_1to1", g['costs_1to1'], r['costs_1to1'])
        if pens:   # the oracle again, on the GPU's penalties
            v0, v1, n0, n1, sd = dp_ref.z_pair(pairs[i][0].shape[1], pairs[i][1].shape[1], max(1, a - 1), max(1, a - 1), 32, levels, pairs[i][4]) + (pairs[i][4],)
            ref = dp_ref.z_oracle(orc, v0, v1, n0, n1, types, W, max_full, sd, del_penalties=pens)
        for depth in sorted(ref):
            g, r, dl = got[depth], ref[depth], "%s depth %d" % (lab, depth)
            if depth == top:
                differ(fails, dl, "x_y_tb", g['x_y_tb'], r['x_y_tb'])
            else:
                compare_band_level(fails, dl, g, r)
                differ(fails, dl, "alignment_scores", g['alignment_scores'], r['alignment_scores'])
            if g.get('alignments') != r['final_alignments' if depth == 0 else 'alignments']:
                fails.append("%s: the level's alignments differ" % dl)
        al, sc, _ = res[i]
        if al != ref[0]['final_alignments']:
            fails.append("%s: final spans differ" % lab)
        differ(fails, lab, "final scores", sc, ref[0]['alignment_scores'])
    assert not fails, "\n".join(fails[:40])


# ------------------------------------------------------------------------------------------ d. straight search
@pytest.mark.parametrize("case", dp_ref.Z_STRAIGHT, ids=[c[0] for c in dp_ref.Z_STRAIGHT])
def test_straight_search_ties_family_z(orc, farm, case):
    """Straight search (SVX_SEARCH_STRAIGHT) against dp_ref.straight_stack with both normalisers supplied: one narrow
    band (the band kernels on a straight path) and, with W >= 33, the tile sweep: both LDS-resident shapes, the general
    shape with MS = 2, 3, 4, 6, 9, 17 moves per slot, int32 back-pointers (--many_to_one 20), the BIGH variant
    ((100,1) with (1,100)) and a batch of three pairs.  Final spans and scores, knob_scores, del_penalty, new_b_offset
    and the node arrays of the level view are bit-equal: a_b_csum and the back-pointers on every band node.  The band
    kernels also fill the band cells outside the lattice (x > size0, y > size1 or a negative coordinate) like the
    reference, +inf / -42, and the narrow case compares them; the tile sweep stores lattice nodes only and leaves those
    cells as the scratch arena had them.  Nothing reads a cell that is no node (every move and the traceback stay inside
    the lattice), and the level view shows the pipeline's working arrays, not copies made for it: filling those cells
    would add a pass over the whole band to every call of the sweep for the view's sake alone.  So this is no fault of
    the sweep: include/svx.h now says that these cells are unspecified there, and the sweep's cases compare the lattice
    nodes, unreachable ones included."""
    from svx.vecalign import dp_utils
    name, sizes, _, W, store, d, levels, seed = case
    types = dp_ref.z_straight_types(case)
    pairs = dp_ref.z_straight_pairs(case)
    refs = farm.get("straight", name)
    pb = dp_utils.PreparedBatch([(to_dev(p[0], store), to_dev(p[1], store)) for p in pairs], types, dp_ref.FRAC, W, 0,
                                dp_ref.SAMPLE, dp_ref.NSAMP, rngs=[np.random.RandomState(p[4]) for p in pairs],
                                norms=[(p[2], p[3]) for p in pairs], search="straight")
    pb.run()
    res = pb.results()
    fails = []
    for i, r in enumerate(refs):
        lab = "%s pair %d" % (name, i)
        assert pb.levels[i] == 1
        g = pb.level_stack(i, 0)
        differ(fails, lab, "knob_scores", g.get('knob_scores', np.zeros(0)), r['knob_scores'])
        if g['del_penalty'] != r['del_penalty']:
            fails.append("%s: del_penalty %r, the oracle's %r" % (lab, g['del_penalty'], r['del_penalty']))
            r = dp_ref.straight_stack(orc, pairs[i][0], pairs[i][1], types, W, pairs[i][4], norms=(pairs[i][2], pairs[i][3]), pen=g['del_penalty'])
        if 'a_b_costs' in g and 'a_b_costs' in r:   # (the tile sweep keeps no cost array)
            differ(fails, lab, "a_b_costs", g['a_b_costs'], r['a_b_costs'])
        differ(fails, lab, "b_offset", g['b_offset'], r['b_offset'])
        compare_band_level(fails, lab, g, r, lattice_only=W >= 33)
        al, sc, _ = res[i]
        if al != r['final_alignments']:
            fails.append("%s: final spans differ" % lab)
        differ(fails, lab, "final scores", sc, r['alignment_scores'])
    assert not fails, "\n".join(fails[:40])
