"""svx_band_contact on the GPU (include/svx.h) against tests/contact_ref.py: the four numbers are integers and must be
equal, both to the reference applied to the GPU's own level views (PreparedBatch.level_stack) and to the reference
applied to the CPU oracle's stack of the same search.  float32 inputs, d = 32."""
import ctypes

import numpy as np
import pytest

from around_ref import SVX_ERR_ARG, SVX_ERR_TRACEBACK, around_stack, block_deletion_pair, block_prior
from contact_ref import INT32_MAX, contact, contact_of_stack
from dp_ref import straight_stack
from synth import alignment_types, make_pair

pytestmark = pytest.mark.gpu
TYPES5 = alignment_types(5)
NONE = (-1, -1, -1, -1)


def to_dev(v):
    import torch
    return torch.from_numpy(v).cuda()


def batch(docs, W, seeds, search="straight", priors=None, max_full=300):
    from svx.vecalign import dp_utils
    kw = dict(priors=priors) if search in ("around", "around_wide") else {}
    return dp_utils.PreparedBatch([(to_dev(a), to_dev(b)) for a, b in docs], TYPES5, 0.2, W, max_full, 20000, 100,
                                  rngs=[np.random.RandomState(s) for s in seeds], search=search, **kw)


def got_rows(pb, level=0, guard=0):
    return [tuple(r) for r in pb.band_contact(level, guard).cpu().numpy().tolist()]


def from_views(pb, i, level, guard=0):
    """contact_ref on the GPU's own view of pair i at `level`; a level without a band gives the -1 row."""
    if level >= pb.levels[i]:
        return NONE
    st = pb.level_stack(i, level)
    if 'new_b_offset' not in st:
        return NONE
    return contact(st['alignments'], st['new_b_offset'], st['a_b_csum'].shape[1], st['size0'], st['size1'], guard)


@pytest.fixture(scope="module")
def deletion_pair():
    return block_deletion_pair(seed=0)


# ---------------------------------------------------------------------------------------------- 1
def test_straight_band_on_the_block_deletion_pair(orc, deletion_pair):
    v0, v1, _ = deletion_pair
    pb = batch([(v0, v1)], 7, [11])
    pb.run()
    ref = straight_stack(orc, v0, v1, TYPES5, 7, 11)
    for guard, want in ((0, (20, 11, 0, 220)), (2, (59, 37, 0, 220))):
        got = got_rows(pb, 0, guard)
        assert got == [want]
        assert got == [from_views(pb, 0, 0, guard)] and got == [contact_of_stack(ref, guard)]


# ---------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("W, guard, deletions", [(7, 0, 10), (3, 1, 40)])
def test_coarse_to_fine_levels(orc, W, guard, deletions):
    """300 x 280 with max_size_full_dp = 100: levels 0 and 1 have a band, level 2 is the dense stage (-1 row), and so is
    every level the pair does not have.  W = 3 with guard 1 touches at both refined levels."""
    v0, v1 = make_pair(300, 280, 4, 32, 0, deletions=deletions)
    pb = batch([(v0, v1)], W, [11], search="coarse_to_fine", max_full=100)
    pb.run()
    ref = orc.vecalign(v0.copy(), v1.copy(), TYPES5, 0.2, W, 100, 20000, 100, rng=np.random.RandomState(11))
    assert len(ref) == 3 and pb.levels[0] == 3
    for level in (0, 1):
        got = got_rows(pb, level, guard)
        assert got == [from_views(pb, 0, level, guard)] and got == [contact_of_stack(ref[level], guard, W)]
        assert (got[0][0] > 0) == (guard == 1)
    assert got_rows(pb, 2, guard) == [NONE] and got_rows(pb, 3, guard) == [NONE] and got_rows(pb, 15, guard) == [NONE]


# ---------------------------------------------------------------------------------------------- 3
def test_around_a_block_prior(orc, deletion_pair):
    v0, v1, src = deletion_pair
    prior = block_prior(src, 300)
    pb = batch([(v0, v1)], 7, [11], search="around", priors=[prior])
    pb.run()
    ref = around_stack(orc, v0, v1, TYPES5, 7, 11, prior)
    got = got_rows(pb)
    assert got == [(0, 0, 3, 285)] and got == [from_views(pb, 0, 0)] and got == [contact_of_stack(ref)]
    assert got_rows(pb, 0, 3)[0][0] > 0 and got_rows(pb, 0, 3) == [contact_of_stack(ref, 3)]


# ---------------------------------------------------------------------------------------------- 4
def test_tile_sweep_band_of_80_cells(orc, deletion_pair):
    """around_wide at W = 40 runs the tile sweep, which writes new_b_offset itself."""
    v0, v1, src = deletion_pair
    prior = [(list(range(300)), list(range(180)))]
    pb = batch([(v0, v1)], 40, [11], search="around_wide", priors=[prior])
    pb.run()
    assert 'a_b_costs' not in pb.level_stack(0, 0)
    ref = around_stack(orc, v0, v1, TYPES5, 40, 11, prior)
    for guard in (0, 15):
        got = got_rows(pb, 0, guard)
        assert got == [from_views(pb, 0, 0, guard)] and got == [contact_of_stack(ref, guard)]
    assert got_rows(pb) == [(0, 0, 15, 285)] and got_rows(pb, 0, 15)[0][0] > 0


def test_band_wider_than_the_lattice_has_no_real_side():
    v0, v1 = make_pair(60, 50, 4, 32, 2, deletions=2)
    pb = batch([(v0, v1)], 61, [5])
    pb.run()
    got = got_rows(pb, 0, 1000)
    assert got[0][:3] == (0, 0, INT32_MAX) and got == [from_views(pb, 0, 0, 1000)]


# ---------------------------------------------------------------------------------------------- 5
def test_ragged_batch_with_a_failed_prior(orc):
    import torch
    sizes = [(300, 280), (211, 333), (120, 97), (64, 1)]
    docs = [make_pair(n, m, 4, 32, seed=40 + i) for i, (n, m) in enumerate(sizes)]
    whole = [[(list(range(n)), list(range(m)))] for n, m in sizes]
    failed = (torch.tensor([[0, 60, 0, 50], [60, 60, 50, 47]], dtype=torch.int32).cuda(),
              torch.tensor([2, SVX_ERR_TRACEBACK], dtype=torch.int32).cuda())
    priors = [whole[0], whole[1], failed, whole[3]]
    seeds = [900, 901, 902, 903]
    pb = batch(docs, 7, seeds, search="around", priors=priors)
    pb.run()
    for guard in (0, 2):
        got = got_rows(pb, 0, guard)
        assert got[2] == NONE
        for i in (0, 1, 3):
            ref = around_stack(orc, docs[i][0], docs[i][1], TYPES5, 7, seeds[i], whole[i])
            assert got[i] == from_views(pb, i, 0, guard) and got[i] == contact_of_stack(ref, guard), i
    assert pb.info.cpu().numpy()[2].tolist() == [0, SVX_ERR_TRACEBACK]


# ---------------------------------------------------------------------------------------------- 6
def test_pipeline_on_covers_both_halves(orc):
    from svx import _lib
    trio = [block_deletion_pair(seed=s) for s in range(3)]
    docs = [(a, b) for a, b, _ in trio]
    ctx = _lib.context()
    try:
        ctx.set_pipeline(True)
        pb = batch(docs, 7, [11, 11, 11])
        pb.run()                      # the second half's chain is still held back: svx_band_contact flushes
        got = got_rows(pb)
        got2 = got_rows(pb, 0, 2)
    finally:
        ctx.set_pipeline(False)
    assert [g[0] for g in got] == [20, 26, 40]
    for i, (a, b) in enumerate(docs):
        ref = straight_stack(orc, a, b, TYPES5, 7, 11)
        assert got[i] == contact_of_stack(ref) and got2[i] == contact_of_stack(ref, 2)
        assert got[i] == from_views(pb, i, 0)


# ---------------------------------------------------------------------------------------------- 7
def test_runs_across_waves_and_stretches(orc):
    """520 nodes: three stretches of 256, runs of up to 98 nodes (guard 2) that cross wave and stretch boundaries."""
    v0, v1, _ = block_deletion_pair(N=700, lo=250, hi=500, seed=3)
    pb = batch([(v0, v1)], 7, [11])
    pb.run()
    ref = straight_stack(orc, v0, v1, TYPES5, 7, 11)
    assert got_rows(pb) == [(63, 15, 0, 520)] and got_rows(pb, 0, 2) == [(178, 98, 0, 520)]
    for guard in (0, 1, 2, 5, 13):
        got = got_rows(pb, 0, guard)
        assert got == [contact_of_stack(ref, guard)] and got == [from_views(pb, 0, 0, guard)]


# ---------------------------------------------------------------------------------------------- 8
def test_argument_errors_queue_nothing(deletion_pair):
    import torch
    from svx import _lib
    v0, v1, _ = deletion_pair
    pb = batch([(v0, v1)], 7, [11])
    pb.run()
    ctx = pb.ctx
    out = torch.full((1, 4), -7, dtype=torch.int32).cuda()
    ptr = ctypes.c_void_p(out.data_ptr())
    for args in ((-1, 0, ptr), (0, -1, ptr), (0, 0, None)):
        with pytest.raises(_lib.SvxError) as e:
            ctx.check(ctx.lib.svx_band_contact(ctx.h, *args))
        assert e.value.code == SVX_ERR_ARG and len(str(e.value)) > 10
    assert ctx.lib.svx_band_contact(None, 0, 0, ptr) == SVX_ERR_ARG
    fresh = _lib.Context(0)           # a context without an earlier call
    fresh.use_current_stream()
    with pytest.raises(_lib.SvxError) as e:
        fresh.check(fresh.lib.svx_band_contact(fresh.h, 0, 0, ptr))
    assert e.value.code == SVX_ERR_ARG and "no earlier" in str(e.value)
    ctx.sync()
    assert (out.cpu().numpy() == -7).all()
    assert got_rows(pb) == [(20, 11, 0, 220)]          # the context still works
    # a call that fails while it lays out its batch leaves no batch behind: the descriptors of the one before are gone
    from svx.vecalign import dp_utils
    bad = dp_utils.PreparedBatch([(to_dev(v0), to_dev(v1))], alignment_types(7), 0.2, 7, 300, 20000, 100,
                                 rngs=[np.random.RandomState(1)], search="straight")
    with pytest.raises(Exception, match="overlaps"):
        bad.run()
    with pytest.raises(_lib.SvxError) as e:
        pb.band_contact()
    assert e.value.code == SVX_ERR_ARG and "no earlier" in str(e.value)
    ctx.sync()
    assert (out.cpu().numpy() == -7).all()
