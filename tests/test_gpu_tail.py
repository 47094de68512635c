"""The refinement chain's tail on the GPU -- svx_sparse_traceback, svx_search_path, svx_dense_traceback and the fused
traceback of svx_align_batch -- against the CPU oracle, on tables and alignments that no DP produced (tests/tail_ref.py;
tests/test_tail_ref_cpu.py pins the oracle to the real reference on them and shows which kernel mode each case reaches).

Spans, paths and statuses are exact.  The per-op scores are exact too (np.array_equal): one float64 subtraction, one
clip and two divisions in the oracle's order.  Rows of the buffers beyond the count are scratch and are not looked at.
Failure cases assert the status the kernel reports; every one of them is answered by a guard in front of the access
(include/svx.h states the rule), none relies on what an access outside the tables would do:

  sparse traceback (svx_dp.hip, tb_walk / sparse_traceback_block)
    end node or a walk node left / right of the band   the diagonal is tested against [window start, a_out) before
                                                       b_offset_out is read, the column against [0, B) before the
                                                       back-pointers are read, on every step, the first included
    -42, (0,0), px > x, py > y at a walk node          the step is tested after it is read and before it is taken, so
                                                       x, y and the diagonal never go negative
    origin outside the band (b_offset_out[0] = 1, -B)  tested after the walk, before the score pass; that pass reads
                                                       csum at walk nodes and at the origin only, all of them tested
    a_out < 1, B < 1, a negative size                  refused before anything is loaded
  dense traceback (dense_traceback_thread)
    3, -1, 7, 4 at a node of the walk                  the final else of the move table
    0 / 2 at x == 0, 0 / 1 at y == 0                   refused before the move, so no index goes negative and the walk
                                                       ends after at most s0 + s1 rows
  search path: xmax > size0 or ymax > size1            SVX_ERR_EXTEND before the first point is written"""
import numpy as np
import pytest

import tail_ref as T

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("name", list(T.TB_OK))
def test_sparse_traceback_on_foreign_tables(orc, name):
    from svx.vecalign import dp_utils
    t = T.tb_ok_case(name)
    args = (t['csum'], t['xp'], t['yp'], t['boff'], t['N'], t['M'])
    al_o, sc_o = orc.sparse_traceback(*args)
    al_g, sc_g = dp_utils.sparse_traceback(*args)
    assert al_g == al_o
    assert np.array_equal(sc_g, sc_o)


@pytest.mark.parametrize("spec", T.TB_FAIL, ids=T.tb_fail_id)
def test_sparse_traceback_failures(orc, spec):
    """SVX_ERR_TRACEBACK = the reference's 'traceback bug', in an LDS mode (B = 14, three windows) and from global memory
    (B = 160), with the offending node in the topmost, a middle and the lowest window."""
    from svx.vecalign import dp_utils
    t = T.tb_fail_case(spec)
    args = (t['csum'], t['xp'], t['yp'], t['boff'], t['N'], t['M'])
    with pytest.raises(Exception, match='^traceback bug$'):
        orc.sparse_traceback(*args)
    with pytest.raises(Exception, match='^traceback bug$'):
        dp_utils.sparse_traceback(*args)


def test_traceback_status_codes():
    """The raw counts behind the mirror's exceptions: -SVX_ERR_TRACEBACK, -SVX_ERR_EXTEND, -SVX_ERR_BP, and the texts
    _lib.DEVICE_ERRORS promises for them."""
    import torch
    from svx import _lib
    from svx.vecalign import dp_utils
    ctx = _lib.context()
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(ctx.tdev)
    p = dp_utils._p
    t = T.tb_fail_case(('origin_1', None, 14))
    cap = t['N'] + t['M'] + 2
    rows, scores = torch.zeros((cap, 4), dtype=torch.int32, device=ctx.tdev), torch.zeros(cap, dtype=torch.float64, device=ctx.tdev)
    cnt = torch.zeros(1, dtype=torch.int32, device=ctx.tdev)
    keep = [dev(t['csum'], np.float64), dev(t['xp'], np.int32), dev(t['yp'], np.int32), dev(t['boff'], np.int32)]
    ctx.check(ctx.lib.svx_sparse_traceback(ctx.h, p(keep[0]), p(keep[1]), p(keep[2]), p(keep[3]), int(t['csum'].shape[0]), int(t['B']),
                                           int(t['N']), int(t['M']), p(rows), p(scores), p(cnt)))
    assert int(cnt.cpu()[0]) == -_lib.SVX_ERR_TRACEBACK
    bp, _ = T.dense_fail_case(("value", 7, "middle"))
    dbp = dev(bp, np.int32)
    drows = torch.zeros((bp.shape[0] + bp.shape[1], 4), dtype=torch.int32, device=ctx.tdev)
    ctx.check(ctx.lib.svx_dense_traceback(ctx.h, p(dbp), bp.shape[0] - 1, bp.shape[1] - 1, p(drows), p(cnt)))
    assert int(cnt.cpu()[0]) == -_lib.SVX_ERR_BP
    al = T.sp_alignment((50, 0.5, True))
    xm, ym = T.up_max(al)
    arows = dev(dp_utils.alignments_to_rows(al), np.int32)
    na = dev(np.array([len(al)]), np.int32)
    path = torch.zeros((xm + ym + 4, 2), dtype=torch.int32, device=ctx.tdev)
    ctx.check(ctx.lib.svx_search_path(ctx.h, p(arows), p(na), 1, xm - 1, ym, p(path), p(cnt)))
    assert int(cnt.cpu()[0]) == -_lib.SVX_ERR_EXTEND
    assert _lib.DEVICE_ERRORS[_lib.SVX_ERR_TRACEBACK] == 'traceback bug'
    assert _lib.DEVICE_ERRORS[_lib.SVX_ERR_BP] == 'got unknown value'
    assert _lib.DEVICE_ERRORS[_lib.SVX_ERR_EXTEND] == T.EXTEND_TEXT


# ------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("g", T.SP_GRID, ids=T.sp_id)
def test_search_path_on_foreign_alignments(orc, g):
    from svx.vecalign import dp_utils
    al = T.sp_alignment(g)
    for label, up, s0, s1 in T.sp_calls(al):
        want = orc.search_path(al, up, s0, s1)
        got = dp_utils.make_search_path(al, s0, s1, upsample=True) if up else dp_utils.alignment_to_search_path(al)
        assert got == want, label
    xm, ym = T.up_max(al)
    assert dp_utils.make_search_path(al, xm, ym, upsample=True) == orc.search_path(al, True, xm, ym)   # 2X - 1, 2Y - 1 do not raise
    for s0, s1, bad in ((xm - 1, ym + 5, xm > 0), (xm + 5, ym - 1, ym > 0)):
        if bad:
            with pytest.raises(Exception, match=T.EXTEND_TEXT):
                orc.search_path(al, True, s0, s1)
            with pytest.raises(Exception, match=T.EXTEND_TEXT):
                dp_utils.make_search_path(al, s0, s1, upsample=True)


def test_search_path_lds_limit(orc):
    """9597 rows: search_path_block; the same alignment plus one row: search_path_thread.  Both against the oracle, and
    the points of the first 9597 rows agree between the two forms."""
    from svx.vecalign import dp_utils
    long = T.sp_long(T.SP_LDS_ROWS + 1)
    got = {}
    for rows in (T.SP_LDS_ROWS, T.SP_LDS_ROWS + 1):
        al = long[:rows]
        for label, up, s0, s1 in T.sp_calls(al)[:3]:
            assert T.sp_form(rows, s0, s1) == ('block' if rows == T.SP_LDS_ROWS else 'thread')
            got[rows, label] = dp_utils.make_search_path(al, s0, s1, upsample=True) if up else dp_utils.alignment_to_search_path(al)
            assert got[rows, label] == orc.search_path(al, up, s0, s1), (rows, label)
    short = long[:T.SP_LDS_ROWS]
    k = 1 + sum(len(a) + len(b) for a, b in short)
    assert got[T.SP_LDS_ROWS, "same"] == got[T.SP_LDS_ROWS + 1, "same"][:k]
    for label in ("up_0_0", "up_1_0"):
        assert got[T.SP_LDS_ROWS, label][:2 * k - 1] == got[T.SP_LDS_ROWS + 1, label][:2 * k - 1]


# ------------------------------------------------------------------------------------------ C
def test_dense_traceback_shapes_and_failures(orc):
    from svx.vecalign import dp_utils
    for name in T.DENSE_OK:
        bp = T.dense_ok_case(name)
        assert dp_utils.dense_traceback(bp) == orc.dense_traceback(bp), name
    for spec in T.DENSE_FAIL:   # unknown values at the first / a middle / the last step; moves off the lattice at each border
        bp, _ = T.dense_fail_case(spec)
        with pytest.raises(Exception, match='^got unknown value$'):
            orc.dense_traceback(bp)
        with pytest.raises(Exception, match='^got unknown value$'):
            dp_utils.dense_traceback(bp)


# ------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("W", sorted(T.SHIFTED))
def test_fused_traceback_with_a_drifting_walk(orc, W):
    """Straight search on a shifted pair: the walk's band column moves by one per diagonal across J / 2 columns and back.
    W = 158: packed back-pointers in 64-diagonal windows (tb_walk<1>); 159 / 160 / 161: packed, global memory (tb_walk<0>);
    168: the smallest corridor (tb_walk<3>, origins 0 and 16); 400: a wide corridor whose origin moves several times;
    79 / 80 with a (20, 1) type: int32 back-pointers in windows (tb_walk<2>) and from global memory.  Identical spans,
    scores within SCORE_TOL of the oracle's straight pipeline."""
    import dp_ref
    from stage_check import SCORE_TOL
    from svx.vecalign import dp_utils
    v0, v1, types, rseed = T.shifted_case(W)
    st = dp_ref.straight_stack(orc, v0, v1, types, W, rseed)
    al_g, sc_g = dp_utils.align_band(v0, v1, types, dp_ref.FRAC, W, dp_ref.SAMPLE, dp_ref.NSAMP, rng=np.random.RandomState(rseed))
    assert al_g == st['final_alignments']
    assert np.abs(np.asarray(sc_g) - st['alignment_scores']).max() <= SCORE_TOL
