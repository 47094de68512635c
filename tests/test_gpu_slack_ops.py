"""svx_sparse_dp_backward and svx_path_slack against slack_ref, bit for bit, on exact costs (family P of dp_ref: float32
k/8 costs, a tenth +inf, dyadic penalty -- every float64 sum is exact, ties are the norm).  The forward planes come from
svx_sparse_dp.  Covers every kernel the backward sweep can take: the LDS-staged sweep at B = 14 / 24 / 40 over every type
count, the strided kernel with its ring in LDS (B = 96) and without (B = 2000), and the edges: no types, 1 x 1 and 1 x 9
documents, steps of 17, an end node on the outermost cell of its diagonal or outside the band, and rows of garbage."""
import numpy as np
import pytest

import dp_ref
import slack_ref

pytestmark = pytest.mark.gpu


def same_bits(got, want):
    """Equal bit for bit where finite, the same infinities, NaN where NaN."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def first_diff(got, want):
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    return "%d of %d entries differ, first at %s: %r vs %r" % (len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def run_case(f, bo, types, pen, N, M, extra_rows=None, want_path=True):
    """-> (bsum, slack, rows, csum) of the GPU, after comparing all of it with slack_ref."""
    from svx.vecalign import dp_core, dp_utils
    csum, xp, yp, bout = dp_core.sparse_dp(f, bo, types, pen, N, M)
    bk = dp_utils.sparse_dp_backward(f, bo, types, pen, N, M)
    want_bk = slack_ref.backward(f, bo, types, pen, N, M)
    assert same_bits(bk, want_bk), "bsum: " + first_diff(bk, want_bk)
    B = f.shape[2]
    end = slack_ref.end_cell(bout, B, N, M)
    rows = np.zeros((0, 4), np.int32)
    if want_path and end is not None and np.isfinite(csum[end]):
        rows = slack_ref.traceback(xp, yp, bout, B, N, M)
    if extra_rows is not None:
        rows = np.concatenate([rows, np.asarray(extra_rows, np.int32).reshape(-1, 4)])
    sl = dp_utils.path_slack(f, bo, types, pen, N, M, csum, bk, rows)
    want_sl = slack_ref.slack(f, bo, types, pen, N, M, csum, want_bk, rows)
    assert same_bits(sl, want_sl), "slack: " + first_diff(sl, want_sl)
    return bk, sl, rows, csum


@pytest.mark.parametrize("case", dp_ref.P_SPARSE, ids=[c[0] for c in dp_ref.P_SPARSE])
def test_backward_and_slack_family_p(case):
    f, bo, types, pen, N, M = dp_ref.p_sparse_inputs(case)
    bk, sl, rows, csum = run_case(f, bo, types, pen, N, M)
    bout = slack_ref.b_offset_out(bo)
    end = slack_ref.end_cell(bout, f.shape[2], N, M)
    assert end is not None
    total = csum[end]
    if not len(rows):
        assert not np.isfinite(total)
        return
    # exact sums: the invariants hold with ==
    assert not np.isnan(sl).any() and sl.min() >= 0.0
    nodes = [(0, 0)] + [(r[0] + r[1], r[2] + r[3]) for r in rows.tolist()]
    for x, y in nodes:
        cell = (x + y, y - int(bout[x + y]))
        assert csum[cell] + bk[cell] == total, (x, y)
    if case[6] in ("equal", "zero"):
        assert (sl == 0.0).any()


def small_inputs(N, M, types, B, pen, seed, L=3, shift=None):
    """Family-P costs on a band of B cells around the straight path of an N x M lattice."""
    A = N + M - 1
    rs = np.random.RandomState(seed)
    sh = B // 2 if shift is None else shift
    bo = np.asarray([((k + 2) * M + (N + M) // 2) // (N + M) - 1 - sh for k in range(A)], np.int32)
    return dp_ref.p_costs(rs, (len(types), A, B), L), bo, list(types), pen, N, M


def test_no_types_deletions_only():
    f, bo, types, pen, N, M = small_inputs(9, 7, [], 6, 0.25, 1)
    bk, sl, rows, _ = run_case(f, bo, types, pen, N, M)
    assert len(rows) == N + M and np.isfinite(bk).any()


@pytest.mark.parametrize("N,M", [(1, 1), (1, 9)])
def test_tiny_documents(N, M):
    f, bo, types, pen, N, M = small_inputs(N, M, dp_ref.alignment_types(3), 6, 0.375, 10 + M)
    run_case(f, bo, types, pen, N, M)


def test_steps_of_17_ring_depth():
    types = [(1, 1), (16, 1), (1, 16), (8, 9), (2, 1), (1, 2)]
    f, bo, types, pen, N, M = small_inputs(40, 37, types, 30, 0.375, 3)
    bk, sl, rows, _ = run_case(f, bo, types, pen, N, M)
    assert np.isfinite(bk).any()


@pytest.mark.parametrize("edge", ["first", "last"])
def test_end_node_on_the_outermost_cell(edge):
    B = 8
    f, bo, types, pen, N, M = small_inputs(20, 18, dp_ref.alignment_types(4), B, 0.25, 4)
    bo = bo.copy()
    bo[-1] = (M - 1) if edge == "first" else (M - 1) - (B - 1)   # b of (N, M) = M - (bo[-1] + 1)
    bout = slack_ref.b_offset_out(bo)
    assert slack_ref.end_cell(bout, B, N, M) == (N + M, 0 if edge == "first" else B - 1)
    bk, _, _, _ = run_case(f, bo, types, pen, N, M)
    assert bk[N + M, 0 if edge == "first" else B - 1] == 0.0


def test_end_node_outside_the_band_is_all_inf():
    f, bo, types, pen, N, M = small_inputs(20, 18, dp_ref.alignment_types(4), 8, 0.25, 5)
    bo = bo.copy()
    bo[-1] = M + 3
    assert slack_ref.end_cell(slack_ref.b_offset_out(bo), 8, N, M) is None
    bk, sl, _, _ = run_case(f, bo, types, pen, N, M, extra_rows=[(0, 1, 0, 1), (0, 0, 0, 1)], want_path=False)
    assert np.isposinf(bk).all()
    assert np.isnan(sl).all()   # alt and total are both +inf


def test_garbage_rows_give_nan_and_touch_nothing_else():
    """Rows that hold anything: NaN, no fault, and the words around `slack` keep their values."""
    import ctypes
    import torch
    from svx import _lib
    from svx.vecalign import dp_core, dp_utils
    from svx.vecalign.dp_core import _types
    f, bo, types, pen, N, M = small_inputs(30, 28, dp_ref.alignment_types(5), 14, 0.375, 6)
    csum, xp, yp, bout = dp_core.sparse_dp(f, bo, types, pen, N, M)
    bk = dp_utils.sparse_dp_backward(f, bo, types, pen, N, M)
    good = slack_ref.traceback(xp, yp, bout, 14, N, M)
    big = 2 ** 31 - 1
    bad = np.asarray([(-1, 1, 0, 1), (0, 1, -1, 1), (0, -1, 0, 1), (0, 1, 0, -1), (0, 0, 0, 0), (big, 1, big, 1), (big, big, big, big),
                      (-big - 1, 1, 5, 1), (N, 1, M, 1), (N + 5, 1, 0, 1), (0, 1, M + 9, 1), (3, 7, 3, 7), (0, 2, 0, 0), (5, 1, 25, 1),
                      (N - 1, 1, M - 1, 2)], np.int32)
    rows = np.concatenate([good[:5], bad, good[5:]])
    n, guard = len(rows), 16
    ctx = _lib.context()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    buf = torch.full((guard + n + guard,), -7.25, dtype=torch.float64, device="cuda")
    d = [dev(x) for x in (f, bo, csum, bk, rows, np.asarray([n], np.int32))]
    tarr, T = _types(types)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    ctx.check(ctx.lib.svx_path_slack(ctx.h, p(d[0]), p(d[1]), N + M - 1, 14, tarr, T, float(pen), N, M, p(d[2]), p(d[3]), p(d[4]), p(d[5]),
                                     n, ctypes.c_void_p(buf.data_ptr() + 8 * guard)))
    out = buf.cpu().numpy()
    assert (out[:guard] == -7.25).all() and (out[guard + n:] == -7.25).all()
    sl = out[guard:guard + n]
    want = slack_ref.slack(f, bo, types, pen, N, M, csum, bk, rows)
    assert np.isnan(want[5:5 + len(bad)]).all() and not np.isnan(want[:5]).any()
    assert same_bits(sl, want), first_diff(sl, want)
    # a count below the capacity: nothing past it is written
    buf.fill_(-7.25)
    d[5] = dev(np.asarray([3], np.int32))
    ctx.check(ctx.lib.svx_path_slack(ctx.h, p(d[0]), p(d[1]), N + M - 1, 14, tarr, T, float(pen), N, M, p(d[2]), p(d[3]), p(d[4]), p(d[5]),
                                     n, ctypes.c_void_p(buf.data_ptr() + 8 * guard)))
    out = buf.cpu().numpy()
    assert same_bits(out[guard:guard + 3], want[:3]) and (out[guard + 3:] == -7.25).all() and (out[:guard] == -7.25).all()
