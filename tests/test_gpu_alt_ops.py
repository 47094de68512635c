"""svx_path_alternatives against alt_ref, bit for bit and row for row, on exact costs (family P of dp_ref: float32 k/8
costs, a tenth +inf, dyadic penalty -- every float64 sum is exact, ties are the norm, so the order key decides most edges).
The planes come from svx_sparse_dp and svx_sparse_dp_backward; the rows are the back-pointer walk's.  Covers every band
width class of the cut scan (B = 14 / 24 / 40 / 96 / 2000) over every type count, and the edges: no types, 1 x 1 and 1 x 9
documents, steps of 17, an end node outside the band, detours cut short by max_detour and max_slack, rows of garbage."""
import ctypes

import numpy as np
import pytest

import alt_ref
import dp_ref
import slack_ref
from test_gpu_slack_ops import first_diff, same_bits, small_inputs

pytestmark = pytest.mark.gpu
INF = np.inf


def garbage_rows(N, M):
    big = 2 ** 31 - 1
    return np.asarray([(-1, 1, 0, 1), (0, 1, -1, 1), (0, -1, 0, 1), (0, 1, 0, -1), (0, 0, 0, 0), (big, 1, big, 1), (big, big, big, big),
                       (-big - 1, 1, 5, 1), (N, 1, M, 1), (N + 5, 1, 0, 1), (0, 1, M + 9, 1), (3, 7, 3, 7), (0, 2, 0, 0), (5, 1, 25, 1),
                       (N - 1, 1, M - 1, 2)], np.int32)


def given_rows(rows, types, N, M, seed):
    """The path's own rows, 40 random rows of the lattice with moves of the list, and rows of garbage."""
    rs = np.random.RandomState(seed)
    mv = dp_ref._moves(types)
    rnd = [(rs.randint(0, N + 1), mv[k][0], rs.randint(0, M + 1), mv[k][1]) for k in rs.randint(0, len(mv), 40)]
    return np.concatenate([rows.reshape(-1, 4), np.asarray(rnd, np.int32), garbage_rows(N, M)]).astype(np.int32)


def compare(got, want, K, label=""):
    n = len(want['slack'])
    assert same_bits(got['slack'], want['slack']), label + " slack: " + first_diff(got['slack'], want['slack'])
    assert np.array_equal(got['edge'], want['edge']), (label, np.flatnonzero((got['edge'] != want['edge']).any(1))[:5])
    assert np.array_equal(got['span'], want['span']), (label, [(int(r), got['span'][r].tolist(), want['span'][r].tolist())
                                                               for r in np.flatnonzero((got['span'] != want['span']).any(1))[:5]])
    if 'detour' not in got:
        return
    for r in range(n):
        k = 0
        if want['span'][r, 3] == 0:
            drows, dsc = want['detours'][r]
            k = len(drows)
            assert np.array_equal(got['detour'][r, :k], drows), (label, r, got['detour'][r, :k].tolist(), drows.tolist())
            assert same_bits(got['detour_scores'][r, :k], dsc), (label, r)
        assert (got['detour'][r, k:] == -1).all() and np.isnan(got['detour_scores'][r, k:]).all(), (label, r, "slots past the detour")


def run_case(f, bo, types, pen, N, M, K, max_slack=INF, given=None, rows=None, detour=True, label=""):
    """-> (GPU result, reference, rows) after comparing all of it; the reference also carries the planes csum and bsum."""
    from svx.vecalign import dp_core, dp_utils
    csum, xp, yp, bout = dp_core.sparse_dp(f, bo, types, pen, N, M)
    bk = dp_utils.sparse_dp_backward(f, bo, types, pen, N, M)
    B = f.shape[2]
    end = slack_ref.end_cell(bout, B, N, M)
    if rows is None:
        rows = np.zeros((0, 4), np.int32)
        if end is not None and np.isfinite(csum[end]):
            rows = slack_ref.traceback(xp, yp, bout, B, N, M)
    if isinstance(given, str) and given == "mixed":
        given = given_rows(rows, types, N, M, 7 + N + B)
    got = dp_utils.path_alternatives(f, bo, types, pen, N, M, csum, bk, xp, yp, rows, max_detour=K, max_slack=max_slack, given=given,
                                     detour=detour)
    want = alt_ref.alternatives(f, bo, types, pen, N, M, csum, bk, xp, yp, rows, K, max_slack, want_detours=detour)
    compare(got, want, K, label)
    if given is not None:
        wr = alt_ref.regret(f, bo, types, pen, N, M, csum, bk, given)
        assert same_bits(got['regret'], wr), label + " regret: " + first_diff(got['regret'], wr)
        want['regret'] = wr
    want['csum'], want['bsum'] = csum, bk
    return got, want, rows


@pytest.mark.parametrize("case", dp_ref.P_SPARSE, ids=[c[0] for c in dp_ref.P_SPARSE])
def test_alternatives_family_p(case):
    f, bo, types, pen, N, M = dp_ref.p_sparse_inputs(case)
    got, want, rows = run_case(f, bo, types, pen, N, M, 136, given="mixed", label=case[0])
    if not len(rows):
        return
    assert not (got['span'][:, 3] == 1).any()   # no detour of these inputs has more than 136 rows
    assert (got['span'][:, 3] == 0).any()
    assert same_bits(got['slack'], slack_ref.slack(f, bo, types, pen, N, M, want['csum'], want['bsum'], rows))
    n = len(rows)
    assert np.array_equal(got['regret'][:n], np.zeros(n))                      # the returned rows
    assert np.isnan(np.delete(got['regret'][n + 40:], 13)).all()               # the garbage ((5, 1, 25, 1) is an edge of the wider bands)
    for r in np.flatnonzero(got['span'][:, 3] == 0):
        lo, hi = got['span'][r, :2]
        assert lo <= r < hi


def test_slack_bits_are_path_slack_bits():
    from svx.vecalign import dp_utils
    f, bo, types, pen, N, M = dp_ref.p_sparse_inputs(dp_ref.P_SPARSE[2])
    got, want, rows = run_case(f, bo, types, pen, N, M, 16)
    assert same_bits(got['slack'], dp_utils.path_slack(f, bo, types, pen, N, M, want['csum'], want['bsum'], rows))


def test_steps_of_17():
    types = [(1, 1), (16, 1), (1, 16), (8, 9), (2, 1), (1, 2)]
    f, bo, types, pen, N, M = small_inputs(40, 37, types, 30, 0.375, 3)
    got, _, rows = run_case(f, bo, types, pen, N, M, 80, given="mixed")
    assert len(rows) and (got['span'][:, 3] == 0).any()


@pytest.mark.parametrize("N,M", [(1, 1), (1, 9)])
def test_tiny_documents(N, M):
    f, bo, types, pen, N, M = small_inputs(N, M, dp_ref.alignment_types(3), 6, 0.375, 10 + M)
    run_case(f, bo, types, pen, N, M, 16, given="mixed")


def test_no_types_deletions_only():
    f, bo, types, pen, N, M = small_inputs(9, 7, [], 6, 0.25, 1)
    got, _, rows = run_case(f, bo, types, pen, N, M, 20, given="mixed")
    assert len(rows) == N + M and (got['edge'][:, 0] >= 0).any()


def test_end_node_outside_the_band():
    f, bo, types, pen, N, M = small_inputs(20, 18, dp_ref.alignment_types(4), 8, 0.25, 5)
    bo = bo.copy()
    bo[-1] = M + 3
    assert slack_ref.end_cell(slack_ref.b_offset_out(bo), 8, N, M) is None
    rows = np.asarray([(0, 1, 0, 1), (1, 0, 1, 1), (1, 1, 2, 1)], np.int32)
    got, _, _ = run_case(f, bo, types, pen, N, M, 16, given=rows, rows=rows)
    assert (got['span'] == (-1, -1, -1, 2)).all() and (got['edge'] == -1).all()
    assert np.isnan(got['regret']).all() and np.isnan(got['slack']).all()


def test_max_slack_and_edges_only():
    f, bo, types, pen, N, M = dp_ref.p_sparse_inputs([c for c in dp_ref.P_SPARSE if c[0] == "B24_T10"][0])
    full, _, rows = run_case(f, bo, types, pen, N, M, 136)
    part, _, _ = run_case(f, bo, types, pen, N, M, 136, max_slack=0.0)
    measured = part['span'][:, 3] != 2
    assert measured.any() and not measured.all()
    assert np.array_equal(measured, full['slack'] <= 0.0)
    none, _, _ = run_case(f, bo, types, pen, N, M, 136, max_slack=-1.0)
    assert (none['span'][:, 3] == 2).all() and np.array_equal(none['edge'], full['edge'])
    edges, _, _ = run_case(f, bo, types, pen, N, M, 136, detour=False)
    assert (edges['span'] == (-1, -1, -1, 2)).all() and np.array_equal(edges['edge'], full['edge'])


def test_short_cap_leaves_slots_and_guard_words_alone():
    """K = 2: most detours are too long.  Sentinel-filled detour slots of rows without a written detour and the guard words
    around every output keep their values; a row count below the capacity writes nothing past it."""
    import torch
    from svx import _lib
    from svx.vecalign import dp_core, dp_utils
    from svx.vecalign.dp_core import _types
    case = [c for c in dp_ref.P_SPARSE if c[0] == "B14_T10"][0]
    f, bo, types, pen, N, M = dp_ref.p_sparse_inputs(case)
    K, B, G = 2, f.shape[2], 16
    csum, xp, yp, bout = dp_core.sparse_dp(f, bo, types, pen, N, M)
    bk = dp_utils.sparse_dp_backward(f, bo, types, pen, N, M)
    rows = slack_ref.traceback(xp, yp, bout, B, N, M)
    given = given_rows(rows, types, N, M, 3)
    n, ng = len(rows), len(given)
    want = alt_ref.alternatives(f, bo, types, pen, N, M, csum, bk, xp, yp, rows, K)
    assert (want['span'][:, 3] == 1).any() and (want['span'][:, 3] == 0).any()
    ctx = _lib.context()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = [dev(x) for x in (f, bo, csum, bk, xp, yp, rows)]
    tarr, T = _types(types)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    sizes = dict(slack=(n, torch.float64), edge=(4 * n, torch.int32), span=(4 * n, torch.int32), detour=(4 * K * n, torch.int32),
                 detour_scores=(K * n, torch.float64), regret=(ng, torch.float64))

    def call(count):
        bufs = {k: torch.full((G + sz + G,), -7 if dt == torch.int32 else -7.25, dtype=dt, device="cuda") for k, (sz, dt) in sizes.items()}
        one = _lib.Alt()
        for k, b in bufs.items():
            setattr(one, k, b.data_ptr() + G * b.element_size())
        dg, dinfo, dcnt = dev(given), dev(np.asarray([ng, 0], np.int32)), dev(np.asarray([count], np.int32))
        one.given, one.given_info, one.given_cap = dg.data_ptr(), dinfo.data_ptr(), ng
        ctx.check(ctx.lib.svx_path_alternatives(ctx.h, p(d[0]), p(d[1]), N + M - 1, B, tarr, T, float(pen), N, M, p(d[2]), p(d[3]), p(d[4]),
                                                p(d[5]), p(d[6]), p(dcnt), n, ctypes.byref(one), K, float("inf")))
        out = {k: b.cpu().numpy() for k, b in bufs.items()}
        for k, a in out.items():
            sentinel = -7 if a.dtype == np.int32 else -7.25
            assert (a[:G] == sentinel).all() and (a[-G:] == sentinel).all(), k + ": guard words"
        return {k: a[G:-G] for k, a in out.items()}

    out = call(n)
    assert same_bits(out['slack'], want['slack'])
    assert np.array_equal(out['edge'].reshape(n, 4), want['edge']) and np.array_equal(out['span'].reshape(n, 4), want['span'])
    det, sc = out['detour'].reshape(n, K, 4), out['detour_scores'].reshape(n, K)
    for r in range(n):
        k = 0
        if want['span'][r, 3] == 0:
            k = len(want['detours'][r][0])
            assert np.array_equal(det[r, :k], want['detours'][r][0]) and same_bits(sc[r, :k], want['detours'][r][1])
        assert (det[r, k:] == -7).all() and (sc[r, k:] == -7.25).all(), r
    assert same_bits(out['regret'], alt_ref.regret(f, bo, types, pen, N, M, csum, bk, given))
    # ---- a count below the capacity
    out = call(3)
    assert same_bits(out['slack'][:3], want['slack'][:3]) and (out['slack'][3:] == -7.25).all()
    assert (out['edge'][12:] == -7).all() and (out['span'][12:] == -7).all() and (out['detour'][4 * K * 3:] == -7).all()


def test_argument_errors():
    import torch
    from svx import _lib
    from svx.vecalign.dp_core import _types
    f, bo, types, pen, N, M = small_inputs(9, 7, dp_ref.alignment_types(3), 6, 0.25, 1)
    ctx = _lib.context()
    buf = torch.zeros(4096, dtype=torch.int32, device="cuda")
    tarr, T = _types(types)
    vp = ctypes.c_void_p
    b = buf.data_ptr()

    def call(K=4, max_slack=0.5, **kw):
        one = _lib.Alt()
        one.edge, one.span, one.detour = b, b + 1024, b + 2048
        for k, v in kw.items():
            setattr(one, k, v)
        return ctx.lib.svx_path_alternatives(ctx.h, vp(b), vp(b), N + M - 1, 6, tarr, T, 0.25, N, M, vp(b), vp(b), vp(b), vp(b), vp(b), vp(b),
                                             4, ctypes.byref(one), K, max_slack)
    for kw, text in ((dict(K=0), "max_detour 0 outside [1, 256]"), (dict(K=257), "max_detour 257 outside [1, 256]"),
                     (dict(max_slack=float("nan")), "max_slack is NaN"), (dict(edge=None), "null edge / span"),
                     (dict(span=b + 4), "16-byte aligned"), (dict(detour=b + 8), "16-byte aligned"),
                     (dict(given=b, given_info=b), "given rows need regret")):
        rc = call(**kw)
        assert rc != 0 and text in ctx.lib.svx_last_error(ctx.h).decode(), (text, ctx.lib.svx_last_error(ctx.h).decode())
    ctx.sync()
    assert not buf.cpu().numpy().any()
