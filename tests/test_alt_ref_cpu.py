"""alt_ref against brute force and against its own invariants (CPU only).

Family-P costs (dp_ref.p_costs: float32 k/8, a tenth +inf, dyadic penalty) make every float64 sum exact, so the totals of
enumerated paths, alt, the spliced paths' totals and the regrets are compared with ==."""
import numpy as np
import pytest

import alt_ref
import dp_ref
import slack_ref
from test_slack_ref_cpu import CASES, Brute, case_id, make_case

INF = np.inf


def planes(f, bo, types, pen, N, M):
    csum, xp, yp, bout = dp_ref.sparse_dp(f, bo, types, pen, N, M)
    bk = slack_ref.backward(f, bo, types, pen, N, M)
    end = slack_ref.end_cell(bout, f.shape[2], N, M)
    rows = np.zeros((0, 4), np.int32)
    if end is not None and np.isfinite(csum[end]):
        rows = slack_ref.traceback(xp, yp, bout, f.shape[2], N, M)
    return csum, bk, xp, yp, bout, rows


def used_set(L, rows):
    """The path as Brute.paths() names it: frozenset of ((diagonal, cell) of u, move)."""
    return frozenset(((x0 + y0, L.cell(x0, y0)), (xl, yl)) for x0, xl, y0, yl in np.asarray(rows).reshape(-1, 4).tolist())


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_alternatives_vs_brute_force(case):
    N, M, a, band, mode = case
    f, bo, types, pen, N, M = make_case(N, M, a, band, mode, 31 * N + 7 * M + a)
    csum, bk, xp, yp, bout, rows = planes(f, bo, types, pen, N, M)
    if not len(rows):
        return
    paths = Brute(f, bo, types, pen, N, M).paths()
    by_set = {used: tot for tot, used in paths}
    L = alt_ref.Lattice(f, bo, types, pen, N, M, csum, bk, xp, yp)
    alt = alt_ref.alternatives(f, bo, types, pen, N, M, csum, bk, xp, yp, rows, max_detour=N + M + 2)
    assert alt['summary'][0] == len(rows) and alt['summary'][3] == 0
    for r, row in enumerate(rows.tolist()):
        key = ((row[0] + row[2], L.cell(row[0], row[2])), (row[1], row[3]))
        want = min((t for t, used in paths if key not in used), default=INF)
        assert alt['alt'][r] == want, (r, row)
        assert alt['slack'][r] == want - L.total
        if want == INF:
            assert tuple(alt['edge'][r]) == alt_ref.NO_EDGE and tuple(alt['span'][r]) == (-1, -1, -1, 2)
            continue
        lo, hi, nd, status = alt['span'][r]
        assert status == 0 and lo <= r < hi
        drows, dsc = alt['detours'][r]
        assert len(drows) == nd and tuple(alt['edge'][r]) in [tuple(d) for d in drows.tolist()]
        spliced = alt_ref.splice(rows, alt['span'][r], drows)
        used = used_set(L, spliced)
        assert used in by_set, (r, row, "the spliced path is no path of the search space")
        assert key not in used
        assert by_set[used] == want and alt_ref.path_total(L, spliced) == want
        # a row's score is its own cost, clipped and averaged, 0 for a deletion
        for d, s in zip(drows.tolist(), dsc.tolist()):
            assert s == (0.0 if d[1] == 0 or d[3] == 0 else max(L.weight(L.move_index(d[1], d[3]), d[0] + d[1] + d[2] + d[3],
                                                                         L.cell(d[0] + d[1], d[2] + d[3])), 0.0) / (d[1] * d[3]))


P96 = [c for c in dp_ref.P_SPARSE if c[2] <= 96]


@pytest.mark.parametrize("case", P96, ids=[c[0] for c in P96])
def test_properties_on_family_p(case):
    assert len(P96) == 27
    f, bo, types, pen, N, M = dp_ref.p_sparse_inputs(case)
    csum, bk, xp, yp, bout, rows = planes(f, bo, types, pen, N, M)
    if not len(rows):
        return
    L = alt_ref.Lattice(f, bo, types, pen, N, M, csum, bk, xp, yp)
    alt = alt_ref.alternatives(f, bo, types, pen, N, M, csum, bk, xp, yp, rows, max_detour=N + M + 2)
    sl = slack_ref.slack(f, bo, types, pen, N, M, csum, bk, rows)
    assert np.array_equal(alt['alt'] - L.total, sl) and np.array_equal(alt['slack'], sl)          # 1: alt - total is the slack
    own = [tuple(r) for r in rows.tolist()]
    for r in range(len(rows)):
        if not np.isfinite(alt['alt'][r]):
            assert alt['span'][r, 3] == 2
            continue
        lo, hi, nd, status = alt['span'][r]
        assert status == 0
        assert lo <= r < hi                                                                      # 2: the row is inside the span
        drows, _ = alt['detours'][r]
        assert own[r] not in [tuple(d) for d in drows.tolist()]                                  # 3: the detour avoids the row
        spliced = alt_ref.splice(rows, alt['span'][r], drows)
        assert (spliced[0, 0], spliced[0, 2]) == (0, 0) and (spliced[-1, 0] + spliced[-1, 1], spliced[-1, 2] + spliced[-1, 3]) == (N, M)
        assert np.array_equal(spliced[1:, 0], spliced[:-1, 0] + spliced[:-1, 1]) and np.array_equal(spliced[1:, 2], spliced[:-1, 2] + spliced[:-1, 3])
        assert alt_ref.path_total(L, spliced) == alt['alt'][r]                                   # 4, 5: the spliced total is alt
    # the regret of the returned rows is 0, and max_slack / max_detour only ever remove detours
    assert np.array_equal(alt_ref.regret(f, bo, types, pen, N, M, csum, bk, rows), np.zeros(len(rows)))
    cut = alt_ref.alternatives(f, bo, types, pen, N, M, csum, bk, xp, yp, rows, max_detour=3, max_slack=pen)
    assert np.array_equal(cut['edge'], alt['edge'])
    for r in range(len(rows)):
        st = cut['span'][r, 3]
        if alt['span'][r, 3] == 0 and alt['slack'][r] <= pen:
            assert st == (0 if alt['span'][r, 2] <= 3 else 1)
            if st == 0:
                assert np.array_equal(cut['span'][r], alt['span'][r]) and np.array_equal(cut['detours'][r][0], alt['detours'][r][0])
        else:
            assert st == 2


def test_spliced_total_on_continuous_costs():
    """On costs that are no dyadic fractions the spliced path's total, summed from the origin, differs from alt = (F(u) + w) +
    Bk(v) by rounding alone: each of the at most A + 2 additions of either sum is off by half an ulp of a partial sum."""
    types = dp_ref.take_types(10)
    for seed in range(6):
        rs = np.random.RandomState(50 + seed)
        N, M, B = 60, 50, 14
        A = N + M - 1
        bo = np.asarray([((k + 2) * M + (N + M) // 2) // (N + M) - 1 - B // 2 for k in range(A)], np.int32)
        f = rs.rand(len(types), A, B).astype(np.float32)
        pen = 0.3
        csum, bk, xp, yp, bout, rows = planes(f, bo, types, pen, N, M)
        L = alt_ref.Lattice(f, bo, types, pen, N, M, csum, bk, xp, yp)
        alt = alt_ref.alternatives(f, bo, types, pen, N, M, csum, bk, xp, yp, rows, max_detour=N + M + 2)
        bound = 2 * (A + 2) * 2.0 ** -53 * np.abs(csum[np.isfinite(csum)]).max()
        n = 0
        for r in range(len(rows)):
            if alt['span'][r, 3] != 0:
                continue
            lo, hi = alt['span'][r, :2]
            assert lo <= r < hi
            assert abs(alt_ref.path_total(L, alt_ref.splice(rows, alt['span'][r], alt['detours'][r][0])) - alt['alt'][r]) <= bound
            n += 1
        assert n >= len(rows) // 2


def scalar_alt_edge(f, bo, types, pen, N, M, csum, bk, row):
    """The tie rule from the definition alone: every edge of slack_ref.edges that crosses the cut, one by one."""
    mv = dp_ref._moves(types)
    bout = slack_ref.b_offset_out(bo)
    c = row[0] + row[2]
    bu_own = row[2] - int(bout[c])
    best = None
    for au, bu, av, bv, t, w in slack_ref.edges(f, bo, types, pen, N, M):
        if not (au <= c < av) or (au == c and bu == bu_own and mv[t] == (row[1], row[3])):
            continue
        cand = (csum[au, bu] + w) + bk[av, bv]
        if cand < INF and (best is None or (cand, av, bv, t) < best):
            best = (cand, av, bv, t)
    if best is None:
        return INF, alt_ref.NO_EDGE
    cand, av, bv, t = best
    vy = bv + int(bout[av])
    return cand, (av - vy - mv[t][0], mv[t][0], vy - mv[t][1], mv[t][1])


TIES = [c for c in dp_ref.P_SPARSE if c[6] in ("equal", "zero") and c[2] <= 40]


@pytest.mark.parametrize("case", TIES, ids=[c[0] for c in TIES])
def test_order_key_breaks_ties(case):
    f, bo, types, pen, N, M = dp_ref.p_sparse_inputs(case)
    csum, bk, xp, yp, bout, rows = planes(f, bo, types, pen, N, M)
    assert len(rows)
    L = alt_ref.Lattice(f, bo, types, pen, N, M, csum, bk, xp, yp)
    tied = 0
    for row in rows.tolist():
        alt, e = alt_ref.alt_edge(L, row)
        want_alt, want_e = scalar_alt_edge(f, bo, types, pen, N, M, csum, bk, row)
        assert alt == want_alt and (alt_ref.NO_EDGE if e is None else tuple(e[:4])) == want_e, row
        tied += alt == L.total
    assert tied > 0   # (on these inputs nearly every cut has several candidates at the optimum)


def test_rows_that_are_no_edges():
    f, bo, types, pen, N, M = dp_ref.p_sparse_inputs(dp_ref.P_SPARSE[0])
    csum, bk, xp, yp, bout, rows = planes(f, bo, types, pen, N, M)
    bad = np.asarray([(-1, 1, 0, 1), (0, 0, 0, 0), (0, 1, 0, 63), (N, 1, M, 1), (2 ** 30, 1, 2 ** 30, 1), (0, 3, 0, 3)], np.int64)
    assert np.isnan(alt_ref.regret(f, bo, types, pen, N, M, csum, bk, bad)).all()
    alt = alt_ref.alternatives(f, bo, types, pen, N, M, csum, bk, xp, yp, bad)
    assert np.isnan(alt['slack']).all() and (alt['edge'] == -1).all() and (alt['span'] == (-1, -1, -1, 2)).all()
    assert alt['summary'] == [len(bad), 0, 0, 0]


def test_formatters():
    from svx.seg_align.align import format_alt_lines, format_regret_lines
    span = np.asarray([(-1, -1, -1, 2), (1, 3, 2, 0), (-1, -1, -1, 1)], np.int32)
    slack = np.asarray([np.inf, 0.125, 0.5])
    detours = [None, (np.asarray([(1, 2, 1, 1), (3, 0, 2, 1)], np.int32), np.asarray([0.25, 0.0])), None]
    assert format_alt_lines(slack, span, detours) == "1\t0.125000\t1\t3\t[1, 2]:[1]:0.250000\t[]:[2]:0.000000\n"
    assert format_alt_lines(slack[:1], span[:1], detours[:1]) == ""
    rows = np.asarray([(0, 1, 0, 1), (1, 0, 1, 2), (1, 2, 3, 1)], np.int32)
    assert format_regret_lines(rows, np.asarray([0.0, np.nan, np.inf])) == "[0]:[0]:0.000000\n[]:[1, 2]:nan\n[1, 2]:[3]:inf\n"


@pytest.mark.parametrize("flag", ["--alt_dir", "--regret_dir"])
@pytest.mark.parametrize("extra,text", [(["--widen"], "cannot be combined with --widen"),
                                        (["--skip_existing"], "cannot be combined with --skip_existing"),
                                        (["--mode", "band", "--band", "80"], "runs the tile sweep, which keeps no cost array")])
def test_refused_combinations(tmp_path, capsys, flag, extra, text):
    from svx.seg_align import align as A
    from test_gpu_slack_cli import argv
    more = ["--rescore_dir", str(tmp_path / "g"), "--rescore_tsv", str(tmp_path / "g.tsv")] if flag == "--regret_dir" else []
    with pytest.raises(SystemExit) as e:
        A.parse_args(argv(str(tmp_path), str(tmp_path / "out"), [flag, str(tmp_path / "s")] + more + extra))
    assert e.value.code == 2
    assert text in " ".join(capsys.readouterr().err.split())


def test_regret_dir_needs_rescore_dir(tmp_path, capsys):
    from svx.seg_align import align as A
    from test_gpu_slack_cli import argv
    with pytest.raises(SystemExit):
        A.parse_args(argv(str(tmp_path), str(tmp_path / "out"), ["--regret_dir", str(tmp_path / "s")]))
    assert "--regret_dir needs --rescore_dir" in " ".join(capsys.readouterr().err.split())
    with pytest.raises(SystemExit):
        A.parse_args(argv(str(tmp_path), str(tmp_path / "out"), ["--alt_dir", str(tmp_path / "s"), "--alt_max_detour", "300"]))
    assert "--alt_max_detour must be 1 .. 256" in " ".join(capsys.readouterr().err.split())
