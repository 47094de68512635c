"""The cases of tests/tail_ref.py do what they claim, without a GPU: every case lands in the traceback mode it is meant
for (the dispatch restated from svx_dp.hip), the oracle equals what the REAL reference returned on every success case
(tests/golden/tail_records.json, recorded by tests/golden/make_golden.py), every failure case raises in the oracle, the
garbage around the walks discriminates, and the shifted pairs make the traceback's corridor move."""
import json
import os

import numpy as np
import pytest

import tail_ref as T
from cases import digest

RECORDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tail_records.json")


@pytest.fixture(scope="module")
def rec():
    with open(RECORDS) as f:
        return json.load(f)


def test_mode_restatement():
    """The table of modes: chunk sizes and thresholds as svx_dp.hip computes them."""
    assert [T.tb_chunk(B, True) for B in (2, 14, 40, 158, 159, 160, 400)] == [2560, 640, 240, 64, 0, 0, 0]
    assert [T.tb_mode(B, False) for B in (158, 159)] == [(2, 64, 0), (0, 0, 0)]
    assert [T.tb_mode(B, True) for B in (316, 318, 320, 322, 336, 800)] == [(1, 64, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (3, 64, 320), (3, 64, 320)]
    assert T.tb_mode(317, True)[0] == 0 and T.tb_mode(330, True)[0] == 0
    assert T.SP_LDS_ROWS == 9597 and T.sp_lds_rows(9598) == 9598 and T.sp_lds_rows(9599) == 9597
    for W, want in ((158, 1), (159, 0), (160, 0), (161, 0), (168, 3), (400, 3), (79, 2), (80, 0)):
        assert T.shifted_mode(W)[0] == want, W
    assert T.shifted_mode(158)[1] == 64 and T.shifted_mode(79)[1] == 64


def test_sparse_cases_cover_the_modes_and_edges():
    ok = T.TB_OK
    for B in T.LDS_B:
        chunk = T.tb_chunk(B, True)
        assert T.tb_mode(B, False) == (2, chunk, 0)
        assert sorted(ok["win_B%d_r%d" % (B, r)][2] - 2 * chunk for r in (0, 1, chunk - 1)) == [0, 1, chunk - 1]
    for B in T.GLOBAL_B:
        assert T.tb_mode(B, False)[0] == 0 and "global_B%d" % B in ok
    for B in (14, 158):
        assert [len(ok["rows%d_B%d" % (n, B)][1]) for n in T.FLUSH_ROWS] == list(T.FLUSH_ROWS)
        _, steps, a_out = ok["alldel_B%d" % B]
        assert len(steps) == a_out - 3 > 512 and all(sum(s) == 1 for s in steps)
    inside = [name for name in ok if name.startswith("rows")
              and T.window_boundary_inside_block(T.tb_ok_case(name), T.tb_chunk(ok[name][0], True))]
    assert len(inside) >= 2, inside
    every = [s for _, steps, _ in ok.values() for s in steps]
    assert max(max(s) for s in every) == 100 and {(100, 100), (100, 1), (1, 100)} <= set(every)
    assert ok["skip_first_B158"][1][0] == (100, 100)   # 200 diagonals: more than two windows of 64, from the end node on
    assert ok["empty_a1_B14"][1:] == ([], 1) and ok["zeroN_x0_B160"][2] == 8
    # failures: every kind in the topmost, a middle and the lowest window of three, in an LDS mode and a global one
    assert T.tb_mode(14, False) == (2, 640, 0) and T.FAIL_A_OUT > 2 * 640
    for spec in T.TB_FAIL:
        t = T.tb_fail_case(spec)
        kind, where, B = spec
        if where is not None:
            win = sum(t['nodes'][t['bad']]) // 640
            assert win == {'last': 2, 'middle': 1, 'first': 0}[where] and 0 < t['bad'] < len(t['steps'])
        if kind == 'px_gt':
            x, y = t['nodes'][t['bad']]
            assert t['xp'][x + y, t['cols'][t['bad']]] == x + 1 <= 100
        if kind == 'py_gt':
            x, y = t['nodes'][t['bad']]
            assert t['yp'][x + y, t['cols'][t['bad']]] == y + 1 <= 100
    assert int(T.tb_fail_case(('origin_1', None, 14))['boff'][0]) == 1 and int(T.tb_fail_case(('origin_mB', None, 160))['boff'][0]) == -160


@pytest.mark.parametrize("name", list(T.TB_OK))
def test_sparse_success_case(orc, rec, name):
    """Oracle == the reference's recorded result == the plain Python walk; the filling discriminates (a walk that reads
    the neighbouring column or diagonal at any single row fails or returns other spans); a share of the scores is clipped."""
    t = T.tb_ok_case(name)
    al, sc = orc.sparse_traceback(t['csum'], t['xp'], t['yp'], t['boff'], t['N'], t['M'])
    assert {"alignments": digest(al, 'alignments'), "scores": digest(sc)} == rec["sparse_traceback"][name]
    rows = T.py_walk(t)
    assert al == T.rows_to_alignments(rows[::-1]) and len(rows) == len(t['steps'])
    nodes, cols, n = t['nodes'], t['cols'], len(rows)
    assert all(0 <= c < t['B'] for c in cols) and (n < 20 or (0 in cols and t['B'] - 1 in cols))
    a_out = t['xp'].shape[0]
    for r in range(n):   # what a mutant read returns is never the row's own step ...
        a, c = sum(nodes[r]), cols[r]
        for da, db in T.NEIGHBOURS:
            if 0 <= a + da < a_out and 0 <= c + db < t['B']:
                assert (t['xp'][a + da, c + db], t['yp'][a + da, c + db]) != t['steps'][r], (r, da, db)
    pick = range(n) if n <= 70 else sorted(set(np.random.RandomState(n).randint(0, n, 24).tolist() + [0, n - 1, 63, 64]))
    for r in pick:       # ... so the whole mutant walk fails or differs (all rows of the short cases, a sample of the long ones)
        for da, db in T.NEIGHBOURS:
            try:
                assert T.py_walk(t, mutate=(r, da, db)) != rows, (r, da, db)
            except Exception as e:
                assert str(e) == 'traceback bug'
    if n >= 8:           # (with fewer rows a share between 10 % and 90 % means little)
        cs = np.array([t['csum'][x + y, c] for (x, y), c in zip(nodes, cols)])
        neg = float((cs[:-1] - cs[1:] < 0).mean())
        assert 0.1 <= neg <= 0.9, neg
        both = np.array([px > 0 and py > 0 for px, py in t['steps']])[::-1]
        if both.any():
            assert np.array_equal(sc[both] == 0.0, (cs[:-1] - cs[1:] < 0)[::-1][both])


@pytest.mark.parametrize("spec", T.TB_FAIL, ids=T.tb_fail_id)
def test_sparse_failure_case_raises_in_the_oracle(orc, spec):
    t = T.tb_fail_case(spec)
    with pytest.raises(Exception, match='^traceback bug$'):
        orc.sparse_traceback(t['csum'], t['xp'], t['yp'], t['boff'], t['N'], t['M'])
    with pytest.raises(Exception, match='^traceback bug$'):
        T.py_walk(t)


def test_search_path_cases(orc, rec):
    """Oracle == the reference chain's recorded paths; the extensions reach all three branches of extend_alignments;
    one short of the mirror's buffer; the EXTEND failures raise exactly below the largest index."""
    assert {(ex > 0, ey > 0) for ex, ey in T.SP_EXTRA} == {(False, False), (True, False), (False, True), (True, True)}
    ties = 0
    for g in T.SP_GRID:
        al = T.sp_alignment(g)
        assert len(al) == g[0]
        ties += sum(1 for a, b in al if len(a) > 1 and (len(a) == len(b) or len(a) == 3 * len(b) or 3 * len(a) == len(b)))
        for label, up, s0, s1 in T.sp_calls(al):
            p = orc.search_path(al, up, s0, s1)
            assert digest(p, 'searchpath') == rec["search_path"][T.sp_id(g)][label], (g, label)
            assert len(p) <= s0 + s1 + 4
            if up and any(a for a, _ in al) and any(b for _, b in al):
                assert len(p) == s0 + s1 + 3
        xm, ym = T.up_max(al)
        orc.search_path(al, True, xm, ym)
        if xm > 0:
            with pytest.raises(Exception, match=T.EXTEND_TEXT):
                orc.search_path(al, True, xm - 1, ym + 5)
        if ym > 0:
            with pytest.raises(Exception, match=T.EXTEND_TEXT):
                orc.search_path(al, True, xm + 5, ym - 1)
    assert ties >= 10
    sh = [T.sp_alignment(g) for g in T.SP_GRID if g[0] == 400 and g[1] == 0.5]
    assert all(not (a and b) for al in sh for a, b in (al[0], al[-1]))   # deletions first and last


def test_search_path_lds_limit(orc, rec):
    long = T.sp_long(T.SP_LDS_ROWS + 1)
    assert all(a or b for a, b in long)
    for rows, form in ((T.SP_LDS_ROWS, 'block'), (T.SP_LDS_ROWS + 1, 'thread')):
        al = long[:rows]
        for label, up, s0, s1 in T.sp_calls(al)[:3]:
            assert T.sp_form(rows, s0, s1) == form
            assert digest(orc.search_path(al, up, s0, s1), 'searchpath') == rec["search_path_long"][str(rows)][label]


def test_dense_cases(orc, rec):
    for name in T.DENSE_OK:
        assert digest(orc.dense_traceback(T.dense_ok_case(name)), 'alignments') == rec["dense_traceback"][name]
    assert orc.dense_traceback(T.dense_ok_case("1x1")) == []
    assert orc.dense_traceback(T.dense_ok_case("1x9")) == [([], [k]) for k in range(8)]
    assert orc.dense_traceback(T.dense_ok_case("9x1")) == [([k], []) for k in range(8)]
    for spec in T.DENSE_FAIL:
        bp, at = T.dense_fail_case(spec)
        assert bp.shape == (40, 37) and bp[at] == spec[1] and at != (0, 0)
        if spec[0] == "border":   # a move off the lattice at a border node away from the origin
            assert (at[0] == 0 and at[1] > 1) if spec[2] == "x0" else (at[1] == 0 and at[0] > 1)
        with pytest.raises(Exception, match='^got unknown value$'):
            orc.dense_traceback(bp)
        bp[at] = 1 if at[0] == 0 else 2   # (and nothing else is wrong with the table)
        if spec[0] == "border":
            orc.dense_traceback(bp)


@pytest.mark.parametrize("W", sorted(T.SHIFTED))
def test_shifted_pair_drifts(orc, W):
    """The oracle's straight search on a shifted pair: a third of the rows are deletions, the penalty is off the
    percentile knife-edge, and in the corridor modes the simulated window origins move while no read leaves its window."""
    import dp_ref
    import stage_check
    types, S, J = T.SHIFTED[W][:3]
    assert J < W and 2 * (S + J) >= 8 * 64
    v0, v1, types, rseed = T.shifted_case(W)
    st = dp_ref.straight_stack(orc, v0, v1, types, W, rseed)
    al = st['final_alignments']
    assert stage_check.off_knife_edge({0: st}, dp_ref.FRAC) == []
    assert 3 * sum(1 for a, b in al if not a or not b) >= len(al)
    nodes, bo = T.alignment_nodes(al), st['new_b_offset']
    cols = [y - int(bo[x + y]) for x, y in nodes]
    assert max(cols) - min(cols) >= J // 2 - 8
    if T.shifted_mode(W)[0] == 3:
        origins, outside = T.simulate_corridor(nodes, bo, 2 * W)
        assert outside == 0
        assert len(set(origins)) >= (4 if W == 400 else 2), sorted(set(origins))
