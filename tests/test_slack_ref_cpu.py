"""slack_ref against brute force: every path of the search space of a small lattice, one by one (CPU only).

Family-P costs (dp_ref.p_costs: float32 k/8, a tenth +inf, dyadic penalty) make every float64 sum exact, so the totals of
enumerated paths, the forward plane, the backward plane and their differences are compared with ==."""
import functools

import numpy as np
import pytest

import dp_ref
import slack_ref
from synth import alignment_types

INF = np.inf
SIZES = [(1, 1), (1, 4), (2, 3), (4, 4), (5, 3), (5, 5)]


def cover_band(N, M):
    """b_offset_in and B of a band that holds every lattice node."""
    A = N + M - 1
    return np.asarray([max(0, k + 2 - N) - 1 for k in range(A)], np.int32), min(N, M) + 2


def straight_band(N, M):
    """A 4-cell band around the straight path from (0, 0) to (N, M)."""
    A = N + M - 1
    return np.asarray([((k + 2) * M + (N + M) // 2) // (N + M) - 3 for k in range(A)], np.int32), 4


def make_case(N, M, a, band, mode, seed):
    types = alignment_types(a)
    bo, B = (cover_band if band == "cover" else straight_band)(N, M)
    rs = np.random.RandomState(seed)
    costs = dp_ref.p_costs(rs, (len(types), N + M - 1, B), 3, mode)
    pen = 0.25 if mode == "equal" else 0.375
    return costs, bo, types, pen, N, M


CASES = [(N, M, a, band, mode) for (N, M) in SIZES for a in (3, 4) for band in ("cover", "straight")
         for mode in ("rand", "equal")]


def case_id(c):
    return "%dx%d_a%d_%s_%s" % c


def border_chain_in_band(bout, B, N, M):
    """No band cell on a border lacks its border predecessor (the 'traceback bug' corner of include/svx.h does not occur),
    and the origin is a band cell."""
    def in_band(x, y):
        a = x + y
        return 0 <= a < len(bout) and 0 <= y - int(bout[a]) < B
    if not in_band(0, 0):
        return False
    for y in range(1, M + 1):
        if in_band(0, y) and not in_band(0, y - 1):
            return False
    for x in range(1, N + 1):
        if in_band(x, 0) and not in_band(x - 1, 0):
            return False
    return True


class Brute:
    """Every path of E and E_b, explicitly."""

    def __init__(self, costs, bo, types, pen, N, M):
        self.B = costs.shape[2]
        self.bout = slack_ref.b_offset_out(bo)
        self.mv = dp_ref._moves(types)
        self.succ = {}
        for au, bu, av, bv, t, w in slack_ref.edges(costs, bo, types, pen, N, M):
            self.succ.setdefault((au, bu), []).append(((av, bv), self.mv[t], w))
        self.end = slack_ref.end_cell(self.bout, self.B, N, M)
        self.start = (0, 0 - int(self.bout[0]))

    @functools.lru_cache(maxsize=None)
    def suffix_costs(self, u):
        """The cost of every path from u to the end, each summed from the end backwards."""
        if u == self.end:
            return (0.0,)
        return tuple(w + c for v, _, w in self.succ.get(u, ()) for c in self.suffix_costs(v))

    def paths(self):
        """(total, frozenset of (u, move)) of every path from the origin to the end; the total summed from the origin."""
        out = []

        def walk(u, tot, used):
            if u == self.end:
                out.append((tot, frozenset(used)))
                return
            for v, m, w in self.succ.get(u, ()):
                used.append((u, m))
                walk(v, tot + w, used)
                used.pop()
        if self.end is not None:
            walk(self.start, 0.0, [])
        return out


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_slack_ref_vs_brute_force(case):
    N, M, a, band, mode = case
    costs, bo, types, pen, N, M = make_case(N, M, a, band, mode, 31 * N + 7 * M + a)
    T, A, B = costs.shape
    bout = slack_ref.b_offset_out(bo)
    assert border_chain_in_band(bout, B, N, M)
    if band == "cover":
        assert all(0 <= y - int(bout[x + y]) < B for x in range(N + 1) for y in range(M + 1))
    assert slack_ref.end_cell(bout, B, N, M) is not None
    csum, xp, yp, bout2 = dp_ref.sparse_dp(costs, bo, types, pen, N, M)
    assert np.array_equal(bout, bout2)
    bk = slack_ref.backward(costs, bo, types, pen, N, M)
    br = Brute(costs, bo, types, pen, N, M)

    # ---- Bk(u) is the best suffix, on every cell of the band
    for a_ in range(A + 2):
        for b in range(B):
            y = b + int(bout[a_])
            kind = slack_ref._kind(a_ - y, y, a_, N, M, A)
            want = min(br.suffix_costs((a_, b)), default=INF) if kind else INF
            assert bk[a_, b] == want, (a_, b, kind)

    paths = br.paths()
    assert paths
    total = min(t for t, _ in paths)
    end = slack_ref.end_cell(bout, B, N, M)
    assert csum[end] == total and bk[br.start] == total
    if not np.isfinite(total):
        return   # (every path crosses a +inf cell: there is no returned path to look at)
    rows = slack_ref.traceback(xp, yp, bout, B, N, M)

    # ---- F + Bk == total on the nodes of the returned path
    nodes = [(0, 0)] + [(r[0] + r[1], r[2] + r[3]) for r in rows.tolist()]
    for x, y in nodes:
        assert csum[x + y, y - int(bout[x + y])] + bk[x + y, y - int(bout[x + y])] == total

    # ---- slack == (best path without the row) - (best path)
    sl = slack_ref.slack(costs, bo, types, pen, N, M, csum, bk, rows)
    for r, (x0, xl, y0, yl) in enumerate(rows.tolist()):
        key = ((x0 + y0, y0 - int(bout[x0 + y0])), (xl, yl))
        alt = min((t for t, used in paths if key not in used), default=INF)
        assert sl[r] == alt - total, (r, rows[r])
        # every cut the row crosses gives the same value
        for cut in range(1, xl + yl):
            assert slack_ref.slack(costs, bo, types, pen, N, M, csum, bk, rows[r:r + 1], cut=cut)[0] == sl[r]
    assert sl.min() >= 0.0
    if mode == "equal" and N >= 2 and M >= 2 and band == "cover":
        assert (sl == 0.0).any()   # a 1-1 step costs two deletions: the path is one of many optima

    # ---- rows that are no edges get NaN
    bad = np.asarray([(-1, 1, 0, 1), (0, 0, 0, 0), (0, 1, 0, 7), (N, 1, M, 1), (2 ** 30, 1, 2 ** 30, 1)], np.int64)
    assert np.isnan(slack_ref.slack(costs, bo, types, pen, N, M, csum, bk, bad)).all()


def test_end_outside_the_band_is_all_inf():
    N, M = 4, 4
    costs, bo, types, pen, N, M = make_case(N, M, 3, "straight", "rand", 5)
    bo = bo.copy()
    bo[-1] -= 6   # the last diagonal no longer holds (N, M)
    assert slack_ref.end_cell(slack_ref.b_offset_out(bo), costs.shape[2], N, M) is None
    assert np.isposinf(slack_ref.backward(costs, bo, types, pen, N, M)).all()
