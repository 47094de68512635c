"""Row alternatives: float64 numpy restatement of the definitions of include/svx.h (svx_path_alternatives,
svx_row_alternatives); TEST INFRASTRUCTURE (numpy, no GPU).

Notation of slack_ref: costs [T][A][B] float32, bout = b_offset_out, moves = the types in list order, then (0,1), then
(1,0); F = the stored forward plane csum, Bk = slack_ref.backward.  Per returned row:

  alt, edge   the cheapest crossing edge of the row's cut other than the row itself, ties broken by (diagonal of v, cell of
              v, move index); slack = alt - total
  detour      the rows of the best path through that edge between the two nodes of the returned path it leaves and rejoins:
              the stored back-pointers from u back to a path node, first exact-match moves on Bk from v on to a path node
  regret      of any given row: ((F(u) + w) + Bk(v)) - total, NaN when the row is no edge

is_edge restates the rule of the slack kernel itself: range checks, the move is in the list, both nodes are band cells.
Every value is a minimum of singly rounded float64 sums or an equality test on them, so a kernel that follows the
definitions gives THESE BITS and THESE ROWS on any input."""
import numpy as np

from dp_ref import INF, _diagonal, _moves
from slack_ref import b_offset_out, end_cell

NO_EDGE = (-1, -1, -1, -1)
ST_WRITTEN, ST_TOO_LONG, ST_NOT_MEASURED, ST_WALK_FAILED = 0, 1, 2, 3


class Lattice:
    """One pair's planes and the predicates over them."""

    def __init__(self, costs, b_offset_in, types, pen, x_in, y_in, csum, bsum, xp=None, yp=None):
        self.costs = np.asarray(costs, np.float32)
        self.T, self.A, self.B = self.costs.shape
        self.mv = _moves(types)
        self.pen = float(pen)
        self.bout = b_offset_out(b_offset_in)
        self.Aout = self.A + 2
        self.xs, self.ys = int(x_in), int(y_in)
        self.F, self.Bk, self.xp, self.yp = csum, bsum, xp, yp
        self.maxstep = max(xo + yo for xo, yo in self.mv)
        end = end_cell(self.bout, self.B, self.xs, self.ys)
        self.total = float(csum[end]) if end is not None else INF

    def cell(self, x, y):
        """Band cell b of the node (x, y), or None when it has none."""
        a = x + y
        if not 0 <= a < self.Aout:
            return None
        b = y - int(self.bout[a])
        return b if 0 <= b < self.B else None

    def move_index(self, xl, yl):
        for t, m in enumerate(self.mv):
            if m == (xl, yl):
                return t
        return None

    def weight(self, t, av, bv):
        return float(self.costs[t, av - 2, bv]) if t < self.T else self.pen

    def is_edge(self, row):
        """-> (c, bu, bv, t) when the row is an edge (the kernel's rule), else None.  Nothing is indexed before the ranges hold."""
        x0, xl, y0, yl = (int(v) for v in row)
        if min(x0, xl, y0, yl) < 0 or x0 + xl > self.xs or y0 + yl > self.ys or xl + yl < 1 or x0 + y0 + xl + yl >= self.Aout:
            return None
        t = self.move_index(xl, yl)
        if t is None:
            return None
        bu, bv = self.cell(x0, y0), self.cell(x0 + xl, y0 + yl)
        if bu is None or bv is None:
            return None
        return x0 + y0, bu, bv, t

    def out_edge_ok(self, x, y, t):
        """Is node (x, y) -> (x + xo, y + yo) by move t an edge of E or E_b?  -> (av, bv) or None."""
        xo, yo = self.mv[t]
        a, av = x + y, x + y + xo + yo
        if av >= self.Aout:
            return None
        vx, vy = x + xo, y + yo
        bv = vy - int(self.bout[av])
        if not 0 <= bv < self.B:
            return None
        bx = x == 0 and 0 <= y <= self.ys
        by = not bx and y == 0 and 0 <= x <= self.xs
        gen = not bx and not by and 1 <= x <= self.xs and 1 <= y <= self.ys and 0 <= a - 2 < self.A
        ok = (bx or by or gen) and 1 <= vx <= self.xs and 1 <= vy <= self.ys and 0 <= av - 2 < self.A
        if t == self.T:
            ok = ok or (bx and vy <= self.ys)
        elif t == self.T + 1:
            ok = ok or ((by or (bx and y == 0)) and vx <= self.xs)
        return (av, bv) if ok else None

    def score(self, row, t):
        """process_scores of one row taken by move t: a deletion 0.0, a typed row max(cost cell, 0) / (xo yo)."""
        x0, xl, y0, yl = row
        if t >= self.T:
            return 0.0
        av = x0 + xl + y0 + yl
        c = np.float64(self.costs[t, av - 2, (y0 + yl) - int(self.bout[av])])
        return float(np.maximum(c, 0.0) / np.float64(xl * yl))


def node_table(L, rows):
    """diagonal -> (cell, i) of the nodes P_0 .. P_R of the rows: P_i the start of row i, P_R the end of the last row.  A
    node that is no lattice band cell is left out."""
    rows = np.asarray(rows).reshape(-1, 4)
    tab = {}
    nodes = [(int(r[0]), int(r[2])) for r in rows]
    if len(rows):
        r = rows[-1]
        nodes.append((int(r[0]) + int(r[1]), int(r[2]) + int(r[3])))
    for i, (x, y) in enumerate(nodes):
        if 0 <= x <= L.xs and 0 <= y <= L.ys:
            b = L.cell(x, y)
            if b is not None:
                tab[x + y] = (b, i)
    return tab


def alt_edge(L, row):
    """-> (alt, edge) of a row that is an edge: edge = (x_u, xo, y_u, yo, t) of the first candidate with cand == alt in the
    order (diagonal of v, cell of v, move index), None when alt is +inf."""
    c, bus, bvs, _ = L.is_edge(row)
    xl, yl = int(row[1]), int(row[3])
    alt, key = INF, None
    for dv in range(1, L.maxstep + 1):
        av = c + dv
        if av >= L.Aout:
            break
        yy, xx, bx, by, gen = _diagonal(av, L.B, L.bout, L.xs, L.ys, L.A)
        for t, (xo, yo) in enumerate(L.mv):
            st = xo + yo
            au = av - st
            if st < dv or au < 0:
                continue
            ux, uy = xx - xo, yy - yo
            bu = uy - int(L.bout[au])
            inband = (0 <= bu) & (bu < L.B)
            ok = gen & (ux >= 0) & (uy >= 0) & inband
            if t == L.T:
                ok = ok | (bx & (yy >= 1) & inband)
            elif t == L.T + 1:
                ok = ok | (by & (xx >= 1) & inband)
            if (xo, yo) == (xl, yl) and au == c:   # the row's own edge (and any duplicate of its move in the list)
                ok = ok.copy()
                ok[bvs] = False
            if not ok.any():
                continue
            buc = np.clip(bu, 0, L.B - 1)
            w = L.costs[t, av - 2, :].astype(np.float64) if t < L.T else L.pen
            cand = np.where(ok, (L.F[au, buc] + w) + L.Bk[av], INF)
            m = float(cand.min())
            if m == INF:
                continue
            k = (dv, int(np.argmax(cand == m)), t)
            if m < alt or (m == alt and k < key):
                alt, key = m, k
    if key is None:
        return INF, None
    dv, bv, t = key
    av = c + dv
    vy = bv + int(L.bout[av])
    vx = av - vy
    xo, yo = L.mv[t]
    return alt, (vx - xo, xo, vy - yo, yo, t)


def detour(L, tab, edge, K):
    """The two walks -> (status, lo, hi, rows [(x_start, x_len, y_start, y_len)], move indices)."""
    ux, xo, uy, yo, t_e = edge
    back, nb = [], 0
    x, y = ux, uy
    while True:
        a = x + y
        b = y - int(L.bout[a])
        hit = tab.get(a)
        if hit is not None and hit[0] == b:
            lo = hit[1]
            break
        if nb == K - 1:
            return ST_TOO_LONG, -1, -1, [], []
        px, py = int(L.xp[a, b]), int(L.yp[a, b])
        if px < 0 or py < 0 or px + py < 1 or px > x or py > y:
            return ST_WALK_FAILED, -1, -1, [], []
        t = L.move_index(px, py)
        if t is None or L.cell(x - px, y - py) is None:
            return ST_WALK_FAILED, -1, -1, [], []
        back.append(((x - px, px, y - py, py), t))
        x, y = x - px, y - py
        nb += 1
    fwd, nf = [], 0
    x, y = ux + xo, uy + yo
    while True:
        a = x + y
        b = y - int(L.bout[a])
        hit = tab.get(a)
        if hit is not None and hit[0] == b:
            hi = hit[1]
            break
        if nb + 1 + nf == K:
            return ST_TOO_LONG, -1, -1, [], []
        here = L.Bk[a, b]
        for t in range(len(L.mv)):
            s = L.out_edge_ok(x, y, t)
            if s is not None and L.weight(t, *s) + L.Bk[s] == here:
                break
        else:
            return ST_WALK_FAILED, -1, -1, [], []
        mxo, myo = L.mv[t]
        fwd.append(((x, mxo, y, myo), t))
        x, y = x + mxo, y + myo
        nf += 1
    seq = back[::-1] + [((ux, xo, uy, yo), t_e)] + fwd
    return ST_WRITTEN, lo, hi, [r for r, _ in seq], [t for _, t in seq]


def alternatives(costs, b_offset_in, types, pen, x_in, y_in, csum, bsum, xp, yp, rows, max_detour=16, max_slack=INF,
                 want_detours=True):
    """-> dict: slack, alt [n] float64; edge, span [n][4] int32; detours: per row None or (rows [k][4] int32, scores [k]
    float64); summary = (rows, rows with an alternative edge, detours written, detours too long)."""
    L = Lattice(costs, b_offset_in, types, pen, x_in, y_in, csum, bsum, xp, yp)
    rows = np.asarray(rows).reshape(-1, 4)
    n = len(rows)
    tab = node_table(L, rows)
    out = dict(slack=np.full(n, np.nan), alt=np.full(n, np.nan), edge=np.full((n, 4), -1, np.int32),
               span=np.tile(np.asarray([-1, -1, -1, ST_NOT_MEASURED], np.int32), (n, 1)), detours=[None] * n)
    n_edge = n_written = n_long = 0
    for r in range(n):
        if L.is_edge(rows[r]) is None:
            continue
        alt, e = alt_edge(L, rows[r])
        with np.errstate(invalid="ignore"):
            s = np.float64(alt) - np.float64(L.total)
        out['alt'][r], out['slack'][r] = alt, s
        if e is None:
            continue
        n_edge += 1
        out['edge'][r] = e[:4]
        if not want_detours or not s <= max_slack:
            continue
        status, lo, hi, drows, dts = detour(L, tab, e, int(max_detour))
        if status == ST_WRITTEN:
            n_written += 1
            out['span'][r] = (lo, hi, len(drows), status)
            out['detours'][r] = (np.asarray(drows, np.int32).reshape(-1, 4),
                                 np.asarray([L.score(row, t) for row, t in zip(drows, dts)], np.float64))
        else:
            n_long += status == ST_TOO_LONG
            out['span'][r] = (-1, -1, -1, status)
    out['summary'] = [n, n_edge, n_written, int(n_long)]
    return out


def regret(costs, b_offset_in, types, pen, x_in, y_in, csum, bsum, given):
    """regret [len(given)] float64; NaN for a row that is no edge."""
    L = Lattice(costs, b_offset_in, types, pen, x_in, y_in, csum, bsum)
    given = np.asarray(given).reshape(-1, 4)
    out = np.full(len(given), np.nan)
    for g, row in enumerate(given.tolist()):
        e = L.is_edge(row)
        if e is None:
            continue
        c, bu, bv, t = e
        av = c + row[1] + row[3]
        with np.errstate(invalid="ignore"):
            out[g] = (np.float64(L.F[c, bu]) + np.float64(L.weight(t, av, bv))) + np.float64(L.Bk[av, bv]) - np.float64(L.total)
    return out


def splice(rows, span, drows):
    """The returned rows with rows lo .. hi-1 replaced by the detour."""
    rows = np.asarray(rows, np.int32).reshape(-1, 4)
    lo, hi = int(span[0]), int(span[1])
    return np.concatenate([rows[:lo], np.asarray(drows, np.int32).reshape(-1, 4), rows[hi:]])


def path_total(L, rows):
    """The total of a chain of rows summed from the origin, each row priced by the first move of the list it matches."""
    tot = 0.0
    for x0, xl, y0, yl in np.asarray(rows).reshape(-1, 4).tolist():
        t = L.move_index(xl, yl)
        av = x0 + xl + y0 + yl
        tot = tot + L.weight(t, av, (y0 + yl) - int(L.bout[av]))
    return tot
