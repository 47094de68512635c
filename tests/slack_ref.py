"""Row slack: float64 numpy restatement of the definitions of include/svx.h (svx_sparse_dp_backward, svx_path_slack);
TEST INFRASTRUCTURE (numpy, no GPU).

Notation of dp_ref.sparse_dp: costs [T][A][B] float32, bout = b_offset_out, moves = the types in list order, then (0,1),
then (1,0).  Cell (a, b) is the node (x, y) = (a - y, b + bout[a]); its kind -- border-x, border-y, general, outside -- is
dp_ref._diagonal's.  The search space is the edge set E (what the forward loop relaxes: into general cells only) plus the
border edges E_b (what the traceback walks along the closed-form borders):

  edges     every edge, one by one from the definition (scalar loops; for brute force on small lattices)
  backward  Bk [A+2][B]: the cheapest way from every cell to the end cell, vectorised per diagonal like dp_ref.sparse_dp
  slack     per row: min over the edges that cross the cut behind the row's start diagonal, the row's own excluded, of
            ((F(u) + w) + Bk(v)), minus F(end); NaN for a row that is no edge

Every candidate is one float64 addition (two for alt) and a minimum does not depend on the order it is taken in, so a
kernel that follows the definitions gives THESE BITS on any input."""
import numpy as np

from dp_ref import INF, _diagonal, _moves


def b_offset_out(b_offset_in):
    bo = np.asarray(b_offset_in, np.int32)
    out = np.empty(len(bo) + 2, np.int32)
    out[:2] = bo[0]
    out[2:] = bo + 1
    return out


def _kind(x, y, a, x_in, y_in, A):
    """Kind of the node (x, y) on diagonal a: 'bx', 'by', 'gen' or None (outside), tested in that order."""
    if x == 0 and 0 <= y <= y_in:
        return 'bx'
    if y == 0 and 0 <= x <= x_in:
        return 'by'
    if 1 <= x <= x_in and 1 <= y <= y_in and 0 <= a - 2 < A:
        return 'gen'
    return None


def edges(costs, b_offset_in, types, pen, x_in, y_in):
    """Every edge of E and E_b as (au, bu, av, bv, t, w); t indexes the move list."""
    costs = np.asarray(costs, np.float32)
    T, A, B = costs.shape
    mv = _moves(types)
    bout = b_offset_out(b_offset_in)
    Aout = A + 2
    out = []
    for a in range(Aout):
        for b in range(B):
            y = b + int(bout[a])
            x = a - y
            k = _kind(x, y, a, x_in, y_in, A)
            if k == 'gen':
                for t, (xo, yo) in enumerate(mv):
                    ap = a - xo - yo
                    if ap < 0 or x - xo < 0 or y - yo < 0:
                        continue
                    bp = (y - yo) - int(bout[ap])
                    if 0 <= bp < B:
                        out.append((ap, bp, a, b, t, float(costs[t, a - 2, b]) if t < T else float(pen)))
            elif k == 'bx' and y >= 1:          # (0, y-1) -> (0, y), both border-x band cells
                bp = (y - 1) - int(bout[a - 1])
                if 0 <= bp < B:
                    out.append((a - 1, bp, a, b, T, float(pen)))
            elif k == 'by' and x >= 1:          # (x-1, 0) -> (x, 0); (0, 0) is a border-x cell, and included
                bp = 0 - int(bout[a - 1])
                if 0 <= bp < B:
                    out.append((a - 1, bp, a, b, T + 1, float(pen)))
    return out


def end_cell(bout, B, x_in, y_in):
    """(a, b) of the end node, or None when it is no band cell."""
    a = x_in + y_in
    if not 0 <= a < len(bout):
        return None
    b = y_in - int(bout[a])
    return (a, b) if 0 <= b < B else None


def backward(costs, b_offset_in, types, pen, x_in, y_in):
    """Bk [A+2][B] float64."""
    costs = np.asarray(costs, np.float32)
    T, A, B = costs.shape
    mv = _moves(types)
    pen = float(pen)
    bout = b_offset_out(b_offset_in)
    Aout = A + 2
    end = end_cell(bout, B, x_in, y_in)
    bsum = np.full((Aout, B), INF, np.float64)
    for a in range(Aout - 1, -1, -1):
        yy, xx, bx, by, gen = _diagonal(a, B, bout, x_in, y_in, A)
        lat = bx | by | gen
        best = np.full(B, INF)
        for t, (xo, yo) in enumerate(mv):
            av = a + xo + yo
            if av >= Aout:
                continue
            vx, vy = xx + xo, yy + yo
            bv = vy - int(bout[av])
            inband = (0 <= bv) & (bv < B)
            ok = lat & inband & (1 <= vx) & (vx <= x_in) & (1 <= vy) & (vy <= y_in) & (0 <= av - 2 < A)      # E
            if t == T:
                ok = ok | (bx & inband & (vy <= y_in))                                                      # E_b along x == 0
            elif t == T + 1:
                ok = ok | ((by | (bx & (yy == 0))) & inband & (vx <= x_in))                                 # E_b along y == 0
            bvc = np.clip(bv, 0, B - 1)
            w = costs[t, av - 2, bvc].astype(np.float64) if t < T else pen
            cand = w + bsum[av, bvc]
            best = np.where(ok & (cand < best), cand, best)
        if end is not None and end[0] == a:
            best[end[1]] = 0.0
        bsum[a] = best
    return bsum


def traceback(xp, yp, bout, B, x_in, y_in):
    """The rows (x_start, x_len, y_start, y_len) of the back-pointer walk from (x_in, y_in) to (0, 0), in document order."""
    rows = []
    x, y = x_in, y_in
    while (x, y) != (0, 0):
        a = x + y
        b = y - int(bout[a])
        assert 0 <= b < B, "the walk left the band at (%d, %d)" % (x, y)
        xo, yo = int(xp[a, b]), int(yp[a, b])
        assert xo >= 0 and yo >= 0 and xo + yo >= 1, "no back-pointer at (%d, %d)" % (x, y)
        rows.append((x - xo, xo, y - yo, yo))
        x, y = x - xo, y - yo
    return np.asarray(rows[::-1], np.int32).reshape(-1, 4)


def slack(costs, b_offset_in, types, pen, x_in, y_in, csum, bsum, rows, cut=0):
    """slack [len(rows)] float64; rows [n][4] of any integers.  cut: measure at the cut behind diagonal c + cut instead of
    c (the definition's); a row crosses the cuts 0 <= cut < x_len + y_len, and all of them give the same value."""
    costs = np.asarray(costs, np.float32)
    T, A, B = costs.shape
    mv = _moves(types)
    pen = float(pen)
    bout = b_offset_out(b_offset_in)
    Aout = A + 2
    maxstep = max(xo + yo for xo, yo in mv)
    end = end_cell(bout, B, x_in, y_in)
    total = float(csum[end]) if end is not None else INF
    rows = np.asarray(rows).reshape(-1, 4)
    out = np.full(len(rows), np.nan)
    for r, (x0, xl, y0, yl) in enumerate(rows.tolist()):
        c = x0 + y0
        if min(x0, xl, y0, yl) < 0 or xl + yl < 1 or c + xl + yl >= Aout:
            continue
        bus = y0 - int(bout[c])
        bvs = y0 + yl - int(bout[c + xl + yl])
        if not (0 <= bus < B and 0 <= bvs < B):
            continue
        if not 0 <= cut < xl + yl:
            continue
        alt, found = INF, False
        for dv in range(1, maxstep + 1):
            av = c + cut + dv
            if av >= Aout:
                break
            yy, xx, bx, by, gen = _diagonal(av, B, bout, x_in, y_in, A)
            for t, (xo, yo) in enumerate(mv):
                st = xo + yo
                au = av - st
                if st < dv or au < 0:
                    continue
                ux, uy = xx - xo, yy - yo
                bu = uy - int(bout[au])
                inband = (0 <= bu) & (bu < B)
                ok = gen & (ux >= 0) & (uy >= 0) & inband
                if t == T:
                    ok = ok | (bx & (yy >= 1) & inband)
                elif t == T + 1:
                    ok = ok | (by & (xx >= 1) & inband)
                if (xo, yo) == (xl, yl) and au == c:   # the row's own edge (and any duplicate of its move in the list)
                    found = found or bool(ok[bvs])
                    ok = ok.copy()
                    ok[bvs] = False
                buc = np.clip(bu, 0, B - 1)
                w = costs[t, av - 2, :].astype(np.float64) if t < T else pen
                cand = (csum[au, buc] + w) + bsum[av]
                if ok.any():
                    alt = min(alt, float(cand[ok].min()))
        if found:
            with np.errstate(invalid="ignore"):
                out[r] = np.float64(alt) - np.float64(total)
    return out


def summary(sl):
    """(rows, rows with slack == 0, rows with slack == +inf, 0) as svx_row_slack reports it."""
    sl = np.asarray(sl, np.float64)
    return [len(sl), int((sl == 0.0).sum()), int(np.isposinf(sl).sum()), 0]
