"""Row slack in wide bands: numpy restatement of the fused scheme of csrc/svx_tiles_bwd.hip; TEST INFRASTRUCTURE (no GPU).

slack_ref.py stays the normative text (include/svx.h, "row slack").  This file restates HOW the backward tile sweep gets
the same numbers without a stored backward plane per row scan:

  * one backward sweep over the diagonals computes Bk(u) = min (w + Bk(v)) over the edges u -> v of E and E_b
    (slack_ref.backward's edge rule, line by line), and in the same pass prices every edge once,
        cand = (F(u) + w) + Bk(v);
  * an edge from diagonal a(u) with step st crosses the cuts a(u) .. a(u) + st - 1 and feeds each of them, unless u is the
    returned path's node of its diagonal and the move is the row's move (the row's own edge and any duplicate of its move);
  * edges are owned by the tile of u (tile x tile nodes): every tile keeps its own minimum per cut, and cutmin[c] is the
    minimum over the tiles -- what the kernel's one atomic minimum per (tile, cut) computes;
  * slack[r] = cutmin[x_start + y_start] - F(end); NaN for a row that is no edge.

Every candidate is the same two float64 additions as in slack_ref.slack and a minimum does not depend on its order, so
fused(...) == slack_ref.slack(...) bit for bit on any input, for any tile size."""
import numpy as np

from dp_ref import INF, _diagonal, _moves
from slack_ref import b_offset_out, end_cell


def fused(costs, b_offset_in, types, pen, x_in, y_in, csum, rows, tile=32):
    """-> (slack [len(rows)], cutmin [A+2], Bk [A+2][B]) float64."""
    costs = np.asarray(costs, np.float32)
    T, A, B = costs.shape
    mv = _moves(types)
    pen = float(pen)
    bout = b_offset_out(b_offset_in)
    Aout = A + 2
    end = end_cell(bout, B, x_in, y_in)
    total = float(csum[end]) if end is not None else INF
    rows = np.asarray(rows).reshape(-1, 4)
    # the returned path's node on each diagonal: diagonal -> (cell, move); rows that cannot be edges are left out
    node = {}
    valid = np.zeros(len(rows), bool)
    for r, (x0, xl, y0, yl) in enumerate(rows.tolist()):
        c = x0 + y0
        if min(x0, xl, y0, yl) < 0 or xl + yl < 1 or c + xl + yl >= Aout:
            continue
        bus, bvs = y0 - int(bout[c]), y0 + yl - int(bout[c + xl + yl])
        if 0 <= bus < B and 0 <= bvs < B:
            node[c] = (bus, (xl, yl))
            valid[r] = True
    ntj = y_in // tile + 1
    ntiles = (x_in // tile + 1) * ntj
    part = np.full((ntiles, Aout), INF)          # per (owner tile, cut)
    found = np.zeros(Aout, bool)                 # the own edge of the row that starts on the diagonal is an edge
    bsum = np.full((Aout, B), INF, np.float64)
    for a in range(Aout - 1, -1, -1):
        yy, xx, bx, by, gen = _diagonal(a, B, bout, x_in, y_in, A)
        lat = bx | by | gen
        owner = np.where(lat, (xx // tile) * ntj + yy // tile, 0)
        best = np.full(B, INF)
        for t, (xo, yo) in enumerate(mv):
            st = xo + yo
            av = a + st
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
            nxt = bsum[av, bvc]
            tot = w + nxt
            best = np.where(ok & (tot < best), tot, best)
            with np.errstate(invalid="ignore"):
                cand = (csum[a] + w) + nxt
            live = ok.copy()
            if a in node and node[a][1] == (xo, yo):
                found[a] = found[a] or bool(ok[node[a][0]])
                live[node[a][0]] = False
            for k in np.unique(owner[live]):
                m = cand[live & (owner == k)].min()
                part[k, a:av] = np.minimum(part[k, a:av], m)
        if end is not None and end[0] == a:
            best[end[1]] = 0.0
        bsum[a] = best
    cutmin = part.min(axis=0)
    out = np.full(len(rows), np.nan)
    for r, (x0, xl, y0, yl) in enumerate(rows.tolist()):
        if valid[r] and found[x0 + y0] and node[x0 + y0] == (y0 - int(bout[x0 + y0]), (xl, yl)):
            with np.errstate(invalid="ignore"):
                out[r] = np.float64(cutmin[x0 + y0]) - np.float64(total)
    return out, cutmin, bsum
