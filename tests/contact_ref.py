"""Reference for band-edge contact and band doubling (include/svx.h: svx_band_contact, svx_align_widen); TEST
INFRASTRUCTURE (numpy, no GPU).

contact() restates the definition of svx.h: the nodes of a level are (0, 0) and the end of every alignment row; a node's
clearance is its distance in cells to those edges of the band on its diagonal that have a lattice node behind them.
widen_chain() is the doubling loop on the CPU oracle, built from dp_ref.straight_stack / around_ref.around_stack."""
import numpy as np

from around_ref import around_stack
from dp_ref import straight_stack

INT32_MAX = 2 ** 31 - 1


def nodes_of(alignments_or_rows):
    """[(x ids, y ids)] or int rows (x_start, x_len, y_start, y_len) -> [(x, y)] nodes, (0, 0) first."""
    out = [(0, 0)]
    if isinstance(alignments_or_rows, np.ndarray):
        for xs, xl, ys, yl in np.asarray(alignments_or_rows, np.int64).reshape(-1, 4).tolist():
            out.append((xs + xl, ys + yl))
        return out
    x = y = 0
    for xi, yi in alignments_or_rows:   # (the ids of a complete monotone alignment: the ends are the running sums)
        x, y = x + len(xi), y + len(yi)
        out.append((x, y))
    return out


def clearances(nodes, new_b_offset, B, size0, size1):
    out = []
    for x, y in nodes:
        a = x + y
        o = int(new_b_offset[a])
        b = y - o
        c = INT32_MAX
        yl, yh = o - 1, o + B
        if 0 <= a - yl <= size0 and 0 <= yl <= size1:
            c = min(c, b)
        if 0 <= a - yh <= size0 and 0 <= yh <= size1:
            c = min(c, B - 1 - b)
        out.append(c)
    return out


def contact(alignments_or_rows, new_b_offset, B, size0, size1, guard=0):
    """-> (touch, run, clearance, nodes) as svx_band_contact writes them."""
    cl = clearances(nodes_of(alignments_or_rows), new_b_offset, B, size0, size1)
    touch = [c <= guard for c in cl]
    run = best = 0
    for t in touch:
        run = run + 1 if t else 0
        best = max(best, run)
    return (int(sum(touch)), best, int(min(cl)), len(cl))


def contact_of_stack(st, guard=0, W=None):
    """contact() of one stack entry (the oracle's, or PreparedBatch.level_stack's)."""
    B = st['a_b_csum'].shape[1] if W is None else 2 * W
    return contact(st['final_alignments'] if 'final_alignments' in st else st['alignments'], st['new_b_offset'], B,
                   st['size0'], st['size1'], guard)


def end_csum(st):
    """The DP's cumulative cost at node (size0, size1): the total cost of the returned path."""
    n, m = st['size0'], st['size1']
    return float(st['a_b_csum'][n + m, m - int(st['new_b_offset'][n + m])])


def widen_chain(orc, v0, v1, types, W0, seed, guard=0, max_width_over2=None, max_rounds=4, first=None):
    """Band doubling on the oracle -> (stacks per round, report (rounds, final width_over2, touch after round 0, touch
    after the last round)).  Round 0 is the straight search, or `first` = a stack entry the caller made with
    around_stack(..., seed, prior); every round draws from a fresh RandomState(seed): the same depth-0 draws."""
    W0 = max(3, W0)
    max_width_over2 = W0 << max_rounds if max_width_over2 is None else max_width_over2
    st = straight_stack(orc, v0, v1, types, W0, seed) if first is None else first
    stacks, W = [st], W0
    touch0 = touch = contact_of_stack(st, guard)[0]
    rounds = 0
    while touch > 0 and rounds < max_rounds and min(2 * W, max_width_over2) > W:
        W = min(2 * W, max_width_over2)
        st = around_stack(orc, v0, v1, types, W, seed, st['final_alignments'])
        stacks.append(st)
        rounds += 1
        touch = contact_of_stack(st, guard)[0]
    return stacks, (rounds, W, touch0, touch)
