"""Reference for svx_score_alignments (include/svx.h): given alignments at the aligner's prices; TEST INFRASTRUCTURE
(numpy, no GPU).

score() restates the definition of svx.h on one stack entry -- the oracle's (dp_ref.straight_stack,
around_ref.around_stack, oracle.vecalign()[0]) or PreparedBatch.level_stack's: it reads n0, n1, del_penalty, new_b_offset,
size0, size1, alignment_types and the band (a_b_csum's width unless B is passed).  Two flavours of the dot product:

  "f32"  the oracle's: rows normalised by oracle.make_norm1 in float32, the products added one after the other in float32
         (svx_oracle.c), the cost expression in double and stored to float32: on the oracle's own path these are the very
         costs its DP added;
  "f64"  rows normalised and multiplied in float64, the cost left in float64: the truth both others are measured against.

edits() builds the neighbours of a path the optimality tests price."""
import numpy as np

PRICED, DELETION, WIDE, INVALID = 0, 1, 2, 3
INT32_MAX = 2 ** 31 - 1


def rows_of(given):
    """[(x ids, y ids)] or int rows -> int64 [r, 4] rows (x_start, x_len, y_start, y_len); the start of an empty side is the
    end of the row before (svx.vecalign.dp_utils.given_rows_from_alignments)."""
    if isinstance(given, np.ndarray):
        return np.asarray(given, np.int64).reshape(-1, 4)
    out, xe, ye = [], 0, 0
    for x, y in given:
        xs, ys = (x[0] if len(x) else xe), (y[0] if len(y) else ye)
        out.append((xs, len(x), ys, len(y)))
        xe, ye = xs + len(x), ys + len(y)
    return np.asarray(out, np.int64).reshape(-1, 4)


def classify(rows, n, m, k0, k1):
    out = []
    for xs, p, ys, q in rows.tolist():
        cls = INVALID
        if xs >= 0 and p >= 0 and ys >= 0 and q >= 0 and xs + p <= n and ys + q <= m:
            if p >= 1 and q >= 1:
                cls = WIDE if (p > k0 or q > k1) else PRICED
            elif p + q == 1:
                cls = DELETION
        out.append(cls)
    return np.asarray(out, np.int64)


def outside(x, y, new_b_offset, B, n, m):
    if not (0 <= x <= n and 0 <= y <= m):
        return True
    a = x + y
    if a >= len(new_b_offset):
        return True
    return not 0 <= y - int(new_b_offset[a]) < B


def _unit_f32(v):
    import oracle
    u = np.array(v, np.float32, copy=True)
    oracle.make_norm1(u)
    return u


def _unit_f64(v):
    v = np.asarray(v, np.float64)
    return v / (np.sqrt((v * v).sum(axis=-1, keepdims=True)) + 1e-5)


def score(st, v0, v1, given, flavour="f32", B=None):
    """-> dict(rows, cls [r], costs [r] (float64 values; NaN where the row is not PRICED), scores [r], total, report (8
    ints), del_penalty).  v0, v1: the candidate tensors [K][n][d] as the aligner got them (float32 values)."""
    assert flavour in ("f32", "f64")
    rows = rows_of(given)
    n, m = int(st['size0']), int(st['size1'])
    k0, k1 = v0.shape[0], v1.shape[0]
    B = int(st['a_b_csum'].shape[1]) if B is None else int(B)
    bout = np.asarray(st['new_b_offset'])
    pen = float(st['del_penalty'])
    types = {(int(x), int(y)) for x, y in st['alignment_types']}
    cls = classify(rows, n, m, k0, k1)
    pr = np.nonzero(cls == PRICED)[0]
    p, q = rows[pr, 1], rows[pr, 3]
    xe, ye = rows[pr, 0] + p - 1, rows[pr, 2] + q - 1
    costs = np.full(len(rows), np.nan)
    if len(pr):
        na = np.asarray(st['n0'], np.float32)[p - 1, xe].astype(np.float64)
        nb = np.asarray(st['n1'], np.float32)[q - 1, ye].astype(np.float64)
        if flavour == "f32":
            a, b = _unit_f32(v0)[p - 1, xe], _unit_f32(v1)[q - 1, ye]
            s = np.zeros(len(pr), np.float32)
            for j in range(a.shape[1]):
                s = (s + (a[:, j] * b[:, j]).astype(np.float32)).astype(np.float32)
            c = ((((2.0 * p) * q) * (1.0 - s.astype(np.float64))) / ((1e-6 + na) + nb)).astype(np.float32).astype(np.float64)
        else:
            a, b = _unit_f64(np.asarray(v0)[p - 1, xe]), _unit_f64(np.asarray(v1)[q - 1, ye])
            c = (((2.0 * p) * q) * (1.0 - (a * b).sum(axis=1))) / ((1e-6 + na) + nb)
        costs[pr] = c
    scores = np.full(len(rows), np.nan)
    scores[cls == DELETION] = 0.0
    if len(pr):
        scores[pr] = np.maximum(costs[pr], 0.0) / (p * q)
    total = 0.0
    for c in costs[pr].tolist():     # row order
        total += c
    dels = int((cls == DELETION).sum())
    total += pen * dels
    nodes = [(0, 0)] + [(int(r[0] + r[1]), int(r[2] + r[3])) for r in rows]
    n_out = sum(1 for x, y in nodes if outside(x, y, bout, B, n, m))
    complete = len(rows) > 0 and not (cls == INVALID).any() and nodes[-1] == (n, m) and \
        all((int(r[0]), int(r[2])) == nodes[i] for i, r in enumerate(rows))
    off_type = sum(1 for i in pr.tolist() if (int(rows[i, 1]), int(rows[i, 3])) not in types)
    report = (len(rows), len(pr), dels, int((cls == WIDE).sum()), int((cls == INVALID).sum()), off_type, n_out, int(complete))
    return dict(rows=rows, cls=cls, costs=costs, scores=scores, total=total, report=report, del_penalty=pen)


def tolerance(*scored):
    """The bound of the optimality tests on total(given) - total(found): every priced cost of either path may sit
    4 * 2^-24 |c| from its true value, and each float64 sum carries rows * 2^-52 * total."""
    tol = 0.0
    for s in scored:
        c = s['costs'][np.isfinite(s['costs'])]
        tol += 4 * 2.0 ** -24 * float(np.abs(c).sum()) + len(s['rows']) * 2.0 ** -52 * abs(s['total'])
    return tol


def truth_path(src_of_target, n):
    """around_ref.block_deletion_pair's truth: the 1-1 pairs of src_of_target, unit deletions for every other source
    segment -> complete alignments [(x ids, y ids)]."""
    out, x = [], 0
    for j, i in enumerate(np.asarray(src_of_target).tolist()):
        out += [([u], []) for u in range(x, i)]
        out.append(([i], [j]))
        x = i + 1
    return out + [([u], []) for u in range(x, n)]


def edits(alignments, types, count, rng):
    """`count` complete paths, each one random edit away from `alignments`: two neighbouring rows merged (when the merged
    type is in `types`), a row split into unit deletions, or a deletion peeled off a row's end."""
    types = {(int(x), int(y)) for x, y in types}
    out = []
    while len(out) < count:
        al = [(list(x), list(y)) for x, y in alignments]
        i = int(rng.randint(0, len(al)))
        kind = int(rng.randint(0, 3))
        x, y = al[i]
        if kind == 0 and i + 1 < len(al):
            x2, y2 = al[i + 1]
            if (len(x) + len(x2), len(y) + len(y2)) not in types:
                continue
            al[i:i + 2] = [(x + x2, y + y2)]
        elif kind == 1 and x and y:
            al[i:i + 1] = [([u], []) for u in x] + [([], [v]) for v in y]
        elif kind == 2 and ((len(x) >= 2 and y) or (len(y) >= 2 and x)):
            if len(x) >= 2 and (len(y) < 2 or rng.randint(0, 2)):
                if (len(x) - 1, len(y)) not in types:
                    continue
                al[i:i + 1] = [(x[:-1], y), ([x[-1]], [])]
            else:
                if (len(x), len(y) - 1) not in types:
                    continue
                al[i:i + 1] = [(x, y[:-1]), ([], [y[-1]])]
        else:
            continue
        out.append(al)
    return out
