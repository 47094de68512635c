"""References for the band search around a prior alignment (include/svx.h: svx_align_around, svx_time_prior): the oracle's
level-0 refinement started from a supplied alignment, the prior ingest rules and the time prior, in numpy."""
import numpy as np

SVX_ERR_ARG, SVX_ERR_TRACEBACK, SVX_ERR_EXTEND, SVX_ERR_PATH = 1, 4, 6, 7


def around_stack(orc, v0, v1, types, W, seed, prior_alignments, norms=None, pen=None):
    """dp_ref.straight_stack with the search path of `prior_alignments` (alignment_to_search_path, dp_utils.py:199-225)
    instead of the straight line: make_sparse_costs + sparse_dp + sparse_traceback around it, depth-0 normalisers and
    deletion penalty drawn from RandomState(seed) in straight_stack's order.  The prior must cover both documents."""
    N, M = v0.shape[1], v1.shape[1]
    a, b = v0.copy(), v1.copy()
    orc.make_norm1(a)
    orc.make_norm1(b)
    rs = seed if isinstance(seed, np.random.RandomState) else np.random.RandomState(seed)
    if norms is None:
        n0, n1 = orc.compute_norms(a, b, 100, rs), orc.compute_norms(b, a, 100, rs)
    else:
        n0, n1 = norms
    est, knob = orc.make_del_penalty(a[0], b[0], n0[0], n1[0], 20000, 0.2, rs)
    path = orc.search_path(prior_alignments, False, N, M)
    f, bo = orc.make_sparse_costs(a, b, n0, n1, path, types, W)
    use = est if pen is None else float(pen)
    csum, xp, yp, bout = orc.sparse_dp(f, bo, types, use, N, M)
    al, sc = orc.sparse_traceback(csum, xp, yp, bout, N, M)
    return dict(searchpath=path, a_b_costs=f, b_offset=bo, a_b_csum=csum, a_b_xp=xp, a_b_yp=yp, new_b_offset=bout,
                final_alignments=al, alignment_scores=sc, del_penalty=use, del_penalty_estimated=est, knob_scores=knob,
                size0=N, size1=M, alignment_types=list(types), n0=n0, n1=n1)


def ingest_ref(rows, count, n, m, code=0, cap=None):
    """The prior ingest of svx_align_around -> (lengths [r, 2] as the search path sees them, 0) or (None, SVX_ERR_*)."""
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    cap = len(rows) if cap is None else cap
    if code != 0:
        return None, int(code)
    if count < 0 or count > cap:
        return None, SVX_ERR_ARG
    xl, yl = rows[:count, 1], rows[:count, 3]
    if ((xl < 0) | (yl < 0) | ((xl == 0) & (yl == 0))).any():
        return None, SVX_ERR_PATH
    sx, sy = int(xl.sum()), int(yl.sum())
    if sx > n or sy > m:
        return None, SVX_ERR_EXTEND
    out = [(int(a), int(b)) for a, b in zip(xl, yl)]
    if sx < n or sy < m:
        out.append((n - sx, m - sy))
    return np.asarray(out, np.int64).reshape(-1, 2), 0


def lengths_to_alignments(lengths):
    """[(x_len, y_len)] -> [([x ids], [y ids])] with running starts."""
    out, x, y = [], 0, 0
    for a, b in np.asarray(lengths).tolist():
        out.append((list(range(x, x + a)), list(range(y, y + b))))
        x, y = x + a, y + b
    return out


def time_prior_ref(F0, F1, window, lag):
    """svx_time_prior -> (rows int32 [r, 4], 0) or (empty rows, SVX_ERR_PATH)."""
    s0 = np.asarray(F0, np.int64).reshape(-1, 2)[:, 0]
    s1 = np.asarray(F1, np.int64).reshape(-1, 2)[:, 0]
    if (np.diff(s0) < 0).any() or (np.diff(s1) < 0).any():
        return np.zeros((0, 4), np.int32), SVX_ERR_PATH
    w0 = s0 // int(window)                                # (numpy's // on int64 is the floor)
    w1 = np.maximum(s1 - int(lag), 0) // int(window)
    rows = []
    for w in sorted(set(w0.tolist()) | set(w1.tolist())):
        rows.append((int((w0 < w).sum()), int((w0 == w).sum()), int((w1 < w).sum()), int((w1 == w).sum())))
    return np.asarray(rows, np.int32).reshape(-1, 4), 0


def layered(base, K):
    """synth.make_pair's candidate layout: layer k row i = sum of base rows i-k..i, rows i < k zero."""
    n, d = base.shape
    out = np.zeros((K, n, d), np.float32)
    cs = np.concatenate([np.zeros((1, d), np.float32), np.cumsum(base.astype(np.float64), axis=0).astype(np.float32)])
    for k in range(K):
        if n > k:
            out[k, k:] = cs[k + 1:n + 1] - cs[:n - k]
    return out


def block_deletion_pair(N=300, lo=100, hi=220, K=4, d=32, seed=0, noise=0.5):
    """Source of N segments; the target is a noisy copy with source segments lo..hi-1 missing.
    -> (v0, v1, src_of_target [M]: the source segment every target segment was copied from)."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((N, d)).astype(np.float32)
    tgt = base + noise * rng.standard_normal((N, d)).astype(np.float32)
    src = np.concatenate([np.arange(lo), np.arange(hi, N)])
    return layered(base, K), layered(tgt[src], K), src


def true_pairs_found(alignments, src_of_target):
    """How many target segments j sit in a 1-1 alignment with the source segment they were copied from."""
    return sum(1 for x, y in alignments if len(x) == 1 and len(y) == 1 and src_of_target[y[0]] == x[0])


def block_prior(src_of_target, N, step=20):
    """Blocks of `step` source segments each, with the target segments copied from them."""
    src = np.asarray(src_of_target)
    out = []
    for x0 in range(0, N, step):
        x1 = min(N, x0 + step)
        ys = np.nonzero((src >= x0) & (src < x1))[0]
        out.append((list(range(x0, x1)), ys.tolist()))
    return out
