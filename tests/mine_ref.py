"""References for margin-based mining (csrc/svx_mine.hip: k_list_means, k_margin_candidates; svx_mine_greedy;
svx/postprocess/mine.py).  numpy only; shared by test_mine_ref_cpu.py (no GPU) and test_gpu_mine.py; TEST INFRASTRUCTURE.

(a) `list_means`, `candidates`, `select` with dtype float32: the contract of include/svx.h in numpy's fp32, one rounded
    operation per step in the header's order (the list sum by a sequential column loop; fp32 division and addition are
    correctly rounded in numpy).  The GPU must return these bits.
(b) the same functions with dtype float64, on the same fp32 inputs.
(c) `laser_*`: LASER's mine_bitexts.py restated literally with Python loops and scalars, for tiny inputs: the double
    loop of score_candidates, the argmax per row, the four retrievals and the greedy seen_src / seen_trg pass.  Where
    LASER leaves something open, the contract decides: an id of -1 or out of range scores -inf, the first maximum wins
    (np.argmax's rule too), a row whose maximum is -inf has no candidate, candidates are ordered by a stable sort.

`synthetic_lists` builds lists that come from no search, with the edge rows the kernels must handle."""
import numpy as np

MARGINS = ("ratio", "distance", "absolute")
RETRIEVALS = ("max", "forward", "backward", "intersection")
ROW_KINDS = 8


# ------------------------------------------------------------------------------------------------ (a) and (b)
def list_means(sims, dtype=np.float32):
    """(((s0 + s1) + ...) + s[k-1]) / k in `dtype`."""
    s = np.asarray(sims).astype(dtype)
    tot = s[:, 0].copy()
    with np.errstate(invalid="ignore"):
        for j in range(1, s.shape[1]):
            tot = tot + s[:, j]
        return (tot / dtype(s.shape[1])).astype(dtype)


def candidates(sims, ids, mean_q, mean_db, margin, id_base=0, dtype=np.float32):
    """-> (scores [n, k] dtype, best_id [n] int64, best_score [n] dtype)."""
    assert margin in MARGINS, margin
    s = np.asarray(sims).astype(dtype)
    ids = np.asarray(ids, np.int64)
    n, k = s.shape
    n_db = len(mean_db)
    mq = np.asarray(mean_q).astype(dtype)
    md = np.asarray(mean_db).astype(dtype)
    valid = (ids != -1) & (ids >= id_base) & (ids - np.int64(id_base) < n_db)
    row = np.where(valid, ids - np.int64(id_base), 0)
    scores = np.empty((n, k), dtype)
    best_id = np.full(n, -1, np.int64)
    best_score = np.full(n, -np.inf, dtype)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for j in range(k):
            if margin == "absolute":
                sc = s[:, j].copy()
            else:
                b = (mq + (md[row[:, j]] if n_db else mq)) * dtype(0.5)
                sc = s[:, j] / b if margin == "ratio" else s[:, j] - b
            sc = np.where(valid[:, j], sc, dtype(-np.inf)).astype(dtype)
            scores[:, j] = sc
            better = sc > best_score
            best_score = np.where(better, sc, best_score)
            best_id = np.where(better, ids[:, j], best_id)
    return scores, best_id, best_score


def greedy(order, src, tgt):
    """The kept candidate indices of `order`, in order."""
    seen_src, seen_tgt, kept = set(), set(), []
    for c in order:
        c = int(c)
        if int(src[c]) in seen_src or int(tgt[c]) in seen_tgt:
            continue
        seen_src.add(int(src[c]))
        seen_tgt.add(int(tgt[c]))
        kept.append(c)
    return np.asarray(kept, np.int64)


def select(fwd_best, fwd_score, bwd_best, bwd_score, retrieval, threshold=None):
    """The retrieval step -> (scores, src int64, tgt int64) in output order."""
    assert retrieval in RETRIEVALS, retrieval
    fwd_best, bwd_best = np.asarray(fwd_best, np.int64), np.asarray(bwd_best, np.int64)
    rows_x, rows_y = np.arange(fwd_best.shape[0], dtype=np.int64), np.arange(bwd_best.shape[0], dtype=np.int64)
    if retrieval == "forward":
        src, tgt, score = rows_x, fwd_best, fwd_score
    elif retrieval == "backward":
        src, tgt, score = bwd_best, rows_y, bwd_score
    elif retrieval == "intersection":
        keep = fwd_best >= 0
        keep[keep] = bwd_best[fwd_best[keep]] == rows_x[keep]
        src, tgt, score = rows_x[keep], fwd_best[keep], fwd_score[keep]
    else:
        src, tgt, score = np.concatenate([rows_x, bwd_best]), np.concatenate([fwd_best, rows_y]), np.concatenate([fwd_score, bwd_score])
    valid = (src >= 0) & (tgt >= 0)
    src, tgt, score = src[valid], tgt[valid], np.asarray(score)[valid]
    order = np.argsort(-score, kind="stable")
    src, tgt, score = src[order], tgt[order], score[order]
    if retrieval == "max":
        kept = greedy(np.arange(src.shape[0]), src, tgt)
        src, tgt, score = src[kept], tgt[kept], score[kept]
    if threshold is not None:
        keep = score > score.dtype.type(threshold)
        src, tgt, score = src[keep], tgt[keep], score[keep]
    return score, src, tgt


def mine(sims_xy, ids_xy, sims_yx, ids_yx, margin, dtype=np.float32):
    """Steps 3 and 4 of mine_bitexts on the lists of the two searches -> (fwd_best, fwd_score, bwd_best, bwd_score)."""
    mean_x, mean_y = list_means(sims_xy, dtype), list_means(sims_yx, dtype)
    _, fwd_best, fwd_score = candidates(sims_xy, ids_xy, mean_x, mean_y, margin, 0, dtype)
    _, bwd_best, bwd_score = candidates(sims_yx, ids_yx, mean_y, mean_x, margin, 0, dtype)
    return fwd_best, fwd_score, bwd_best, bwd_score


# ------------------------------------------------------------------------------------------------ (c) LASER, literally
def _laser_margin(margin):
    if margin == "absolute":
        return lambda a, b: a
    if margin == "distance":
        return lambda a, b: a - b
    assert margin == "ratio"
    return lambda a, b: a / b


def laser_score_candidates(sims, ids, fwd_mean, bwd_mean, margin, id_base=0):
    """score_candidates: scores[i, j] = margin(sim(i, j), (fwd_mean[i] + bwd_mean[ids[i, j]]) / 2), fp32 scalars."""
    fn = _laser_margin(margin)
    n, k = np.shape(sims)
    scores = np.zeros((n, k), np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i in range(n):
            for j in range(k):
                r = int(ids[i][j]) - int(id_base)
                if int(ids[i][j]) == -1 or r < 0 or r >= len(bwd_mean):
                    scores[i, j] = -np.inf
                elif margin == "absolute":
                    scores[i, j] = np.float32(sims[i][j])
                else:
                    scores[i, j] = fn(np.float32(sims[i][j]), (np.float32(fwd_mean[i]) + np.float32(bwd_mean[r])) / np.float32(2))
    return scores


def laser_best(scores, ids):
    """x2y_ind[np.arange(n), scores.argmax(axis=1)] and scores.max(axis=1); NaN never wins, a row of -inf has no candidate."""
    best_id, best_score = [], []
    for i in range(scores.shape[0]):
        row = np.where(np.isnan(scores[i]), -np.inf, scores[i])
        j = int(np.argmax(row))
        if row[j] == -np.inf:
            best_id.append(-1)
            best_score.append(np.float32(-np.inf))
        else:
            best_id.append(int(ids[i][j]))
            best_score.append(np.float32(row[j]))
    return np.asarray(best_id, np.int64), np.asarray(best_score, np.float32)


def laser_retrieve(fwd_best, fwd_score, bwd_best, bwd_score, retrieval, threshold=None):
    """The `--retrieval` branches of mine_bitexts.py -> list of (score, src, tgt)."""
    nx, ny = len(fwd_best), len(bwd_best)
    if retrieval == "forward":
        cand = [(fwd_score[i], i, int(fwd_best[i])) for i in range(nx)]
    elif retrieval == "backward":
        cand = [(bwd_score[j], int(bwd_best[j]), j) for j in range(ny)]
    elif retrieval == "intersection":
        cand = [(fwd_score[i], i, int(j)) for i, j in enumerate(fwd_best) if j >= 0 and bwd_best[j] == i]
    else:
        assert retrieval == "max"
        cand = [(fwd_score[i], i, int(fwd_best[i])) for i in range(nx)] + [(bwd_score[j], int(bwd_best[j]), j) for j in range(ny)]
    cand = [c for c in cand if c[1] >= 0 and c[2] >= 0]
    cand = sorted(cand, key=lambda c: -c[0])        # (sorted() is stable)
    out = []
    if retrieval == "max":
        seen_src, seen_trg = set(), set()
        for score, src_ind, trg_ind in cand:
            if src_ind not in seen_src and trg_ind not in seen_trg:
                seen_src.add(src_ind)
                seen_trg.add(trg_ind)
                out.append((score, src_ind, trg_ind))
    else:
        out = cand
    if threshold is not None:
        out = [c for c in out if c[0] > threshold]
    return out


def as_triples(result):
    """(scores, src, tgt) arrays -> list of (score bits, src, tgt) for comparisons that include the order."""
    score, src, tgt = result
    bits = np.ascontiguousarray(score, np.float32).view(np.uint32)
    return [(int(b), int(s), int(t)) for b, s, t in zip(bits, src, tgt)]


def triples_of_list(cands):
    return [(int(np.float32(c[0]).view(np.uint32)), int(c[1]), int(c[2])) for c in cands]


# ------------------------------------------------------------------------------------------------ synthetic lists
def synthetic_lists(n, k, n_db, id_base, seed, shift=0):
    """Lists [n, k] that no search produced -> dict(sims, ids, mean_q, mean_db, kind [n]).  n_db >= k.  Row i is of kind
    (i + shift) % 8:
      0  plain: similarities descending, distinct ids in range
      1  trailing (-inf, -1) entries (the whole row when k = 1)
      2  some ids outside [id_base, id_base + n_db): just below, just past, far past, and small ones when id_base > 0
      3  exact score ties: one similarity throughout and neighbours whose means repeat, the best score among them
      4  no valid candidate: all (-inf, -1)
      5  no valid candidate: finite similarities, every id out of range
      6  b = 0 at the first neighbour (mean_q = -mean_db: +inf for ratio) and a similarity of 0 there in every other row
         of this kind (0 / 0: NaN must not win)
      7  duplicated similarities and a -0.0
    The means of the database take few distinct values, so equal (similarity, mean) pairs are common everywhere."""
    assert n_db >= k
    rs = np.random.RandomState([seed, n, k, n_db % 65521, shift])
    sims = -np.sort(-(rs.randint(13107, 58982, size=(n, k)).astype(np.float32) / np.float32(65536)), axis=1)
    # k distinct ids per row: one random set of offsets behind a random first row
    ids = (rs.randint(n_db, size=(n, 1)) + rs.permutation(n_db)[None, :k]) % n_db + np.int64(id_base)
    mean_q = (rs.randint(6553, 39321, size=n).astype(np.float32) / np.float32(65536))
    mean_db = (rs.randint(8, 24, size=n_db).astype(np.float32) / np.float32(32))
    kind = ((np.arange(n) + shift) % ROW_KINDS).astype(np.int64)
    for i in range(n):
        kd = kind[i]
        if kd == 1:
            t = k if k == 1 else int(rs.randint(1, k))
            sims[i, k - t:] = -np.inf
            ids[i, k - t:] = -1
        elif kd == 2:
            bad = [id_base - 1, id_base + n_db, id_base + n_db + 5, np.int64(1) << 40]
            if id_base > 0:
                bad += [3, 0]
            for j in rs.permutation(k)[:max(1, k // 3)]:
                ids[i, j] = bad[int(rs.randint(len(bad)))]
        elif kd == 3:
            sims[i, :] = sims[i, 0]
            if k > 1:   # the two smallest means of the row made equal: the best score (smallest b) occurs twice
                m = mean_db[ids[i] - id_base]
                a, b = np.argsort(m, kind="stable")[:2]
                mean_db[ids[i, b] - id_base] = m[a]
        elif kd == 4:
            sims[i, :] = -np.inf
            ids[i, :] = -1
        elif kd == 5:
            ids[i, :] = id_base + n_db + np.arange(k)
        elif kd == 6:
            mean_q[i] = -mean_db[ids[i, 0] - id_base]
            if (i // ROW_KINDS) % 2:
                sims[i, 0] = 0.0
        elif kd == 7:
            if k > 1:
                sims[i, 1::2] = sims[i, 0:k - 1:2][:sims[i, 1::2].shape[0]]
            sims[i, k - 1] = -0.0
    return dict(sims=np.ascontiguousarray(sims), ids=np.ascontiguousarray(ids), mean_q=mean_q, mean_db=mean_db, kind=kind)


# ------------------------------------------------------------------------------------------------ real rows
def example_lists_f64(x, y, k):
    """x, y [n, d] rows -> the exact float64 search of both directions on the float64-normalised rows:
    (sims_xy, ids_xy, sims_yx, ids_yx), similarities float64."""
    import search_ref as sr
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    xn = x / np.sqrt((x * x).sum(axis=1, keepdims=True))
    yn = y / np.sqrt((y * y).sum(axis=1, keepdims=True))
    S = xn @ yn.T
    sims_xy, ids_xy = sr.search_exact(S, k)
    sims_yx, ids_yx = sr.search_exact(np.ascontiguousarray(S.T), k)
    return sims_xy, ids_xy, sims_yx, ids_yx


def top_two_gap(scores):
    """Per row the difference between the two largest finite entries of scores [n, k] (inf where there is one or none)."""
    s = np.where(np.isfinite(scores), scores, -np.inf).astype(np.float64)
    srt = -np.sort(-s, axis=1)
    if srt.shape[1] < 2:
        return np.full(s.shape[0], np.inf)
    with np.errstate(invalid="ignore"):
        gap = srt[:, 0] - srt[:, 1]
    return np.where(np.isfinite(gap), gap, np.inf)
