"""python -m svx.postprocess.mine --src_index P --tgt_index P --out F [--k 16] [--margin ratio|distance|absolute]
    [--retrieval max|forward|backward|intersection] [--threshold T] [--gpu_type fp16-shard]

Margin-based mining over two exact databases (Artetxe & Schwenk, https://aclanthology.org/P19-1309 sec. 3; the global
mining of LASER's mine_bitexts.py, the baseline Speech-Vecalign is compared against), and xSIM, its error rate on
parallel rows.  Every row of one side is searched in the other with `FlatIndex.search` (both directions), the mean of
every k-NN list is taken (svx_knn_list_means), every neighbour is re-scored with the margin and the best one per row
kept (svx_margin_candidates); the retrieval step then selects pairs:

    forward       every (i, fwd_best[i])                                    stable sort, score descending
    backward      every (bwd_best[j], j)                                    stable sort, score descending
    intersection  (i, fwd_best[i]) where bwd_best[fwd_best[i]] == i         stable sort, score descending
    max           forward candidates (rows ascending) then backward ones, stable sort by score descending, then the
                  greedy pass that keeps a pair when neither of its rows was kept before (svx_mine_greedy)

Rows without a valid neighbour (best id -1) are dropped before the sort; `threshold` keeps score > threshold and is
applied after the selection, as in LASER.  Output lines: score<TAB>source row<TAB>target row.

Local mining -- the same inside every parallel document pair, the paper's second baseline -- is `mine_local` (all pairs of
a batch at once: one grouped search per direction, `FlatIndex.search_groups`); its CLI is svx.postprocess.mine_local."""
import argparse
import ctypes
import logging
from pathlib import Path

import numpy as np

from .. import _lib
from .flat_index import FlatIndex

logger = logging.getLogger(__name__)
MARGINS = {"ratio": _lib.SVX_MARGIN_RATIO, "distance": _lib.SVX_MARGIN_DISTANCE, "absolute": _lib.SVX_MARGIN_ABSOLUTE}
RETRIEVALS = ("max", "forward", "backward", "intersection")


def _margin_code(margin):
    if margin not in MARGINS:
        raise ValueError(f"Wrong margin type: {margin}")
    return MARGINS[margin]


def _context_of(sims):
    if not hasattr(sims, "data_ptr") or not sims.is_cuda:
        raise ValueError("sims must be a device tensor (FlatIndex.search returns one)")
    return _lib.context(sims.device.index)


def _lists(ctx, sims, ids=None):
    """The [n, k] device tensors a search left, checked."""
    t = ctx.torch
    for name, a, dt in (("sims", sims, t.float32), ("ids", ids, t.int64)):
        if a is None:
            continue
        if not hasattr(a, "data_ptr") or a.ndim != 2 or a.dtype != dt or not a.is_cuda or not a.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {str(dt).split('.')[-1]} [n, k] device tensor")
    if ids is not None and tuple(ids.shape) != tuple(sims.shape):
        raise ValueError(f"sims {tuple(sims.shape)} and ids {tuple(ids.shape)} differ in shape")
    return int(sims.shape[0]), int(sims.shape[1])


def _vector(ctx, a, name):
    t = ctx.torch
    if not hasattr(a, "data_ptr") or a.ndim != 1 or a.dtype != t.float32 or not a.is_cuda or not a.is_contiguous():
        raise ValueError(f"{name} must be a contiguous float32 device vector")
    return a


def list_means(sims):
    """sims float32 [n, k] (FlatIndex.search) -> float32 [n] on the device: the k values of a row added one by one in
    fp32, j ascending, divided by k (svx_knn_list_means)."""
    ctx = _context_of(sims)
    n, k = _lists(ctx, sims)
    out = ctx.torch.empty((n,), dtype=ctx.torch.float32, device=sims.device)
    ctx.check(ctx.lib.svx_knn_list_means(ctx.h, ctypes.c_void_p(sims.data_ptr()), n, k, ctypes.c_void_p(out.data_ptr())))
    return out


def candidate_scores(sims, ids, mean_q, mean_db, margin, id_base=0, want_scores=False):
    """The neighbours (sims, ids) [n, k] of n queries re-scored with the margin between mean_q [n] (the queries' list
    means) and mean_db (the list means of the other side, row ids[i][j] - id_base) -> (best_id int64 [n], best_score
    float32 [n], scores float32 [n, k] or None), device tensors (svx_margin_candidates: the first best neighbour wins,
    an id of -1 or out of range scores -inf, a row without a valid neighbour comes back as (-1, -inf))."""
    code = _margin_code(margin)
    ctx = _context_of(sims)
    t = ctx.torch
    n, k = _lists(ctx, sims, ids)
    mean_q, mean_db = _vector(ctx, mean_q, "mean_q"), _vector(ctx, mean_db, "mean_db")
    if mean_q.shape[0] != n:
        raise ValueError(f"mean_q has {mean_q.shape[0]} entries for {n} queries")
    best_id = t.empty((n,), dtype=t.int64, device=sims.device)
    best_score = t.empty((n,), dtype=t.float32, device=sims.device)
    scores = t.empty((n, k), dtype=t.float32, device=sims.device) if want_scores else None
    ctx.check(ctx.lib.svx_margin_candidates(
        ctx.h, ctypes.c_void_p(sims.data_ptr()), ctypes.c_void_p(ids.data_ptr()), n, k, ctypes.c_void_p(mean_q.data_ptr()),
        ctypes.c_void_p(mean_db.data_ptr() if mean_db.shape[0] else None), int(mean_db.shape[0]), int(id_base), code,
        ctypes.c_void_p(scores.data_ptr()) if want_scores else None, ctypes.c_void_p(best_id.data_ptr()),
        ctypes.c_void_p(best_score.data_ptr())))
    return best_id, best_score, scores


def best_candidates(idx_x: FlatIndex, idx_y: FlatIndex, k: int, margin: str):
    """Both searches, both list means and both candidate scorings -> (fwd_best int64 [n_x], fwd_score float32 [n_x],
    bwd_best int64 [n_y], bwd_score float32 [n_y]) on the device: the best target row of every source row and the best
    source row of every target row."""
    _margin_code(margin)
    if idx_x.ntotal < k or idx_y.ntotal < k:
        raise ValueError(f"the indexes hold {idx_x.ntotal} and {idx_y.ntotal} rows, fewer than k = {k}")
    sims_xy, ids_xy = idx_y.search(idx_x.rows, k)   # x among the targets
    sims_yx, ids_yx = idx_x.search(idx_y.rows, k)   # y among the sources
    mean_x, mean_y = list_means(sims_xy), list_means(sims_yx)
    fwd_best, fwd_score, _ = candidate_scores(sims_xy, ids_xy, mean_x, mean_y, margin)
    bwd_best, bwd_score, _ = candidate_scores(sims_yx, ids_yx, mean_y, mean_x, margin)
    return fwd_best, fwd_score, bwd_best, bwd_score


def mine_greedy(order: np.ndarray, src: np.ndarray, tgt: np.ndarray, n_src: int, n_tgt: int) -> np.ndarray:
    """svx_mine_greedy on host arrays -> the kept candidate indices, in order."""
    lib = _lib.load()
    order, src, tgt = (np.ascontiguousarray(a, dtype=np.int64) for a in (order, src, tgt))
    if src.shape != tgt.shape or src.ndim != 1 or order.shape != src.shape:
        raise ValueError(f"order {order.shape}, src {src.shape} and tgt {tgt.shape} must be vectors of one length")
    out = np.empty(order.shape, dtype=np.int64)
    kept = lib.svx_mine_greedy(ctypes.c_void_p(order.ctypes.data), int(order.shape[0]), ctypes.c_void_p(src.ctypes.data),
                               ctypes.c_void_p(tgt.ctypes.data), int(n_src), int(n_tgt), ctypes.c_void_p(out.ctypes.data))
    if kept < 0:
        raise ValueError("svx_mine_greedy: a candidate index or a row is out of range")
    return out[:kept]


def select_pairs(fwd_best, fwd_score, bwd_best, bwd_score, retrieval="max", threshold=None):
    """The retrieval step on the device tensors of `best_candidates` -> (scores float32 [p], src int64 [p], tgt int64 [p])
    numpy arrays."""
    if retrieval not in RETRIEVALS:
        raise ValueError(f"retrieval {retrieval!r}: one of {', '.join(RETRIEVALS)}")
    import torch as t
    n_x, n_y = int(fwd_best.shape[0]), int(bwd_best.shape[0])
    rows_x = t.arange(n_x, dtype=t.int64, device=fwd_best.device)
    rows_y = t.arange(n_y, dtype=t.int64, device=bwd_best.device)
    if retrieval == "forward":
        src, tgt, score = rows_x, fwd_best, fwd_score
    elif retrieval == "backward":
        src, tgt, score = bwd_best, rows_y, bwd_score
    elif retrieval == "intersection":
        src, tgt, score = rows_x, fwd_best, fwd_score
        back = bwd_best[fwd_best.clamp(min=0)] if n_y else t.full_like(fwd_best, -1)
        keep = (fwd_best >= 0) & (back == rows_x)
        src, tgt, score = src[keep], tgt[keep], score[keep]
    else:
        src, tgt, score = t.cat([rows_x, bwd_best]), t.cat([fwd_best, rows_y]), t.cat([fwd_score, bwd_score])
    valid = (src >= 0) & (tgt >= 0)
    src, tgt, score = src[valid], tgt[valid], score[valid]
    score, order = t.sort(score, stable=True, descending=True)
    src, tgt, score = src[order].cpu().numpy(), tgt[order].cpu().numpy(), score.cpu().numpy()
    if retrieval == "max":
        kept = mine_greedy(np.arange(src.shape[0], dtype=np.int64), src, tgt, n_x, n_y)
        src, tgt, score = src[kept], tgt[kept], score[kept]
    if threshold is not None:
        keep = score > np.float32(threshold)
        src, tgt, score = src[keep], tgt[keep], score[keep]
    return score, src, tgt


def mine_bitexts(idx_x: FlatIndex, idx_y: FlatIndex, k: int = 16, margin: str = "ratio", retrieval: str = "max", threshold=None):
    """Mine the rows of idx_x (sources) against the rows of idx_y (targets) -> (scores float32 [p], src int64 [p],
    tgt int64 [p]) on the host, in output order (module docstring)."""
    _margin_code(margin)
    if retrieval not in RETRIEVALS:
        raise ValueError(f"retrieval {retrieval!r}: one of {', '.join(RETRIEVALS)}")
    return select_pairs(*best_candidates(idx_x, idx_y, k, margin), retrieval=retrieval, threshold=threshold)


# ------------------------------------------------------------------------------------------------ local mining
def _group_offsets(x_off, y_off):
    offs = []
    for name, a in (("x_off", x_off), ("y_off", y_off)):
        a = np.asarray(a)
        if a.ndim != 1 or a.shape[0] < 1 or a.dtype.kind not in "iu":
            raise ValueError(f"{name} must be a vector of n_groups + 1 integers")
        a = np.ascontiguousarray(a, dtype=np.int64)
        if a[0] != 0 or (np.diff(a) < 0).any():
            raise ValueError(f"{name} must start at 0 and never decrease")
        offs.append(a)
    if offs[0].shape != offs[1].shape:
        raise ValueError(f"x_off has {offs[0].shape[0]} entries, y_off {offs[1].shape[0]}")
    return offs


def small_groups(x_off, y_off, k: int) -> np.ndarray:
    """bool [n_groups]: the pairs with fewer than k rows on either side, which local mining leaves out."""
    x_off, y_off = _group_offsets(x_off, y_off)
    return (np.diff(x_off) < k) | (np.diff(y_off) < k)


def _pack_groups(rows, off, kept):
    """The rows of the groups `kept`, packed -> (rows, their offsets)."""
    import torch as t
    sel = np.concatenate([np.arange(off[g], off[g + 1], dtype=np.int64) for g in kept] + [np.zeros(0, np.int64)])
    return rows.index_select(0, t.from_numpy(sel).to(rows.device)), np.concatenate([[0], np.cumsum(np.diff(off)[kept])]).astype(np.int64)


def best_candidates_local(x_unit, y_unit, x_off, y_off, k: int, margin: str):
    """`best_candidates` inside every document pair: x_unit [n_x, d], y_unit [n_y, d] are contiguous fp16 / bf16 device
    tensors of unit rows, pair g holds the source rows [x_off[g], x_off[g+1]) and the target rows [y_off[g], y_off[g+1]).
    One grouped search per direction (FlatIndex.search_groups), then the list means and the candidate scoring once each
    over all rows with global row ids -> (fwd_best int64 [n_x], fwd_score float32 [n_x], bwd_best int64 [n_y], bwd_score
    float32 [n_y]) on the device; the best rows are global row numbers, always inside the row's own pair.  Every pair needs
    k rows on both sides (as `best_candidates`); `mine_local` leaves the smaller ones out first."""
    _margin_code(margin)
    x_off, y_off = _group_offsets(x_off, y_off)
    idx_x, idx_y = FlatIndex.over(x_unit), FlatIndex.over(y_unit)
    if idx_x.d != idx_y.d or idx_x.storage != idx_y.storage:
        raise ValueError("the two sides differ in dimension or storage type")
    if int(x_off[-1]) != idx_x.ntotal or int(y_off[-1]) != idx_y.ntotal:
        raise ValueError(f"the offsets end at {int(x_off[-1])} and {int(y_off[-1])} for {idx_x.ntotal} and {idx_y.ntotal} rows")
    small = small_groups(x_off, y_off, k)
    if small.any():
        g = int(np.nonzero(small)[0][0])
        raise ValueError(f"pair {g} holds {int(x_off[g + 1] - x_off[g])} and {int(y_off[g + 1] - y_off[g])} rows, fewer than k = {k}")
    sims_xy, ids_xy = idx_y.search_groups(x_unit, k, x_off, y_off)   # x among the targets of its pair
    sims_yx, ids_yx = idx_x.search_groups(y_unit, k, y_off, x_off)   # y among the sources of its pair
    mean_x, mean_y = list_means(sims_xy), list_means(sims_yx)
    fwd_best, fwd_score, _ = candidate_scores(sims_xy, ids_xy, mean_x, mean_y, margin)
    bwd_best, bwd_score, _ = candidate_scores(sims_yx, ids_yx, mean_y, mean_x, margin)
    return fwd_best, fwd_score, bwd_best, bwd_score


def mine_local(x_unit, y_unit, x_off, y_off, k: int = 16, margin: str = "ratio", retrieval: str = "max", threshold=None,
               stats: dict = None):
    """Local mining: `mine_bitexts` inside every document pair, all pairs at once -> (scores float32 [p], src int64 [p],
    tgt int64 [p], group int64 [p]) on the host, grouped by pair (ascending) and in `mine_bitexts`' output order inside a
    pair; src and tgt are row numbers inside the pair's two documents.  A pair with fewer than k rows on either side is
    left out before the search and yields nothing; stats["small_pairs"] (when a dict is given) counts them.
    The retrieval step runs once over all pairs (`select_pairs` on global row numbers: one stable sort, for `max` one
    greedy pass), then a stable partition by pair: pairs share no rows and a stable sort keeps each pair's internal order,
    so this equals the per-pair passes."""
    _margin_code(margin)
    if retrieval not in RETRIEVALS:
        raise ValueError(f"retrieval {retrieval!r}: one of {', '.join(RETRIEVALS)}")
    x_off, y_off = _group_offsets(x_off, y_off)
    small = small_groups(x_off, y_off, k)
    if stats is not None:
        stats["small_pairs"] = int(small.sum())
    kept = np.nonzero(~small)[0]
    if small.any():
        x_unit, x_off = _pack_groups(x_unit, x_off, kept)
        y_unit, y_off = _pack_groups(y_unit, y_off, kept)
    if kept.size == 0:
        return np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    score, src, tgt = select_pairs(*best_candidates_local(x_unit, y_unit, x_off, y_off, k, margin), retrieval=retrieval, threshold=threshold)
    group = np.searchsorted(x_off, src, side="right") - 1
    order = np.argsort(group, kind="stable")
    score, src, tgt, group = score[order], src[order], tgt[order], group[order]
    return score, src - x_off[group], tgt - y_off[group], kept[group]


def xsim(x, y, k: int = 16, margin: str = "ratio", storage: str = "fp16") -> float:
    """xSIM of parallel rows x [n, d], y [n, d] (row i of y translates row i of x): the share of rows of x whose
    margin-best target is not their own row."""
    _margin_code(margin)
    if x.ndim != 2 or tuple(x.shape) != tuple(y.shape):
        raise ValueError(f"xsim needs two [n, d] arrays of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    d = int(x.shape[1])
    idx_x, idx_y = FlatIndex(d, storage), FlatIndex(d, storage)
    idx_x.add(x)
    idx_y.add(y)
    fwd_best = best_candidates(idx_x, idx_y, k, margin)[0]
    own = idx_x.ctx.torch.arange(fwd_best.shape[0], dtype=fwd_best.dtype, device=fwd_best.device)
    return int((fwd_best != own).sum().item()) / int(fwd_best.shape[0])


def format_pairs(scores: np.ndarray, src: np.ndarray, tgt: np.ndarray) -> str:
    """`score<TAB>src<TAB>tgt` lines; the float32 score is printed as score_align.write_to_output prints one."""
    return "".join(f"{s}\t{i}\t{j}\n" for s, i, j in zip(scores, src, tgt))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--src_index", type=str, required=True, help="Flat index file of the source rows.")
    p.add_argument("--tgt_index", type=str, required=True, help="Flat index file of the target rows.")
    p.add_argument("--out", type=str, required=True, help="output file: score, source row, target row per line.")
    p.add_argument("--k", type=int, default=16, help="number of nearest number.")
    p.add_argument("--margin", type=str, default="ratio", choices=sorted(MARGINS), help="See: https://aclanthology.org/P19-1309")
    p.add_argument("--retrieval", type=str, default="max", choices=RETRIEVALS)
    p.add_argument("--threshold", type=float, default=None, help="keep pairs with a score above it.")
    p.add_argument("--gpu_type", type=str, default="fp16-shard", help="fp16* keeps the database in fp16, bf16* in bf16.")
    a = p.parse_args(argv)
    logger.info(a)
    storage = "bf16" if a.gpu_type.startswith("bf16") else "fp16"
    logger.info(f"Loading {a.src_index} and {a.tgt_index} ({storage})")
    idx_x = FlatIndex.read(a.src_index, storage=storage)
    idx_y = FlatIndex.read(a.tgt_index, storage=storage)
    scores, src, tgt = mine_bitexts(idx_x, idx_y, a.k, a.margin, a.retrieval, a.threshold)
    logger.info(f"Writing {scores.shape[0]} pairs to {a.out}...")
    tmp = a.out + ".tmp"
    with open(tmp, "w") as fp:  # write-then-rename, the repo's crash-safety idiom
        fp.write(format_pairs(scores, src, tgt))
    Path(tmp).replace(a.out)
    logger.info("Done!")


if __name__ == '__main__':
    main()
