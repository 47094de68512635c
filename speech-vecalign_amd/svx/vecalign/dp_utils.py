"""Drop-in for the reference's svecalign/vecalign/dp_utils.py on MI355X.

`vecalign()` keeps the reference signature (dp_utils.py:381-390) and returns a `stack` dict whose
level 0 holds 'final_alignments' and 'alignment_scores' (what every caller of the reference reads,
vecalign.py:276-285).  The whole recursion -- unit-normalisation, pyramid, normalisers, deletion
penalties, coarse dense DP, path up-sampling, band costs, band DP, tracebacks -- runs on the
device as one batched launch sequence (svx_align_batch, include/svx.h); the only host work is
drawing the random row indices, which uses numpy's legacy global stream in the reference's exact
call order so that `np.random.seed(s)` selects the same samples as the reference.

Differences from the reference, by design:
  * vecs0/vecs1 are NOT normalised in place (the reference mutates its inputs, dp_utils.py:396-397);
    pass `normalize_inputs_inplace=True` to get that side effect for float32 numpy inputs.
  * inputs may be float32, float16 or bfloat16 (numpy or torch CUDA tensors); the reference
    only takes float32 arrays that were up-cast from fp16 files.
  * `align_batch()` aligns many document pairs per call (the reference loops in Python,
    seg_align/align.py:206-230).
"""
import ctypes
import logging
from collections import OrderedDict
from math import ceil

import numpy as np

from .. import _lib

logger = logging.getLogger('vecalign')  # same logger name as the reference (dp_utils.py:29)


# ------------------------------------------------------------------------------------- helpers
_pool = None


def _draw_pool():
    """Threads for the GIL-free native host helpers (index drawing, file parsing)."""
    global _pool
    if _pool is None:
        import os
        from multiprocessing.pool import ThreadPool
        _pool = ThreadPool(max(2, min(16, (os.cpu_count() or 4))))
    return _pool


def _ctx():
    return _lib.context()


def _p(x):
    return ctypes.c_void_p(x.data_ptr()) if x is not None else ctypes.c_void_p(0)


def _dev(ctx, a):
    t = ctx.torch
    if hasattr(a, "data_ptr"):
        return a.to(ctx.tdev).contiguous()
    return t.from_numpy(np.ascontiguousarray(a)).to(ctx.tdev)


def _svx_dtype(ctx, x):
    t = ctx.torch
    if x.dtype == t.float32:
        return _lib.SVX_F32
    if x.dtype == t.float16:
        return _lib.SVX_F16
    if x.dtype == t.bfloat16:
        return _lib.SVX_BF16
    raise ValueError("Buffer dtype mismatch, expected 'float' (or float16/bfloat16) but got '%s'" % x.dtype)


def rows_to_alignments(rows):
    """[(x_start, x_len, y_start, y_len)] -> the reference's list of ([x ids], [y ids])."""
    return [(list(range(r[0], r[0] + r[1])), list(range(r[2], r[2] + r[3]))) for r in np.asarray(rows).tolist()]


def alignments_to_rows(alignments):
    rows = np.zeros((max(1, len(alignments)), 4), dtype=np.int32)
    for i, (x, y) in enumerate(alignments):
        rows[i] = (x[0] if len(x) else 0, len(x), y[0] if len(y) else 0, len(y))
    return rows


def prior_rows_from_alignments(alignments):
    """[([x ids], [y ids])] as read_alignments returns them -> int32 [r, 4] rows (x_start, x_len, y_start, y_len) of a
    prior for search="around": the lengths are len() of the two lists, the starts the running sums of the lengths in
    front (what the ids of a complete monotone alignment are; the ids themselves are not read, so a deletion's empty
    list needs no start)."""
    rows = np.zeros((len(alignments), 4), dtype=np.int32)
    xs = ys = 0
    for i, (x, y) in enumerate(alignments):
        rows[i] = (xs, len(x), ys, len(y))
        xs += len(x)
        ys += len(y)
    return rows


def complete_alignments(alignments, n, m):
    """[(x ids, y ids)] in document order, as read_alignments returns them, possibly with gaps -> the complete monotone
    list over n x m segments: every segment no line names becomes a unit deletion ([i], []) / ([], [j]) in front of the
    line that follows it (source side first), and a one-sided line of several segments is split into unit deletions --
    what svx_score_alignments prices (include/svx.h).  Lines with both sides are kept as they are, whatever their size.
    Raises ValueError naming the line (from 1) when a side is not a contiguous ascending run, runs backwards, or leaves
    the document."""
    out, cx, cy = [], 0, 0
    for no, (x, y) in enumerate(alignments, 1):
        x, y = [int(v) for v in x], [int(v) for v in y]
        for name, ids, cur, size in (("source", x, cx, n), ("target", y, cy, m)):
            if any(b != a + 1 for a, b in zip(ids, ids[1:])):
                raise ValueError("line %d: the %s side %s is not a contiguous ascending run" % (no, name, ids))
            if ids and ids[0] < cur:
                raise ValueError("line %d: the %s side %s runs backwards (segment %d is already aligned)" % (no, name, ids, ids[0]))
            if ids and ids[-1] >= size:
                raise ValueError("line %d: the %s side %s leaves the document (%d segments)" % (no, name, ids, size))
        if not x and not y:
            raise ValueError("line %d: both sides are empty" % no)
        out += [([i], []) for i in range(cx, x[0] if x else cx)]
        out += [([], [j]) for j in range(cy, y[0] if y else cy)]
        if x and y:
            out.append((x, y))
        else:
            out += [([i], []) for i in x] + [([], [j]) for j in y]
        cx, cy = (x[-1] + 1 if x else cx), (y[-1] + 1 if y else cy)
    out += [([i], []) for i in range(cx, n)]
    out += [([], [j]) for j in range(cy, m)]
    return out


def given_rows_from_alignments(alignments):
    """[(x ids, y ids)] -> int32 [r, 4] rows (x_start, x_len, y_start, y_len) for svx_score_alignments: the start of a
    non-empty side is its first id, that of an empty side the end of the row before (so a complete path chains)."""
    rows = np.zeros((len(alignments), 4), dtype=np.int32)
    xe = ye = 0
    for i, (x, y) in enumerate(alignments):
        xs, ys = (int(x[0]) if len(x) else xe), (int(y[0]) if len(y) else ye)
        rows[i] = (xs, len(x), ys, len(y))
        xe, ye = xs + len(x), ys + len(y)
    return rows


REPORT_FIELDS = ("rows", "priced", "deletions", "wide", "invalid", "off_type", "outside", "complete")


def search_error(found_total, given_total, given_report):
    """The verdict of search-error analysis for one pair: "unpriced" when the given path has a row
    without a price or is no complete path (wide > 0, invalid > 0 or complete == 0 in its svx_score_alignments report),
    "search" when it is cheaper than the path the DP returned (the search missed it), "model" otherwise (the model
    prefers the returned path: no band width will find the given one).  A plain comparison of two doubles."""
    rep = [int(v) for v in given_report]
    if rep[3] > 0 or rep[4] > 0 or rep[7] != 1:
        return "unpriced"
    return "search" if float(given_total) < float(found_total) else "model"


class GivenScores:
    """What PreparedBatch.score_alignments() left on the device: scores [sum of caps] float64, total [pairs, 2] float64,
    report [pairs, 8] int32 and the row offsets of the pairs in `scores`; skipped[i]: pair i was not scored; cgiven: the
    svx_given array of the call (profiles/given_bench.py repeats the call with it)."""

    def __init__(self, scores, total, report, offs, skipped, keep, cgiven=None):
        self.scores, self.total, self.report, self.offs, self.skipped = scores, total, report, offs, skipped
        self._keep, self.cgiven = keep, cgiven

    def fetch(self):
        """-> per pair None (skipped) or dict(report (8 ints, REPORT_FIELDS), total, del_penalty, scores [rows]); the
        copies are the only synchronisation."""
        total, report, scores = self.total.cpu().numpy(), self.report.cpu().numpy(), self.scores.cpu().numpy()
        out = []
        for i, skip in enumerate(self.skipped):
            if skip:
                out.append(None)
                continue
            o, cnt = int(self.offs[i]), max(0, int(report[i, 0]))
            out.append(dict(report=tuple(int(v) for v in report[i]), total=float(total[i, 0]), del_penalty=float(total[i, 1]),
                            scores=scores[o:o + cnt].copy()))
        return out


def prior_width(rows_or_alignments, n, m):
    """Host twin of svx_prior_width (include/svx.h): the width_over2 from which the band around a prior holds every node
    of every block of that prior -- 1 + max over the ingested rows, the remainder row included, of min(x_len, y_len),
    never less than 3; 0 for a prior the ingest of svx_align_around would fail.
    rows_or_alignments: int [r, 4] rows (x_start, x_len, y_start, y_len), of which the lengths are read, or a list of
    alignments [(x ids, y ids), ...] as read_alignments returns."""
    if isinstance(rows_or_alignments, np.ndarray):
        rows = rows_or_alignments
    elif len(rows_or_alignments) and isinstance(rows_or_alignments[0], tuple) and len(rows_or_alignments[0]) == 2:
        rows = prior_rows_from_alignments(rows_or_alignments)
    else:
        rows = np.asarray(rows_or_alignments)
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    xl, yl = rows[:, 1], rows[:, 3]
    if ((xl < 0) | (yl < 0) | ((xl == 0) & (yl == 0))).any():
        return 0
    sx, sy = int(xl.sum()), int(yl.sum())
    if sx > n or sy > m:
        return 0
    best = int(np.minimum(xl, yl).max()) if len(rows) else 0
    best = max(best, min(n - sx, m - sy))
    return max(3, best + 1)


def level_sizes(n, m, max_size_full_dp):
    """Sizes per depth, dp_utils.py:403-408."""
    L = _lib.load().svx_num_levels(int(n), int(m), int(max_size_full_dp))
    return [(n >> l, m >> l) for l in range(L + 1)]


# ------------------------------------------------------------------------------------- sampling
def draw_indices(n, m, k0, k1, max_size_full_dp, costs_sample_size, num_samps_for_norm, rng=None,
                 have_norms0=False, have_norms1=False):
    """All random row indices of one vecalign() call, drawn in the reference's order from `rng`
    (default: numpy's global legacy stream, like the reference).

    Order (dp_utils.py:423-444 then :450-456): for every depth, compute_norms(v0, v1) draws one
    choice(range(size1), ceil(num/k1)) per overlap layer of side 1, then compute_norms(v1, v0) draws
    per layer of side 0; after all depths, make_del_knob draws x then y per depth, or enumerates
    all pairs when size0*size1 < sample size.  Returns (norm_idx, knob_idx) int32 arrays laid out
    as include/svx.h:svx_pair documents."""
    rng = np.random if rng is None else rng
    sizes = level_sizes(n, m, max_size_full_dp)
    norm_parts, knob_parts = [], []
    for depth, (s0, s1) in enumerate(sizes):
        for size_other, k_other, skip in ((s1, k1, depth == 0 and have_norms0), (s0, k0, depth == 0 and have_norms1)):
            spo = ceil(num_samps_for_norm / k_other)
            if skip or not (size_other and spo):
                continue
            for _ in range(k_other):
                norm_parts.append(rng.choice(size_other, size=spo, replace=True).astype(np.int32))
    for s0, s1 in sizes:
        if s0 * s1 < costs_sample_size:
            knob_parts.append(np.repeat(np.arange(s0, dtype=np.int32), s1))
            knob_parts.append(np.tile(np.arange(s1, dtype=np.int32), s0))
        else:
            knob_parts.append(rng.choice(s0, size=costs_sample_size, replace=True).astype(np.int32))
            knob_parts.append(rng.choice(s1, size=costs_sample_size, replace=True).astype(np.int32))
    norm_idx = np.concatenate(norm_parts) if norm_parts else np.zeros(1, np.int32)
    knob_idx = np.concatenate(knob_parts)
    return norm_idx, knob_idx


def index_counts(n, m, k0, k1, max_size_full_dp, costs_sample_size, num_samps_for_norm, have_norms0=False, have_norms1=False):
    """(len(norm_idx), len(knob_idx)) of draw_indices for a pair of these sizes."""
    lib = _lib.load()
    return (int(lib.svx_norm_index_count(n, m, k0, k1, max_size_full_dp, num_samps_for_norm, int(have_norms0), int(have_norms1))),
            int(lib.svx_knob_index_count(n, m, max_size_full_dp, costs_sample_size)))


def draw_indices_into(norm_out, knob_out, n, m, k0, k1, max_size_full_dp, costs_sample_size, num_samps_for_norm, rng=None,
                      have_norms0=False, have_norms1=False):
    """draw_indices() written straight into int32 buffers (numpy views, e.g. of pinned staging memory), by the
    native MT19937 restatement of RandomState.choice (svx_draw_indices): the same stream, bit for bit, at a
    fraction of the cost, and without the GIL, so a thread pool can draw for many pairs at once.  `rng` is a
    numpy RandomState (advanced like the numpy calls would) or None for numpy's global legacy stream."""
    lib = _lib.load()
    st = np.random.get_state() if rng is None else rng.get_state()
    if st[0] != 'MT19937':
        raise ValueError("draw_indices_into needs a legacy MT19937 RandomState")
    key = np.ascontiguousarray(st[1], dtype=np.uint32).copy()
    pos = ctypes.c_int32(int(st[2]))
    assert norm_out.dtype == np.int32 and knob_out.dtype == np.int32 and norm_out.flags.c_contiguous and knob_out.flags.c_contiguous
    rc = lib.svx_draw_indices(ctypes.c_void_p(key.ctypes.data), ctypes.byref(pos), int(n), int(m), int(k0), int(k1),
                              int(max_size_full_dp), int(costs_sample_size), int(num_samps_for_norm), int(have_norms0),
                              int(have_norms1), ctypes.c_void_p(norm_out.ctypes.data if norm_out.size else 0),
                              ctypes.c_void_p(knob_out.ctypes.data))
    if rc != 0:
        raise ValueError("svx_draw_indices: bad argument")
    new = ('MT19937', key, int(pos.value), st[3], st[4])
    if rng is None:
        np.random.set_state(new)
    else:
        rng.set_state(new)


# ------------------------------------------------------------------------------------- batch
def tile_shape(types):
    """Host twin of the tile sweep's shape choice (csrc/svx_tiles.hip: svxl_band_tiles_shape): 0 = at most 10 types on at
    most 8 overlap layers, 1 = at most 16 types on at most 12 layers (both with sizes up to 8: the LDS-resident shapes, which
    have a backward sweep, svx_row_slack_wide), 2 = the general shape."""
    types = [(int(x), int(y)) for x, y in types]
    layers = len({x for x, _ in types}) + len({y for _, y in types})
    if types and max(max(x, y) for x, y in types) <= 8:
        if len(types) <= 10 and layers <= 8:
            return 0
        if len(types) <= 16 and layers <= 12:
            return 1
    return 2


class PreparedBatch:
    """A batch of document pairs resident on the device, ready for `run()` (svx_align_batch).
    Everything the timed path touches -- embeddings, sampled indices, output buffers, descriptors --
    is built here once."""

    def __init__(self, pairs, final_alignment_types, del_percentile_frac, width_over2, max_size_full_dp,
                 costs_sample_size, num_samps_for_norm, rngs=None, norms=None, device=None, search="coarse_to_fine", frames=None,
                 priors=None):
        """frames: per pair (src, tgt) segment timestamps, [n, 2] and [m, 2] (start, end) sample positions (read_segments);
        kept on the device as int32 for concat_rows().
        search: "coarse_to_fine" (the reference's recursion) or "straight" (band of half-width `width_over2`
        around the straight line from (0,0) to (N,M): Sakoe-Chiba / dense search, include/svx.h SVX_SEARCH_STRAIGHT;
        no pyramid, so `max_size_full_dp` is ignored), or "around": the straight search with the band laid around a prior
        alignment instead of the straight line (svx_align_around; band of at most 64 cells), or "around_wide": the same
        with any band (SVX_SEARCH_AROUND_WIDE: above 64 cells the tile sweep of the wide straight search runs around the
        prior's path; prior_width() gives the width that covers the prior's blocks).
        priors (search="around" and "around_wide" only): per pair one of (rows, info) device tensors (int32 [cap, 4] and [2]); another
        PreparedBatch (its align / info slices: same pair order and sizes, read on the device when run() is called, with
        no host round trip); a host list of alignments [(x_ids, y_ids), ...] as read_alignments returns
        (prior_rows_from_alignments); or None, to be filled by time_prior() before run()."""
        if search not in ("coarse_to_fine", "straight", "around", "around_wide"):
            raise ValueError("search must be 'coarse_to_fine', 'straight', 'around' or 'around_wide'")
        if (priors is not None) != (search in ("around", "around_wide")):
            raise ValueError("priors go with search='around' / 'around_wide', and only with them")
        if search != "coarse_to_fine":
            max_size_full_dp = 1 << 30  # depth 0 only: the random draws of a vecalign() call without pyramid levels
        ctx = _lib.context(device)
        self.ctx = ctx
        t = ctx.torch
        if width_over2 < 3:
            logger.warning('width_over2 was set to %d, which does not make sense. increasing to 3.', width_over2)
            width_over2 = 3
        self.width_over2 = width_over2
        self.types = [tuple(int(v) for v in xy) for xy in final_alignment_types]
        prm = _lib.AlignParams()
        self.vecs = [(_dev(ctx, a), _dev(ctx, b)) for a, b in pairs]
        if not self.vecs:
            raise ValueError("empty batch")
        dts = {_svx_dtype(ctx, v) for ab in self.vecs for v in ab}
        if len(dts) != 1:
            raise ValueError("all embeddings of a batch must share one dtype")
        for a, b in self.vecs:
            if a.dim() != 3 or b.dim() != 3:
                raise ValueError("Buffer has wrong number of dimensions (expected 3, got %d)" % a.dim())
            assert a.shape[2] == b.shape[2]
        self.frames = self.cframes = None
        if frames is not None:
            if len(frames) != len(self.vecs):
                raise ValueError("frames: one (src, tgt) pair of timestamp arrays per document pair")
            self.frames = []
            self.cframes = (_lib.Frames * len(self.vecs))()
            for i, ((a, b), fr) in enumerate(zip(self.vecs, frames)):
                dev = []
                for v, f in zip((a, b), fr):
                    f = t.as_tensor(np.asarray(f).reshape(-1, 2) if not t.is_tensor(f) else f)
                    if tuple(f.shape) != (int(v.shape[1]), 2):
                        raise ValueError("frames of pair %d: shape %s for %d segments" % (i, tuple(f.shape), int(v.shape[1])))
                    dev.append(f.to(device=ctx.tdev, dtype=t.int32).contiguous())
                self.frames.append(tuple(dev))
                self.cframes[i].src, self.cframes[i].tgt = dev[0].data_ptr(), dev[1].data_ptr()
        prm.dtype = dts.pop()
        prm.d = int(self.vecs[0][0].shape[2])
        prm.n_types = len(self.types)
        if prm.n_types > _lib.SVX_MAX_TYPES:
            raise ValueError("too many alignment types")
        for i, (x, y) in enumerate(self.types):
            assert (x > 0)
            assert (y > 0)
            prm.types[2 * i], prm.types[2 * i + 1] = x, y
        prm.width_over2 = int(width_over2)
        prm.max_size_full_dp = int(max_size_full_dp)
        prm.costs_sample_size = int(costs_sample_size)
        prm.num_samps_for_norm = int(num_samps_for_norm)
        prm.del_percentile_frac = float(del_percentile_frac)
        prm.search_mode = {"straight": _lib.SVX_SEARCH_STRAIGHT, "around": _lib.SVX_SEARCH_AROUND,
                           "around_wide": _lib.SVX_SEARCH_AROUND_WIDE}.get(search, _lib.SVX_SEARCH_COARSE_TO_FINE)
        self.prm = prm
        npairs = len(self.vecs)
        self.cpairs = (_lib.Pair * npairs)()
        self.keep = []
        self.levels = []
        # one allocation per output kind, sliced per pair
        caps = [int(a.shape[1] + b.shape[1] + 2) for a, b in self.vecs]
        offs = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
        self.offs = offs
        self.align = t.zeros((int(offs[-1]), 4), dtype=t.int32, device=ctx.tdev)
        self.scores = t.zeros(int(offs[-1]), dtype=t.float64, device=ctx.tdev)
        self.info = t.zeros((npairs, 2), dtype=t.int32, device=ctx.tdev)
        self.del_pen = t.zeros((npairs, _lib.SVX_MAX_LEVELS), dtype=t.float64, device=ctx.tdev)
        # sampled indices: sizes are a function of the shapes, so one pinned staging buffer per kind is laid out
        # first and filled in place (native generator; per-pair streams are independent, so they fill in parallel)
        norm_offs, knob_offs = [0], [0]
        for i, (a, b) in enumerate(self.vecs):
            k0, n = int(a.shape[0]), int(a.shape[1])
            k1, m = int(b.shape[0]), int(b.shape[1])
            nrm = norms[i] if norms is not None else (None, None)
            nn, kn = index_counts(n, m, k0, k1, max_size_full_dp, costs_sample_size, num_samps_for_norm,
                                  nrm[0] is not None, nrm[1] is not None)
            norm_offs.append(norm_offs[-1] + nn)
            knob_offs.append(knob_offs[-1] + kn)
            self.levels.append(len(level_sizes(n, m, max_size_full_dp)))
        h_norm = t.empty(max(1, norm_offs[-1]), dtype=t.int32, pin_memory=True)
        h_knob = t.empty(max(1, knob_offs[-1]), dtype=t.int32, pin_memory=True)
        hn, hk = h_norm.numpy(), h_knob.numpy()

        def draw(i):
            a, b = self.vecs[i]
            nrm = norms[i] if norms is not None else (None, None)
            draw_indices_into(hn[norm_offs[i]:norm_offs[i + 1]], hk[knob_offs[i]:knob_offs[i + 1]], int(a.shape[1]), int(b.shape[1]),
                              int(a.shape[0]), int(b.shape[0]), max_size_full_dp, costs_sample_size, num_samps_for_norm,
                              rngs[i] if rngs is not None else None, nrm[0] is not None, nrm[1] is not None)
        if rngs is not None and npairs >= 8:
            _draw_pool().map(draw, range(npairs))
        else:  # the global stream is consumed pair after pair, like the reference's serial loop
            for i in range(npairs):
                draw(i)
        self.norm_idx = h_norm.to(ctx.tdev, non_blocking=True)
        self.knob_idx = h_knob.to(ctx.tdev, non_blocking=True)
        self.keep.append((h_norm, h_knob))
        for i, (a, b) in enumerate(self.vecs):
            c = self.cpairs[i]
            c.vecs0, c.vecs1 = a.data_ptr(), b.data_ptr()
            c.k0, c.n = int(a.shape[0]), int(a.shape[1])
            c.k1, c.m = int(b.shape[0]), int(b.shape[1])
            c.norm_idx = self.norm_idx.data_ptr() + 4 * norm_offs[i]
            c.knob_idx = self.knob_idx.data_ptr() + 4 * knob_offs[i]
            nrm = norms[i] if norms is not None else (None, None)
            for j, name in enumerate(("norms0", "norms1")):
                if nrm[j] is not None:
                    side = (a, b)[j]
                    if tuple(nrm[j].shape) != tuple(side.shape[:2]):
                        raise Exception('%s wrong shape' % name)  # dp_utils.py:429-432,438-441
                    dn = _dev(ctx, nrm[j]).to(t.float32).contiguous()
                    self.keep.append(dn)
                    setattr(c, name, dn.data_ptr())
            c.align = self.align.data_ptr() + 16 * int(offs[i])
            c.scores = self.scores.data_ptr() + 8 * int(offs[i])
            c.info = self.info.data_ptr() + 8 * i
            c.del_pen = self.del_pen.data_ptr() + 8 * _lib.SVX_MAX_LEVELS * i
        self.cpriors = None
        if search in ("around", "around_wide"):
            self._set_priors(priors)

    def _set_priors(self, priors):
        ctx, t = self.ctx, self.ctx.torch
        npairs = len(self.vecs)
        if isinstance(priors, PreparedBatch):
            priors = [priors] * npairs
        if len(priors) != npairs:
            raise ValueError("priors: one per document pair")
        self.cpriors = (_lib.Prior * npairs)()
        self.prior_own = [None] * npairs   # (rows, info) tensors of this batch's own: what time_prior() fills
        for i, pr in enumerate(priors):
            c = self.cpriors[i]
            if isinstance(pr, PreparedBatch):
                if i >= len(pr.vecs) or int(pr.offs[i + 1] - pr.offs[i]) != int(self.offs[i + 1] - self.offs[i]):
                    raise ValueError("prior batch: pair %d differs in size" % i)
                c.rows = pr.align.data_ptr() + 16 * int(pr.offs[i])
                c.info = pr.info.data_ptr() + 8 * i
                c.cap = int(pr.offs[i + 1] - pr.offs[i])
                self.keep.append(pr)
                continue
            if pr is None:
                cap = int(self.offs[i + 1] - self.offs[i])
                rows = t.zeros((cap, 4), dtype=t.int32, device=ctx.tdev)
                info = t.zeros(2, dtype=t.int32, device=ctx.tdev)   # (no rows: the straight search, until time_prior())
                self.prior_own[i] = (rows, info)
            elif isinstance(pr, tuple) and len(pr) == 2 and t.is_tensor(pr[0]):
                rows, info = pr
                if rows.dtype != t.int32 or info.dtype != t.int32 or not rows.is_cuda or not info.is_cuda:
                    raise ValueError("prior %d: (rows, info) must be int32 device tensors" % i)
                if rows.dim() != 2 or rows.shape[1] != 4 or info.numel() < 2 or not rows.is_contiguous() or not info.is_contiguous():
                    raise ValueError("prior %d: rows [cap, 4] and info [2], contiguous" % i)
            else:
                h = prior_rows_from_alignments(pr)
                rows = t.from_numpy(h if len(h) else np.zeros((1, 4), np.int32)).to(ctx.tdev)
                info = t.tensor([len(h), 0], dtype=t.int32).to(ctx.tdev)
            c.rows, c.info, c.cap = rows.data_ptr(), info.data_ptr(), int(rows.shape[0])
            self.keep.append((rows, info))

    def time_prior(self, window, lag=0):
        """Fill the priors of a search="around" batch from the segments' timestamps (svx_time_prior, include/svx.h): one
        block per window of `window` samples, the target side shifted by `lag` samples.  Needs `frames` and priors given
        as None.  Asynchronous on the current stream; run() then reads the rows on the device."""
        if self.cpriors is None or any(o is None for o in self.prior_own):
            raise ValueError("time_prior() needs search='around' / 'around_wide' with priors=[None, ...]")
        if self.cframes is None:
            raise ValueError("time_prior() needs the batch's frames")
        ctx = self.ctx
        ctx.use_current_stream()
        ctx.check(ctx.lib.svx_time_prior(ctx.h, self.cpairs, self.cframes, len(self.vecs), int(window), int(lag), self.cpriors))

    def prior_width_async(self):
        """svx_prior_width on the batch's priors (include/svx.h): -> int32 device tensor [pairs], the width_over2 that
        covers each pair's prior (0 for a prior the ingest would fail).  Asynchronous on the current stream."""
        if self.cpriors is None:
            raise ValueError("prior_width() needs search='around' or 'around_wide'")
        ctx = self.ctx
        ctx.use_current_stream()
        ctx.flush()   # (a prior may be the output of a batch the pipeline still holds back)
        self.widths = ctx.torch.empty(len(self.vecs), dtype=ctx.torch.int32, device=ctx.tdev)
        ctx.check(ctx.lib.svx_prior_width(ctx.h, self.cpairs, self.cpriors, len(self.vecs), _p(self.widths)))
        return self.widths

    def prior_width(self):
        """prior_width_async() read back: an int32 numpy array [pairs] (one small copy, which synchronises the stream)."""
        return self.prior_width_async().cpu().numpy()

    def run(self):
        """Launch the whole pipeline for the batch (asynchronous on the current torch stream)."""
        ctx = self.ctx
        ctx.use_current_stream()
        self.rows = self.h_rows = None   # (alignment_rows() of an earlier run)
        try:
            priors = getattr(self, "cpriors", None)
            if priors is not None:
                ctx.check(ctx.lib.svx_align_around(ctx.h, ctypes.byref(self.prm), self.cpairs, priors, len(self.vecs)))
            else:
                ctx.check(ctx.lib.svx_align_batch(ctx.h, ctypes.byref(self.prm), self.cpairs, len(self.vecs)))
        finally:   # a call that fails half way may already have queued work that reads this batch
            ctx.hold(self)

    def band_contact(self, level=0, guard=0):
        """svx_band_contact for the last run() on the context (include/svx.h): -> int32 device tensor [pairs, 4] =
        (touching nodes, longest run of them, minimum clearance in cells, nodes) per pair, -1 in all four for a failed
        pair or a level the pair did not refine.  Asynchronous on the current stream."""
        ctx = self.ctx
        ctx.use_current_stream()
        out = ctx.torch.empty((len(self.vecs), 4), dtype=ctx.torch.int32, device=ctx.tdev)
        ctx.check(ctx.lib.svx_band_contact(ctx.h, int(level), int(guard), _p(out)))
        return out

    def score_alignments(self, given):
        """svx_score_alignments for the last run() on the context (include/svx.h): price given alignments with that
        call's normalisers, deletion penalty, band and type set.  given: one entry per pair -- a list of (x ids, y ids)
        (given_rows_from_alignments; complete_alignments() fills a file's gaps first), an int [rows, 4] array of
        (x_start, x_len, y_start, y_len), None to skip the pair, or "own" for the batch's own result, whose total is the
        cost of the path the DP returned.  -> GivenScores (device tensors; .fetch() reads them back).  Asynchronous on the
        current stream: host rows travel through pinned memory, nothing waits for the device."""
        ctx = self.ctx
        t = ctx.torch
        npairs = len(self.vecs)
        if len(given) != npairs:
            raise ValueError("score_alignments: one entry per document pair (%d given, %d pairs)" % (len(given), npairs))
        ctx.use_current_stream()
        host, caps = [], []
        for i, g in enumerate(given):
            if g is None or (isinstance(g, str) and g == "own"):
                host.append(None)
                caps.append(0 if g is None else int(self.offs[i + 1] - self.offs[i]))
                continue
            if isinstance(g, str):
                raise ValueError("score_alignments: pair %d: %r (only the string 'own' is known)" % (i, g))
            rows = np.asarray(g) if isinstance(g, np.ndarray) or t.is_tensor(g) else None
            if rows is None:
                rows = given_rows_from_alignments(g)
            elif rows.ndim != 2 or rows.shape[1] != 4 or rows.dtype.kind not in "iu":
                raise ValueError("score_alignments: pair %d: rows must be an int [rows, 4] array" % i)
            host.append(np.ascontiguousarray(rows, dtype=np.int32))
            caps.append(len(rows))
        offs = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
        scores = t.full((max(1, int(offs[-1])),), float("nan"), dtype=t.float64, device=ctx.tdev)
        total = t.full((npairs, 2), float("nan"), dtype=t.float64, device=ctx.tdev)
        report = t.zeros((npairs, 8), dtype=t.int32, device=ctx.tdev)
        n_host = int(sum(len(h) for h in host if h is not None))
        h_rows = t.zeros((max(1, n_host), 4), dtype=t.int32, pin_memory=True)
        h_info = t.zeros((npairs, 2), dtype=t.int32, pin_memory=True)
        at, starts = 0, []
        for i, h in enumerate(host):
            starts.append(at)
            if h is not None:
                h_rows.numpy()[at:at + len(h)] = h
                h_info.numpy()[i, 0] = len(h)
                at += len(h)
        d_rows = h_rows.to(ctx.tdev, non_blocking=True)
        d_info = h_info.to(ctx.tdev, non_blocking=True)
        cg = (_lib.Given * npairs)()
        for i, g in enumerate(given):
            c = cg[i]
            if g is None:
                continue
            if host[i] is None:   # "own"
                c.rows, c.info = self.align.data_ptr() + 16 * int(self.offs[i]), self.info.data_ptr() + 8 * i
            else:
                c.rows, c.info = d_rows.data_ptr() + 16 * starts[i], d_info.data_ptr() + 8 * i
            c.cap = caps[i]
            c.scores = scores.data_ptr() + 8 * int(offs[i])
            c.total = total.data_ptr() + 16 * i
            c.report = report.data_ptr() + 32 * i
        ctx.check(ctx.lib.svx_score_alignments(ctx.h, cg, npairs))
        return GivenScores(scores, total, report, offs, [g is None for g in given], (h_rows, h_info, d_rows, d_info, self), cg)

    def row_slack(self):
        """svx_row_slack for the last run() on the context (include/svx.h): the slack of every returned row at level 0 --
        the total of the best path of the same band that does NOT contain the row, minus the total of the returned path.
        0: a second optimum exists (the row was picked by the tie rule); small: ambiguous; several deletion penalties:
        solid.  Not clamped: float64 rounding may leave a tiny negative value.  -> (slack, summary): a float64 device
        tensor laid out like self.scores (pair i at self.offs[i]; NaN past a pair's rows), and an int32 device tensor
        [pairs, 4] = (rows, rows with slack == 0, rows with slack == +inf, 0), -1 in all four for a failed pair.
        A run that took the tile sweep (band above 64 cells in the straight and around-wide modes) keeps no cost array and
        raises SvxError.  Asynchronous on the current stream."""
        ctx = self.ctx
        t = ctx.torch
        npairs = len(self.vecs)
        ctx.use_current_stream()
        slack = t.full((max(1, int(self.offs[-1])),), float("nan"), dtype=t.float64, device=ctx.tdev)
        summary = t.zeros((npairs, 4), dtype=t.int32, device=ctx.tdev)
        ptrs = (ctypes.c_void_p * max(1, npairs))()
        for i in range(npairs):
            ptrs[i] = slack.data_ptr() + 8 * int(self.offs[i])
        ctx.check(ctx.lib.svx_row_slack(ctx.h, ptrs, _p(summary), npairs))
        self.slack, self.slack_summary, self._slack_ptrs = slack, summary, ptrs   # alive as long as the batch
        ctx.hold(self)
        return slack, summary

    def took_tile_sweep(self):
        """Does run() take the wide-band tile sweep (a band above 64 cells in the straight and around modes), which keeps no
        cost array?  Then row_slack_wide() measures slack, otherwise row_slack()."""
        return int(self.prm.search_mode) != _lib.SVX_SEARCH_COARSE_TO_FINE and 2 * int(self.prm.width_over2) > 64

    def row_slack_wide(self, return_plane=False):
        """svx_row_slack_wide for the last run() on the context (include/svx.h): row_slack() for a run that took the tile
        sweep -- the same definition, computed by a backward tile sweep that folds the cut minimum while it runs, with the
        sweep's own fp32 costs.  -> (slack, summary) laid out as row_slack()'s.  return_plane: -> (slack, summary, planes),
        planes[i] a float64 device tensor [n + m + 6, 2 * width_over2] holding Bk on the lattice nodes that are band cells of
        diagonals 0 .. path length + 1 (other cells unspecified).  A last call on a band of at most 64 cells, or a type set
        on the general tile shape, raises SvxError; so does a call behind run_widen(), whose last round holds only the pairs
        it searched again.  Asynchronous on the current stream."""
        ctx = self.ctx
        t = ctx.torch
        npairs = len(self.vecs)
        ctx.use_current_stream()
        slack = t.full((max(1, int(self.offs[-1])),), float("nan"), dtype=t.float64, device=ctx.tdev)
        summary = t.zeros((npairs, 4), dtype=t.int32, device=ctx.tdev)
        B = 2 * int(self.prm.width_over2)
        planes = [t.full((int(a.shape[1]) + int(b.shape[1]) + 6, B), float("nan"), dtype=t.float64, device=ctx.tdev)
                  for a, b in self.vecs] if return_plane else None
        sw = (_lib.SlackWide * max(1, npairs))()
        for i in range(npairs):
            sw[i].slack = slack.data_ptr() + 8 * int(self.offs[i])
            sw[i].bsum = planes[i].data_ptr() if return_plane else None
        ctx.check(ctx.lib.svx_row_slack_wide(ctx.h, sw, _p(summary), npairs))
        self.slack, self.slack_summary, self._slack_ptrs = slack, summary, (sw, planes)   # alive as long as the batch
        ctx.hold(self)
        return (slack, summary, planes) if return_plane else (slack, summary)

    def row_alternatives(self, max_detour=16, max_slack=float("inf"), given=None, detour=True, skip=()):
        """svx_row_alternatives for the last run() on the context (include/svx.h): per returned row at level 0 the edge that
        wins the row's cut when the row is forbidden, and -- for rows with slack <= max_slack -- the detour, the at most
        `max_detour` rows of the best path through that edge which replace returned rows lo .. hi-1.
        given: None, or one entry per pair -- None, or int rows [g, 4] = (x_start, x_len, y_start, y_len) -- whose regret is
        wanted: the total of the best path containing the row minus the returned total (NaN: no edge of the band).
        detour=False: edges and slack only.  skip: indices of pairs to leave out (nothing of them is written).  -> dict of device tensors laid out like self.scores (pair i at self.offs[i]):
        slack [rows] float64 (the bits of row_slack()), edge [rows, 4] int32 (x_u, xo, y_u, yo; -1 without one), span
        [rows, 4] int32 (lo, hi, n_detour, status: 0 written, 1 too long, 2 not measured, 3 walk failed), detour [rows,
        max_detour, 4] int32 and detour_scores [rows, max_detour] float64 (-1 / NaN where nothing is written), summary
        [pairs, 4] int32 = (rows, rows with an edge, detours written, detours too long; -1 x 4 for a failed pair); with given
        also regret [given rows] float64 and given_offs (numpy: pair i's given rows start at given_offs[i]).  A run that took
        the tile sweep keeps no cost array and raises SvxError.  Asynchronous on the current stream."""
        ctx = self.ctx
        t = ctx.torch
        npairs = len(self.vecs)
        if given is not None and len(given) != npairs:
            raise ValueError("row_alternatives: one `given` entry per document pair (%d given, %d pairs)" % (len(given), npairs))
        ctx.use_current_stream()
        K = int(max_detour)
        n = max(1, int(self.offs[-1]))
        out = dict(slack=t.full((n,), float("nan"), dtype=t.float64, device=ctx.tdev),
                   edge=t.full((n, 4), -1, dtype=t.int32, device=ctx.tdev),
                   span=t.full((n, 4), -1, dtype=t.int32, device=ctx.tdev),
                   summary=t.zeros((npairs, 4), dtype=t.int32, device=ctx.tdev))
        if detour:
            out['detour'] = t.full((n, max(1, K), 4), -1, dtype=t.int32, device=ctx.tdev)
            out['detour_scores'] = t.full((n, max(1, K)), float("nan"), dtype=t.float64, device=ctx.tdev)
        keep = []
        if given is not None:
            host = [None if g is None else np.ascontiguousarray(np.asarray(g).reshape(-1, 4), dtype=np.int32) for g in given]
            goffs = np.concatenate([[0], np.cumsum([0 if h is None else len(h) for h in host])]).astype(np.int64)
            h_rows = t.zeros((max(1, int(goffs[-1])), 4), dtype=t.int32, pin_memory=True)
            h_info = t.zeros((npairs, 2), dtype=t.int32, pin_memory=True)
            for i, h in enumerate(host):
                if h is not None:
                    h_rows.numpy()[goffs[i]:goffs[i + 1]] = h
                    h_info.numpy()[i, 0] = len(h)
            d_rows, d_info = h_rows.to(ctx.tdev, non_blocking=True), h_info.to(ctx.tdev, non_blocking=True)
            out['regret'] = t.full((max(1, int(goffs[-1])),), float("nan"), dtype=t.float64, device=ctx.tdev)
            out['given_offs'] = goffs
            keep = [h_rows, h_info, d_rows, d_info]
        ca = (_lib.Alt * max(1, npairs))()
        for i in range(npairs):
            if i in skip:
                continue
            o, c = int(self.offs[i]), ca[i]
            c.slack, c.edge, c.span = out['slack'].data_ptr() + 8 * o, out['edge'].data_ptr() + 16 * o, out['span'].data_ptr() + 16 * o
            if detour:
                c.detour = out['detour'].data_ptr() + 16 * K * o
                c.detour_scores = out['detour_scores'].data_ptr() + 8 * K * o
            if given is not None and host[i] is not None:
                c.given, c.given_info = d_rows.data_ptr() + 16 * int(goffs[i]), d_info.data_ptr() + 8 * i
                c.given_cap, c.regret = len(host[i]), out['regret'].data_ptr() + 8 * int(goffs[i])
        ctx.check(ctx.lib.svx_row_alternatives(ctx.h, ca, K, float(max_slack), _p(out['summary']), npairs))
        self.alternatives, self._alt_keep = out, (ca, keep)   # alive as long as the batch
        ctx.hold(self)
        return out

    def run_widen(self, guard=0, max_width_over2=None, max_rounds=4):
        """run() followed by band doubling (svx_align_widen, include/svx.h): pairs whose path touches the band edge are
        searched again around that path in twice the band, up to `max_rounds` times and `max_width_over2` (default:
        width_over2 * 2 ** max_rounds).  Synchronous.  -> int32 numpy array [pairs, 4] = (rounds run, final width_over2,
        touching nodes after round 0, touching nodes after the last round; -1 for a failed pair)."""
        ctx = self.ctx
        ctx.use_current_stream()
        self.rows = self.h_rows = None
        wp = _lib.WidenParams()
        wp.guard, wp.max_rounds = int(guard), int(max_rounds)
        wp.max_width_over2 = min(int(self.width_over2) << min(24, max(0, int(max_rounds))), 1 << 30) if max_width_over2 is None else int(max_width_over2)
        report = np.zeros((len(self.vecs), 4), np.int32)
        try:
            ctx.check(ctx.lib.svx_align_widen(ctx.h, ctypes.byref(self.prm), self.cpairs, getattr(self, "cpriors", None),
                                              len(self.vecs), ctypes.byref(wp), ctypes.c_void_p(report.ctypes.data)))
        finally:   # (as run(): a call that fails half way may have queued work that reads this batch)
            ctx.hold(self)
        return report

    def flush(self):
        """With the context's pipeline on (Context.set_pipeline): launch what run() held back and order it in front of
        whatever follows on the current stream."""
        self.ctx.flush()

    def alignment_rows(self, max_score=float("inf"), unit_storage="fp16"):
        """The margin half's inputs for the alignments of the last run() (svx_alignment_rows, include/svx.h): the candidate
        rows of every alignment that is no deletion and whose score is <= max_score, in (pair, alignment) order.
        -> device tensors (x_rows, y_rows [cap, d] of the input dtype, x_unit, y_unit [cap, d] unit-norm rows in
        `unit_storage` = "fp16" | "bf16" (None: no unit rows, both are None), src [cap, 2] int32 = (pair, alignment row),
        count [1] int64).  cap = sum over pairs of min(n, m) -- a kept alignment consumes a segment on each side, so the
        count never exceeds it; only the first `count` rows are defined.  Asynchronous on the current stream:
        rows_count() reads `count`, and that read is the only synchronisation."""
        if unit_storage not in ("fp16", "bf16", None):
            raise ValueError(f"unit_storage {unit_storage!r}: 'fp16', 'bf16' or None")
        ctx = self.ctx
        t = ctx.torch
        ctx.use_current_stream()
        cap = int(sum(min(int(a.shape[1]), int(b.shape[1])) for a, b in self.vecs))
        d, dt = int(self.prm.d), self.vecs[0][0].dtype
        x_rows = t.empty((cap, d), dtype=dt, device=ctx.tdev)
        y_rows = t.empty((cap, d), dtype=dt, device=ctx.tdev)
        x_unit = y_unit = None
        code = _lib.SVX_F16
        if unit_storage is not None:
            udt, code = (t.float16, _lib.SVX_F16) if unit_storage == "fp16" else (t.bfloat16, _lib.SVX_BF16)
            x_unit = t.empty((cap, d), dtype=udt, device=ctx.tdev)
            y_unit = t.empty((cap, d), dtype=udt, device=ctx.tdev)
        src = t.empty((cap, 2), dtype=t.int32, device=ctx.tdev)
        count = t.empty((1,), dtype=t.int64, device=ctx.tdev)
        ctx.check(ctx.lib.svx_alignment_rows(ctx.h, int(self.prm.dtype), d, self.cpairs, len(self.vecs), float(max_score), cap,
                                             _p(x_rows), _p(y_rows), _p(x_unit), _p(y_unit), code, _p(src), _p(count)))
        self.rows = (x_rows, y_rows, x_unit, y_unit, src, count)
        return self.rows

    def concat_rows(self, params, unit_storage="fp16"):
        """alignment_rows() behind the reference's post-filter chain filter_by_cost -> concat_aligns -> filter_by_dur
        (svx_concat_rows, include/svx.h): the candidate rows of every joined alignment that fits a candidate.
        params: dict(max_score, max_num_align, max_sil, max_dur, both_sides, min_frames, sample_rate) -- missing keys take
        (inf, 1, 1.0, 20.0, False, 0, 16000) -- or a _lib.ConcatParams.  Joining and the duration filter need the batch's
        `frames`.  -> device tensors (x_rows, y_rows, x_unit, y_unit as alignment_rows(), meta [cap, 8] int32 = (pair, first
        row, last row, rows joined, x_start, x_len, y_start, y_len), counts [2] int64 = (fitting rows, wide rows)).
        cap = max_num_align * sum over pairs of min(n, m).  rows_count() and fetch_async() work as after alignment_rows()
        (h_rows = (counts, meta))."""
        if unit_storage not in ("fp16", "bf16", None):
            raise ValueError(f"unit_storage {unit_storage!r}: 'fp16', 'bf16' or None")
        ctx = self.ctx
        t = ctx.torch
        ctx.use_current_stream()
        if isinstance(params, _lib.ConcatParams):
            prm = params
        else:
            unknown = set(params) - {"max_score", "max_num_align", "max_sil", "max_dur", "both_sides", "min_frames", "sample_rate"}
            if unknown:
                raise ValueError("concat_rows: unknown parameters %s" % sorted(unknown))
            prm = _lib.ConcatParams()
            prm.max_score = float(params.get("max_score", float("inf")))
            prm.max_num_align = int(params.get("max_num_align", 1))
            prm.sample_rate = int(params.get("sample_rate", 16000))
            prm.max_sil = float(params.get("max_sil", 1.0))
            prm.max_dur = float(params.get("max_dur", 20.0))
            prm.both_sides = 1 if params.get("both_sides", False) else 0
            prm.min_frames = int(params.get("min_frames", 0))
        cap = max(1, int(prm.max_num_align)) * int(sum(min(int(a.shape[1]), int(b.shape[1])) for a, b in self.vecs))
        d, dt = int(self.prm.d), self.vecs[0][0].dtype
        x_rows = t.empty((cap, d), dtype=dt, device=ctx.tdev)
        y_rows = t.empty((cap, d), dtype=dt, device=ctx.tdev)
        x_unit = y_unit = None
        code = _lib.SVX_F16
        if unit_storage is not None:
            udt, code = (t.float16, _lib.SVX_F16) if unit_storage == "fp16" else (t.bfloat16, _lib.SVX_BF16)
            x_unit = t.empty((cap, d), dtype=udt, device=ctx.tdev)
            y_unit = t.empty((cap, d), dtype=udt, device=ctx.tdev)
        meta = t.empty((cap, 8), dtype=t.int32, device=ctx.tdev)
        counts = t.empty((2,), dtype=t.int64, device=ctx.tdev)
        ctx.check(ctx.lib.svx_concat_rows(ctx.h, int(self.prm.dtype), d, self.cpairs, self.cframes, len(self.vecs), ctypes.byref(prm), cap,
                                          _p(x_rows), _p(y_rows), _p(x_unit), _p(y_unit), code, _p(meta), _p(counts)))
        self.rows = (x_rows, y_rows, x_unit, y_unit, meta, counts)
        return self.rows

    def rows_count(self):
        """Number of rows alignment_rows() / concat_rows() kept.  Uses the copy of fetch_async() when there is one (after its event);
        otherwise this read synchronises the stream."""
        if getattr(self, "h_rows", None) is not None:
            return int(self.h_rows[0][0])
        if getattr(self, "rows", None) is None:
            raise RuntimeError("rows_count() before alignment_rows()")
        return int(self.rows[5][0].item())

    def fetch_async(self):
        """Queue the device -> pinned-host copies of the outputs behind run() on the current stream and return
        an event that fires when they have landed (the host pipeline formats batch i while batch i+1 computes).
        After alignment_rows() its `count` and `src` travel along (h_rows = (count, src)); after concat_rows() its `counts`
        and `meta`."""
        t = self.ctx.torch
        self.ctx.flush()  # (a no-op unless the pipeline is on)
        self.h_out = tuple(t.empty(x.shape, dtype=x.dtype, pin_memory=True) for x in (self.info, self.align, self.scores, self.del_pen))
        for h, d in zip(self.h_out, (self.info, self.align, self.scores, self.del_pen)):
            h.copy_(d, non_blocking=True)
        if getattr(self, "widths", None) is not None:   # (prior_width_async(): the covering widths ride along)
            self.h_widths = t.empty(self.widths.shape, dtype=self.widths.dtype, pin_memory=True)
            self.h_widths.copy_(self.widths, non_blocking=True)
        if getattr(self, "rows", None) is not None:
            self.h_rows = tuple(t.empty(x.shape, dtype=x.dtype, pin_memory=True) for x in (self.rows[5], self.rows[4]))
            for h, d in zip(self.h_rows, (self.rows[5], self.rows[4])):
                h.copy_(d, non_blocking=True)
        ev = t.cuda.Event()
        ev.record(t.cuda.current_stream(self.ctx.tdev))
        return ev

    def raw_results(self):
        """-> (info [P][2], rows [sum][4], scores [sum], del_pen [P][levels], offsets) as numpy arrays, after
        checking every pair's status.  Uses the copies of fetch_async() when there are any."""
        if getattr(self, "h_out", None) is not None:
            info, align, scores, pens = (h.numpy() for h in self.h_out)
        else:
            self.ctx.sync()
            info, align, scores, pens = (x.cpu().numpy() for x in (self.info, self.align, self.scores, self.del_pen))
        bad = np.nonzero((info[:, 1] != 0) | (info[:, 0] < 0))[0]
        if len(bad):
            cnt, err = int(info[bad[0], 0]), int(info[bad[0], 1])
            code = err if err != 0 else -cnt
            raise Exception(_lib.DEVICE_ERRORS.get(code, "device failure %d" % code))
        return info, align, scores, pens, self.offs

    def level_stack(self, i, depth):
        """The reference's stack[depth] entries (dp_utils.py:412-537) of pair `i` of the last run(), copied from
        the device (svx_debug_level): n0, n1, del_penalty, and for refined levels searchpath, a_b_costs [T][A][B],
        b_offset, a_b_csum, a_b_xp, a_b_yp, new_b_offset, alignments, alignment_scores; the coarsest level of a
        pyramid has costs_1to1 and x_y_tb (dp_utils.py:465-473); levels >= 1 have v0_layer0 / v1_layer0 = v0[0] / v1[0]."""
        ctx = self.ctx
        t = ctx.torch
        v = _lib.LevelView()
        ctx.check(ctx.lib.svx_debug_level(ctx.h, int(i), int(depth), ctypes.byref(v)))

        npdt = {t.float32: np.float32, t.float64: np.float64, t.int32: np.int32, t.uint8: np.uint8}

        def arr(ptr, shape, dt):
            if not ptr:
                return None
            out = np.empty(shape, dtype=npdt[dt])
            if out.size:
                ctx.check(ctx.lib.svx_copy_to_host(ctx.h, ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), out.nbytes))
            return out
        d = {'size0': v.size0, 'size1': v.size1,
             'alignment_types': list(self.types) if depth == 0 else [(1, 1)],
             'n0': arr(v.n0, (v.k0, v.size0), t.float32), 'n1': arr(v.n1, (v.k1, v.size1), t.float32),
             'del_penalty': float(arr(v.del_penalty, (1,), t.float64)[0])}
        if v.alignments and v.n_align >= 0:
            d['alignments'] = rows_to_alignments(arr(v.alignments, (v.n_align, 4), t.int32))
        if v.knob_scores and v.n_knob > 0:
            d['knob_scores'] = arr(v.knob_scores, (v.n_knob,), t.float32)
        if v.costs_1to1:  # the coarsest level's dense stage (dp_utils.py:465-473)
            s0, s1 = v.size0, v.size1
            d['costs_1to1'] = arr(v.costs_1to1, (s0, s1), t.float32)
            diag = arr(v.x_y_tb_diag, (s0 + s1 + 1, s0 + 1), t.int32)
            xs, ys = np.meshgrid(np.arange(s0 + 1), np.arange(s1 + 1), indexing='ij')
            d['x_y_tb'] = np.ascontiguousarray(diag[xs + ys, xs])
        if v.v0_l0:
            dim = int(self.prm.d)
            d['v0_layer0'] = arr(v.v0_l0, (v.size0, dim), t.float32)
            d['v1_layer0'] = arr(v.v1_l0, (v.size1, dim), t.float32)
        if v.searchpath:
            A, B, T = v.path_len, v.band, v.n_types
            d['searchpath'] = [tuple(p) for p in arr(v.searchpath, (A, 2), t.int32).tolist()]
            d['b_offset'] = arr(v.b_offset, (A,), t.int32)
            if v.a_b_costs:
                d['a_b_costs'] = np.ascontiguousarray(arr(v.a_b_costs, (A, T, B), t.float32).transpose(1, 0, 2))
            d['a_b_csum'] = arr(v.a_b_csum, (A + 2, B), t.float64)
            if v.a_b_bp:
                bp = arr(v.a_b_bp, (A + 2, B), t.uint8).astype(np.int32)
                d['a_b_xp'] = np.where(bp == 255, -42, bp >> 4).astype(np.int32)
                d['a_b_yp'] = np.where(bp == 255, -42, bp & 15).astype(np.int32)
            else:
                d['a_b_xp'], d['a_b_yp'] = arr(v.a_b_xp, (A + 2, B), t.int32), arr(v.a_b_yp, (A + 2, B), t.int32)
            d['new_b_offset'] = arr(v.new_b_offset, (A + 2,), t.int32)
            if v.alignment_scores and v.n_align >= 0:
                d['alignment_scores'] = arr(v.alignment_scores, (v.n_align,), t.float64)
        return d

    def results(self):
        """-> list of (alignments, scores, del_penalties) per pair; raises on a device-side failure."""
        info, align, scores, pens, offs = self.raw_results()
        out = []
        for i in range(len(self.vecs)):
            cnt, o = int(info[i, 0]), int(offs[i])
            out.append((rows_to_alignments(align[o:o + cnt]), scores[o:o + cnt].copy(), pens[i, :self.levels[i]].copy()))
        return out


def align_batch(pairs, final_alignment_types, del_percentile_frac, width_over2, max_size_full_dp,
                costs_sample_size, num_samps_for_norm, rngs=None, norms=None, device=None, search="coarse_to_fine"):
    """vecalign() for a list of (vecs0, vecs1) pairs in one device pass.
    rngs: optional per-pair numpy RandomState objects (shard-invariant sampling); default = the
    global numpy stream consumed pair after pair, exactly like the reference's serial loop."""
    pb = PreparedBatch(pairs, final_alignment_types, del_percentile_frac, width_over2, max_size_full_dp,
                       costs_sample_size, num_samps_for_norm, rngs=rngs, norms=norms, device=device, search=search)
    pb.run()
    return pb.results()


def vecalign(vecs0, vecs1, final_alignment_types, del_percentile_frac, width_over2, max_size_full_dp,
             costs_sample_size, num_samps_for_norm, norms0=None, norms1=None, normalize_inputs_inplace=False,
             full_stack=False, given=None, search="coarse_to_fine", return_slack=False, return_alternatives=False):
    """dp_utils.py:381-537.  Returns {0: {'final_alignments', 'alignment_scores', 'del_penalty',
    'size0', 'size1', 'alignment_types'}, d: {'del_penalty', 'size0', 'size1'} ...}; with full_stack=True every
    depth also carries the intermediates the reference keeps (n0, n1, searchpath, a_b_costs, b_offset, a_b_csum,
    a_b_xp, a_b_yp, new_b_offset, alignments: PreparedBatch.level_stack), copied back from the device.
    given: alignments [(x ids, y ids)] (or int rows [r, 4]) to price with this call's costs (svx_score_alignments); then
    stack[0]['given'] = dict(verdict, found_total, given_total, del_penalty, report, scores) (search_error()).
    search: "coarse_to_fine" (the reference) or "straight" (PreparedBatch: depth 0 only).
    return_slack: stack[0]['row_slack'] = float64 array, the slack of every final alignment (PreparedBatch.row_slack), and
    stack[0]['slack_summary'] = (rows, rows with slack 0, rows with slack +inf, 0).
    return_alternatives: True, or a dict of PreparedBatch.row_alternatives' keyword arguments (max_detour, max_slack, given:
    int rows [g, 4] whose regret is wanted): stack[0]['alternatives'] = alternatives_to_host() of the call."""
    if search != "coarse_to_fine":
        max_size_full_dp = 1 << 30
    pb = PreparedBatch([(vecs0, vecs1)], final_alignment_types, del_percentile_frac, width_over2, max_size_full_dp,
                       costs_sample_size, num_samps_for_norm, norms=[(norms0, norms1)], search=search)
    timed = logger.isEnabledFor(logging.INFO)
    if timed:
        pb.ctx.check(pb.ctx.lib.svx_set_profiling(pb.ctx.h, 1))
    try:
        pb.run()
        alignments, scores, pens = pb.results()[0]
        if timed:
            log_phase_times(pb.ctx)
    finally:
        if timed:
            pb.ctx.lib.svx_set_profiling(pb.ctx.h, 0)
    sizes = level_sizes(vecs0.shape[1], vecs1.shape[1], max_size_full_dp)
    stack = {}
    for depth, (s0, s1) in enumerate(sizes):
        stack[depth] = {'size0': s0, 'size1': s1, 'del_penalty': float(pens[depth]),
                        'alignment_types': list(final_alignment_types) if depth == 0 else [(1, 1)]}
        if full_stack:
            stack[depth].update(pb.level_stack(0, depth))
    stack[0]['final_alignments'] = alignments
    stack[0]['alignment_scores'] = scores
    if given is not None:
        own, got = pb.score_alignments(["own"]), pb.score_alignments([given])
        own, got = own.fetch()[0], got.fetch()[0]
        stack[0]['given'] = dict(verdict=search_error(own['total'], got['total'], got['report']), found_total=own['total'],
                                 given_total=got['total'], del_penalty=got['del_penalty'], report=got['report'],
                                 scores=got['scores'])
    if return_slack:   # (a run on the tile sweep keeps no cost array: the backward tile sweep measures it)
        sl, summ = pb.row_slack_wide() if pb.took_tile_sweep() else pb.row_slack()
        stack[0]['row_slack'] = sl.cpu().numpy()[:len(alignments)].copy()
        stack[0]['slack_summary'] = tuple(int(v) for v in summ.cpu().numpy()[0])
    if return_alternatives:
        kw = dict(return_alternatives) if isinstance(return_alternatives, dict) else {}
        if kw.get('given') is not None:
            kw['given'] = [kw['given']]
        stack[0]['alternatives'] = alternatives_to_host(pb.row_alternatives(**kw), len(alignments))
    if normalize_inputs_inplace:
        make_norm1(vecs0)
        make_norm1(vecs1)
    return stack


# the reference's phases (dp_utils.py:400,415-419,446,457,462-475,518-528) and the device stages that do their work;
# the fused pyramid pass of level 0 also produces that level's row norms and n0 / n1, so it is the "normalize" phase
PHASES = (('Downsample embeddings', ('pyr1', 'pyrN', 'pyr_aux')),
          ('Normalize embeddings', ('pyr0',)),
          ('Compute deletion penalties', ('knob_sort', 'knob_scores0', 'knob_scoresN', 'knob')),
          ('Full DP make features', ('dense_costs',)),
          ('Full DP', ('dense_dp',)),
          ('Upsample DP compute costs', ('path', 'band_costsN')),
          ('Upsample DP', ('band_dpN', 'traceback')),
          ('Final DP compute costs', ('path0', 'band_costs0', 'tiles')),
          ('Final DP', ('band_dp0', 'traceback0')))


def log_phase_times(ctx):
    """The reference's closing timing log (dp_utils.py:530-535: 'key took ....... 0.1234s' at INFO on logger
    'vecalign', phases above 5e-5 s only), from the device stage timers of the last call (svx_stage_ms; needs
    svx_set_profiling(1) around the call)."""
    runtimes = OrderedDict()
    for key, stages in PHASES:
        runtimes[key] = sum(max(0.0, float(ctx.lib.svx_stage_ms(ctx.h, s.encode()))) for s in stages) * 1e-3
    max_key_str_len = max(len(key) for key in runtimes)
    for key in runtimes:
        if runtimes[key] > 5e-5:
            logger.info(key + ' took ' + '.' * (max_key_str_len + 5 - len(key)) + ('%.4fs' % runtimes[key]).rjust(7))
    return runtimes


# ------------------------------------------------------------------------------------- per-function mirrors
def make_norm1(vecs0):
    """dp_utils.py:32-40, in place on a float32 numpy array [K, n, d] (or torch CUDA tensor)."""
    ctx = _ctx()
    x = _dev(ctx, vecs0)
    if x.dtype != ctx.torch.float32:
        raise ValueError("make_norm1 needs float32")
    ctx.check(ctx.lib.svx_make_norm1(ctx.h, _p(x), int(x.shape[0] * x.shape[1]), int(x.shape[2])))
    if not hasattr(vecs0, "data_ptr"):
        vecs0[...] = x.cpu().numpy()
    elif x.data_ptr() != vecs0.data_ptr():
        vecs0.copy_(x)


def downsample_vectors(vecs1):
    """dp_utils.py:362-378"""
    ctx = _ctx()
    t = ctx.torch
    x = _dev(ctx, vecs1)
    a, b, c = x.shape
    half = t.empty((a, b // 2, c), dtype=t.float32, device=ctx.tdev)
    ctx.check(ctx.lib.svx_downsample(ctx.h, _p(x), int(a), int(b), int(c), _p(half)))
    return half if hasattr(vecs1, "data_ptr") else half.cpu().numpy()


def compute_norms(vecs0, vecs1, num_samples, overlaps_to_use=None):
    """dp_utils.py:326-359 (draws from numpy's global stream like the reference)"""
    overlaps1, size1, dim = vecs1.shape
    overlaps0, size0, dim0 = vecs0.shape
    assert (dim == dim0)
    if overlaps_to_use is not None:
        if overlaps_to_use > overlaps1:
            raise Exception('Cannot use more overlaps than provided. You may want to re-run make_verlaps.py with a larger -n value')
    else:
        overlaps_to_use = overlaps1
    samps_per_overlap = ceil(num_samples / overlaps_to_use)
    if not (size1 and samps_per_overlap):
        return np.ones((overlaps0, size0)).astype(np.float32)
    idx = np.stack([np.random.choice(size1, size=samps_per_overlap, replace=True) for _ in range(overlaps_to_use)]).astype(np.int32)
    ctx = _ctx()
    t = ctx.torch
    norms0 = t.empty((overlaps0, size0), dtype=t.float32, device=ctx.tdev)
    v0, v1, di = _dev(ctx, vecs0), _dev(ctx, vecs1), _dev(ctx, idx)  # keep alive across the call
    ctx.check(ctx.lib.svx_compute_norms(ctx.h, _p(v0), overlaps0, size0, _p(v1), overlaps_to_use,
                                        size1, dim, _p(di), samps_per_overlap, _p(norms0)))
    return norms0.cpu().numpy()


class DeletionKnob(object):
    """dp_utils.py:43-79; the histogram/cdf/interp run on the device (svx_del_penalty)."""

    def __init__(self, samp, res_min, res_max):
        self.samp = np.ascontiguousarray(samp, dtype=np.float32)
        self.res_min, self.res_max = res_min, res_max

    def percentile_frac_to_del_penalty(self, knob_val):
        ctx = _ctx()
        t = ctx.torch
        out = t.zeros(1, dtype=t.float64, device=ctx.tdev)
        s = _dev(ctx, self.samp)
        ctx.check(ctx.lib.svx_del_penalty(ctx.h, _p(s), int(s.numel()), float(knob_val), _p(out)))
        return float(out.cpu().numpy()[0])


def make_del_knob(e_laser, f_laser, e_laser_norms, f_laser_norms, sample_size):
    """dp_utils.py:278-323"""
    from .dp_core import score_path
    e_size, f_size = e_laser.shape[0], f_laser.shape[0]
    if e_size > 0 and f_size > 0 and sample_size > 0:
        if e_size * f_size < sample_size:
            x_idxs = np.repeat(np.arange(e_size, dtype=np.int32), f_size)
            y_idxs = np.tile(np.arange(f_size, dtype=np.int32), e_size)
        else:
            x_idxs = np.random.choice(e_size, size=sample_size, replace=True).astype(np.int32)
            y_idxs = np.random.choice(f_size, size=sample_size, replace=True).astype(np.int32)
        random_scores = np.empty(len(x_idxs), dtype=np.float32)
        score_path(x_idxs, y_idxs, e_laser_norms, f_laser_norms, e_laser, f_laser, random_scores)
        return DeletionKnob(random_scores, 0, max(random_scores))
    return DeletionKnob(np.array([0.0, 0.5, 1.0]), 0, 1)


def dense_traceback(x_y_tb):
    """dp_utils.py:146-174"""
    ctx = _ctx()
    t = ctx.torch
    bp = _dev(ctx, np.ascontiguousarray(x_y_tb, dtype=np.int32))
    s0, s1 = bp.shape[0] - 1, bp.shape[1] - 1
    rows = t.zeros((max(1, s0 + s1), 4), dtype=t.int32, device=ctx.tdev)
    cnt = t.zeros(1, dtype=t.int32, device=ctx.tdev)
    ctx.check(ctx.lib.svx_dense_traceback(ctx.h, _p(bp), s0, s1, _p(rows), _p(cnt)))
    n = int(cnt.cpu().numpy()[0])
    if n < 0:
        raise Exception('got unknown value')
    return rows_to_alignments(rows.cpu().numpy()[:n])


def sparse_traceback(a_b_csum, a_b_xp, a_b_yp, b_offset, xsize, ysize):
    """dp_utils.py:105-143"""
    ctx = _ctx()
    t = ctx.torch
    csum = _dev(ctx, np.ascontiguousarray(a_b_csum, dtype=np.float64))
    cap = xsize + ysize + 2
    rows = t.zeros((cap, 4), dtype=t.int32, device=ctx.tdev)
    scores = t.zeros(cap, dtype=t.float64, device=ctx.tdev)
    cnt = t.zeros(1, dtype=t.int32, device=ctx.tdev)
    xp = _dev(ctx, np.ascontiguousarray(a_b_xp, dtype=np.int32))
    yp = _dev(ctx, np.ascontiguousarray(a_b_yp, dtype=np.int32))
    bo = _dev(ctx, np.ascontiguousarray(b_offset, dtype=np.int32))
    ctx.check(ctx.lib.svx_sparse_traceback(ctx.h, _p(csum), _p(xp), _p(yp), _p(bo),
                                           int(csum.shape[0]), int(csum.shape[1]), int(xsize), int(ysize),
                                           _p(rows), _p(scores), _p(cnt)))
    n = int(cnt.cpu().numpy()[0])
    if n < 0:
        raise Exception('traceback bug')
    return rows_to_alignments(rows.cpu().numpy()[:n]), scores.cpu().numpy()[:n].copy()


def sparse_dp_backward(a_b_costs, b_offset_in, alignment_types, del_penalty, x_in_size, y_in_size):
    """svx_sparse_dp_backward (include/svx.h): the backward band DP over the edges sparse_dp relaxes -> Bk [A+2][B]
    float64, the cheapest way from every band cell to the end node (+inf where there is none)."""
    from .dp_core import _typed, _types
    ctx = _ctx()
    t = ctx.torch
    a_b_costs = _typed(a_b_costs, np.float32, 3, "a_b_costs")
    b_offset_in = _typed(b_offset_in, np.int32, 1, "b_offset_in")
    types, T = _types(alignment_types)
    Tc, A, B = a_b_costs.shape
    assert Tc == T
    bsum = t.empty((A + 2, B), dtype=t.float64, device=ctx.tdev)
    c = _dev(ctx, a_b_costs) if a_b_costs.size else t.empty(1, dtype=t.float32, device=ctx.tdev)
    bin_ = _dev(ctx, b_offset_in)
    ctx.check(ctx.lib.svx_sparse_dp_backward(ctx.h, _p(c), _p(bin_), A, B, types, T, float(del_penalty), int(x_in_size),
                                             int(y_in_size), _p(bsum)))
    return bsum.cpu().numpy()


def path_slack(a_b_costs, b_offset_in, alignment_types, del_penalty, x_in_size, y_in_size, a_b_csum, a_b_bsum, rows):
    """svx_path_slack (include/svx.h): the slack of int rows [n, 4] = (x_start, x_len, y_start, y_len) on the planes
    a_b_csum (sparse_dp) and a_b_bsum (sparse_dp_backward) -> float64 [n]; NaN for a row that is no edge of the band."""
    from .dp_core import _typed, _types
    ctx = _ctx()
    t = ctx.torch
    a_b_costs = _typed(a_b_costs, np.float32, 3, "a_b_costs")
    b_offset_in = _typed(b_offset_in, np.int32, 1, "b_offset_in")
    types, T = _types(alignment_types)
    Tc, A, B = a_b_costs.shape
    assert Tc == T
    rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 4)
    n = len(rows)
    csum = _dev(ctx, np.ascontiguousarray(a_b_csum, dtype=np.float64))
    bsum = _dev(ctx, np.ascontiguousarray(a_b_bsum, dtype=np.float64))
    assert tuple(csum.shape) == (A + 2, B) and tuple(bsum.shape) == (A + 2, B)
    c = _dev(ctx, a_b_costs) if a_b_costs.size else t.empty(1, dtype=t.float32, device=ctx.tdev)
    bin_ = _dev(ctx, b_offset_in)
    drows = _dev(ctx, rows if n else np.zeros((1, 4), np.int32))
    cnt = t.tensor([n], dtype=t.int32).to(ctx.tdev)
    out = t.full((max(1, n),), float("nan"), dtype=t.float64, device=ctx.tdev)
    ctx.check(ctx.lib.svx_path_slack(ctx.h, _p(c), _p(bin_), A, B, types, T, float(del_penalty), int(x_in_size), int(y_in_size),
                                     _p(csum), _p(bsum), _p(drows), _p(cnt), n, _p(out)))
    return out.cpu().numpy()[:n].copy()


def alternatives_to_host(alt, n_rows, offset=0, pair=0):
    """One pair's share of PreparedBatch.row_alternatives' device tensors as numpy: slack, edge, span, summary, detours (per
    row None, or (rows [k, 4], scores [k]) of a written detour) and, when asked for, regret."""
    o = int(offset)
    span = alt['span'][o:o + n_rows].cpu().numpy()
    out = dict(slack=alt['slack'][o:o + n_rows].cpu().numpy(), edge=alt['edge'][o:o + n_rows].cpu().numpy(), span=span,
               summary=tuple(int(v) for v in alt['summary'][pair].cpu().numpy()))
    if 'detour' in alt:
        det, sc = alt['detour'][o:o + n_rows].cpu().numpy(), alt['detour_scores'][o:o + n_rows].cpu().numpy()
        out['detours'] = [(det[r, :span[r, 2]].copy(), sc[r, :span[r, 2]].copy()) if span[r, 3] == 0 else None for r in range(n_rows)]
    if 'regret' in alt:
        g = alt['given_offs']
        out['regret'] = alt['regret'][int(g[pair]):int(g[pair + 1])].cpu().numpy()
    return out


def path_alternatives(a_b_costs, b_offset_in, alignment_types, del_penalty, x_in_size, y_in_size, a_b_csum, a_b_bsum, a_b_xp, a_b_yp,
                      rows, max_detour=16, max_slack=float("inf"), given=None, detour=True):
    """svx_path_alternatives (include/svx.h): the alternatives of int rows [n, 4] that form a path, on the planes a_b_csum,
    a_b_xp, a_b_yp (sparse_dp) and a_b_bsum (sparse_dp_backward) -> dict of numpy arrays: slack [n], edge [n, 4], span [n,
    4], detour [n, max_detour, 4] and detour_scores [n, max_detour] (-1 / NaN where nothing is written; absent with
    detour=False), regret [len(given)] when given (int rows [g, 4]) is not None."""
    from .dp_core import _typed, _types
    ctx = _ctx()
    t = ctx.torch
    a_b_costs = _typed(a_b_costs, np.float32, 3, "a_b_costs")
    b_offset_in = _typed(b_offset_in, np.int32, 1, "b_offset_in")
    types, T = _types(alignment_types)
    Tc, A, B = a_b_costs.shape
    assert Tc == T
    rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 4)
    n, K = len(rows), int(max_detour)
    planes = [_dev(ctx, np.ascontiguousarray(x, dtype=dt)) for x, dt in ((a_b_csum, np.float64), (a_b_bsum, np.float64),
                                                                          (a_b_xp, np.int32), (a_b_yp, np.int32))]
    assert all(tuple(x.shape) == (A + 2, B) for x in planes)
    c = _dev(ctx, a_b_costs) if a_b_costs.size else t.empty(1, dtype=t.float32, device=ctx.tdev)
    bin_ = _dev(ctx, b_offset_in)
    drows = _dev(ctx, rows if n else np.zeros((1, 4), np.int32))
    cnt = t.tensor([n], dtype=t.int32).to(ctx.tdev)
    m = max(1, n)
    out = dict(slack=t.full((m,), float("nan"), dtype=t.float64, device=ctx.tdev),
               edge=t.full((m, 4), -1, dtype=t.int32, device=ctx.tdev), span=t.full((m, 4), -1, dtype=t.int32, device=ctx.tdev))
    one = _lib.Alt()
    one.slack, one.edge, one.span = out['slack'].data_ptr(), out['edge'].data_ptr(), out['span'].data_ptr()
    if detour:
        out['detour'] = t.full((m, max(1, K), 4), -1, dtype=t.int32, device=ctx.tdev)
        out['detour_scores'] = t.full((m, max(1, K)), float("nan"), dtype=t.float64, device=ctx.tdev)
        one.detour, one.detour_scores = out['detour'].data_ptr(), out['detour_scores'].data_ptr()
    if given is not None:
        g = np.ascontiguousarray(given, dtype=np.int32).reshape(-1, 4)
        dg = _dev(ctx, g if len(g) else np.zeros((1, 4), np.int32))
        dinfo = _dev(ctx, np.asarray([len(g), 0], np.int32))
        out['regret'] = t.full((max(1, len(g)),), float("nan"), dtype=t.float64, device=ctx.tdev)
        one.given, one.given_info, one.given_cap, one.regret = dg.data_ptr(), dinfo.data_ptr(), len(g), out['regret'].data_ptr()
    ctx.check(ctx.lib.svx_path_alternatives(ctx.h, _p(c), _p(bin_), A, B, types, T, float(del_penalty), int(x_in_size), int(y_in_size),
                                            _p(planes[0]), _p(planes[1]), _p(planes[2]), _p(planes[3]), _p(drows), _p(cnt), n,
                                            ctypes.byref(one), K, float(max_slack)))
    res = {k: v.cpu().numpy()[:n].copy() for k, v in out.items() if k != 'regret'}
    if given is not None:
        res['regret'] = out['regret'].cpu().numpy()[:len(g)].copy()
    return res


def make_search_path(alignments, size0=0, size1=0, upsample=False):
    """upsample_alignment + extend_alignments + alignment_to_search_path (dp_utils.py:261-275,
    228-258, 199-225) in one device call; with upsample=False it is alignment_to_search_path."""
    ctx = _ctx()
    t = ctx.torch
    rows = alignments_to_rows(alignments)
    if not upsample:
        size0 = max(size0, int(sum(r[1] for r in rows)))
        size1 = max(size1, int(sum(r[3] for r in rows)))
    path = t.zeros((size0 + size1 + 4, 2), dtype=t.int32, device=ctx.tdev)
    plen = t.zeros(1, dtype=t.int32, device=ctx.tdev)
    na = _dev(ctx, np.array([len(alignments)], dtype=np.int32))
    drows = _dev(ctx, rows)
    ctx.check(ctx.lib.svx_search_path(ctx.h, _p(drows), _p(na), 1 if upsample else 0, int(size0), int(size1),
                                      _p(path), _p(plen)))
    n = int(plen.cpu().numpy()[0])
    if n == -_lib.SVX_ERR_EXTEND:
        raise Exception('asked to extend alignments but already bigger than requested')
    if n < 0:
        raise Exception('search path failure %d' % -n)
    return [tuple(p) for p in path.cpu().numpy()[:n].tolist()]


def alignment_to_search_path(algn):
    """dp_utils.py:199-225"""
    return make_search_path(algn, upsample=False)


# ------------------------------------------------------------------------------------- Sakoe-Chiba mode
def align_band(vecs0, vecs1, final_alignment_types, del_percentile_frac, width_over2, costs_sample_size,
               num_samps_for_norm, rng=None):
    """Banded alignment around the straight diagonal (Sakoe-Chiba, BASELINE.json configs[3]; with
    width_over2 > max(N, M) the dense mode): the same recurrence as the refinement step of vecalign() --
    make_sparse_costs + sparse_dp + sparse_traceback (dp_core.pyx:165-404, dp_utils.py:105-143) with the final
    alignment types -- but the search path is the straight line from (0,0) to (N,M) (append_slant,
    dp_utils.py:177-196) with band half-width `width_over2` instead of an up-sampled coarse alignment.  Norms and
    the deletion penalty are those of depth 0 of vecalign() (same random draws, same order).  One svx_align_batch
    call (SVX_SEARCH_STRAIGHT): bands wider than 64 cells run as a wavefront of MFMA cost tiles + DP over all
    CUs.  Inputs of any storage type ([K, N, d] float32 / float16 / bfloat16).  Returns (alignments, scores)."""
    res = align_band_batch([(vecs0, vecs1)], final_alignment_types, del_percentile_frac, width_over2, costs_sample_size,
                           num_samps_for_norm, rngs=None if rng is None else [rng])
    return res[0][0], res[0][1]


def align_band_batch(pairs, final_alignment_types, del_percentile_frac, width_over2, costs_sample_size, num_samps_for_norm,
                     rngs=None, device=None):
    """align_band() for a list of pairs in one device pass -> [(alignments, scores, [del_penalty])]."""
    return align_batch(pairs, final_alignment_types, del_percentile_frac, width_over2, 1 << 30, costs_sample_size,
                       num_samps_for_norm, rngs=rngs, device=device, search="straight")
