"""svx_score_alignments on the GPU (include/svx.h) against tests/given_ref.py: given alignments priced with the costs of
the last svx_align_batch / svx_align_around call.  Reports are integers and must be equal; priced costs are held to the rule
of tests/stage_check.py against the float64 flavour of the reference on the GPU's own level view; totals to the float64
sum of the GPU's own costs; the found path to the DP's own cumulative cost."""
import ctypes

import numpy as np
import pytest

import given_ref
from around_ref import SVX_ERR_ARG, block_deletion_pair, block_prior
from contact_ref import end_csum, widen_chain
from fuzz_gpu_vs_oracle import store_round, to_devs
from synth import alignment_types, make_pair

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-4
U = 2.0 ** -24
TYPES5 = alignment_types(5)
NONE8 = (-1,) * 8


def batch(docs, W, seeds, search="straight", priors=None, max_full=300, store="f32"):
    from svx.vecalign import dp_utils
    kw = dict(priors=priors) if search in ("around", "around_wide") else {}
    return dp_utils.PreparedBatch(to_devs(docs, store), TYPES5, 0.2, W, max_full, 20000, 100,
                                  rngs=[np.random.RandomState(s) for s in seeds], search=search, **kw)


def costs_of(got, rows):
    """The fp32 costs behind the scores of the priced rows (score = max(c, 0) / (p q), so a clipped cost reads 0)."""
    pq = (rows[:, 1] * rows[:, 3]).astype(np.float64)
    return (got['scores'] * pq).astype(np.float32).astype(np.float64)


def check_against_ref(got, st, v0, v1, given, label=""):
    """Report exact; every priced cost by the stage rule; the total against the float64 sum of the GPU's own costs."""
    f64 = given_ref.score(st, v0, v1, given, "f64")
    f32 = given_ref.score(st, v0, v1, given, "f32")
    rows = f64['rows']
    assert got['report'] == f64['report'], (label, got['report'], f64['report'])
    assert got['del_penalty'] == st['del_penalty']
    pr = f64['cls'] == given_ref.PRICED
    assert np.array_equal(np.isnan(got['scores']), np.isnan(f64['scores'])), label
    assert (got['scores'][f64['cls'] == given_ref.DELETION] == 0.0).all()
    c_gpu = costs_of(got, rows)[pr]
    t = np.maximum(f64['costs'][pr], 0.0)
    if pr.any():
        e_gpu = float(np.abs(c_gpu - t).max())
        e_orc = float(np.abs(np.maximum(f32['costs'][pr], 0.0) - t).max())
        bound = max(2 * e_orc, 4 * U * float(np.abs(t).max()))
        print("%s: E_gpu %.3e  E_orc %.3e  bound %.3e over %d costs" % (label, e_gpu, e_orc, bound, int(pr.sum())))
        assert e_gpu <= bound, (label, e_gpu, e_orc, bound)
    want = 0.0
    for c in c_gpu.tolist():
        want += c
    want += got['del_penalty'] * got['report'][2]
    assert abs(got['total'] - want) <= max(1, len(rows)) * 2.0 ** -52 * abs(want), (label, got['total'], want)
    return f64


def every_layer_pair(n, m):
    """A complete path over n x m whose first 16 rows use every (p, q) <= (4, 4), then 1-1 rows, then deletions."""
    al, x, y = [], 0, 0
    for p in range(1, 5):
        for q in range(1, 5):
            al.append((list(range(x, x + p)), list(range(y, y + q))))
            x, y = x + p, y + q
    while x < n and y < m:
        al.append(([x], [y]))
        x, y = x + 1, y + 1
    return al + [([i], []) for i in range(x, n)] + [([], [j]) for j in range(y, m)]


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("d", [8, 40, 1024, 2048])
@pytest.mark.parametrize("store", ["f32", "f16", "bf16"])
def test_parity_matrix(store, d):
    seed = 100 + d % 97
    v0, v1 = make_pair(60, 50, 4, d, seed, zero_rows=3, deletions=2)
    v0, v1 = store_round(v0, store), store_round(v1, store)
    pb = batch([(v0, v1)], 7, [seed], store=store)
    pb.run()
    own = pb.score_alignments(["own"])
    hand = every_layer_pair(60, 50)
    given = pb.score_alignments([hand])
    own, given = own.fetch()[0], given.fetch()[0]
    st = pb.level_stack(0, 0)
    ref = check_against_ref(own, st, v0, v1, st['alignments'], "own %s d=%d" % (store, d))
    assert ref['report'][3:6] == (0, 0, 0) and ref['report'][6:] == (0, 1)
    ref = check_against_ref(given, st, v0, v1, hand, "hand %s d=%d" % (store, d))
    assert ref['report'][:6] == (len(hand), 26, len(hand) - 26, 0, 0, 6) and ref['report'][7] == 1


# ---------------------------------------------------------------------------------------------- 2
def own_path_checks(pb, i=0):
    got = pb.score_alignments(["own" if j == i else None for j in range(len(pb.vecs))]).fetch()[i]
    st = pb.level_stack(i, 0)
    pb.ctx.sync()
    cnt = int(pb.info.cpu().numpy()[i, 0])
    o = int(pb.offs[i])
    rows = pb.align.cpu().numpy()[o:o + cnt].astype(np.int64)
    dels = int(((rows[:, 1] == 0) | (rows[:, 3] == 0)).sum())
    assert cnt > 0 and got['report'] == (cnt, cnt - dels, dels, 0, 0, 0, 0, 1)
    assert np.abs(got['scores'] - pb.scores.cpu().numpy()[o:o + cnt]).max() <= SCORE_TOL
    c = costs_of(got, rows)
    total = end_csum(st)
    tol = 2 * (4 * U * float(np.abs(c).sum()) + cnt * 2.0 ** -52 * abs(total))   # both prices of the path: the DP's and this call's
    print("own path: total %.9f, end csum %.9f, tol %.3e" % (got['total'], total, tol))
    assert abs(got['total'] - total) <= tol, (got['total'], total, tol)
    return got, st


def test_own_path_coarse_to_fine_three_levels():
    v0, v1 = make_pair(300, 280, 4, 32, 0, deletions=10)
    pb = batch([(v0, v1)], 7, [11], search="coarse_to_fine", max_full=60)
    pb.run()
    assert pb.levels[0] >= 3             # 300 x 280 -> 150 x 140 -> 75 x 70 refined, the dense stage above them
    own_path_checks(pb)


def test_own_path_straight_band_14():
    v0, v1 = make_pair(200, 190, 4, 32, 5, deletions=3)
    pb = batch([(v0, v1)], 7, [11])
    pb.run()
    got, st = own_path_checks(pb)
    assert st['a_b_csum'].shape[1] == 14


def test_own_path_tile_sweep():
    """W = 20 touches on the block-deletion pair; the round at 80 cells is the tile sweep, which keeps no cost array."""
    v0, v1, _ = block_deletion_pair(seed=0)
    pb = batch([(v0, v1)], 20, [11])
    assert pb.run_widen().tolist() == [[1, 40, 10, 0]]
    got, st = own_path_checks(pb)
    assert 'a_b_costs' not in st and st['a_b_csum'].shape[1] == 80


@pytest.mark.parametrize("search, W", [("around", 7), ("around_wide", 40)])
def test_own_path_around_a_prior(search, W):
    v0, v1, src = block_deletion_pair(seed=0)
    prior = block_prior(src, 300) if search == "around" else [(list(range(300)), list(range(180)))]
    pb = batch([(v0, v1)], W, [11], search=search, priors=[prior])
    pb.run()
    got, st = own_path_checks(pb)
    assert st['a_b_csum'].shape[1] == 2 * W


# ---------------------------------------------------------------------------------------------- 3
def test_block_deletion_pair_search_error_then_model_error(orc):
    from svx.vecalign.dp_utils import search_error
    v0, v1, src = block_deletion_pair(seed=0)
    truth = given_ref.truth_path(src, 300)
    stacks, _ = widen_chain(orc, v0, v1, TYPES5, 7, 11)
    want_truth = given_ref.score(stacks[0], v0, v1, truth)['total']
    pb = batch([(v0, v1)], 7, [11])
    pb.run()
    found, got = pb.score_alignments(["own"]), pb.score_alignments([truth])
    found, got = found.fetch()[0], got.fetch()[0]
    assert got['report'] == (300, 180, 120, 0, 0, 0, 206, 1)
    assert search_error(found['total'], got['total'], got['report']) == "search"
    assert abs(found['total'] - end_csum(stacks[0])) <= SCORE_TOL * found['report'][0]
    assert abs(got['total'] - want_truth) <= SCORE_TOL * 300
    assert pb.run_widen().tolist() == [[2, 28, 20, 0]]        # the last call is the round at 56 cells, of this one pair
    found, got = pb.score_alignments(["own"]), pb.score_alignments([truth])
    found, got = found.fetch()[0], got.fetch()[0]
    assert got['report'] == (300, 180, 120, 0, 0, 0, 0, 1)
    assert search_error(found['total'], got['total'], got['report']) == "model"
    assert abs(found['total'] - end_csum(stacks[2])) <= SCORE_TOL * found['report'][0]
    assert abs(got['total'] - want_truth) <= SCORE_TOL * 300
    assert round(found['total'], 2) == 118.58 and round(got['total'], 2) == 120.57


# ---------------------------------------------------------------------------------------------- 4
def test_no_neighbour_of_the_found_path_is_cheaper():
    """64 one-edit neighbours of the found path, inside the band, as a 64-pair batch of the same document."""
    v0, v1 = make_pair(200, 190, 4, 32, 5, deletions=3)
    pb = batch([(v0, v1)] * 64, 7, [11] * 64)
    pb.run()
    st = pb.level_stack(0, 0)
    own_ref = given_ref.score(st, v0, v1, st['alignments'])
    rng = np.random.RandomState(2019)
    paths = []
    while len(paths) < 64:
        for al in given_ref.edits(st['alignments'], TYPES5, 64, rng):
            s = given_ref.score(st, v0, v1, al)
            if s['report'][6] == 0 and len(paths) < 64:
                paths.append((al, s))
    found, got = pb.score_alignments(["own"] * 64), pb.score_alignments([al for al, _ in paths])
    found, got = found.fetch(), got.fetch()
    assert len({f['total'] for f in found}) == 1 and found[0]['report'] == own_ref['report']
    low = []
    for (al, s), g in zip(paths, got):
        assert g['report'] == s['report']
        low.append(g['total'] - found[0]['total'])
        assert g['total'] >= found[0]['total'] - given_ref.tolerance(s, own_ref), (g['report'], g['total'], found[0]['total'])
    print("smallest total(neighbour) - total(found): %.3e" % min(low))
    assert max(low) > 0.1


# ---------------------------------------------------------------------------------------------- 5
def long_path(al):
    """The found path with most two-sided rows split into unit deletions: more than 512 rows, rows 256 and 511 deletions."""
    out = []
    for i, (x, y) in enumerate(al):
        if x and y and i % 8 != 0:
            out += [([u], []) for u in x] + [([], [v]) for v in y]
        else:
            out.append((x, y))
    for r in (256, 511):
        x, y = out[r]
        if x and y:
            out[r:r + 1] = [([u], []) for u in x] + [([], [v]) for v in y]
    return out


def test_chunk_edges():
    from svx.vecalign.dp_utils import given_rows_from_alignments
    v0, v1 = make_pair(300, 280, 4, 32, 0, deletions=40)
    pb = batch([(v0, v1)] * 4, 7, [11] * 4)
    pb.run()
    st = pb.level_stack(0, 0)
    rows = given_rows_from_alignments(long_path(st['alignments']))
    assert len(rows) > 512 and all((rows[r, 1] + rows[r, 3]) == 1 for r in (256, 511))
    given = [rows]
    for r in (256, 511):                     # the empty side of a deletion starts one segment late: its price does not change
        b = rows.copy()
        b[r, 2 if b[r, 3] == 0 else 0] += 1
        given.append(b)
    given.append(rows[:-1].copy())           # the last row is missing: the path stops short of (n, m)
    got = pb.score_alignments(given).fetch()
    refs = [check_against_ref(g, st, v0, v1, r.astype(np.int64), "chunk edges %d" % i) for i, (g, r) in enumerate(zip(got, given))]
    assert got[0]['report'][7] == 1 and got[0]['report'][3:5] == (0, 0)
    for g in got[1:3]:
        assert g['report'][:6] == got[0]['report'][:6] and g['report'][7] == 0
        assert g['total'] == got[0]['total'] and g['scores'].tobytes() == got[0]['scores'].tobytes()
    assert got[3]['report'][0] == len(rows) - 1 and got[3]['report'][7] == 0
    assert got[3]['scores'].tobytes() == got[0]['scores'][:-1].tobytes()


# ---------------------------------------------------------------------------------------------- raw calls
def raw_call(pb, entries, n_pairs=None):
    """svx_score_alignments on caller-made buffers.  entries: per pair None or dict(rows tensor, info tensor, cap, scores,
    total, report) -> the return code."""
    from svx import _lib
    cg = (_lib.Given * len(entries))()
    for c, e in zip(cg, entries):
        if e is None:
            continue
        for k in ("rows", "info", "scores", "total", "report"):
            v = e.get(k)
            setattr(c, k, (v if isinstance(v, int) else v.data_ptr()) if v is not None else None)
        c.cap = e["cap"]
    pb.ctx.use_current_stream()
    return pb.ctx.lib.svx_score_alignments(pb.ctx.h, cg, len(entries) if n_pairs is None else n_pairs)


def buffers(rows, count, cap, code=0):
    """Device buffers of one given path, pre-filled: rows past the host rows hold INT32_MAX, scores -7, total -7, report -7."""
    import torch
    r = torch.full((cap, 4), given_ref.INT32_MAX, dtype=torch.int32)
    r[:len(rows)] = torch.from_numpy(np.ascontiguousarray(rows, np.int32))
    return dict(rows=r.cuda(), info=torch.tensor([count, code], dtype=torch.int32).cuda(), cap=cap,
                scores=torch.full((cap,), -7.0, dtype=torch.float64).cuda(), total=torch.full((2,), -7.0, dtype=torch.float64).cuda(),
                report=torch.full((8,), -7, dtype=torch.int32).cuda())


def read(e):
    return e["scores"].cpu().numpy(), e["total"].cpu().numpy(), tuple(e["report"].cpu().numpy().tolist())


# ---------------------------------------------------------------------------------------------- 6
def test_poisoned_rows_are_never_read():
    from svx.vecalign.dp_utils import given_rows_from_alignments
    v0, v1 = make_pair(200, 190, 4, 32, 5, deletions=3)
    pb = batch([(v0, v1)], 7, [11])
    pb.run()
    st = pb.level_stack(0, 0)
    rows = given_rows_from_alignments(st['alignments']).astype(np.int64)
    n = len(rows)
    clean = buffers(rows, n, n + 10)
    assert raw_call(pb, [clean]) == 0
    bad = rows.copy()
    big = given_ref.INT32_MAX
    bad[3] = (-1, 1, 5, 1)                                # a negative field
    bad[5] = (big, big, big, big)
    bad[7] = (bad[7][0], 0, bad[7][2], 0)                 # p = q = 0
    bad[9] = (bad[9][0], 2, bad[9][2], 0)                 # a deletion of two segments
    bad[11] = (bad[11][0], 5, bad[11][2], 1)              # wider than a candidate
    bad[13] = (199, 2, bad[13][2], 1)                     # x_start + p = n + 1
    bad[15] = (0, 1, -big - 1, 1)
    poison = [3, 5, 7, 9, 11, 13, 15]
    dirty = buffers(bad, n, n + 10)
    assert raw_call(pb, [dirty]) == 0
    (cs, ct, cr), (ds, dt, dr) = read(clean), read(dirty)
    ref = given_ref.score(st, v0, v1, bad)
    assert dr == ref['report'] and dr[3] == 1 and dr[4] == 6 and dr[7] == 0
    assert cr[3:6] == (0, 0, 0) and cr[7] == 1
    assert np.isnan(ds[poison]).all()
    keep = np.setdiff1d(np.arange(n), poison)
    assert ds[keep].tobytes() == cs[keep].tobytes() and np.isfinite(cs[:n]).all()
    assert (ds[n:] == -7.0).all() and (cs[n:] == -7.0).all()
    assert dt[1] == ct[1] == st['del_penalty'] and np.isfinite(dt[0]) and dt[0] < ct[0]


# ---------------------------------------------------------------------------------------------- 7
def ragged_run(pipeline):
    from svx import _lib
    from svx.vecalign.dp_utils import given_rows_from_alignments
    sizes = [(300, 280), (211, 333), (120, 97)]
    docs = [make_pair(n, m, 4, 32, seed=40 + i, deletions=3) for i, (n, m) in enumerate(sizes)]
    ctx = _lib.context()
    out = []
    try:
        ctx.set_pipeline(pipeline)
        pb = batch(docs, 7, [900, 901, 902])
        pb.run()                               # with the pipeline on the second half is still held back: the call flushes
        own = pb.score_alignments(["own"] * 3)
        hand = pb.score_alignments([every_layer_pair(n, m) for n, m in sizes])
        out += [own.fetch(), hand.fetch()]
        rows = [given_rows_from_alignments(every_layer_pair(n, m)) for n, m in sizes]
        e = [buffers(rows[0], len(rows[0]), len(rows[0])), buffers(rows[1], len(rows[1]), len(rows[1]), code=1),
             buffers(rows[2], len(rows[2]) + 1, len(rows[2]))]
        skipped = dict(e[0])
        assert raw_call(pb, [None, e[1], e[2]]) == 0
        out.append([read(x) for x in (skipped, e[1], e[2])])
        stacks = [pb.level_stack(i, 0) for i in range(3)]
    finally:
        ctx.set_pipeline(False)
    return docs, sizes, stacks, out


def test_ragged_batch_skips_and_failed_pairs():
    docs, sizes, stacks, (own, hand, raw) = ragged_run(False)
    for i, (n, m) in enumerate(sizes):
        check_against_ref(own[i], stacks[i], docs[i][0], docs[i][1], stacks[i]['alignments'], "ragged own %d" % i)
        check_against_ref(hand[i], stacks[i], docs[i][0], docs[i][1], every_layer_pair(n, m), "ragged hand %d" % i)
    for k, (scores, total, report) in enumerate(raw):
        assert (scores == -7.0).all(), k
        if k == 0:                                        # rows == NULL: nothing of the pair is written
            assert (total == -7.0).all() and report == (-7,) * 8
        else:                                             # info[1] != 0; a count above cap
            assert np.isnan(total).all() and report == NONE8
    _, _, _, piped = ragged_run(True)
    for a, b in zip(own + hand, piped[0] + piped[1]):
        assert a['report'] == b['report'] and a['total'] == b['total'] and a['scores'].tobytes() == b['scores'].tobytes()
    for a, b in zip(raw, piped[2]):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


# ---------------------------------------------------------------------------------------------- 8
def test_argument_errors_queue_nothing():
    import torch
    from svx import _lib
    from svx.vecalign.dp_utils import given_rows_from_alignments
    v0, v1 = make_pair(60, 50, 4, 32, 2, deletions=2)
    pb = batch([(v0, v1)], 7, [5])
    pb.run()
    ctx = pb.ctx
    rows = given_rows_from_alignments(every_layer_pair(60, 50))
    e = buffers(rows, len(rows), len(rows))
    odd = torch.full((12,), -7, dtype=torch.int32).cuda()
    cases = [
        ("null given", lambda: ctx.lib.svx_score_alignments(ctx.h, None, 1)),
        ("negative n_pairs", lambda: raw_call(pb, [e], n_pairs=-1)),
        ("count mismatch", lambda: raw_call(pb, [e, e])),
        ("null info", lambda: raw_call(pb, [dict(e, info=None)])),
        ("null total", lambda: raw_call(pb, [dict(e, total=None)])),
        ("null report", lambda: raw_call(pb, [dict(e, report=None)])),
        ("misaligned report", lambda: raw_call(pb, [dict(e, report=odd.data_ptr() + 4)])),
        ("negative cap", lambda: raw_call(pb, [dict(e, cap=-1)])),
    ]
    for name, call in cases:
        assert call() == SVX_ERR_ARG, name
        assert len(ctx.lib.svx_last_error(ctx.h)) > 10, name
    assert ctx.lib.svx_score_alignments(None, None, 1) == SVX_ERR_ARG
    fresh = _lib.Context(0)               # a context without an earlier call
    fresh.use_current_stream()
    cg = (_lib.Given * 1)()
    assert fresh.lib.svx_score_alignments(fresh.h, cg, 1) == SVX_ERR_ARG
    assert b"no earlier" in fresh.lib.svx_last_error(fresh.h)
    ctx.sync()
    scores, total, report = read(e)
    assert (scores == -7.0).all() and (total == -7.0).all() and report == (-7,) * 8 and (odd.cpu().numpy() == -7).all()
    assert raw_call(pb, [e]) == 0           # the context still works
    assert read(e)[2][:6] == (len(rows), 26, len(rows) - 26, 0, 0, 6)


# ---------------------------------------------------------------------------------------------- 9
def test_two_calls_back_to_back_take_turns_in_the_scratch():
    from svx import _lib
    v0, v1, src = block_deletion_pair(seed=0)
    truth = given_ref.truth_path(src, 300)
    pb = batch([(v0, v1)], 7, [11])
    pb.run()
    a, b, c = pb.score_alignments(["own"]), pb.score_alignments([truth]), pb.score_alignments(["own"])   # nothing waits in between
    a, b, c = a.fetch()[0], b.fetch()[0], c.fetch()[0]
    dev = pb.ctx.device
    old = _lib._ctxs[dev]
    try:
        _lib._ctxs[dev] = _lib.Context(dev)           # a fresh context: its scratch has seen no other call
        pb2 = batch([(v0, v1)], 7, [11])
        pb2.run()
        b2 = pb2.score_alignments([truth]).fetch()[0]
        a2 = pb2.score_alignments(["own"]).fetch()[0]
    finally:
        _lib._ctxs[dev] = old
    for x, y in ((a, a2), (b, b2), (c, a2)):
        assert x['report'] == y['report'] and x['total'] == y['total'] and x['scores'].tobytes() == y['scores'].tobytes()
    assert b['report'][6] == 206 and a['report'][6] == 0
