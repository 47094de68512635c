"""PreparedBatch.row_slack_wide() (svx_row_slack_wide: the backward tile sweep with the fused cut minimum) against
slack_ref, the normative restatement of include/svx.h's slack section.

Family Z (zero embeddings, normalisers drawn from a few levels: dp_ref.z_pair) makes the tile sweep's fp32 costs the
oracle's bits, so the reference is slack_ref on the oracle's a_b_costs, the GPU's own csum (masked to the lattice nodes,
all the sweep stores) and the GPU's own rows, and everything is compared bit for bit: slack with np.array_equal, the
summary exactly, the Bk plane with == on the lattice nodes of the band.

Continuous data: the GPU's costs are its own MFMA results, so the rows must equal the oracle's and the slack is held to
slack_ref on the oracle's tables within the project's cost tolerance (tile_cost_ref's per-plane bound), two paths of at
most n + m edges each:  |slack - ref| <= 2 (n + m) max_t bound[t] + 4 (A + 2) 2^-53 max |csum|."""
import functools

import numpy as np
import pytest

import dp_ref
import slack_ref
from around_ref import SVX_ERR_TRACEBACK, around_stack
from synth import alignment_types, make_pair

pytestmark = pytest.mark.gpu
T5, T6 = alignment_types(5), alignment_types(6)


def to_dev(v, store):
    import torch
    return torch.from_numpy(v).cuda().to({"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[store])


def lattice_mask(nbo, B, size0, size1):
    yy = np.arange(B)[None, :] + np.asarray(nbo)[:, None]
    xx = np.arange(len(nbo))[:, None] - yy
    return (0 <= xx) & (xx <= size0) & (0 <= yy) & (yy <= size1)


def z_batch(pairs, types, W, store, search="straight", priors=None):
    from svx.vecalign import dp_utils
    kw = dict(priors=priors) if priors is not None else {}
    return dp_utils.PreparedBatch([(to_dev(p[0], store), to_dev(p[1], store)) for p in pairs], types, dp_ref.FRAC, W, 0, dp_ref.SAMPLE,
                                  dp_ref.NSAMP, rngs=[np.random.RandomState(p[4]) for p in pairs], norms=[(p[2], p[3]) for p in pairs],
                                  search=search, **kw)


def check_exact(pb, refs, label, failed=()):
    """row_slack_wide(return_plane=True) of a family-Z batch against slack_ref, bit for bit.  refs[i]: the oracle's stack
    entry of pair i (its a_b_costs are the sweep's bits)."""
    from svx.vecalign.dp_utils import prior_rows_from_alignments
    slack, summary, planes = pb.row_slack_wide(return_plane=True)
    pb.ctx.sync()
    slack, summary = slack.cpu().numpy(), summary.cpu().numpy()
    for i in range(len(pb.vecs)):
        o, cap = int(pb.offs[i]), int(pb.offs[i + 1] - pb.offs[i])
        if i in failed:
            assert summary[i].tolist() == [-1, -1, -1, -1]
            assert np.isnan(slack[o:o + cap]).all()   # untouched: as row_slack_wide() allocated it
            continue
        g, ref = pb.level_stack(i, 0), refs[i]
        assert 'a_b_costs' not in g                   # the tile sweep
        n, m, types, pen = g['size0'], g['size1'], g['alignment_types'], g['del_penalty']
        rows = prior_rows_from_alignments(g['alignments'])
        costs, bo = ref['a_b_costs'], ref['b_offset']
        assert np.array_equal(bo, g['b_offset']) and np.array_equal(slack_ref.b_offset_out(bo), g['new_b_offset'])
        B = costs.shape[2]
        keep = lattice_mask(g['new_b_offset'], B, n, m)
        csum = np.where(keep, g['a_b_csum'], np.inf)
        bk = slack_ref.backward(costs, bo, types, pen, n, m)
        want = slack_ref.slack(costs, bo, types, pen, n, m, csum, bk, rows)
        got = slack[o:o + len(rows)]
        print("%s pair %d: %d rows, %d with slack 0, %d positive, max %.4f" % (label, i, len(rows), int((got == 0).sum()),
                                                                          int((got > 0).sum()), float(np.nanmax(got))))
        assert np.array_equal(got, want, equal_nan=True), "%s pair %d: %d of %d rows differ, first %r" % (
            label, i, int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum()), len(rows),
            [(int(k), rows[k].tolist(), got[k], want[k]) for k in np.flatnonzero(got != want)[:3]])
        assert not np.isnan(got).any()
        assert summary[i].tolist() == slack_ref.summary(want)
        assert np.isnan(slack[o + len(rows):o + cap]).all()   # nothing past the rows is written
        # ties and decided rows are both in the case -- but for dp_ref.Z_STRAIGHT's a6_W33_bf16: its six normaliser levels
        # leave no two paths with equal float64 totals (226 rows, smallest slack 1.1e-13 in slack_ref on the oracle's own
        # tables: ties of exact arithmetic that rounding breaks), so there the tie count is held to the reference's, 0
        assert (got > 0.0).any() and (got == 0.0).any() == (label != "a6_W33_bf16")
        plane = planes[i].cpu().numpy()[:bk.shape[0]]
        assert np.array_equal(plane[keep], bk[keep]), "%s pair %d: Bk differs on %d lattice nodes" % (label, i, int((plane[keep] != bk[keep]).sum()))


def z_case(sizes, types, W, store, levels, seed):
    """-> (pairs, the oracle's straight stacks) of a family-Z case given like a dp_ref.Z_STRAIGHT row."""
    import oracle
    case = ("wide", sizes, types, W, store, 32, levels, seed)
    pairs = dp_ref.z_straight_pairs(case)
    return pairs, [dp_ref.straight_stack(oracle, p[0], p[1], types, W, p[4], norms=(p[2], p[3])) for p in pairs]


Z_CASES = {
    "a5_W40": ([(300, 280)], T5, 40, "f32", dp_ref.LEVELS2, 22),               # dp_ref.Z_STRAIGHT: <E, 8, 5, 5>
    "a6_W33_bf16": ([(330, 310)], T6, 33, "bf16", dp_ref.LEVELS6, 23),         # dp_ref.Z_STRAIGHT: <E, 12, 8, 2>
    "below_one_tile": ([(20, 25)], T5, 40, "f32", dp_ref.LEVELS2, 51),
    "tile_corners": ([(64, 96)], T5, 40, "f16", dp_ref.LEVELS2, 52),           # the end node is the first node of a tile
    "steep": ([(330, 120)], T5, 120, "f32", dp_ref.LEVELS2, 53),
    "dense": ([(150, 140)], T5, 200, "bf16", dp_ref.LEVELS2, 54),
    "batch3_a6_W60": ([(210, 200), (330, 310), (120, 260)], T6, 60, "f32", dp_ref.LEVELS2, 55),   # tickets over pairs
}


def test_z_straight_cases_are_the_named_ones():
    for name in ("a5_W40", "a6_W33_bf16"):
        case = [c for c in dp_ref.Z_STRAIGHT if c[0] == name][0]
        assert (case[1], case[2], case[3], case[4], case[6], case[7]) == Z_CASES[name]


@pytest.mark.parametrize("name", list(Z_CASES))
def test_family_z_bit_for_bit(name):
    sizes, types, W, store, levels, seed = Z_CASES[name]
    pairs, refs = z_case(sizes, types, W, store, levels, seed)
    pb = z_batch(pairs, types, W, store)
    pb.run()
    check_exact(pb, refs, name)
    # a second call on the same run gives the same bits (its flags, ticket and cut minima are its own)
    first = pb.slack.cpu().numpy().copy()
    again, _ = pb.row_slack_wide()
    assert np.array_equal(again.cpu().numpy(), first, equal_nan=True)


def test_around_wide_bent_band_with_a_failed_pair():
    import oracle
    import torch
    sizes = [(300, 280), (120, 97), (211, 333)]
    case = ("bent", sizes, T5, 40, "f32", 32, dp_ref.LEVELS2, 56)
    pairs = dp_ref.z_straight_pairs(case)
    bent = [[(list(range(0, 100)), list(range(0, 30))), (list(range(100, 180)), list(range(30, 200))), (list(range(180, 300)), list(range(200, 280)))],
            None,
            [(list(range(0, 60)), list(range(0, 150))), (list(range(60, 211)), list(range(150, 333)))]]
    failed = (torch.tensor([[0, 60, 0, 50], [60, 60, 50, 47]], dtype=torch.int32).cuda(), torch.tensor([2, SVX_ERR_TRACEBACK], dtype=torch.int32).cuda())
    pb = z_batch(pairs, T5, 40, "f32", search="around_wide", priors=[bent[0], failed, bent[2]])
    pb.run()
    pb.ctx.sync()
    assert pb.info.cpu().numpy()[:, 1].tolist()[1] != 0
    refs = [around_stack(oracle, p[0], p[1], T5, 40, p[4], bent[i], norms=(p[2], p[3])) if i != 1 else None for i, p in enumerate(pairs)]
    check_exact(pb, refs, "around_wide", failed=(1,))


RAGGED = [(150, 137), (70, 90), (40, 200)]


@pytest.mark.parametrize("a", [5, 6])
def test_ragged_batch_with_the_middle_pair_skipped(a):
    """Three pairs of different sizes in one batch (9, 5 and 8 tile anti-diagonals: the ticket table is ragged), on both
    LDS-resident shapes.  All three measured: slack_ref, bit for bit.  Then svx_row_slack_wide with the middle pair's
    slack NULL: pairs 0 and 2 get the bits they get when each is aligned and measured alone, and nothing of the middle
    pair is written (its tiles are claimed and dropped, and the reverse entry lookup walks across them)."""
    import ctypes
    import torch
    from svx import _lib
    types, W, SENT, ISENT = alignment_types(a), 40, -7.0, -9
    nd = [(n + 32) // 32 + (m + 32) // 32 - 1 for n, m in RAGGED]       # tile anti-diagonals that hold nodes 0 .. n, 0 .. m
    assert sorted(nd) == [5, 8, 9]
    pairs, refs = z_case(RAGGED, types, W, "f32", dp_ref.LEVELS2, 57 + a)
    alone = {}
    for i in (0, 2):
        one = z_batch([pairs[i]], types, W, "f32")
        one.run()
        sl, sm = one.row_slack_wide()
        one.ctx.sync()
        alone[i] = (sl.cpu().numpy(), sm.cpu().numpy()[0].tolist())
    pb = z_batch(pairs, types, W, "f32")
    pb.run()
    check_exact(pb, refs, "ragged_a%d" % a)
    ctx = pb.ctx
    slack = torch.full((int(pb.offs[-1]),), SENT, dtype=torch.float64, device="cuda")
    summary = torch.full((3, 4), ISENT, dtype=torch.int32, device="cuda")
    sw = (_lib.SlackWide * 3)()
    for i in (0, 2):
        sw[i].slack = slack.data_ptr() + 8 * int(pb.offs[i])
    ctx.use_current_stream()
    ctx.check(ctx.lib.svx_row_slack_wide(ctx.h, sw, ctypes.c_void_p(summary.data_ptr()), 3))
    ctx.sync()
    slack, summary = slack.cpu().numpy(), summary.cpu().numpy()
    for i in (0, 2):
        o, cap, (want, wsum) = int(pb.offs[i]), int(pb.offs[i + 1] - pb.offs[i]), alone[i]
        rows = wsum[0]
        assert 0 < rows <= cap and summary[i].tolist() == wsum
        assert np.array_equal(slack[o:o + rows].view(np.int64), want[:rows].view(np.int64)), "pair %d: not the bits of the pair alone" % i
        assert (slack[o + rows:o + cap] == SENT).all()
    o, cap = int(pb.offs[1]), int(pb.offs[2] - pb.offs[1])
    assert cap > 0 and (slack[o:o + cap] == SENT).all() and (summary[1] == ISENT).all()


# ------------------------------------------------------------------------------------------ continuous data
@functools.lru_cache(maxsize=None)
def cost_bound(n, m, K, d, store, W, seed):
    """(oracle stack, per-plane bound of tile_cost_ref without the float64 term) for make_pair(n, m, K, d) in `store`."""
    import oracle
    import stage_ref
    import tile_cost_ref as tcr
    v0, v1 = make_pair(n, m, K, d, seed=seed)
    v0, v1 = tcr.store_round(v0, store), tcr.store_round(v1, store)
    st = dp_ref.straight_stack(oracle, v0, v1, T5, W, seed)
    v0n, v1n = stage_ref.norm1(v0), stage_ref.norm1(v1)
    path = oracle.search_path([(list(range(n)), list(range(m)))], False, n, m)
    dots, xx, yy = tcr.band_dots(v0n, v1n, np.asarray(path, np.int64).reshape(-1, 2), st['b_offset'], T5, W)
    dr = stage_ref.replay_draws(oracle, seed, n, m, K, K, 1 << 30, tcr.SAMPLE, tcr.NSAMP)[0]
    n0, n1 = stage_ref.norms(v0n, v1n, dr['idx0']), stage_ref.norms(v1n, v0n, dr['idx1'])   # float64, on the oracle's draws
    err = tcr.pair_errors(st['a_b_costs'], tcr.costs_from_dots(dots, xx, yy, n0, n1, T5))
    return (v0, v1), st, tcr.bounds(err['E_orc'], err['cmax'])


CONT = [(300, 280, 4, 72, "f32", 40), (300, 280, 4, 72, "f16", 40), (300, 280, 4, 72, "bf16", 40), (700, 640, 4, 1024, "bf16", 40)]


@pytest.mark.parametrize("n,m,K,d,store,W", CONT, ids=lambda v: str(v))
def test_continuous_data_within_the_cost_tolerance(n, m, K, d, store, W):
    from svx.vecalign import dp_utils
    from svx.vecalign.dp_utils import prior_rows_from_alignments
    seed = 7
    (v0, v1), st, bound = cost_bound(n, m, K, d, store, W, seed)
    pb = dp_utils.PreparedBatch([(to_dev(v0, store), to_dev(v1, store))], T5, 0.2, W, 0, 20000, 100, rngs=[np.random.RandomState(seed)],
                                search="straight")
    pb.run()
    assert pb.results()[0][0] == st['final_alignments'], "the GPU's rows are not the oracle's"
    slack, summary = pb.row_slack_wide()
    rows = prior_rows_from_alignments(st['final_alignments'])
    got = slack.cpu().numpy()[:len(rows)]
    args = (st['a_b_costs'], st['b_offset'], T5, st['del_penalty'], n, m)
    csum = st['a_b_csum']
    want = slack_ref.slack(*args, csum, slack_ref.backward(*args), rows)
    cs_max = np.abs(csum[np.isfinite(csum)]).max()
    A2 = csum.shape[0]
    tol = 2 * (n + m) * float(bound.max()) + 4 * A2 * 2.0 ** -53 * cs_max
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin]).max()
    print("%dx%d d=%d %s: %d rows, max |slack - ref| = %.3e (tolerance %.3e), min slack %.3e, median %.4f" % (
        n, m, d, store, len(rows), err, tol, float(got.min()), float(np.median(got))))
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], want[~fin])
    assert err <= tol
    assert got.min() >= -2 * A2 * 2.0 ** -53 * cs_max          # the rounding bound of DESIGN 6d
    assert summary.cpu().numpy()[0].tolist() == [len(rows), int((got == 0).sum()), int(np.isposinf(got).sum()), 0]


# ------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_queue_nothing():
    import ctypes
    import torch
    from svx import _lib
    from svx.vecalign import dp_utils
    buf = torch.zeros(1024, dtype=torch.float64, device="cuda")
    summ = torch.zeros(16, dtype=torch.int32, device="cuda")
    vp = ctypes.c_void_p

    def sw_of(slack, bsum=None):
        sw = (_lib.SlackWide * 2)()
        for k in range(2):
            sw[k].slack, sw[k].bsum = slack, bsum
        return sw
    # ---- a narrow-band last call keeps its cost array: svx_row_slack measures it
    v0, v1 = make_pair(60, 50, 4, 32, seed=5)
    narrow = dp_utils.PreparedBatch([(to_dev(v0, "f32"), to_dev(v1, "f32"))], T5, 0.2, 7, 300, 20000, 100, rngs=[np.random.RandomState(1)])
    narrow.run()
    with pytest.raises(_lib.SvxError, match="did not run the tile sweep"):
        narrow.row_slack_wide()
    # ---- a type set on the general tile shape
    v0, v1 = make_pair(90, 80, 6, 32, seed=6)
    gen = dp_utils.PreparedBatch([(to_dev(v0, "f32"), to_dev(v1, "f32"))], alignment_types(7), 0.2, 40, 0, 20000, 100,
                                 rngs=[np.random.RandomState(2)], search="straight")
    gen.run()
    with pytest.raises(_lib.SvxError, match="general tile shape"):
        gen.row_slack_wide()
    # ---- a wrong pair count, null and misaligned arguments (on a call that could be measured)
    v0, v1 = make_pair(90, 80, 4, 32, seed=7)
    ok = dp_utils.PreparedBatch([(to_dev(v0, "f32"), to_dev(v1, "f32"))], T5, 0.2, 40, 0, 20000, 100, rngs=[np.random.RandomState(3)],
                                search="straight")
    ok.run()
    ctx = ok.ctx
    good = sw_of(buf.data_ptr())
    for args, text in (((good, vp(summ.data_ptr()), 2), "2 pairs given, the last call had 1"),
                       ((None, vp(summ.data_ptr()), 1), "null argument"),
                       ((good, vp(0), 1), "null argument"),
                       ((good, vp(summ.data_ptr() + 4), 1), "16-byte aligned"),
                       ((sw_of(buf.data_ptr() + 4), vp(summ.data_ptr()), 1), "8-byte aligned"),
                       ((sw_of(buf.data_ptr(), buf.data_ptr() + 2), vp(summ.data_ptr()), 1), "8-byte aligned"),
                       ((good, vp(summ.data_ptr()), -1), "negative n_pairs")):
        rc = ctx.lib.svx_row_slack_wide(ctx.h, *args)
        assert rc != 0 and text in ctx.lib.svx_last_error(ctx.h).decode(), (text, ctx.lib.svx_last_error(ctx.h).decode())
    ctx.sync()
    assert not buf.cpu().numpy().any() and not summ.cpu().numpy().any()
    # ---- a NULL slack skips the pair: nothing of it is written
    rc = ctx.lib.svx_row_slack_wide(ctx.h, sw_of(None), vp(summ.data_ptr()), 1)
    assert rc == 0
    ctx.sync()
    assert not summ.cpu().numpy().any()
    # ---- no earlier call: a context of its own
    fresh = _lib.Context(ctx.device)
    rc = fresh.lib.svx_row_slack_wide(fresh.h, good, vp(summ.data_ptr()), 1)
    assert rc != 0 and "no earlier svx_align_batch" in fresh.lib.svx_last_error(fresh.h).decode()


def test_return_slack_picks_the_wide_entry():
    """vecalign(return_slack=True) on a run that took the tile sweep: the slack of row_slack_wide(), not the refusal of row_slack()."""
    from svx.vecalign import dp_utils
    v0, v1 = make_pair(150, 140, 4, 32, seed=9)
    a, b = to_dev(v0, "f32"), to_dev(v1, "f32")
    np.random.seed(3)
    st = dp_utils.vecalign(a, b, T5, 0.2, 40, 300, 20000, 100, search="straight", return_slack=True)
    np.random.seed(3)
    pb = dp_utils.PreparedBatch([(a, b)], T5, 0.2, 40, 300, 20000, 100, search="straight")
    assert pb.took_tile_sweep()
    pb.run()
    sl, summ = pb.row_slack_wide()
    n = len(st[0]['final_alignments'])
    assert pb.results()[0][0] == st[0]['final_alignments']
    assert np.array_equal(st[0]['row_slack'], sl.cpu().numpy()[:n]) and not np.isnan(st[0]['row_slack']).any()
    assert st[0]['slack_summary'] == tuple(int(v) for v in summ.cpu().numpy()[0]) and st[0]['slack_summary'][0] == n


def test_stage_time_and_scratch_are_what_the_header_says():
    """svx_stage_ms("tiles_bwd") is set by the call when profiling is on, and svx_scratch_bytes grows by at least the Bk
    plane, cutmin and the node table of the pair when the caller gives no plane."""
    from svx import _lib
    from svx.vecalign import dp_utils
    n, m, W = 150, 140, 40
    v0, v1 = make_pair(n, m, 4, 32, seed=12)
    ctx = _lib.Context(_lib.context().device)          # a context of its own: its post-processing scratch starts empty
    pb = dp_utils.PreparedBatch([(to_dev(v0, "f32"), to_dev(v1, "f32"))], T5, 0.2, W, 0, 20000, 100, rngs=[np.random.RandomState(4)],
                                search="straight")
    pb.ctx = ctx
    lib = ctx.lib
    lib.svx_set_profiling(ctx.h, 1)
    try:
        pb.run()
        before = int(lib.svx_scratch_bytes(ctx.h))
        assert lib.svx_stage_ms(ctx.h, b"tiles") > 0.0 and lib.svx_stage_ms(ctx.h, b"tiles_bwd") == 0.0
        sl, summ = pb.row_slack_wide()
        assert lib.svx_stage_ms(ctx.h, b"tiles_bwd") > 0.0 and lib.svx_stage_launches(ctx.h, b"tiles_bwd") == 1
    finally:
        lib.svx_set_profiling(ctx.h, 0)
    ctx.sync()
    cap2 = n + m + 4 + 2                                # path capacity + 2 diagonals
    assert int(lib.svx_scratch_bytes(ctx.h)) - before >= cap2 * 2 * W * 8 + cap2 * 8 + cap2 * 8
    assert summ.cpu().numpy()[0, 0] == len(pb.results()[0][0])
    # with the caller's plane the scratch holds no plane: a fresh context grows by less than one
    ctx2 = _lib.Context(ctx.device)
    pb2 = dp_utils.PreparedBatch([(to_dev(v0, "f32"), to_dev(v1, "f32"))], T5, 0.2, W, 0, 20000, 100, rngs=[np.random.RandomState(4)],
                                 search="straight")
    pb2.ctx = ctx2
    pb2.run()
    before2 = int(ctx2.lib.svx_scratch_bytes(ctx2.h))
    sl2, _, _ = pb2.row_slack_wide(return_plane=True)
    ctx2.sync()
    grown = int(ctx2.lib.svx_scratch_bytes(ctx2.h)) - before2
    assert cap2 * 16 <= grown < cap2 * 2 * W * 8
    assert np.array_equal(sl2.cpu().numpy(), sl.cpu().numpy(), equal_nan=True)
