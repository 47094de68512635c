"""PreparedBatch.row_alternatives() (svx_row_alternatives) against alt_ref on what the call itself left on the device: after
run(), level 0 of every pair is read back (svx_debug_level: costs, csum, back-pointers, b_offset, penalty, rows) and fed to
the float64 restatement.  Both sides start from the same bits, every value is a minimum of singly rounded sums or an
equality test on them, so edges, spans, detours, scores, slack and regret are compared with ==, on any input."""
import ctypes
import os

import numpy as np
import pytest

import alt_ref
import dp_ref
import slack_ref
from around_ref import SVX_ERR_TRACEBACK
from synth import alignment_types, make_pair
from test_gpu_alt_ops import compare, given_rows
from test_gpu_row_slack import TRIM, to_dev

pytestmark = pytest.mark.gpu
SIZES = [(60, 50), (33, 47), (51, 58)]


def check_batch(pb, label, K=16, max_slack=np.inf, failed=(), skip=(), detour=True, with_given=True):
    """-> per pair (host result, reference, level view) after comparing row_alternatives() with the reference."""
    from svx.vecalign.dp_utils import alternatives_to_host, prior_rows_from_alignments
    refs, given = [], []
    for i in range(len(pb.vecs)):
        if i in failed:
            refs.append(None)
            given.append(np.asarray([(0, 1, 0, 1)], np.int32) if with_given else None)
            continue
        g = pb.level_stack(i, 0)
        rows = prior_rows_from_alignments(g['alignments'])
        refs.append((g, rows))
        given.append(given_rows(rows, g['alignment_types'], g['size0'], g['size1'], 5 + i) if with_given and i % 2 == 0 else None)
    sl, _ = pb.row_slack()
    alt = pb.row_alternatives(K, max_slack, given=given if with_given else None, detour=detour, skip=skip)
    pb.ctx.sync()
    sl = sl.cpu().numpy()
    summary = alt['summary'].cpu().numpy()
    out = []
    for i in range(len(pb.vecs)):
        o, cap = int(pb.offs[i]), int(pb.offs[i + 1] - pb.offs[i])
        if i in failed or i in skip:
            assert summary[i].tolist() == ([-1] * 4 if i in failed else [0] * 4)
            got = alternatives_to_host(alt, cap, o, i)   # untouched: as row_alternatives() allocated it
            assert np.isnan(got['slack']).all() and (got['edge'] == -1).all() and (got['span'] == -1).all()
            assert 'regret' not in got or np.isnan(got['regret']).all()
            out.append(None)
            continue
        g, rows = refs[i]
        n, m = g['size0'], g['size1']
        args = (g['a_b_costs'], g['b_offset'], g['alignment_types'], g['del_penalty'], n, m)
        bk = slack_ref.backward(*args)
        want = alt_ref.alternatives(*args, g['a_b_csum'], bk, g['a_b_xp'], g['a_b_yp'], rows, K, max_slack, want_detours=detour)
        got = alternatives_to_host(alt, len(rows), o, i)
        raw = {k: alt[k][o:o + cap].cpu().numpy() for k in ('slack', 'edge', 'span', 'detour', 'detour_scores') if k in alt}
        compare({k: v[:len(rows)] for k, v in raw.items()}, want, K, "%s pair %d" % (label, i))
        assert np.array_equal(got['slack'], sl[o:o + len(rows)], equal_nan=True)      # the bits of svx_row_slack
        assert list(got['summary']) == want['summary']
        assert np.isnan(raw['slack'][len(rows):]).all() and (raw['edge'][len(rows):] == -1).all()   # nothing past the rows
        if 'detour' in raw:
            assert (raw['detour'][len(rows):] == -1).all()
        if given[i] is not None:
            wr = alt_ref.regret(*args, g['a_b_csum'], bk, given[i])
            assert np.array_equal(got['regret'], wr, equal_nan=True), (label, i)
            csum = g['a_b_csum']
            bound = 2 * csum.shape[0] * 2.0 ** -53 * np.abs(csum[np.isfinite(csum)]).max()
            assert np.abs(wr[:len(rows)]).max() <= bound                              # the returned rows: 0 up to rounding
        out.append((got, want, g))
    return out


def batch(docs, types, W, max_full, search="coarse_to_fine", store="f32", **kw):
    from svx.vecalign import dp_utils
    return dp_utils.PreparedBatch([(to_dev(a, store), to_dev(b, store)) for a, b in docs], types, 0.2, W, max_full, 20000, 100,
                                  rngs=[np.random.RandomState(700 + i) for i in range(len(docs))], search=search, **kw)


@pytest.mark.parametrize("pipeline", [False, True], ids=["plain", "pipeline"])
def test_ragged_pairs_coarse_to_fine(pipeline):
    from svx import _lib
    from svx.vecalign import dp_utils
    docs = [make_pair(n, m, 4, 32, seed=60 + i) for i, (n, m) in enumerate(SIZES)]
    ctx = _lib.context()
    was = ctx.pipeline
    try:
        ctx.set_pipeline(pipeline)
        pb = batch(docs, alignment_types(5), 7, 20)
        pb.run()
        res = check_batch(pb, "ragged", K=16)
        assert all(len(dp_utils.level_sizes(n, m, 20)) >= 2 for n, m in SIZES)   # (level 0 is a refinement step)
        check_batch(pb, "ragged_K3", K=3, max_slack=0.5 * res[0][2]['del_penalty'])
    finally:
        ctx.set_pipeline(was)
    st = np.concatenate([got['span'][:, 3] for got, _, _ in res])
    assert (st == 0).any()


def test_types_that_do_not_pack_into_four_bits():
    """A type of 16 segments: the call keeps int32 pointer planes instead of packed bytes."""
    from svx import _lib
    types = [(1, 1), (16, 1), (1, 16), (1, 2), (2, 1)]
    docs = [make_pair(60, 50, 16, 32, seed=70), make_pair(40, 44, 16, 32, seed=71)]
    pb = batch(docs, types, 16, 0, search="straight")
    pb.run()
    v = _lib.LevelView()
    pb.ctx.check(pb.ctx.lib.svx_debug_level(pb.ctx.h, 0, 0, ctypes.byref(v)))
    assert not v.a_b_bp and v.a_b_xp and v.a_b_yp
    check_batch(pb, "int32 planes", K=24)


def test_wide_band_with_a_cost_array():
    """W = 40: 80 cells per diagonal, the strided backward kernel; coarse-to-fine keeps the cost array at any width."""
    docs = [make_pair(n, m, 4, 32, seed=80 + i) for i, (n, m) in enumerate(SIZES[:2])]
    pb = batch(docs, alignment_types(5), 40, 20)
    pb.run()
    check_batch(pb, "W40", K=16)


def test_around_with_a_failed_and_a_skipped_pair():
    import torch
    docs = [make_pair(n, m, 4, 32, seed=40 + i) for i, (n, m) in enumerate(SIZES)] + [make_pair(44, 41, 4, 32, seed=49)]

    def split_prior(n, m, blocks):
        xs, ys = [n * i // blocks for i in range(blocks + 1)], [m * i // blocks for i in range(blocks + 1)]
        return [(list(range(xs[i], xs[i + 1])), list(range(ys[i], ys[i + 1]))) for i in range(blocks)]
    failed = (torch.tensor([[0, 20, 0, 20], [20, 13, 20, 27]], dtype=torch.int32).cuda(), torch.tensor([2, SVX_ERR_TRACEBACK], dtype=torch.int32).cuda())
    pb = batch(docs, alignment_types(5), 7, 300, search="around",
               priors=[split_prior(60, 50, 6), failed, split_prior(51, 58, 5), split_prior(44, 41, 4)])
    pb.run()
    pb.ctx.sync()
    assert pb.info.cpu().numpy()[:, 1].tolist()[1] != 0
    check_batch(pb, "around", K=16, failed=(1,), skip=(3,))
    check_batch(pb, "around edges only", K=16, failed=(1,), detour=False, with_given=False)


def test_real_example_pair():
    from svx.vecalign import dp_utils
    from svx.vecalign.vecalign import load_document, resolve_search_params
    types, src_k, tgt_k, W = resolve_search_params(6, None, 5)
    docs = []
    for lang, k, side in (("en", src_k, "src"), ("de", tgt_k, "tgt")):
        _, v = load_document(os.path.join(TRIM, f"segments_{lang}.txt"),
                             [os.path.join(TRIM, f"cat_segs_{lang}.txt"), os.path.join(TRIM, f"embeds_{lang}.f16")], False, True, k,
                             os.path.join(TRIM, f"ignore_{side}.txt"), True)
        docs.append(v)
    pb = dp_utils.PreparedBatch([tuple(docs)], types, 0.2, W, 300, 20000, 100, rngs=[np.random.RandomState(0)])
    pb.run()
    (got, want, g), = check_batch(pb, "example_trim", K=16)
    nd = got['span'][got['span'][:, 3] == 0, 2]
    print("example_trim: rows, with an edge, detours written, too long at K = 16: %s; written detours: median %s rows, max %s" % (
        list(got['summary']), np.median(nd) if len(nd) else None, nd.max() if len(nd) else None))
    for r in np.flatnonzero(got['span'][:, 3] == 0):   # every written detour rejoins the returned path around its row
        lo, hi, k, _ = got['span'][r]
        assert lo <= r < hi and k == len(got['detours'][r][0])


def test_vecalign_returns_alternatives():
    from svx.vecalign import dp_utils
    v0, v1 = make_pair(60, 50, 4, 32, seed=5)
    rows = np.asarray([(0, 1, 0, 1), (3, 1, 2, 2), (70, 1, 0, 1)], np.int32)
    np.random.seed(3)
    st = dp_utils.vecalign(v0, v1, alignment_types(5), 0.2, 7, 20, 20000, 100, return_slack=True,
                           return_alternatives=dict(max_detour=8, given=rows))
    alt = st[0]['alternatives']
    n = len(st[0]['final_alignments'])
    assert alt['summary'][0] == n and len(alt['detours']) == n and alt['edge'].shape == (n, 4)
    assert np.array_equal(alt['slack'], st[0]['row_slack'], equal_nan=True)
    assert alt['regret'].shape == (3,) and np.isnan(alt['regret'][2])


def test_argument_errors_queue_nothing():
    import torch
    from svx import _lib
    # ---- the tile sweep keeps no cost array
    case = [c for c in dp_ref.Z_STRAIGHT if c[0] == "a5_W40"][0]
    pairs = dp_ref.z_straight_pairs(case)
    from svx.vecalign import dp_utils
    pb = dp_utils.PreparedBatch([(to_dev(p[0], "f32"), to_dev(p[1], "f32")) for p in pairs], dp_ref.z_straight_types(case), dp_ref.FRAC, 40, 0,
                                dp_ref.SAMPLE, dp_ref.NSAMP, rngs=[np.random.RandomState(p[4]) for p in pairs],
                                norms=[(p[2], p[3]) for p in pairs], search="straight")
    pb.run()
    with pytest.raises(_lib.SvxError, match="tile sweep, which keeps no cost array"):
        pb.row_alternatives()
    # ---- a wrong pair count, null and misaligned arguments, limits out of range (on a call that could be measured)
    v0, v1 = make_pair(60, 50, 4, 32, seed=5)
    ok = batch([(v0, v1)], alignment_types(5), 7, 300)
    ok.run()
    ctx = ok.ctx
    buf = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")
    summ = torch.zeros(16, dtype=torch.int32, device="cuda")
    vp = ctypes.c_void_p
    b = buf.data_ptr()

    def alts(**kw):
        a = (_lib.Alt * 2)()
        for c in a:
            c.edge, c.span, c.detour, c.detour_scores = b, b + 4096, b + 8192, b + 65536
            for k, v in kw.items():
                setattr(c, k, v)
        return a
    inf = float("inf")
    for args, text in (((alts(), 4, inf, vp(summ.data_ptr()), 2), "2 pairs given, the last call had 1"),
                       ((None, 4, inf, vp(summ.data_ptr()), 1), "null argument"),
                       ((alts(), 4, inf, vp(0), 1), "null argument"),
                       ((alts(), 4, inf, vp(summ.data_ptr() + 4), 1), "16-byte aligned"),
                       ((alts(), 4, inf, vp(summ.data_ptr()), -1), "negative n_pairs"),
                       ((alts(), 0, inf, vp(summ.data_ptr()), 1), "max_detour 0 outside [1, 256]"),
                       ((alts(), 257, inf, vp(summ.data_ptr()), 1), "max_detour 257 outside [1, 256]"),
                       ((alts(), 4, float("nan"), vp(summ.data_ptr()), 1), "max_slack is NaN"),
                       ((alts(span=None), 4, inf, vp(summ.data_ptr()), 1), "null edge / span"),
                       ((alts(edge=b + 4), 4, inf, vp(summ.data_ptr()), 1), "16-byte aligned"),
                       ((alts(given=b + 4), 4, inf, vp(summ.data_ptr()), 1), "16-byte aligned"),
                       ((alts(given=b, given_info=b), 4, inf, vp(summ.data_ptr()), 1), "given rows need regret")):
        rc = ctx.lib.svx_row_alternatives(ctx.h, *args)
        assert rc != 0 and text in ctx.lib.svx_last_error(ctx.h).decode(), (text, ctx.lib.svx_last_error(ctx.h).decode())
    ctx.sync()
    assert not buf.cpu().numpy().any() and not summ.cpu().numpy().any()
    # ---- no earlier call: a context of its own
    fresh = _lib.Context(ctx.device)
    rc = fresh.lib.svx_row_alternatives(fresh.h, alts(), 4, inf, vp(summ.data_ptr()), 1)
    assert rc != 0 and "no earlier svx_align_batch" in fresh.lib.svx_last_error(fresh.h).decode()
