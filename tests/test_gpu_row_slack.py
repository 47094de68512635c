"""PreparedBatch.row_slack() (svx_row_slack) against slack_ref on what the call itself left on the device: after run(),
level 0 of every pair is read back (svx_debug_level / svx_copy_to_host: costs, csum, b_offset, penalty, rows) and fed to
the float64 restatement.  Both sides start from the same bits and every value is a minimum of singly rounded sums, so the
slack is compared bit for bit and the summary exactly, on any input."""
import os

import numpy as np
import pytest

import dp_ref
import slack_ref
from around_ref import SVX_ERR_TRACEBACK
from synth import alignment_types, make_pair

pytestmark = pytest.mark.gpu
TRIM = os.path.join(os.path.dirname(__file__), "golden", "example_trim")


def to_dev(v, store):
    import torch
    return torch.from_numpy(v).cuda().to({"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[store])


def reference(pb, i):
    """slack_ref on level 0 of pair i of the last run -> (slack, level view, rows)."""
    from svx.vecalign.dp_utils import prior_rows_from_alignments
    g = pb.level_stack(i, 0)
    rows = prior_rows_from_alignments(g['alignments'])   # (a complete path: the starts are the running sums)
    n, m = g['size0'], g['size1']
    args = (g['a_b_costs'], g['b_offset'], g['alignment_types'], g['del_penalty'], n, m)
    assert np.array_equal(slack_ref.b_offset_out(g['b_offset']), g['new_b_offset'])
    bk = slack_ref.backward(*args)
    return slack_ref.slack(*args, g['a_b_csum'], bk, rows), g, rows


def check_batch(pb, label, failed=()):
    """-> per pair (slack, level view) after comparing row_slack() with the reference."""
    slack, summary = pb.row_slack()
    pb.ctx.sync()
    slack, summary = slack.cpu().numpy(), summary.cpu().numpy()
    out = []
    for i in range(len(pb.vecs)):
        o, cap = int(pb.offs[i]), int(pb.offs[i + 1] - pb.offs[i])
        if i in failed:
            assert summary[i].tolist() == [-1, -1, -1, -1]
            assert np.isnan(slack[o:o + cap]).all()   # untouched: as row_slack() allocated it
            out.append(None)
            continue
        want, g, rows = reference(pb, i)
        got = slack[o:o + len(rows)]
        assert np.array_equal(got, want, equal_nan=True), "%s pair %d: %d of %d rows differ, first %r" % (
            label, i, int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum()), len(rows),
            [(int(k), got[k], want[k]) for k in np.flatnonzero(got != want)[:3]])
        assert not np.isnan(got).any()
        assert summary[i].tolist() == slack_ref.summary(want)
        assert np.isnan(slack[o + len(rows):o + cap]).all()   # nothing past the rows is written
        out.append((got, g))
    return out


FUSED = ["a5_W7_f32_6lv", "a5_W7_f32_6lv_pipeline", "a5_W7_f32_ragged4", "a5_W7_bf16_d1024"]


@pytest.mark.parametrize("name", FUSED)
def test_coarse_to_fine_family_z(name):
    from svx import _lib
    from svx.vecalign import dp_utils
    case = [c for c in dp_ref.Z_FUSED if c[0] == name][0]
    _, sizes, a, W, store, d, levels, max_full, seed, pipeline = case
    pairs = dp_ref.z_fused_pairs(case)
    ctx = _lib.context()
    was = ctx.pipeline
    try:
        ctx.set_pipeline(pipeline)
        pb = dp_utils.PreparedBatch([(to_dev(p[0], store), to_dev(p[1], store)) for p in pairs], alignment_types(a), dp_ref.FRAC, W,
                                    max_full, dp_ref.SAMPLE, dp_ref.NSAMP, rngs=[np.random.RandomState(p[4]) for p in pairs],
                                    norms=[(p[2], p[3]) for p in pairs])
        pb.run()
        res = check_batch(pb, name)
    finally:
        ctx.set_pipeline(was)
    for sl, g in res:   # zero embeddings, a handful of normaliser values: ties are the norm
        assert (sl == 0.0).any()


def test_straight_narrow_band():
    from svx.vecalign import dp_utils
    case = [c for c in dp_ref.Z_STRAIGHT if c[0] == "narrow_a5_W16"][0]
    name, sizes, _, W, store, d, levels, seed = case
    pairs = dp_ref.z_straight_pairs(case)
    pb = dp_utils.PreparedBatch([(to_dev(p[0], store), to_dev(p[1], store)) for p in pairs], dp_ref.z_straight_types(case), dp_ref.FRAC, W, 0,
                                dp_ref.SAMPLE, dp_ref.NSAMP, rngs=[np.random.RandomState(p[4]) for p in pairs],
                                norms=[(p[2], p[3]) for p in pairs], search="straight")
    pb.run()
    check_batch(pb, name)


def test_around_band_14_with_a_failed_pair():
    import torch
    from svx.vecalign import dp_utils
    sizes = [(300, 280), (120, 97), (211, 333)]
    docs = [make_pair(n, m, 4, 32, seed=40 + i) for i, (n, m) in enumerate(sizes)]

    def split_prior(n, m, blocks):
        xs, ys = [n * i // blocks for i in range(blocks + 1)], [m * i // blocks for i in range(blocks + 1)]
        return [(list(range(xs[i], xs[i + 1])), list(range(ys[i], ys[i + 1]))) for i in range(blocks)]
    failed = (torch.tensor([[0, 60, 0, 50], [60, 60, 50, 47]], dtype=torch.int32).cuda(), torch.tensor([2, SVX_ERR_TRACEBACK], dtype=torch.int32).cuda())
    pb = dp_utils.PreparedBatch([(to_dev(a, "f32"), to_dev(b, "f32")) for a, b in docs], alignment_types(5), 0.2, 7, 300, 20000, 100,
                                rngs=[np.random.RandomState(900 + i) for i in range(3)], search="around",
                                priors=[split_prior(300, 280, 15), failed, split_prior(211, 333, 9)])
    pb.run()
    pb.ctx.sync()
    assert pb.info.cpu().numpy()[:, 1].tolist()[1] != 0
    check_batch(pb, "around", failed=(1,))


def test_real_example_pair_and_the_rounding_bound():
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
    (sl, g), = check_batch(pb, "example_trim")
    csum = g['a_b_csum']
    bound = 2 * csum.shape[0] * 2.0 ** -53 * np.abs(csum[np.isfinite(csum)]).max()
    print("example_trim: %d rows, min slack %.3e (bound -%.3e), median %.4f, del_penalty %.4f" % (
        len(sl), sl.min(), bound, float(np.median(sl)), g['del_penalty']))
    assert sl.min() >= -bound


def test_argument_errors_queue_nothing():
    import ctypes
    import torch
    from svx import _lib
    from svx.vecalign import dp_utils
    # ---- the tile sweep keeps no cost array
    case = [c for c in dp_ref.Z_STRAIGHT if c[0] == "a5_W40"][0]
    pairs = dp_ref.z_straight_pairs(case)
    pb = dp_utils.PreparedBatch([(to_dev(p[0], "f32"), to_dev(p[1], "f32")) for p in pairs], dp_ref.z_straight_types(case), dp_ref.FRAC, 40, 0,
                                dp_ref.SAMPLE, dp_ref.NSAMP, rngs=[np.random.RandomState(p[4]) for p in pairs],
                                norms=[(p[2], p[3]) for p in pairs], search="straight")
    pb.run()
    with pytest.raises(_lib.SvxError, match="tile sweep, which keeps no cost array"):
        pb.row_slack()
    # ---- a wrong pair count, null and misaligned arguments (on a call that could be measured)
    v0, v1 = make_pair(60, 50, 4, 32, seed=5)
    ok = dp_utils.PreparedBatch([(to_dev(v0, "f32"), to_dev(v1, "f32"))], alignment_types(5), 0.2, 7, 300, 20000, 100,
                                rngs=[np.random.RandomState(1)])
    ok.run()
    ctx = ok.ctx
    buf = torch.zeros(256, dtype=torch.float64, device="cuda")
    summ = torch.zeros(16, dtype=torch.int32, device="cuda")
    ptrs = (ctypes.c_void_p * 2)(buf.data_ptr(), buf.data_ptr())
    vp = ctypes.c_void_p
    for args, text in (((ptrs, vp(summ.data_ptr()), 2), "2 pairs given, the last call had 1"),
                       ((None, vp(summ.data_ptr()), 1), "null argument"),
                       ((ptrs, vp(0), 1), "null argument"),
                       ((ptrs, vp(summ.data_ptr() + 4), 1), "16-byte aligned"),
                       ((ptrs, vp(summ.data_ptr()), -1), "negative n_pairs")):
        rc = ctx.lib.svx_row_slack(ctx.h, *args)
        assert rc != 0 and text in ctx.lib.svx_last_error(ctx.h).decode(), (text, ctx.lib.svx_last_error(ctx.h).decode())
    ctx.sync()
    assert not buf.cpu().numpy().any() and not summ.cpu().numpy().any()
    # ---- no earlier call: a context of its own
    fresh = _lib.Context(ctx.device)
    rc = fresh.lib.svx_row_slack(fresh.h, ptrs, vp(summ.data_ptr()), 1)
    assert rc != 0 and "no earlier svx_align_batch" in fresh.lib.svx_last_error(fresh.h).decode()
