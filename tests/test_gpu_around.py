"""Band search around a prior alignment on the GPU (svx_align_around, svx_time_prior; include/svx.h) against the CPU
oracle's level-0 refinement started from the same prior (tests/around_ref.py).  Tolerances are those of
tests/test_gpu_pipeline.py: identical spans, scores within 1e-4, integer views exact, costs 4e-6, sums 1e-4 (1 + max)."""
import ctypes
import os
import shutil

import numpy as np
import pytest

from around_ref import (SVX_ERR_ARG, SVX_ERR_EXTEND, SVX_ERR_PATH, SVX_ERR_TRACEBACK, around_stack, block_deletion_pair,
                        ingest_ref, lengths_to_alignments, time_prior_ref)
from synth import alignment_types, make_pair, round_bf16

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-4
TRIM = os.path.join(os.path.dirname(__file__), "golden", "example_trim")
TYPES5 = alignment_types(5)


def to_dev(v, dt):
    import torch
    t = torch.from_numpy(v).cuda()
    return {"f32": t, "f16": t.half(), "bf16": t.bfloat16()}[dt]


def storage(v, dt):
    """The float32 values the device sees for storage type dt."""
    return {"f32": lambda a: a, "f16": lambda a: a.astype(np.float16).astype(np.float32), "bf16": round_bf16}[dt](v)


def batch(docs, priors, W=7, seeds=None, types=TYPES5, dt="f32", frames=None, search="around"):
    from svx.vecalign import dp_utils
    seeds = list(range(900, 900 + len(docs))) if seeds is None else seeds
    kw = dict(priors=priors) if search == "around" else {}
    return dp_utils.PreparedBatch([(to_dev(a, dt), to_dev(b, dt)) for a, b in docs], types, 0.2, W, 300, 20000, 100,
                                  rngs=[np.random.RandomState(s) for s in seeds], search=search, frames=frames, **kw)


def outputs(pb):
    """(info, align, scores) as they stand on the device, failed pairs included."""
    pb.ctx.sync()
    return pb.info.cpu().numpy(), pb.align.cpu().numpy(), pb.scores.cpu().numpy()


def check_result(res, ref):
    assert res[0] == ref['final_alignments']
    assert np.abs(res[1] - ref['alignment_scores']).max() < SCORE_TOL


def check_views(got, ref):
    assert got['searchpath'] == [tuple(p) for p in ref['searchpath']]
    assert np.array_equal(got['b_offset'], ref['b_offset']) and np.array_equal(got['new_b_offset'], ref['new_b_offset'])
    a, b = got['a_b_costs'], ref['a_b_costs']
    assert a.shape == b.shape and np.array_equal(np.isinf(a), np.isinf(b))
    assert np.abs(a[np.isfinite(a)] - b[np.isfinite(b)]).max() < 4e-6
    assert np.array_equal(got['a_b_xp'], ref['a_b_xp']) and np.array_equal(got['a_b_yp'], ref['a_b_yp'])
    fin = np.isfinite(ref['a_b_csum'])
    assert np.array_equal(np.isfinite(got['a_b_csum']), fin)
    assert np.abs(got['a_b_csum'][fin] - ref['a_b_csum'][fin]).max() < 1e-4 * (1 + ref['a_b_csum'][fin].max())


def split_prior(n, m, blocks):
    """`blocks` blocks that cut both documents at the same fractions."""
    xs = [n * i // blocks for i in range(blocks + 1)]
    ys = [m * i // blocks for i in range(blocks + 1)]
    return [(list(range(xs[i], xs[i + 1])), list(range(ys[i], ys[i + 1]))) for i in range(blocks)]


# ---------------------------------------------------------------------------------------------- 1
def test_single_block_and_empty_prior_are_the_straight_search():
    v0, v1 = make_pair(200, 190, 4, 32, seed=5, deletions=3)
    ref_pb = batch([(v0, v1)], None, W=16, seeds=[21], search="straight")
    ref_pb.run()
    want = outputs(ref_pb)
    want_views = ref_pb.level_stack(0, 0)
    for prior in ([(list(range(200)), list(range(190)))], []):
        pb = batch([(v0, v1)], [prior], W=16, seeds=[21])
        pb.run()
        for g, w in zip(outputs(pb), want):
            assert np.array_equal(g, w)
        views = pb.level_stack(0, 0)
        assert set(views) == set(want_views)
        for k in want_views:
            if isinstance(want_views[k], np.ndarray):
                assert np.array_equal(views[k], want_views[k]), k
            else:
                assert views[k] == want_views[k], k


# ---------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_level0_identity(orc, dt):
    """The prior is the oracle's dense 1-1 alignment of the same level: the result is vecalign()'s own (L = 0)."""
    v0, v1 = make_pair(120, 97, 4, 32, seed=3, deletions=6)
    v0, v1 = storage(v0, dt), storage(v1, dt)
    ref = orc.vecalign(v0.copy(), v1.copy(), TYPES5, 0.2, 7, 300, 20000, 100, rng=np.random.RandomState(11))
    assert len(ref) == 1
    pb = batch([(v0, v1)], [ref[0]['alignments']], seeds=[11], dt=dt)
    pb.run()
    check_result(pb.results()[0], ref[0])
    views = pb.level_stack(0, 0)
    assert views['searchpath'] == [tuple(p) for p in ref[0]['searchpath']]
    assert np.array_equal(views['b_offset'], ref[0]['b_offset'])


# ---------------------------------------------------------------------------------------------- 3
def second_frames(starts, dur=12000):
    s = np.asarray(starts, np.int64)
    return np.stack([s, s + dur], axis=1)


def test_block_deletion_through_the_time_prior(orc):
    v0, v1, src = block_deletion_pair(seed=0)
    F0, F1 = second_frames(16000 * np.arange(300)), second_frames(16000 * src + 8000)
    pb = batch([(v0, v1)], [None], seeds=[11], frames=[(F0, F1)])
    pb.time_prior(20 * 16000, 8000)
    pb.run()                                    # chained on the stream: no host copy in between
    res = pb.results()[0]
    rows, info = (x.cpu().numpy() for x in pb.prior_own[0])
    want, code = time_prior_ref(F0, F1, 20 * 16000, 8000)
    assert code == 0 and info.tolist() == [len(want), 0] and np.array_equal(rows[:len(want)], want)
    assert len(want) == 15 and want[:, 1].tolist() == [20] * 15
    ref = around_stack(orc, v0, v1, TYPES5, 7, 11, lengths_to_alignments(want[:, [1, 3]]))
    check_result(res, ref)
    check_views(pb.level_stack(0, 0), ref)


def test_time_prior_d1024_bf16(orc):
    """The 16-bit band-cost instantiation (d = 1024) around a time prior."""
    v0, v1 = make_pair(300, 280, 4, 1024, seed=8, deletions=20)
    v0, v1 = round_bf16(v0), round_bf16(v1)
    F0, F1 = second_frames(16000 * np.arange(300)), second_frames((16000 * np.arange(280) * 300) // 280)
    pb = batch([(v0, v1)], [None], seeds=[12], dt="bf16", frames=[(F0, F1)])
    pb.time_prior(20 * 16000, 0)
    pb.run()
    res = pb.results()[0]
    want, code = time_prior_ref(F0, F1, 20 * 16000, 0)
    assert code == 0 and np.array_equal(pb.prior_own[0][0].cpu().numpy()[:len(want)], want)
    check_result(res, around_stack(orc, v0, v1, TYPES5, 7, 12, lengths_to_alignments(want[:, [1, 3]])))


# ---------------------------------------------------------------------------------------------- 4
def test_ragged_batch_with_failed_priors(orc):
    import torch
    sizes = [(300, 280), (211, 333), (120, 97), (64, 1)]
    docs = [make_pair(n, m, 4, 32, seed=40 + i) for i, (n, m) in enumerate(sizes)]
    p0 = split_prior(300, 280, 15)
    p3 = [(list(range(32)), []), (list(range(32, 64)), [0])]
    too_long = torch.tensor([[0, 100, 0, 100], [100, 112, 100, 100]], dtype=torch.int32).cuda()     # 212 = n + 1
    failed = (torch.tensor([[0, 60, 0, 50], [60, 60, 50, 47]], dtype=torch.int32).cuda(),
              torch.tensor([2, SVX_ERR_TRACEBACK], dtype=torch.int32).cuda())
    priors = [p0, (too_long, torch.tensor([2, 0], dtype=torch.int32).cuda()), failed, p3]
    pb = batch(docs, priors)
    pb.run()
    info, align, scores = outputs(pb)
    assert info[1].tolist() == [0, SVX_ERR_EXTEND] and info[2].tolist() == [0, SVX_ERR_TRACEBACK]
    for i in (1, 2):   # a failed pair writes its code and nothing else
        assert not align[pb.offs[i]:pb.offs[i + 1]].any() and not scores[pb.offs[i]:pb.offs[i + 1]].any()
    for i, prior in ((0, p0), (3, p3)):
        n, m = sizes[i]
        assert info[i, 1] == 0
        o, cnt = int(pb.offs[i]), int(info[i, 0])
        ref = around_stack(orc, docs[i][0], docs[i][1], TYPES5, 7, 900 + i, prior)
        from svx.vecalign.dp_utils import rows_to_alignments
        check_result((rows_to_alignments(align[o:o + cnt]), scores[o:o + cnt]), ref)
        alone = batch([docs[i]], [prior], seeds=[900 + i])
        alone.run()
        ainfo, aalign, ascores = outputs(alone)
        assert ainfo[0].tolist() == info[i].tolist()
        assert np.array_equal(aalign[:cnt], align[o:o + cnt]) and np.array_equal(ascores[:cnt], scores[o:o + cnt])


# ---------------------------------------------------------------------------------------------- 5
def test_two_passes_on_the_device(orc):
    """A coarse-to-fine pass with 1-1 alignments only, then the full types around it: the first batch's output buffers
    are the second's prior, read on the device."""
    from svx.vecalign import dp_utils
    v0, v1 = make_pair(300, 280, 4, 32, seed=51, deletions=8)
    first = dp_utils.PreparedBatch([(to_dev(v0, "f32"), to_dev(v1, "f32"))], [(1, 1)], 0.2, 7, 100, 20000, 100,
                                   rngs=[np.random.RandomState(61)])
    second = batch([(v0, v1)], first, seeds=[62])
    first.run()
    second.run()
    ref1 = orc.vecalign(v0.copy(), v1.copy(), [(1, 1)], 0.2, 7, 100, 20000, 100, rng=np.random.RandomState(61))
    assert len(ref1) > 1
    assert first.results()[0][0] == ref1[0]['final_alignments']
    ref2 = around_stack(orc, v0, v1, TYPES5, 7, 62, ref1[0]['final_alignments'])
    check_result(second.results()[0], ref2)
    check_views(second.level_stack(0, 0), ref2)


# ---------------------------------------------------------------------------------------------- 6
def test_pipeline_does_not_change_results():
    from svx import _lib
    docs = [make_pair(150 + 17 * i, 160 - 9 * i, 4, 32, seed=70 + i, deletions=i) for i in range(8)]
    priors = [split_prior(a.shape[1], b.shape[1], 1 + i) for i, (a, b) in enumerate(docs)]
    ctx = _lib.context()

    def sequence():
        a, b = batch(docs, priors), batch(docs[:3], priors[:3], seeds=[5, 6, 7])
        for pb in (a, b, a):
            pb.run()
        a.flush()
        return [x.copy() for pb in (a, b) for x in outputs(pb)]
    try:
        ctx.set_pipeline(False)
        plain = sequence()
        ctx.set_pipeline(True)
        piped = sequence()
    finally:
        ctx.set_pipeline(False)
    assert (plain[0][:, 1] == 0).all() and (plain[0][:, 0] > 0).all()
    for x, y in zip(plain, piped):
        assert x.tobytes() == y.tobytes()


# ---------------------------------------------------------------------------------------------- 7
def run_time_prior(frames, window, lag, slack=0):
    """svx_time_prior on bare frames -> [(rows [cap, 4], info [2])] per pair (cap = n + m + slack)."""
    import torch
    from svx import _lib
    ctx = _lib.context()
    ctx.use_current_stream()
    n = len(frames)
    cp, cf, co = (_lib.Pair * n)(), (_lib.Frames * n)(), (_lib.Prior * n)()
    keep = []
    for i, (f0, f1) in enumerate(frames):
        d0 = torch.from_numpy(np.asarray(f0, np.int32).reshape(-1, 2)).cuda()
        d1 = torch.from_numpy(np.asarray(f1, np.int32).reshape(-1, 2)).cuda()
        cap = len(d0) + len(d1) + slack
        rows = torch.full((max(1, cap), 4), -7, dtype=torch.int32).cuda()
        info = torch.full((2,), -7, dtype=torch.int32).cuda()
        cp[i].n, cp[i].m = len(d0), len(d1)
        cf[i].src, cf[i].tgt = d0.data_ptr(), d1.data_ptr()
        co[i].rows, co[i].info, co[i].cap = rows.data_ptr(), info.data_ptr(), cap
        keep.append((d0, d1, rows, info))
    ctx.check(ctx.lib.svx_time_prior(ctx.h, cp, cf, n, int(window), int(lag), co))
    ctx.sync()
    return [(k[2].cpu().numpy(), k[3].cpu().numpy()) for k in keep]


def fr(starts):
    return [(s, s + 5) for s in starts]


def test_time_prior_edge_cases():
    rng = np.random.default_rng(3)
    big = (np.sort(rng.integers(0, 400000, 700)), np.sort(rng.integers(0, 400000, 613)))
    cases = [
        (fr([50]), fr([10, 20, 130, 990]), 100, 0),                              # n = 1
        (fr([0, 10, 250, 251, 600]), fr([300]), 100, 0),                         # m = 1
        (fr([1, 2, 3, 99]), fr([0, 50, 98]), 100, 0),                            # all in one window
        (fr([300, 310, 500]), fr([0, 90, 305, 410, 520, 900, 1500]), 100, 0),    # target-only windows at start, middle, end
        (fr([0, 90, 305, 410, 520, 900, 1500]), fr([300, 310, 500]), 100, 0),    # source-only windows
        (fr([100, 200, 300]), fr([0, 130, 260, 390]), 100, -70),                 # negative lag, starts on window edges
        (fr([100, 200, 300]), fr([0, 130, 260, 390]), 100, 200),                 # lag past the first starts: clamped at 0
        (fr(big[0]), fr(big[1]), 4000, 1234),                                    # more than one stretch of 256 per side
        (fr([5, 4, 9]), fr([1, 2]), 100, 0),                                     # decreasing source starts
        (fr([1, 2]), fr([7, 7, 3]), 100, 0),                                     # decreasing target starts
    ]
    got = run_time_prior([(c[0], c[1]) for c in cases[:5]], 100, 0)              # a ragged batch in one call
    got += [run_time_prior([(c[0], c[1])], c[2], c[3], slack=2)[0] for c in cases[5:]]
    for (f0, f1, window, lag), (rows, info) in zip(cases, got):
        want, code = time_prior_ref(f0, f1, window, lag)
        assert info.tolist() == [len(want), code]
        assert np.array_equal(rows[:len(want)], want)
        assert (rows[len(want):] == -7).all()       # nothing past the rows is touched
        if code == 0:
            assert rows[:len(want), 1].sum() == len(f0) and rows[:len(want), 3].sum() == len(f1)
    assert [int(g[1][1]) for g in got[-2:]] == [SVX_ERR_PATH, SVX_ERR_PATH]


# ---------------------------------------------------------------------------------------------- 8
def test_argument_errors_queue_nothing(orc):
    from svx import _lib
    v0, v1 = make_pair(120, 97, 4, 32, seed=3, deletions=6)
    prior = split_prior(120, 97, 4)
    ref = around_stack(orc, v0, v1, TYPES5, 7, 33, prior)
    ctx = _lib.context()

    def expect_arg(pb, call=None):
        pb.align.fill_(-1)
        pb.info.fill_(-1)
        with pytest.raises(_lib.SvxError) as e:
            call() if call else pb.run()
        assert e.value.code == SVX_ERR_ARG and len(str(e.value)) > 10
        info, align, _ = outputs(pb)
        assert (info == -1).all() and (align == -1).all()       # nothing was queued
        good = batch([(v0, v1)], [prior], seeds=[33])           # the context still works
        good.run()
        check_result(good.results()[0], ref)

    expect_arg(batch([(v0, v1)], [prior], W=33, seeds=[33]))                    # band of 66 cells
    pb = batch([(v0, v1)], [prior], seeds=[33])
    pb.prm.search_mode = _lib.SVX_SEARCH_STRAIGHT
    expect_arg(pb)
    pb = batch([(v0, v1)], [None], seeds=[33])                                   # the prior is the pair's own output
    pb.cpriors[0].rows, pb.cpriors[0].info = pb.cpairs[0].align, pb.cpairs[0].info
    expect_arg(pb)
    pb = batch([(v0, v1)], [prior], seeds=[33])
    expect_arg(pb, lambda: ctx.check(ctx.lib.svx_align_around(ctx.h, ctypes.byref(pb.prm), pb.cpairs, None, 1)))
    # svx_align_batch keeps rejecting the new mode
    pb = batch([(v0, v1)], None, seeds=[33], search="straight")
    pb.prm.search_mode = _lib.SVX_SEARCH_AROUND
    expect_arg(pb)


# ---------------------------------------------------------------------------------------------- 9
def build_tree(root):
    stem = "doc0"
    for lang in ("en", "de"):
        for sub in ("seg", "cat", "emb"):
            os.makedirs(os.path.join(root, sub, lang), exist_ok=True)
        shutil.copy(os.path.join(TRIM, f"segments_{lang}.txt"), os.path.join(root, "seg", lang, f"{stem}_{lang}.txt"))
        shutil.copy(os.path.join(TRIM, f"cat_segs_{lang}.txt"), os.path.join(root, "cat", lang, f"{stem}_{lang}.txt"))
        shutil.copy(os.path.join(TRIM, f"embeds_{lang}.f16"), os.path.join(root, "emb", lang, f"{stem}_{lang}.embed"))
    os.makedirs(os.path.join(root, "ign", "en-de"), exist_ok=True)
    for side in ("src", "tgt"):
        shutil.copy(os.path.join(TRIM, f"ignore_{side}.txt"), os.path.join(root, "ign", "en-de", f"{stem}_en-{stem}_de.{side}.txt"))
    with open(os.path.join(root, "metadata.tsv"), "w") as f:
        f.write(f"/audio/{stem}_en.ogg\t/audio/{stem}_de.ogg\n")


@pytest.mark.parametrize("prior", ["dir", "time"])
def test_seg_align_cli_around(orc, tmp_path, monkeypatch, prior):
    from svx.seg_align import align as A
    from svx.seg_align.align import pair_rng
    from svx.utils.file_utils import read_alignments, read_alignments_with_score, read_segments
    from svx.vecalign import dp_utils
    seen = []
    real = dp_utils.PreparedBatch

    class Capture(real):
        def __init__(self, pairs, types, frac, w2, *a, **k):
            seen.append(([(v0.float().cpu().numpy().copy(), v1.float().cpu().numpy().copy()) for v0, v1 in pairs], list(types), w2, k.get("search")))
            super().__init__(pairs, types, frac, w2, *a, **k)

    monkeypatch.setattr(dp_utils, "PreparedBatch", Capture)
    root, out = str(tmp_path / "data"), str(tmp_path / "out")
    build_tree(root)
    argv = [os.path.join(root, "metadata.tsv"), out, "--src_lang", "en", "--tgt_lang", "de", "--seg_dir", os.path.join(root, "seg"),
            "--concat_dir", os.path.join(root, "cat"), "--embed_dir", os.path.join(root, "emb"),
            "--ign_indices_dir", os.path.join(root, "ign"), "--fp16_embed", "--seed", "3", "--mode", "around"]
    if prior == "dir":
        os.makedirs(os.path.join(root, "prior", "en-de"))
        shutil.copy(os.path.join(TRIM, "expected_seed0.txt"), os.path.join(root, "prior", "en-de", "doc0_en-doc0_de.txt"))
        argv += ["--prior_dir", os.path.join(root, "prior")]
    else:
        argv += ["--prior", "time", "--prior_window", "20", "--prior_lag", "0.5"]
    A.main(argv)
    assert len(seen) == 1 and seen[0][3] == "around"
    (v0, v1), = seen[0][0]
    types, w2 = seen[0][1], seen[0][2]
    assert w2 == int(np.ceil((6 - 1) / 2.0)) + 5       # the reference-mode width of the default -a 6
    n, m = v0.shape[1], v1.shape[1]
    if prior == "dir":
        rows = dp_utils.prior_rows_from_alignments(read_alignments(os.path.join(TRIM, "expected_seed0.txt")))
    else:
        rows, code = time_prior_ref(read_segments(os.path.join(TRIM, "segments_en.txt")), read_segments(os.path.join(TRIM, "segments_de.txt")),
                                    20 * 16000, 8000)
        assert code == 0 and len(rows) > 1
    lengths, code = ingest_ref(rows, len(rows), n, m)
    assert code == 0
    ref = around_stack(orc, v0, v1, types, w2, pair_rng(3, 0), lengths_to_alignments(lengths))
    got = read_alignments_with_score(os.path.join(out, "en-de", "doc0_en-doc0_de.txt"))
    assert [(list(a), list(b)) for a, b, _ in got] == [(list(a), list(b)) for a, b in ref['final_alignments']]
    assert max(abs(g[2] - s) for g, s in zip(got, ref['alignment_scores'])) < SCORE_TOL + 5e-7  # (the file has 6 decimals)

