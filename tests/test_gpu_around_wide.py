"""Wide bands around a prior on the GPU (include/svx.h: SVX_SEARCH_AROUND_WIDE, svx_prior_width): the tile sweep of the
wide straight search laid around a prior's search path, against the CPU oracle's refinement around the same prior
(tests/around_ref.py).  Tolerances are those of tests/test_gpu_around.py: identical spans, scores within 1e-4, integer
views exact, sums 1e-4 (1 + max).  The tile sweep stores lattice nodes only (include/svx.h: svx_level_view), so the node
arrays are compared on the band cells that are nodes of the lattice."""
import functools
import os
import shutil

import numpy as np
import pytest

from around_ref import (SVX_ERR_ARG, SVX_ERR_EXTEND, SVX_ERR_PATH, SVX_ERR_TRACEBACK, around_stack, block_deletion_pair,
                        block_prior, ingest_ref, lengths_to_alignments, time_prior_ref)
from dp_ref import straight_stack
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


def batch(docs, priors, W, seeds=None, types=TYPES5, dt="f32", frames=None, search="around_wide"):
    from svx.vecalign import dp_utils
    seeds = list(range(900, 900 + len(docs))) if seeds is None else seeds
    kw = dict(priors=priors) if search in ("around", "around_wide") else {}
    return dp_utils.PreparedBatch([(to_dev(a, dt), to_dev(b, dt)) for a, b in docs], types, 0.2, W, 300, 20000, 100,
                                  rngs=[np.random.RandomState(s) for s in seeds], search=search, frames=frames, **kw)


def outputs(pb):
    """(info, align, scores) as they stand on the device, failed pairs included."""
    pb.ctx.sync()
    return pb.info.cpu().numpy(), pb.align.cpu().numpy(), pb.scores.cpu().numpy()


def check_result(res, ref):
    assert res[0] == ref['final_alignments']
    assert np.abs(res[1] - ref['alignment_scores']).max() < SCORE_TOL


def lattice_mask(nbo, B, size0, size1):
    yy = np.arange(B)[None, :] + np.asarray(nbo)[:, None]
    xx = np.arange(len(nbo))[:, None] - yy
    return (0 <= xx) & (xx <= size0) & (0 <= yy) & (yy <= size1)


def check_wide_views(got, ref):
    """The view of the tile sweep: no a_b_costs; path and offsets exact; csum and back-pointers on lattice nodes."""
    assert 'a_b_costs' not in got
    assert got['searchpath'] == [tuple(p) for p in ref['searchpath']]
    assert np.array_equal(got['b_offset'], ref['b_offset']) and np.array_equal(got['new_b_offset'], ref['new_b_offset'])
    assert got['a_b_csum'].shape == ref['a_b_csum'].shape
    keep = lattice_mask(ref['new_b_offset'], ref['a_b_csum'].shape[1], ref['size0'], ref['size1'])
    fin = np.isfinite(ref['a_b_csum']) & keep
    assert fin.any() and np.array_equal(np.isfinite(got['a_b_csum']) & keep, fin)
    assert np.abs(got['a_b_csum'][fin] - ref['a_b_csum'][fin]).max() < 1e-4 * (1 + ref['a_b_csum'][fin].max())
    for k in ('a_b_xp', 'a_b_yp'):
        assert np.array_equal(np.where(keep, got[k], 0), np.where(keep, ref[k], 0)), k


def same_views(a, b, lattice_only):
    """Two level views bit for bit; with lattice_only the node arrays on lattice nodes (the rest is unspecified)."""
    assert set(a) == set(b)
    keep = None
    if lattice_only:
        keep = lattice_mask(b['new_b_offset'], b['a_b_csum'].shape[1], b['size0'], b['size1'])
    for k in b:
        if isinstance(b[k], np.ndarray):
            if keep is not None and k in ('a_b_csum', 'a_b_xp', 'a_b_yp'):
                assert np.array_equal(a[k][keep], b[k][keep]), k
            else:
                assert np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def split_prior(n, m, blocks):
    """`blocks` blocks that cut both documents at the same fractions."""
    xs = [n * i // blocks for i in range(blocks + 1)]
    ys = [m * i // blocks for i in range(blocks + 1)]
    return [(list(range(xs[i], xs[i + 1])), list(range(ys[i], ys[i + 1]))) for i in range(blocks)]


# ---------------------------------------------------------------------------------------------- 1
def test_single_block_and_empty_prior_are_the_wide_straight_search():
    v0, v1 = make_pair(200, 190, 4, 32, seed=5, deletions=3)
    ref_pb = batch([(v0, v1)], None, W=40, seeds=[21], search="straight")
    ref_pb.run()
    want = outputs(ref_pb)
    want_views = ref_pb.level_stack(0, 0)
    assert 'a_b_costs' not in want_views           # the tile sweep
    for prior in ([(list(range(200)), list(range(190)))], []):
        pb = batch([(v0, v1)], [prior], W=40, seeds=[21])
        pb.run()
        for g, w in zip(outputs(pb), want):
            assert np.array_equal(g, w)
        same_views(pb.level_stack(0, 0), want_views, lattice_only=True)


# ---------------------------------------------------------------------------------------------- 2
@functools.lru_cache(maxsize=None)
def deletion_case(a, dt, d, step):
    """block_deletion_pair(seed=0) with a - 1 overlap layers in storage dt, a block prior, its covering width and the
    oracle's refinement around it (computed once per case)."""
    import oracle as orc
    from svx.vecalign.dp_utils import prior_rows_from_alignments, prior_width
    v0, v1, src = block_deletion_pair(K=a - 1, d=d, seed=0)
    v0, v1 = storage(v0, dt), storage(v1, dt)
    prior = block_prior(src, 300, step)
    W = prior_width(prior_rows_from_alignments(prior), 300, 180)
    return v0, v1, prior, W, around_stack(orc, v0, v1, alignment_types(a), W, 11, prior)


def run_deletion_case(orc, a, dt, d, step, band):
    v0, v1, prior, W, ref = deletion_case(a, dt, d, step)
    assert 2 * W == band
    pb = batch([(v0, v1)], [prior], W=W, seeds=[11], types=alignment_types(a), dt=dt)
    pb.run()
    check_result(pb.results()[0], ref)
    check_wide_views(pb.level_stack(0, 0), ref)


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("a", [5, 6, 7])       # <= 10 types on 8 layers, <= 16 on 12 (the LDS-resident shapes), 21: k_band_tiles_gen
@pytest.mark.parametrize("step,band", [(60, 122), (150, 202)])
def test_block_deletion_pair_at_the_covering_width(orc, step, band, a, dt):
    run_deletion_case(orc, a, dt, 32, step, band)


def test_block_deletion_pair_d1024_bf16(orc):
    run_deletion_case(orc, 5, "bf16", 1024, 60, 122)


# ---------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("case", ["64x1", "lead_y", "lead_x"])
def test_lattice_borders(orc, case):
    """Paths that hug x = 0, y = 0 and y = m."""
    if case == "64x1":
        n, m, prior = 64, 1, [(list(range(32)), []), (list(range(32, 64)), [0])]
    elif case == "lead_y":   # 40 target segments deleted first: the path runs up x = 0
        n, m, prior = 97, 120, [([], list(range(40))), (list(range(97)), list(range(40, 120)))]
    else:                    # 40 source segments deleted first: the path runs along y = 0
        n, m, prior = 97, 120, [(list(range(40)), []), (list(range(40, 97)), list(range(120)))]
    v0, v1 = make_pair(n, m, 4, 32, seed=43, deletions=0 if m == 1 else 4)
    pb = batch([(v0, v1)], [prior], W=33, seeds=[17])
    pb.run()
    ref = around_stack(orc, v0, v1, TYPES5, 33, 17, prior)
    check_result(pb.results()[0], ref)
    check_wide_views(pb.level_stack(0, 0), ref)


def random_prior(rng, n, m, blocks):
    """Random cut points on both sides; equal neighbours give deletion rows, rows with both lengths 0 are dropped."""
    xs = np.sort(np.concatenate([[0, n], rng.integers(0, n + 1, blocks - 1)]))
    ys = np.sort(np.concatenate([[0, m], rng.integers(0, m + 1, blocks - 1)]))
    out = [(list(range(xs[i], xs[i + 1])), list(range(ys[i], ys[i + 1]))) for i in range(blocks)]
    return [r for r in out if r[0] or r[1]]


def test_random_priors_in_one_batch(orc):
    """Six pairs of different sizes with random priors of 2 .. 12 blocks (steep and flat slants, deletion runs) in one
    sweep of 80 cells, whether or not the band covers the blocks."""
    rng = np.random.default_rng(5)
    sizes = [(150, 130), (97, 211), (260, 64), (33, 170), (128, 128), (201, 95)]
    docs = [make_pair(n, m, 4, 32, seed=80 + i, deletions=min(5, m // 20)) for i, (n, m) in enumerate(sizes)]
    priors = [random_prior(rng, n, m, 2 + 2 * i) for i, (n, m) in enumerate(sizes)]
    assert any(not x or not y for p in priors for x, y in p)       # deletion rows are among them
    pb = batch(docs, priors, W=40)
    pb.run()
    res = pb.results()
    for i in range(len(docs)):
        ref = around_stack(orc, docs[i][0], docs[i][1], TYPES5, 40, 900 + i, priors[i])
        check_result(res[i], ref)
        check_wide_views(pb.level_stack(i, 0), ref)


@pytest.mark.parametrize("case", ["m2o50", "a10"])
def test_general_shape_halo_around_slants(orc, case):
    """The general tile shape's halo wait (every band tile in rows I - ceil(Hx / 32) .. I, columns J - ceil(Hy / 32) .. J)
    around a steep many-to-many slant, a deletion run and a flat slant: steps longer than a tile side with int32
    back-pointers (many-to-one 50), and 45 types with steps of 9."""
    from dp_ref import many_to_one_types
    if case == "m2o50":
        n, m, K0, K1, types = 420, 130, 50, 1, many_to_one_types(50)
        prior = [(list(range(200)), list(range(30))), (list(range(200, 260)), []), (list(range(260, 420)), list(range(30, 130)))]
    else:
        n, m, K0, K1, types = 300, 290, 9, 9, alignment_types(10)
        prior = [(list(range(40)), list(range(120))), ([], list(range(120, 150))), (list(range(40, 300)), list(range(150, 290)))]
    v0, v1 = make_pair(n, m, max(K0, K1), 64, 600 + n, deletions=0 if case == "m2o50" else 9)
    v0, v1 = np.ascontiguousarray(v0[:K0]), np.ascontiguousarray(v1[:K1])
    pb = batch([(v0, v1)], [prior], W=40, seeds=[41], types=types)
    pb.run()
    ref = around_stack(orc, v0, v1, types, 40, 41, prior)
    check_result(pb.results()[0], ref)
    check_wide_views(pb.level_stack(0, 0), ref)


# ---------------------------------------------------------------------------------------------- 4
RAGGED = [(300, 280), (211, 333), (120, 97), (64, 1)]


def ragged_priors(third):
    """-> (docs, priors): pair 0 and 3 good, pair 1 SVX_ERR_EXTEND, pair 2 SVX_ERR_PATH or a propagated info[1]."""
    import torch
    docs = [make_pair(n, m, 4, 32, seed=40 + i) for i, (n, m) in enumerate(RAGGED)]
    p0 = split_prior(300, 280, 15)
    p3 = [(list(range(32)), []), (list(range(32, 64)), [0])]
    too_long = torch.tensor([[0, 100, 0, 100], [100, 112, 100, 100]], dtype=torch.int32).cuda()     # 212 = n + 1
    if third == "path":
        bad = (torch.tensor([[0, 60, 0, 50], [60, 0, 50, 0]], dtype=torch.int32).cuda(), torch.tensor([2, 0], dtype=torch.int32).cuda())
    else:
        bad = (torch.tensor([[0, 60, 0, 50], [60, 60, 50, 47]], dtype=torch.int32).cuda(),
               torch.tensor([2, SVX_ERR_TRACEBACK], dtype=torch.int32).cuda())
    return docs, [p0, (too_long, torch.tensor([2, 0], dtype=torch.int32).cuda()), bad, p3]


@pytest.mark.parametrize("third", ["path", "propagated"])
def test_ragged_batch_with_failed_priors(orc, third):
    from svx.vecalign.dp_utils import rows_to_alignments
    docs, priors = ragged_priors(third)
    pb = batch(docs, priors, W=33)
    pb.run()
    info, align, scores = outputs(pb)
    assert info[1].tolist() == [0, SVX_ERR_EXTEND]
    assert info[2].tolist() == [0, SVX_ERR_PATH if third == "path" else SVX_ERR_TRACEBACK]
    for i in (1, 2):   # a failed pair writes its code and nothing else
        assert not align[pb.offs[i]:pb.offs[i + 1]].any() and not scores[pb.offs[i]:pb.offs[i + 1]].any()
    for i in (0, 3):
        assert info[i, 1] == 0
        o, cnt = int(pb.offs[i]), int(info[i, 0])
        ref = around_stack(orc, docs[i][0], docs[i][1], TYPES5, 33, 900 + i, priors[i])
        check_result((rows_to_alignments(align[o:o + cnt]), scores[o:o + cnt]), ref)
        alone = batch([docs[i]], [priors[i]], W=33, seeds=[900 + i])
        alone.run()
        ainfo, aalign, ascores = outputs(alone)
        assert ainfo[0].tolist() == info[i].tolist()
        assert np.array_equal(aalign[:cnt], align[o:o + cnt]) and np.array_equal(ascores[:cnt], scores[o:o + cnt])


# ---------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("W", [7, 32])
def test_bands_of_at_most_64_cells_are_the_around_search(W):
    docs = [make_pair(150 + 17 * i, 160 - 9 * i, 4, 32, seed=70 + i, deletions=i) for i in range(3)]
    priors = [split_prior(a.shape[1], b.shape[1], 1 + 2 * i) for i, (a, b) in enumerate(docs)]
    narrow, wide = batch(docs, priors, W=W, search="around"), batch(docs, priors, W=W)
    narrow.run()
    want = outputs(narrow)
    want_views = [narrow.level_stack(i, 0) for i in range(3)]
    wide.run()
    for g, w in zip(outputs(wide), want):
        assert g.tobytes() == w.tobytes()
    for i in range(3):
        views = wide.level_stack(i, 0)
        assert 'a_b_costs' in views
        same_views(views, want_views[i], lattice_only=False)


# ---------------------------------------------------------------------------------------------- 6
def test_two_passes_on_the_device(orc):
    """A straight 1-1 pass, then the full types in a band of 66 cells around it: the first batch's output buffers are
    the second's prior, read on the device."""
    v0, v1 = make_pair(300, 280, 4, 32, seed=51, deletions=8)
    first = batch([(v0, v1)], None, W=7, seeds=[61], types=[(1, 1)], search="straight")
    second = batch([(v0, v1)], first, W=33, seeds=[62])
    first.run()
    second.run()
    ref1 = straight_stack(orc, v0, v1, [(1, 1)], 7, 61)
    assert first.results()[0][0] == ref1['final_alignments']
    ref2 = around_stack(orc, v0, v1, TYPES5, 33, 62, ref1['final_alignments'])
    check_result(second.results()[0], ref2)
    check_wide_views(second.level_stack(0, 0), ref2)


# ---------------------------------------------------------------------------------------------- 7
def test_pipeline_does_not_change_results():
    from svx import _lib
    docs = [make_pair(150 + 17 * i, 160 - 9 * i, 4, 32, seed=70 + i, deletions=i) for i in range(4)]
    priors = [split_prior(a.shape[1], b.shape[1], 1 + i) for i, (a, b) in enumerate(docs)]
    ctx = _lib.context()

    def sequence():
        a, b = batch(docs, priors, W=33), batch(docs[:2], priors[:2], W=7, seeds=[5, 6], search="around")
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


# ---------------------------------------------------------------------------------------------- 8
def test_argument_errors_queue_nothing(orc):
    from svx import _lib
    v0, v1 = make_pair(120, 97, 4, 32, seed=3, deletions=6)
    prior = split_prior(120, 97, 4)
    ref = around_stack(orc, v0, v1, TYPES5, 33, 33, prior)

    def expect_arg(pb, text):
        pb.align.fill_(-1)
        pb.info.fill_(-1)
        with pytest.raises(_lib.SvxError) as e:
            pb.run()
        assert e.value.code == SVX_ERR_ARG and text in str(e.value)
        info, align, _ = outputs(pb)
        assert (info == -1).all() and (align == -1).all()       # nothing was queued
        good = batch([(v0, v1)], [prior], W=33, seeds=[33])     # the context still works
        good.run()
        check_result(good.results()[0], ref)

    pb = batch([(v0, v1)], None, W=33, seeds=[33], search="straight")            # svx_align_batch rejects the new mode
    pb.prm.search_mode = _lib.SVX_SEARCH_AROUND_WIDE
    expect_arg(pb, "search_mode")
    pb = batch([(v0, v1)], [prior], W=33, seeds=[33])                            # the empty set: the only one no tile shape takes
    pb.prm.n_types = 0
    expect_arg(pb, "no tile shape")
    pb = batch([(v0, v1)], [prior], W=33, seeds=[33])                            # the limit of SVX_SEARCH_AROUND stands
    pb.prm.search_mode = _lib.SVX_SEARCH_AROUND
    expect_arg(pb, "at most 64 around a prior")


# ---------------------------------------------------------------------------------------------- 9
def second_frames(starts, dur=12000):
    s = np.asarray(starts, np.int64)
    return np.stack([s, s + dur], axis=1)


def test_prior_width_against_the_host_twin():
    from svx import _lib
    from svx.vecalign.dp_utils import prior_rows_from_alignments, prior_width
    for third in ("path", "propagated"):
        docs, priors = ragged_priors(third)
        pb = batch(docs, priors, W=33)
        got = pb.prior_width()
        assert got.dtype == np.int32 and got.tolist() == [
            prior_width(prior_rows_from_alignments(priors[0]), 300, 280), 0, 0, prior_width(prior_rows_from_alignments(priors[3]), 64, 1)]
        assert got.tolist() == [20, 0, 0, 3]
    # rows with sums below (n, m): the remainder row counts; count < cap: rows past count are not read
    import torch
    rows = torch.tensor([[0, 10, 0, 30], [10, 0, 30, 5], [10, 50, 35, 45], [0, 999, 0, 999]], dtype=torch.int32).cuda()
    pb = batch(docs[:1], [(rows, torch.tensor([3, 0], dtype=torch.int32).cuda())], W=33)
    assert pb.prior_width().tolist() == [prior_width(rows.cpu().numpy()[:3], 300, 280)] == [201]
    # a time prior, chained on the stream
    v0, v1, src = block_deletion_pair(seed=0)
    F0, F1 = second_frames(16000 * np.arange(300)), second_frames(16000 * src + 8000)
    pb = batch([(v0, v1)], [None], W=33, seeds=[11], frames=[(F0, F1)])
    pb.time_prior(100 * 16000, 8000)
    want, code = time_prior_ref(F0, F1, 100 * 16000, 8000)
    assert code == 0 and len(want) == 3
    assert pb.prior_width().tolist() == [prior_width(want, 300, 180)] == [101]
    ctx = _lib.context()
    with pytest.raises(_lib.SvxError) as e:
        ctx.check(ctx.lib.svx_prior_width(ctx.h, pb.cpairs, pb.cpriors, 1, None))
    assert e.value.code == SVX_ERR_ARG


# ---------------------------------------------------------------------------------------------- 10
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


def test_seg_align_cli_prior_band(orc, tmp_path, monkeypatch):
    from svx.seg_align import align as A
    from svx.seg_align.align import pair_rng
    from svx.utils.file_utils import read_alignments_with_score, read_segments
    from svx.vecalign import dp_utils
    seen = []
    real = dp_utils.PreparedBatch

    class Capture(real):
        def __init__(self, pairs, types, frac, w2, *a, **k):
            seen.append(([(v0.float().cpu().numpy().copy(), v1.float().cpu().numpy().copy()) for v0, v1 in pairs], list(types), w2, k.get("search"), self))
            super().__init__(pairs, types, frac, w2, *a, **k)

    monkeypatch.setattr(dp_utils, "PreparedBatch", Capture)
    root, out = str(tmp_path / "data"), str(tmp_path / "out")
    build_tree(root)
    A.main([os.path.join(root, "metadata.tsv"), out, "--src_lang", "en", "--tgt_lang", "de", "--seg_dir", os.path.join(root, "seg"),
            "--concat_dir", os.path.join(root, "cat"), "--embed_dir", os.path.join(root, "emb"),
            "--ign_indices_dir", os.path.join(root, "ign"), "--fp16_embed", "--seed", "3", "--mode", "around",
            "--prior", "time", "--prior_window", "20", "--prior_lag", "0.5", "--prior_band", "80"])
    assert len(seen) == 1 and seen[0][3] == "around_wide" and seen[0][2] == 40
    (v0, v1), = seen[0][0]
    types = seen[0][1]
    n, m = v0.shape[1], v1.shape[1]
    rows, code = time_prior_ref(read_segments(os.path.join(TRIM, "segments_en.txt")), read_segments(os.path.join(TRIM, "segments_de.txt")),
                                20 * 16000, 8000)
    assert code == 0 and len(rows) > 1
    lengths, code = ingest_ref(rows, len(rows), n, m)
    assert code == 0
    # the covering widths rode along with the result fetch (what the job's log line counts)
    assert seen[0][4].h_widths.numpy().tolist() == [dp_utils.prior_width(rows, n, m)]
    ref = around_stack(orc, v0, v1, types, 40, pair_rng(3, 0), lengths_to_alignments(lengths))
    got = read_alignments_with_score(os.path.join(out, "en-de", "doc0_en-doc0_de.txt"))
    assert [(list(a), list(b)) for a, b, _ in got] == [(list(a), list(b)) for a, b in ref['final_alignments']]
    assert max(abs(g[2] - s) for g, s in zip(got, ref['alignment_scores'])) < SCORE_TOL + 5e-7  # (the file has 6 decimals)
