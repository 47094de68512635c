"""svx_align_widen on the GPU (include/svx.h): band doubling in the library.  Its outputs and report must equal, bit for
bit, those of the sequence of public calls it is defined as (svx_align_batch / svx_align_around, svx_band_contact, then per
round svx_align_around in SVX_SEARCH_AROUND_WIDE around the current result + svx_band_contact), which explicit() builds
from copies of the batch's own Pair descriptors with the outputs of the later rounds redirected into fresh buffers.
Against the oracle's chain (tests/contact_ref.py): identical spans, scores within SCORE_TOL of tests/test_gpu_around.py."""
import ctypes
import os

import numpy as np
import pytest

from around_ref import SVX_ERR_ARG, around_stack, block_deletion_pair
from contact_ref import widen_chain
from synth import alignment_types, make_pair

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-4
TYPES5 = alignment_types(5)


def to_dev(v):
    import torch
    return torch.from_numpy(v).cuda()


def batch(docs, W, seeds, search="straight", priors=None, max_full=300):
    from svx.vecalign import dp_utils
    kw = dict(priors=priors) if search in ("around", "around_wide") else {}
    return dp_utils.PreparedBatch([(to_dev(a), to_dev(b)) for a, b in docs], TYPES5, 0.2, W, max_full, 20000, 100,
                                  rngs=[np.random.RandomState(s) for s in seeds], search=search, **kw)


def own_outputs(pb):
    """Per pair (info [2], rows [count][4], scores [count]) of the batch's own buffers, as bytes-comparable arrays."""
    pb.ctx.sync()
    info, align, scores = pb.info.cpu().numpy(), pb.align.cpu().numpy(), pb.scores.cpu().numpy()
    out = []
    for i in range(len(pb.vecs)):
        o, cnt = int(pb.offs[i]), max(0, int(info[i, 0]))
        out.append((info[i].copy(), align[o:o + cnt].copy(), scores[o:o + cnt].copy()))
    return out


def explicit(pb, guard, max_w, max_rounds):
    """The public calls svx_align_widen stands for -> (per pair (info, rows, scores), report [pairs][4])."""
    import torch
    from svx import _lib
    ctx, n = pb.ctx, len(pb.vecs)
    pb.run()
    c = pb.band_contact(0, guard).cpu().numpy()
    W = max(3, int(pb.prm.width_over2))
    report = np.array([[0, W, c[i, 0], c[i, 0]] for i in range(n)], np.int32)
    cur = [(int(pb.cpairs[i].align), int(pb.cpairs[i].info)) for i in range(n)]
    redirected = {}
    prm = _lib.AlignParams()
    ctypes.memmove(ctypes.byref(prm), ctypes.byref(pb.prm), ctypes.sizeof(prm))
    prm.search_mode = _lib.SVX_SEARCH_AROUND_WIDE
    for r in range(1, max_rounds + 1):
        idx = [i for i in range(n) if report[i, 3] > 0]
        if min(2 * W, max_w) == W or not idx:
            break
        W = min(2 * W, max_w)
        sub, pri = (_lib.Pair * len(idx))(), (_lib.Prior * len(idx))()
        for j, i in enumerate(idx):
            cap = int(pb.offs[i + 1] - pb.offs[i])
            al = torch.zeros((cap, 4), dtype=torch.int32).cuda()
            sc = torch.zeros(cap, dtype=torch.float64).cuda()
            inf = torch.zeros(2, dtype=torch.int32).cuda()
            ctypes.memmove(ctypes.byref(sub[j]), ctypes.byref(pb.cpairs[i]), ctypes.sizeof(_lib.Pair))
            sub[j].align, sub[j].scores, sub[j].info = al.data_ptr(), sc.data_ptr(), inf.data_ptr()
            pri[j].rows, pri[j].info, pri[j].cap = cur[i][0], cur[i][1], cap
            redirected.setdefault(i, []).append((al, sc, inf))   # (the round before stays alive: it is this round's prior)
            cur[i] = (al.data_ptr(), inf.data_ptr())
        prm.width_over2 = W
        ctx.check(ctx.lib.svx_align_around(ctx.h, ctypes.byref(prm), sub, pri, len(idx)))
        out = torch.empty((len(idx), 4), dtype=torch.int32).cuda()
        ctx.check(ctx.lib.svx_band_contact(ctx.h, 0, guard, ctypes.c_void_p(out.data_ptr())))
        c = out.cpu().numpy()
        for j, i in enumerate(idx):
            report[i] = (r, W, report[i, 2], c[j, 0])
    res = own_outputs(pb)
    for i, bufs in redirected.items():
        al, sc, inf = (x.cpu().numpy() for x in bufs[-1])
        cnt = max(0, int(inf[0]))
        res[i] = (inf.copy(), al[:cnt].copy(), sc[:cnt].copy())
    return res, report


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert u.shape == v.shape and u.tobytes() == v.tobytes()


def check_oracle(res, st):
    from svx.vecalign.dp_utils import rows_to_alignments
    info, rows, scores = res
    assert info.tolist() == [len(st['final_alignments']), 0]
    assert rows_to_alignments(rows) == st['final_alignments']
    assert np.abs(scores - st['alignment_scores']).max() < SCORE_TOL


@pytest.fixture(scope="module")
def trio():
    """block_deletion_pair seed 0, one clean pair, block_deletion_pair seed 1."""
    a, b = block_deletion_pair(seed=0), block_deletion_pair(seed=1)
    return [(a[0], a[1]), make_pair(200, 190, 4, 32, 5, deletions=3), (b[0], b[1])]


SEEDS = [11, 11, 11]


# ---------------------------------------------------------------------------------------------- 1
def test_batch_of_three_from_the_straight_band(orc, trio):
    pb = batch(trio, 7, SEEDS)
    report = pb.run_widen(guard=0, max_width_over2=7 << 4, max_rounds=4)
    assert report.dtype == np.int32 and report.tolist() == [[2, 28, 20, 0], [0, 7, 0, 0], [2, 28, 26, 0]]
    got = own_outputs(pb)
    want, want_report = explicit(batch(trio, 7, SEEDS), 0, 7 << 4, 4)
    assert np.array_equal(report, want_report)
    same(got, want)
    for i, (v0, v1) in enumerate(trio):
        stacks, rep = widen_chain(orc, v0, v1, TYPES5, 7, SEEDS[i])
        assert list(rep) == report[i].tolist()
        check_oracle(got[i], stacks[-1])
    # afterwards the context's last call is the last round's: the two pairs that were searched again, at 56 cells
    import torch
    out = torch.full((3, 4), -7, dtype=torch.int32).cuda()
    pb.ctx.check(pb.ctx.lib.svx_band_contact(pb.ctx.h, 0, 0, ctypes.c_void_p(out.data_ptr())))
    last = out.cpu().numpy()
    assert last[:2, 0].tolist() == [0, 0] and last[:2, 3].tolist() == [285, 280] and (last[2] == -7).all()
    st = pb.level_stack(1, 0)
    assert st['a_b_csum'].shape[1] == 56 and st['size1'] == 180


# ---------------------------------------------------------------------------------------------- 2
def test_one_round_through_the_tile_sweep(orc, trio):
    v0, v1 = trio[0]
    pb = batch([(v0, v1)], 20, [11])
    report = pb.run_widen()
    assert report.tolist() == [[1, 40, 10, 0]]
    assert 'a_b_costs' not in pb.level_stack(0, 0)         # 80 cells: the tile sweep ran the last round
    got = own_outputs(pb)
    want, want_report = explicit(batch([(v0, v1)], 20, [11]), 0, 20 << 4, 4)
    assert np.array_equal(report, want_report)
    same(got, want)
    stacks, rep = widen_chain(orc, v0, v1, TYPES5, 20, 11)
    check_oracle(got[0], stacks[-1])
    c2f = orc.vecalign(v0.copy(), v1.copy(), TYPES5, 0.2, 7, 100, 20000, 100, rng=np.random.RandomState(11))
    from svx.vecalign.dp_utils import rows_to_alignments
    assert rows_to_alignments(got[0][1]) == c2f[0]['final_alignments']


# ---------------------------------------------------------------------------------------------- 3
def test_coarse_to_fine_start():
    """W = 3 with guard 1 touches at level 0 (tests/test_gpu_contact.py); the later rounds read the depth-0 draws at the
    head of the coarse-to-fine index arrays."""
    docs = [make_pair(300, 280, 4, 32, 0, deletions=40), make_pair(200, 190, 4, 32, 5, deletions=3)]
    pb = batch(docs, 3, [11, 12], search="coarse_to_fine", max_full=100)
    report = pb.run_widen(guard=1, max_width_over2=24, max_rounds=3)
    got = own_outputs(pb)
    want, want_report = explicit(batch(docs, 3, [11, 12], search="coarse_to_fine", max_full=100), 1, 24, 3)
    assert np.array_equal(report, want_report)
    assert report[0, 0] >= 1 and report[0, 2] > 0 and (report[:, 1] == 3 * 2 ** report[:, 0]).all()
    same(got, want)
    assert all(int(g[0][1]) == 0 and int(g[0][0]) > 0 for g in got)


# ---------------------------------------------------------------------------------------------- 4
def test_around_start_from_a_single_block_prior(orc, trio):
    v0, v1 = trio[0]
    prior = [(list(range(300)), list(range(180)))]
    pb = batch([(v0, v1)], 7, [11], search="around", priors=[prior])
    report = pb.run_widen()
    assert report.tolist() == [[2, 28, 20, 0]]
    got = own_outputs(pb)
    want, want_report = explicit(batch([(v0, v1)], 7, [11], search="around", priors=[prior]), 0, 7 << 4, 4)
    assert np.array_equal(report, want_report)
    same(got, want)
    stacks, rep = widen_chain(orc, v0, v1, TYPES5, 7, 11, first=around_stack(orc, v0, v1, TYPES5, 7, 11, prior))
    assert rep == (2, 28, 20, 0)
    check_oracle(got[0], stacks[-1])


# ---------------------------------------------------------------------------------------------- 5
def test_width_cap_stops_still_touching(orc, trio):
    v0, v1 = trio[0]
    pb = batch([(v0, v1)], 7, [11])
    report = pb.run_widen(max_width_over2=14)
    assert report.tolist() == [[1, 14, 20, 13]]
    got = own_outputs(pb)
    want, want_report = explicit(batch([(v0, v1)], 7, [11]), 0, 14, 4)
    assert np.array_equal(report, want_report)
    same(got, want)
    stacks, rep = widen_chain(orc, v0, v1, TYPES5, 7, 11, max_width_over2=14)
    check_oracle(got[0], stacks[-1])
    # one round allowed, a wider cap: the same search
    pb = batch([(v0, v1)], 7, [11])
    assert pb.run_widen(max_width_over2=100, max_rounds=1).tolist() == [[1, 14, 20, 13]]
    same(own_outputs(pb), got)


# ---------------------------------------------------------------------------------------------- 6
def test_no_rounds_is_the_plain_call(trio):
    plain = batch(trio, 7, SEEDS)
    plain.run()
    plain.ctx.sync()
    pb = batch(trio, 7, SEEDS)
    report = pb.run_widen(max_rounds=0)
    assert report.tolist() == [[0, 7, 20, 20], [0, 7, 0, 0], [0, 7, 26, 26]]
    for a, b in ((pb.info, plain.info), (pb.align, plain.align), (pb.scores, plain.scores), (pb.del_pen, plain.del_pen)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ---------------------------------------------------------------------------------------------- 7
def test_pipeline_does_not_change_results(trio):
    from svx import _lib
    ctx = _lib.context()
    runs = []
    try:
        for on in (False, True):
            ctx.set_pipeline(on)
            pb = batch(trio, 7, SEEDS)
            report = pb.run_widen()
            runs.append((report, own_outputs(pb)))
    finally:
        ctx.set_pipeline(False)
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][0][:, 0].tolist() == [2, 0, 2]
    same(runs[0][1], runs[1][1])


# ---------------------------------------------------------------------------------------------- 8
def test_argument_errors_queue_nothing(trio):
    from svx import _lib
    pb = batch(trio[:1], 7, [11])
    ctx = pb.ctx
    report = np.full((1, 4), -7, np.int32)
    rp = ctypes.c_void_p(report.ctypes.data)

    def call(guard=0, max_w=28, rounds=2, prm=True, pairs=True, wp=True, rep=rp):
        w = _lib.WidenParams()
        w.guard, w.max_width_over2, w.max_rounds = guard, max_w, rounds
        return ctx.lib.svx_align_widen(ctx.h, ctypes.byref(pb.prm) if prm else None, pb.cpairs if pairs else None, None, 1,
                                       ctypes.byref(w) if wp else None, rep)
    pb.info.fill_(-1)
    pb.align.fill_(-1)
    for kw in (dict(guard=-1), dict(max_w=-1), dict(rounds=-1), dict(max_w=6), dict(prm=False), dict(pairs=False), dict(wp=False),
               dict(rep=None)):
        assert call(**kw) == SVX_ERR_ARG, kw
        assert len(ctx.lib.svx_last_error(ctx.h)) > 10
    pb.prm.search_mode = _lib.SVX_SEARCH_AROUND          # round 0's own argument check, returned as is
    assert call() == SVX_ERR_ARG
    pb.prm.search_mode = _lib.SVX_SEARCH_STRAIGHT
    ctx.sync()
    assert (pb.info.cpu().numpy() == -1).all() and (pb.align.cpu().numpy() == -1).all() and (report == -7).all()
    assert call() == 0 and report.tolist() == [[2, 28, 20, 0]]


# ---------------------------------------------------------------------------------------------- 9
def write_tree(root, v0, v1):
    """The block-deletion pair as a document pair on disk: one-second segments, every candidate span of up to K segments
    with its layer row as fp16 (rows i < k of layer k are spans that do not exist)."""
    for lang, v in (("en", v0), ("de", v1)):
        K, n, d = v.shape
        for sub in ("seg", "cat", "emb"):
            os.makedirs(os.path.join(root, sub, lang), exist_ok=True)
        seg = [(32000 * i, 32000 * i + 16000) for i in range(n)]
        with open(os.path.join(root, "seg", lang, f"doc0_{lang}.txt"), "w") as f:
            f.write("".join("%d %d\n" % s for s in seg))
        lines, rows = [], []
        for i in range(n):
            for k in range(min(K, i + 1)):
                lines.append("%d %d\n" % (seg[i - k][0], seg[i][1]))
                rows.append(v[k, i])
        with open(os.path.join(root, "cat", lang, f"doc0_{lang}.txt"), "w") as f:
            f.write("".join(lines))
        np.stack(rows).astype(np.float16).tofile(os.path.join(root, "emb", lang, f"doc0_{lang}.embed"))
    with open(os.path.join(root, "metadata.tsv"), "w") as f:
        f.write("/audio/doc0_en.ogg\t/audio/doc0_de.ogg\n")


def test_cli_widen_reaches_the_reference_mode_file(tmp_path, caplog):
    """--mode band --band 14 --widen on the block-deletion pair (d = 1024, the dimension of the embedding files): two
    doublings, and the alignment file is the one --mode ref writes."""
    import logging
    from svx.seg_align import align as A
    v0, v1, _ = block_deletion_pair(d=1024, seed=0)
    root = str(tmp_path / "data")
    write_tree(root, v0, v1)
    base = [os.path.join(root, "metadata.tsv"), None, "--src_lang", "en", "--tgt_lang", "de", "--seg_dir", os.path.join(root, "seg"),
            "--concat_dir", os.path.join(root, "cat"), "--embed_dir", os.path.join(root, "emb"), "--fp16_embed", "--seed", "3",
            "-a", "5", "--max_size_full_dp", "100"]

    def run(name, extra):
        argv = list(base)
        argv[1] = str(tmp_path / name)
        A.main(argv + extra)
        return open(os.path.join(argv[1], "en-de", "doc0_en-doc0_de.txt")).read()
    ref = run("ref", [])
    band = run("band", ["--mode", "band", "--band", "14", "--contact_tsv", str(tmp_path / "band.tsv")])
    with caplog.at_level(logging.INFO, logger=A.logger.name):
        wide = run("wide", ["--mode", "band", "--band", "14", "--widen", "--contact_tsv", str(tmp_path / "wide.tsv")])
    assert len(ref.splitlines()) > 250 and band != ref
    assert wide == ref
    assert any("band contact" in r.getMessage() and "1 were searched again" in r.getMessage() for r in caplog.records)
    fields = open(tmp_path / "band.tsv").read().splitlines()
    assert len(fields) == 1
    f = fields[0].split("\t")
    assert f[:2] == ["doc0_en.txt", "doc0_de.txt"] and len(f) == 8
    touch, run_, clearance, nodes, rounds, final_band = (int(x) for x in f[2:])
    assert touch > 0 and 0 < run_ <= touch and clearance == 0 and nodes == len(band.splitlines()) + 1
    assert (rounds, final_band) == (0, 14)
    f = open(tmp_path / "wide.tsv").read().splitlines()[0].split("\t")
    assert f[:2] == ["doc0_en.txt", "doc0_de.txt"] and [int(x) for x in f[2:]] == [0, -1, -1, -1, 2, 56]
    # stats
    stats = {}
    args = A.parse_args([a if a is not None else str(tmp_path / "again") for a in base] + ["--mode", "band", "--band", "14", "--widen", "--widen_max_band", "28"])
    os.makedirs(os.path.join(args.out_dir, "en-de"), exist_ok=True)
    valid = A.validate_inputs(A.read_metadata(args.metadata), *(A.Path(os.path.join(root, s, l)) for s in ("seg", "cat", "emb") for l in ("en", "de")),
                              A.Path(args.out_dir) / "en-de")
    A.align_pairs(valid, args, 4, stats=stats)
    assert stats["widened"] == 1 and stats["still_touching"] == 1
