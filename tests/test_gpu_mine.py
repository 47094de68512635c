"""Margin-based mining on the GPU (csrc/svx_mine.hip: svx_knn_list_means, svx_margin_candidates; svx/postprocess/mine.py)
against the references of tests/mine_ref.py, through the C ABI and the Python API.

(a) test_synthetic: lists that no search produced (mine_ref.synthetic_lists: rows with trailing (-inf, -1) entries, ids
    out of range, exact score ties, rows without a valid candidate, b = 0, -0.0), n in {1, 63, 64, 65, 16384 + 77} x
    k in {1, 15, 16, 64} x n_db in {k, 1000} x id_base in {0, 2^33 + 7}: the list means, and for RATIO, DISTANCE and
    ABSOLUTE the scores, best ids and best scores, equal reference (a) bit for bit, with `scores` requested and with NULL.
    RATIO is held to bits as well: the library is built without fast-math flags and the kernels' fp32 division is the
    correctly rounded one (v_div_scale / v_div_fmas / v_div_fixup in the ISA), so no tolerance is needed anywhere.
    (Two NaNs count as equal whatever their payload: 0 / 0 has no defined sign.)
(b) test_lattice: LATTICE inputs (margin_ref.lattice; test_mine_ref_cpu.py shows the similarities of both directions
    exact in fp32): mine_bitexts equals the reference run on search_ref.search_exact's lists for all four retrievals with
    DISTANCE and ABSOLUTE -- pairs, order and score bits -- and list_means equals FlatIndex.mean_sim bit for bit.
(c) test_real_rows: tests/golden/margin_example.npz, both storages, ratio and distance: the kernels fed the GPU's own
    search output equal (a) on those arrays bit for bit, the mined pairs of the four retrievals equal the reference's
    selection from those arrays, xsim equals the reference's value.  Identity rate and re-ranked share are printed.
(d) test_edges.  (e) test_cli_round_trip.
tests/test_mine_ref_cpu.py checks, without a GPU, the references against one another and the inputs used here."""
import ctypes
import os

import numpy as np
import pytest

import margin_ref as mr
import mine_ref as ref
import search_ref as sr
from test_gpu_margin_matrix import make_index
from test_mine_ref_cpu import LATTICE, lattice_sides

GD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BIG = 16384
NS = (1, 63, 64, 65, BIG + 77)
KS = (1, 15, 16, 64)
ID_BASES = (0, (1 << 33) + 7)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def same_floats(got, want):
    """Bit for bit; two NaNs are equal."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return got.shape == want.shape and bool(((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all())


def first_diff(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype == np.float32:
        bad = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
    else:
        bad = got != want
    at = tuple(int(v[0]) for v in np.nonzero(bad))
    return "%d differ; first at %s: %r, reference %r" % (bad.sum(), at, got[at], want[at])


def check_candidates(label, d, id_base, fails):
    """One synthetic data set through both kernels, every margin, with and without the score matrix."""
    from svx.postprocess import mine
    sims, ids, mq, md = dev(d["sims"]), dev(d["ids"]), dev(d["mean_q"]), dev(d["mean_db"])
    mean = host(mine.list_means(sims))
    want = ref.list_means(d["sims"])
    if not same_floats(mean, want):
        fails.append("%s list_means: %s" % (label, first_diff(mean, want)))
    for margin in ref.MARGINS:
        wscores, wid, wscore = ref.candidates(d["sims"], d["ids"], d["mean_q"], d["mean_db"], margin, id_base)
        for want_scores in (True, False):
            bid, bscore, scores = mine.candidate_scores(sims, ids, mq, md, margin, id_base=id_base, want_scores=want_scores)
            tag = "%s %s%s" % (label, margin, "" if want_scores else " (scores NULL)")
            assert (scores is not None) == want_scores
            if want_scores and not same_floats(host(scores), wscores):
                fails.append("%s scores: %s" % (tag, first_diff(host(scores), wscores)))
            if not np.array_equal(host(bid), wid):
                fails.append("%s best_id: %s" % (tag, first_diff(host(bid), wid)))
            if not same_floats(host(bscore), wscore):
                fails.append("%s best_score: %s" % (tag, first_diff(host(bscore), wscore)))
    return wid


# ---- (a) synthetic lists
@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_synthetic(n, k):
    fails = []
    for n_db in (k, 1000):
        for id_base in ID_BASES:
            # fewer rows than row kinds: every kind comes up in one of the shifted data sets
            shifts = range(ref.ROW_KINDS) if n < ref.ROW_KINDS else (0,)
            kinds = set()
            for shift in shifts:
                d = ref.synthetic_lists(n, k, n_db, id_base, seed=1, shift=shift)
                kinds |= set(d["kind"].tolist())
                wid = check_candidates("n=%d k=%d n_db=%d id_base=%d shift=%d" % (n, k, n_db, id_base, shift), d, id_base, fails)
                assert (wid[np.isin(d["kind"], (4, 5))] == -1).all()   # rows without a valid candidate
                assert (wid[d["kind"] == 0] >= id_base).all()
            assert kinds == set(range(ref.ROW_KINDS))
    assert not fails, "\n".join(fails[:20])


# ---- (b) lattice
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(LATTICE))
def test_lattice(case):
    from svx.postprocess import mine
    n, N, d, k, storage, qtype, order, seed = LATTICE[case]
    x, db, _, S_xy, S_yx = lattice_sides(case)
    idx_x, idx_y = make_index(x, storage), make_index(db, storage)
    import torch
    assert idx_x.rows.dtype == {"f16": torch.float16, "bf16": torch.bfloat16}[qtype]
    lists = sr.search_exact(S_xy.astype(np.float32), k) + sr.search_exact(S_yx.astype(np.float32), k)
    fails = []
    # the searches return the exact lists, in both directions
    for name, (D, I), (wD, wI) in (("x in y", idx_y.search(idx_x.rows, k), lists[:2]), ("y in x", idx_x.search(idx_y.rows, k), lists[2:])):
        if not (same_floats(host(D), wD) and np.array_equal(host(I), wI)):
            fails.append("search %s differs from search_exact" % name)
    D, _ = idx_y.search(idx_x.rows, k)
    mean = host(mine.list_means(D))
    if not same_floats(mean, host(idx_y.mean_sim(idx_x.rows, k))):
        fails.append("list_means differs from FlatIndex.mean_sim")
    if not same_floats(mean, ref.list_means(lists[0])):
        fails.append("list_means differs from the reference")
    for margin in ("distance", "absolute"):
        best = ref.mine(*lists, margin)
        for retrieval in ref.RETRIEVALS:
            for threshold in ((None, float(np.median(best[1]))) if retrieval == "max" else (None,)):
                got = mine.mine_bitexts(idx_x, idx_y, k=k, margin=margin, retrieval=retrieval, threshold=threshold)
                want = ref.select(*best, retrieval, threshold)
                assert got[0].dtype == np.float32 and got[1].dtype == np.int64 and got[2].dtype == np.int64
                if ref.as_triples(got) != ref.as_triples(want):
                    fails.append("%s %s threshold %s: %d pairs, reference %d; pairs, order or score bits differ"
                                 % (margin, retrieval, threshold, len(got[0]), len(want[0])))
    assert not fails, "\n".join(fails)


# ---- (c) real rows
@pytest.mark.gpu
@pytest.mark.parametrize("margin", ["ratio", "distance"])
@pytest.mark.parametrize("storage", mr.STORAGES)
def test_real_rows(storage, margin):
    from svx.postprocess import mine
    from svx.postprocess.flat_index import FlatIndex
    g = np.load(os.path.join(GD, "margin_example.npz"))
    x, y = g["db_src"], g["db_tgt"]
    assert x.shape == y.shape == (347, 1024)
    n, k = x.shape[0], 16
    idx_x, idx_y = FlatIndex(1024, storage), FlatIndex(1024, storage)
    idx_x.add(x)
    idx_y.add(y)
    D_xy, I_xy = idx_y.search(idx_x.rows, k)
    D_yx, I_yx = idx_x.search(idx_y.rows, k)
    lists = host(D_xy), host(I_xy), host(D_yx), host(I_yx)
    mean_x, mean_y = mine.list_means(D_xy), mine.list_means(D_yx)
    wmean_x, wmean_y = ref.list_means(lists[0]), ref.list_means(lists[2])
    fails = []
    if not (same_floats(host(mean_x), wmean_x) and same_floats(host(mean_y), wmean_y)):
        fails.append("list_means differs from the reference on the GPU's own lists")
    for name, (D, I, mq, md, hD, hI, wq, wd) in {"forward": (D_xy, I_xy, mean_x, mean_y, lists[0], lists[1], wmean_x, wmean_y),
                                                "backward": (D_yx, I_yx, mean_y, mean_x, lists[2], lists[3], wmean_y, wmean_x)}.items():
        bid, bscore, scores = mine.candidate_scores(D, I, mq, md, margin, want_scores=True)
        wscores, wid, wscore = ref.candidates(hD, hI, wq, wd, margin)
        s64, id64, _ = ref.candidates(hD, hI, ref.list_means(hD, np.float64), ref.list_means(lists[2] if name == "forward" else lists[0], np.float64),
                                      margin, 0, np.float64)
        e_gpu, e_orc, bound = mr.rule(host(scores), wscores, s64)
        print("%s %s %s: E_gpu %.3e, E_orc %.3e, bound %.3e; identity rate %.3f, re-ranked by the margin %.3f, best differs from float64 in %d rows"
              % (storage, margin, name, e_gpu, e_orc, bound, (host(bid) == np.arange(n)).mean(), (host(bid) != hI[:, 0]).mean(),
                 (host(bid) != id64).sum()))
        if not same_floats(host(scores), wscores):
            fails.append("%s scores: %s" % (name, first_diff(host(scores), wscores)))
        if not np.array_equal(host(bid), wid):
            fails.append("%s best_id: %s" % (name, first_diff(host(bid), wid)))
        if not same_floats(host(bscore), wscore):
            fails.append("%s best_score: %s" % (name, first_diff(host(bscore), wscore)))
    best = ref.mine(*lists, margin)
    for retrieval in ref.RETRIEVALS:
        got = mine.mine_bitexts(idx_x, idx_y, k=k, margin=margin, retrieval=retrieval)
        want = ref.select(*best, retrieval)
        print("%s %s %s: %d pairs" % (storage, margin, retrieval, len(got[0])))
        if ref.as_triples(got) != ref.as_triples(want):
            fails.append("%s: %d pairs, reference %d; pairs, order or score bits differ" % (retrieval, len(got[0]), len(want[0])))
    got = mine.xsim(x, y, k=k, margin=margin, storage=storage)
    want = float((best[0] != np.arange(n)).mean())
    print("%s %s: xsim %.4f" % (storage, margin, got))
    assert isinstance(got, float)
    if got != want:
        fails.append("xsim %r, reference %r" % (got, want))
    assert not fails, "\n".join(fails)


# ---- (d) edges
@pytest.mark.gpu
def test_edges():
    import torch
    from svx import _lib
    from svx.postprocess import mine
    from svx.postprocess.flat_index import FlatIndex
    ctx = _lib.context()
    k = 16
    # n = 0
    e_s, e_i = torch.empty((0, k), dtype=torch.float32, device="cuda"), torch.empty((0, k), dtype=torch.int64, device="cuda")
    e_m = torch.empty((0,), dtype=torch.float32, device="cuda")
    assert tuple(mine.list_means(e_s).shape) == (0,)
    bid, bscore, scores = mine.candidate_scores(e_s, e_i, e_m, torch.ones(5, device="cuda"), "ratio", want_scores=True)
    assert tuple(bid.shape) == tuple(bscore.shape) == (0,) and tuple(scores.shape) == (0, k) and bid.dtype == torch.int64
    assert ctx.lib.svx_knn_list_means(ctx.h, None, 0, k, None) == _lib.SVX_OK
    assert ctx.lib.svx_margin_candidates(ctx.h, None, None, 0, k, None, None, 0, 0, _lib.SVX_MARGIN_RATIO, None, None, None) == _lib.SVX_OK
    # an empty other side: every id is out of range
    d = ref.synthetic_lists(9, 4, 4, 0, seed=2)
    bid, bscore, _ = mine.candidate_scores(dev(d["sims"]), dev(d["ids"]), dev(d["mean_q"]), e_m, "distance")
    assert (host(bid) == -1).all() and np.isneginf(host(bscore)).all()
    # argument errors of the C ABI
    sims, ids, mq, md = dev(d["sims"]), dev(d["ids"]), dev(d["mean_q"]), dev(d["mean_db"])
    out_i, out_s = torch.empty(9, dtype=torch.int64, device="cuda"), torch.empty(9, dtype=torch.float32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def cand(n=9, kk=4, margin=_lib.SVX_MARGIN_RATIO, s=p(sims), i=p(ids), q=p(mq), m=p(md), n_db=4, bi=p(out_i), bs=p(out_s)):
        return ctx.lib.svx_margin_candidates(ctx.h, s, i, n, kk, q, m, n_db, 0, margin, None, bi, bs)

    assert cand() == _lib.SVX_OK
    for bad, text in ((dict(kk=0), "supported 1..64"), (dict(kk=65), "supported 1..64"), (dict(margin=3), "Wrong margin type: 3"),
                      (dict(margin=-1), "Wrong margin type: -1"), (dict(n=-1), "negative"), (dict(n_db=-1), "negative"),
                      (dict(s=None), "null"), (dict(i=None), "null"), (dict(q=None), "null"), (dict(m=None), "null"),
                      (dict(bi=None), "null"), (dict(bs=None), "null")):
        assert cand(**bad) == _lib.SVX_ERR_ARG, bad
        assert text in ctx.lib.svx_last_error(ctx.h).decode(), (bad, ctx.lib.svx_last_error(ctx.h).decode())
    assert cand(margin=_lib.SVX_MARGIN_ABSOLUTE, q=None, m=None) == _lib.SVX_OK   # the absolute score reads no mean
    for bad, text in ((dict(k=0), "supported 1..64"), (dict(k=65), "supported 1..64"), (dict(n=-1), "negative"), (dict(s=None), "null"), (dict(o=None), "null")):
        a = dict(s=p(sims), n=9, k=4, o=p(out_s))
        a.update(bad)
        assert ctx.lib.svx_knn_list_means(ctx.h, a["s"], a["n"], a["k"], a["o"]) == _lib.SVX_ERR_ARG, bad
        assert text in ctx.lib.svx_last_error(ctx.h).decode()
    ctx.sync()
    # svx_margin_scores still rejects the absolute margin
    rows = torch.ones((3, 32), dtype=torch.float32, device="cuda")
    ones = torch.ones(3, dtype=torch.float32, device="cuda")
    rc = ctx.lib.svx_margin_scores(ctx.h, p(rows), p(rows), _lib.SVX_F32, 3, 32, p(ones), p(ones), _lib.SVX_MARGIN_ABSOLUTE, p(ones))
    assert rc == _lib.SVX_ERR_ARG and "Wrong margin type: 2" in ctx.lib.svx_last_error(ctx.h).decode()
    # the Python API
    q, db = mr.lattice(40, 60, 96, 8, 3, "shuffled")
    x = (q / np.sqrt((q.astype(np.float64) ** 2).sum(axis=1))[:, None]).astype(np.float32)
    idx_x, idx_y = make_index(x, "fp16"), make_index(db, "fp16")
    small = make_index(db[:7], "fp16")
    for a, b in ((idx_x, small), (small, idx_y)):
        with pytest.raises(ValueError, match="fewer than k"):
            mine.mine_bitexts(a, b, k=8)
    with pytest.raises(ValueError, match="Wrong margin type: cosine"):
        mine.mine_bitexts(idx_x, idx_y, k=8, margin="cosine")
    with pytest.raises(ValueError, match="Wrong margin type"):
        mine.candidate_scores(sims, ids, mq, md, "cosine")
    with pytest.raises(ValueError, match="retrieval"):
        mine.mine_bitexts(idx_x, idx_y, k=8, retrieval="union")
    with pytest.raises(ValueError):
        mine.xsim(x, db, k=8)
    with pytest.raises(ValueError, match="fewer than k"):
        mine.xsim(x[:5], x[:5], k=8)
    # threshold removes exactly the pairs with score <= threshold, after the selection
    for retrieval in ref.RETRIEVALS:
        full = mine.mine_bitexts(idx_x, idx_y, k=8, margin="distance", retrieval=retrieval)
        assert len(full[0]) > 4
        th = float(full[0][len(full[0]) // 2])     # a score that occurs: the pair itself goes too
        cut = mine.mine_bitexts(idx_x, idx_y, k=8, margin="distance", retrieval=retrieval, threshold=th)
        keep = full[0] > np.float32(th)
        assert 0 < keep.sum() < len(keep) and not keep[len(keep) // 2]
        assert ref.as_triples(cut) == ref.as_triples(tuple(a[keep] for a in full))


# ---- (e) CLI
@pytest.mark.gpu
def test_cli_round_trip(tmp_path):
    from svx.postprocess import mine
    from svx.postprocess.flat_index import FlatIndex, write_faiss_flat
    g = np.load(os.path.join(GD, "margin_example.npz"))
    paths = {}
    for side, rows in (("src", g["db_src"]), ("tgt", g["db_tgt"])):
        idx = FlatIndex(1024, "fp16")
        idx.add(rows)
        paths[side] = str(tmp_path / ("%s.populate.idx" % side))
        write_faiss_flat(paths[side], idx.rows.float().cpu().numpy())
    for args, kw in (([], dict()), (["--margin", "distance", "--retrieval", "intersection", "--k", "8", "--threshold", "0.01", "--gpu_type", "bf16-shard"],
                                   dict(k=8, margin="distance", retrieval="intersection", threshold=0.01))):
        out = str(tmp_path / "mined.tsv")
        mine.main(["--src_index", paths["src"], "--tgt_index", paths["tgt"], "--out", out] + args)
        storage = "bf16" if "bf16-shard" in args else "fp16"
        scores, src, tgt = mine.mine_bitexts(FlatIndex.read(paths["src"], storage), FlatIndex.read(paths["tgt"], storage), **kw)
        # the score as score_align.write_to_output prints a float32: the f-string of the numpy scalar
        want = "".join(f"{s}\t{int(i)}\t{int(j)}\n" for s, i, j in zip(scores, src, tgt))
        assert len(scores) > 100 and isinstance(scores[0], np.float32)
        with open(out) as f:
            assert f.read() == want
        assert sorted(os.listdir(tmp_path)) == ["mined.tsv", "src.populate.idx", "tgt.populate.idx"]   # no .tmp left behind
    with pytest.raises(SystemExit):
        mine.main(["--src_index", paths["src"], "--tgt_index", paths["tgt"], "--out", out, "--margin", "cosine"])
