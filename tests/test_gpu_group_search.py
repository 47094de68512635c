"""FlatIndex.search_groups (svx_knn_search_groups, csrc/svx_groupsearch.hip), local mining (svx/postprocess/mine.py:
mine_local) and its CLI (svx/postprocess/mine_local.py), all through the C ABI or its Python mirror.

k_knn_search_groups<BF, QE> has the 2 x 3 = 6 instantiations of k_knn_search (database storage x query type) and its shape:
64 queries of ONE group per workgroup.  References: tests/group_search_ref.py; the properties of the inputs these
comparisons rest on are checked without a GPU in tests/test_group_search_ref_cpu.py.

(a) test_lattice: LATTICE group sets (every similarity exact in fp32).  Values as float32 bits and ids equal
    search_groups_exact, nothing exempt, and equal, bit for bit, a loop of FlatIndex.merge_search calls with
    id_base = db_off[g] over the group slices.  Query counts {0, 1, 5, 63, 64, 65, 129} and database counts
    {0, k - 1, k, 33, 49, 65, 241} per group, d in {32, 96, 544, 992, 1024}, k in {1, 15, 16, 24, 64}, the four database
    orders, the six instantiations; one set of 320 groups of 40 .. 70 queries (more than 256 workgroups, most last
    workgroups partly masked); one set with a single group.
(b) test_leak: consecutive groups hold the same lattice rows, `rising` next to `falling`: the rows just outside a range
    tie with or beat rows inside it.  Every id lies in its group's range and the result equals the reference.
(c) test_real_rows: tests/golden/example_full (1148 / 1035 rows, d = 1024) at k = 16, both directions, both storages, three
    cuts.  Per group under search_ref's rule (test_gpu_search.rule_fails, unchanged): values within e of the float64
    similarity, ids equal at every position that is not ambiguous.  Bit for bit against the per-group loop.
(d) test_mine_local_lattice / test_mine_local_example: mine_local equals per-pair mine_bitexts for the four retrievals and
    the three margins, with and without a threshold (scores as bits, src and tgt exactly), and mine_local_ref on the lattice
    pairs; a pair below k rows is left out and counted.
(e) test_cli: a tree of three pairs (example_full, example_trim, a 10-row document).
(f) test_edges.
No tolerance here is taken from what the kernel produces."""
import ctypes
import os

import numpy as np
import pytest

import group_search_ref as gr
import margin_ref as mr
import mine_ref as mnr
import search_ref as sr
from test_gpu_margin_matrix import bits, make_index, typed
from test_gpu_search import exact_fails, host, rule_fails
from test_group_search_ref_cpu import MINE_PAIRS, all_sets

GD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = 16


def device_rows(idx, a):
    from svx.postprocess.flat_index import to_device_rows
    return to_device_rows(idx.ctx, a)


def loop_search(idx, qd, k, q_off, db_off):
    """The per-group loop on the existing entry point: merge_search of the group's queries in an index over the group's
    rows with id_base = db_off[g] -> (values, ids) numpy, the groups' rows one after the other."""
    import torch
    from svx.postprocess.flat_index import FlatIndex
    rows = idx.rows
    D, I = [], []
    for g in range(len(q_off) - 1):
        qs, qe, ds, de = int(q_off[g]), int(q_off[g + 1]), int(db_off[g]), int(db_off[g + 1])
        if qe == qs:
            continue
        part = FlatIndex.over(rows[ds:de])
        d_, i_ = part.merge_search(qd[qs:qe], k, None, id_base=ds)
        D.append(d_)
        I.append(i_)
    if not D:
        return np.zeros((0, k), np.float32), np.zeros((0, k), np.int64)
    return torch.cat(D).cpu().numpy(), torch.cat(I).cpu().numpy()


def same_as_loop(label, got, loop):
    if not (np.array_equal(bits(got[0]), bits(loop[0])) and np.array_equal(got[1], loop[1])):
        bad = np.nonzero((bits(got[0]) != bits(loop[0])).any(axis=1) | (got[1] != loop[1]).any(axis=1))[0]
        return ["%s: %d rows differ from the per-group loop of FlatIndex.merge_search; first row %d" % (label, bad.size, int(bad[0]))]
    return []


def in_range_fails(label, ids, q_off, db_off):
    fails = []
    for g in range(len(q_off) - 1):
        part = ids[int(q_off[g]):int(q_off[g + 1])]
        if not ((part == -1) | ((part >= db_off[g]) & (part < db_off[g + 1]))).all():
            fails.append("%s: group %d returns ids outside its range [%d, %d)" % (label, g, db_off[g], db_off[g + 1]))
    return fails


# ---- (a) lattice groups
@pytest.mark.gpu
@pytest.mark.parametrize("name", [s[0] for s in all_sets()])
def test_lattice(name):
    _, d, k, storage, qtype, order, seed, counts = next(s for s in all_sets() if s[0] == name)
    q, db, q_off, db_off, sims = gr.lattice_groups(counts, d, k, seed, order)
    want = gr.search_groups_exact(sims, k, db_off)
    idx = make_index(db, storage)
    qd = device_rows(idx, typed(q, qtype))
    D, I = idx.search_groups(qd, k, q_off, db_off)
    assert D.is_cuda and I.is_cuda and tuple(D.shape) == tuple(I.shape) == (q.shape[0], k)
    got = host((D, I))
    fails = exact_fails("search_groups", got, want)
    fails += in_range_fails("search_groups", got[1], q_off, db_off)
    fails += same_as_loop("search_groups", got, loop_search(idx, qd, k, q_off, db_off))
    for g, (nq, N) in enumerate(counts):   # trailing (-inf, -1) entries of a group with fewer than k database rows
        if nq and N < k:
            part = slice(int(q_off[g]), int(q_off[g + 1]))
            assert np.isneginf(got[0][part, N:]).all() and (got[1][part, N:] == -1).all()
    if len(counts) == 1:   # a single group is plain search
        assert not exact_fails("search", host(idx.search(qd, k)), got)
    assert not fails, "\n".join(fails)


# ---- (b) leak
@pytest.mark.gpu
@pytest.mark.parametrize("storage", mr.STORAGES)
@pytest.mark.parametrize("N", gr.LEAK_DB_ROWS)
def test_leak(N, storage):
    q, db, q_off, db_off, sims = gr.leak_groups(6, 70, N, 96, K, 5)
    idx = make_index(db, storage)
    qd = device_rows(idx, q)
    got = host(idx.search_groups(qd, K, q_off, db_off))
    fails = in_range_fails("leak", got[1], q_off, db_off)
    fails += exact_fails("leak", got, gr.search_groups_exact(sims, K, db_off))
    fails += same_as_loop("leak", got, loop_search(idx, qd, K, q_off, db_off))
    assert not fails, "\n".join(fails)


# ---- (c) real rows
@pytest.fixture(scope="module")
def example():
    """The example rows and, per (direction, storage), the stored database and the float64 / sequential-fp32 matrices;
    computed once and left unchanged."""
    x, y = gr.example_rows(GD)
    cache = {}

    def get(direction, storage):
        if (direction, storage) not in cache:
            q, rows = (x, y) if direction == "x_in_y" else (y, x)
            db = mr.round_storage(rows.astype(np.float32), storage)
            cache[direction, storage] = (q, db, gr.example_reference(q, db, storage))
        return cache[direction, storage]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("storage", mr.STORAGES)
@pytest.mark.parametrize("direction", ["x_in_y", "y_in_x"])
@pytest.mark.parametrize("cut", list(gr.EXAMPLE_CUTS))
def test_real_rows(cut, direction, storage, example):
    q, db, ref = example(direction, storage)
    xe, ye = gr.EXAMPLE_CUTS[cut]
    q_off, db_off = (np.asarray(e, np.int64) for e in ((xe, ye) if direction == "x_in_y" else (ye, xe)))
    idx = make_index(db, storage)
    qd = device_rows(idx, q[:q_off[-1]])
    D, I = idx.search_groups(qd, K, q_off, db_off)
    got = host((D, I))
    fails = in_range_fails(cut, got[1], q_off, db_off)
    assert not fails, "\n".join(fails)
    for g in range(len(q_off) - 1):
        qs, qe, ds, de = int(q_off[g]), int(q_off[g + 1]), int(db_off[g]), int(db_off[g + 1])
        e = gr.block_bound(ref, qs, qe, ds, de)
        fails += rule_fails("%s %s %s group %d" % (cut, direction, storage, g), got[0][qs:qe], got[1][qs:qe] - ds,
                            ref["S64"][qs:qe, ds:de], e, K)
    fails += same_as_loop(cut, got, loop_search(idx, qd, K, q_off, db_off))
    assert not fails, "\n".join(fails)


# ---- (d) local mining
def per_pair_mine(x, y, x_off, y_off, k, margin, retrieval, threshold):
    """mine_bitexts pair by pair on indexes over the pair's rows -> (scores, src, tgt, group, pairs below k rows)."""
    from svx.postprocess import mine
    from svx.postprocess.flat_index import FlatIndex
    parts, small = [], 0
    for g in range(len(x_off) - 1):
        ix, iy = FlatIndex.over(x[int(x_off[g]):int(x_off[g + 1])]), FlatIndex.over(y[int(y_off[g]):int(y_off[g + 1])])
        if ix.ntotal < k or iy.ntotal < k:
            small += 1
            continue
        s, a, b = mine.mine_bitexts(ix, iy, k=k, margin=margin, retrieval=retrieval, threshold=threshold)
        parts.append((s, a, b, np.full(a.shape, g, np.int64)))
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4)) + (small,)


def mined_equal(got, want):
    return mnr.as_triples(got[:3]) == mnr.as_triples(want[:3]) and np.array_equal(got[3], want[3])


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(MINE_PAIRS))
def test_mine_local_lattice(case):
    import torch
    from svx.postprocess import mine
    d, k, storage, order, seed, counts = MINE_PAIRS[case]
    x, y, x_off, y_off, S_xy, S_yx, _ = gr.lattice_pairs(counts, d, k, storage, seed, order)
    tdt = torch.float16 if storage == "fp16" else torch.bfloat16
    xd, yd = (torch.from_numpy(a).cuda().to(tdt) for a in (x, y))
    assert torch.equal(xd.float().cpu(), torch.from_numpy(x)) and torch.equal(yd.float().cpu(), torch.from_numpy(y))
    n_small = sum(n < k or N < k for n, N in counts)
    fails = []
    for margin in mnr.MARGINS:
        for retrieval in mnr.RETRIEVALS:
            base = per_pair_mine(xd, yd, x_off, y_off, k, margin, retrieval, None)
            assert base[4] == n_small and len(base[0]) > 20
            for threshold in (None, float(np.median(base[0]))):
                stats = {}
                got = mine.mine_local(xd, yd, x_off, y_off, k, margin, retrieval, threshold, stats=stats)
                assert got[0].dtype == np.float32 and all(a.dtype == np.int64 for a in got[1:])
                assert stats["small_pairs"] == n_small   # a pair below k rows is left out and counted
                label = "%s %s threshold %s" % (margin, retrieval, threshold)
                if not mined_equal(got, per_pair_mine(xd, yd, x_off, y_off, k, margin, retrieval, threshold)):
                    fails.append("%s: differs from per-pair mine_bitexts" % label)
                if margin != "ratio":   # (the reference's fp32 division is numpy's; the lattice makes the other two exact)
                    want = gr.mine_local_ref(S_xy, S_yx, k, margin, retrieval, threshold)
                    if not mined_equal(got, want) or want[4] != n_small:
                        fails.append("%s: differs from mine_local_ref" % label)
    assert not fails, "\n".join(fails)
    with pytest.raises(ValueError, match="fewer than k"):
        mine.best_candidates_local(xd, yd, x_off, y_off, k, "ratio")


@pytest.mark.gpu
@pytest.mark.parametrize("storage", mr.STORAGES)
def test_mine_local_example(storage):
    from svx.postprocess import mine
    from svx.postprocess.flat_index import FlatIndex
    x, y = gr.example_rows(GD)
    ix, iy = FlatIndex(1024, storage), FlatIndex(1024, storage)
    ix.add(x)
    iy.add(y)
    fails = []
    for cut in ("two", "three"):
        x_off, y_off = (np.asarray(e, np.int64) for e in gr.EXAMPLE_CUTS[cut])
        xd, yd = ix.rows[:x_off[-1]], iy.rows[:y_off[-1]]
        for margin in mnr.MARGINS:
            for retrieval in mnr.RETRIEVALS:
                base = per_pair_mine(xd, yd, x_off, y_off, K, margin, retrieval, None)
                for threshold in (None, float(np.median(base[0]))):
                    got = mine.mine_local(xd, yd, x_off, y_off, K, margin, retrieval, threshold)
                    want = base if threshold is None else per_pair_mine(xd, yd, x_off, y_off, K, margin, retrieval, threshold)
                    assert len(want[0]) > 50
                    if not mined_equal(got, want):
                        fails.append("%s %s %s threshold %s: differs from per-pair mine_bitexts" % (cut, margin, retrieval, threshold))
    assert not fails, "\n".join(fails)


# ---- (e) CLI
def build_tree(tmp_path):
    """Three pairs: example_full, example_trim and the first 10 rows of example_full.  -> (metadata path, {stem pair:
    (source rows, target rows, source lines, target lines)})."""
    docs = {}
    for lang in ("en", "de"):
        os.makedirs(tmp_path / "cat" / lang)
        os.makedirs(tmp_path / "emb" / lang)
    meta = []
    for name, folder, rows in (("full", "example_full", None), ("trim", "example_trim", None), ("tiny", "example_full", 10)):
        sides = []
        for lang in ("en", "de"):
            emb = np.fromfile(os.path.join(GD, folder, "embeds_%s.f16" % lang), dtype=np.float16).reshape(-1, 1024)[:rows]
            with open(os.path.join(GD, folder, "cat_segs_%s.txt" % lang)) as f:
                lines = [line.strip() for line in f][:rows]
            assert len(lines) == emb.shape[0]
            emb.tofile(tmp_path / "emb" / lang / ("%s_%s.embed" % (name, lang)))
            (tmp_path / "cat" / lang / ("%s_%s.txt" % (name, lang))).write_text("".join(l + "\n" for l in lines))
            sides += [emb, lines]
        docs["%s_en-%s_de.txt" % (name, name)] = (sides[0], sides[2], sides[1], sides[3])
        meta.append("/audio/%s_en.wav\t/audio/%s_de.wav" % (name, name))
    (tmp_path / "meta.tsv").write_text("\n".join(meta) + "\n")
    return str(tmp_path / "meta.tsv"), docs


def read_dir(path):
    out = {}
    for name in sorted(os.listdir(path)):
        with open(os.path.join(path, name)) as f:
            out[name] = f.read()
    return out


@pytest.mark.gpu
def test_cli(tmp_path, monkeypatch):
    monkeypatch.setenv("LOCAL_RANK", "0")   # both shards of the in-process runs below work on this process's GPU
    from svx.postprocess import mine, mine_local
    from svx.postprocess.flat_index import FlatIndex
    meta, docs = build_tree(tmp_path)
    common = ["--src_lang", "en", "--tgt_lang", "de", "--concat_dir", str(tmp_path / "cat"), "--embed_dir", str(tmp_path / "emb"), "--fp16_embed"]
    configs = (("a", [], dict(k=16), "fp16"),
               ("b", ["--k", "8", "--margin", "distance", "--retrieval", "intersection", "--threshold", "0.01", "--gpu_type", "bf16-shard",
                      "--batch_rows", "1200"], dict(k=8, margin="distance", retrieval="intersection", threshold=0.01), "bf16"))
    for tag, flags, kw, storage in configs:
        out = tmp_path / ("out_" + tag)
        stats = {}
        mine_local.main([meta, str(out)] + common + flags, stats=stats)
        got = read_dir(out / "en-de")
        assert sorted(got) == sorted(docs)   # (and no .tmp left behind)
        for name, (xs, ys, xl, yl) in docs.items():
            ix, iy = FlatIndex(1024, storage), FlatIndex(1024, storage)
            ix.add(xs)
            iy.add(ys)
            if min(ix.ntotal, iy.ntotal) < kw["k"]:
                want = ""
            else:
                scores, src, tgt = mine.mine_bitexts(ix, iy, **kw)
                assert len(scores) > 3 or name.startswith("tiny")
                want = "".join(f"{s}\t{xl[i]}\t{yl[j]}\n" for s, i, j in zip(scores, src, tgt))
            assert got[name] == want, "%s %s" % (tag, name)
        if tag == "a":
            assert got["tiny_en-tiny_de.txt"] == "" and stats["small"] == 1 and stats["mined"] == 2   # the 10-row pair
        else:
            assert stats["small"] == 0 and stats["mined"] == 3   # at k = 8 the 10-row pair is mined
        # the two shards, one after the other, write the same files
        sharded = tmp_path / ("shard_" + tag)
        for rank in (0, 1):
            mine_local.main([meta, str(sharded)] + common + flags + ["--rank", str(rank), "--n_shard", "2"])
        assert read_dir(sharded / "en-de") == got
        # --skip_existing recomputes nothing
        (out / "en-de" / "trim_en-trim_de.txt").write_text("kept\n")
        stats = {}
        mine_local.main([meta, str(out)] + common + flags + ["--skip_existing"], stats=stats)
        assert stats["existing"] == 3 and stats["mined"] == 0 and stats["lines"] == 0
        assert read_dir(out / "en-de") == dict(got, **{"trim_en-trim_de.txt": "kept\n"})
    # a count mismatch: skipped with an error line and an empty file, the other pairs are mined
    with open(tmp_path / "cat" / "de" / "trim_de.txt", "a") as f:
        f.write("1 2\n")
    stats = {}
    mine_local.main([meta, str(tmp_path / "out_c")] + common, stats=stats)
    last = read_dir(tmp_path / "out_c" / "en-de")
    assert stats["skipped"] == 1 and last["trim_en-trim_de.txt"] == "" and last["full_en-full_de.txt"] == read_dir(tmp_path / "out_a" / "en-de")["full_en-full_de.txt"]


# ---- (f) edges
@pytest.mark.gpu
def test_edges():
    import torch
    from svx import _lib
    from svx.postprocess.flat_index import FlatIndex
    k, d = 16, 96
    counts = [(70, 40), (0, 20), (5, 0), (64, 33)]
    q, db, q_off, db_off, sims = gr.lattice_groups(counts, d, k, 31, "shuffled")
    want = gr.search_groups_exact(sims, k, db_off)
    idx = make_index(db, "fp16")
    ctx = idx.ctx
    lib = ctx.lib
    qd, rows = device_rows(idx, q), idx.rows
    n = q.shape[0]
    SENT_S, SENT_I = 12345.0, -777
    out_s = torch.full((n, k), SENT_S, dtype=torch.float32, device="cuda")
    out_i = torch.full((n, k), SENT_I, dtype=torch.int64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    arr = lambda a: np.ascontiguousarray(a, np.int64)

    def call(h=ctx.h, qq=p(qd), q_dtype=_lib.SVX_F32, dbp=p(rows), db_dtype=_lib.SVX_F16, dd=d, kk=k, qo=q_off, do=db_off, ng=None,
             s=p(out_s), i=p(out_i)):
        qo_p = None if qo is None else ctypes.c_void_p(qo.ctypes.data)
        do_p = None if do is None else ctypes.c_void_p(do.ctypes.data)
        ng = (len(qo) - 1 if qo is not None else 1) if ng is None else ng
        return lib.svx_knn_search_groups(h, qq, q_dtype, dbp, db_dtype, dd, kk, qo_p, do_p, ng, s, i)

    dec = arr([0, 70, 60, 75, 139])
    errors = (
        (dict(kk=0), "supported 1..64"), (dict(kk=65), "supported 1..64"), (dict(dd=40), "multiple of 32"), (dict(dd=1056), "multiple of 32"),
        (dict(dd=0), "multiple of 32"), (dict(db_dtype=_lib.SVX_F32), "fp16 or bf16"), (dict(q_dtype=7), "unknown query dtype"),
        (dict(qq=None), "null"), (dict(dbp=None), "null"), (dict(s=None), "null"), (dict(i=None), "null"),
        (dict(qo=None), "null"), (dict(do=None), "null"),
        (dict(qo=arr(q_off + 1)), "not at 0"), (dict(do=arr(db_off + 1)), "not at 0"),
        (dict(qo=dec), "decrease"), (dict(do=arr([0, 40, 30, 60, 93])), "decrease"),
        (dict(ng=-1), "negative n_groups"),
        (dict(qo=arr([0, 1 << 37]), do=arr([0, 93])), "2^31 or more workgroups"),
    )
    for bad, text in errors:
        assert call(**bad) == _lib.SVX_ERR_ARG, bad
        msg = lib.svx_last_error(ctx.h).decode()
        assert text in msg, (bad, msg)
    assert call(h=None) == _lib.SVX_ERR_ARG and "NULL" in lib.svx_last_error(None).decode()
    ctx.sync()
    # nothing was queued: the outputs are untouched
    assert bool((out_s == SENT_S).all()) and bool((out_i == SENT_I).all())
    # n_groups = 0 and all-empty groups are legal and write nothing
    zero = arr([0])
    assert call(qo=zero, do=zero) == _lib.SVX_OK
    assert call(qo=zero, do=zero, qq=None, dbp=None, s=None, i=None) == _lib.SVX_OK
    assert call(qo=arr([0, 0, 0]), do=arr([0, 0, 0])) == _lib.SVX_OK
    assert call(qo=arr([0, 0, 0]), do=arr([0, 50, 93])) == _lib.SVX_OK
    ctx.sync()
    assert bool((out_s == SENT_S).all()) and bool((out_i == SENT_I).all())
    # the offsets are copied before the call returns: the caller may overwrite them at once
    qo, do = q_off.copy(), db_off.copy()
    assert call(qo=qo, do=do) == _lib.SVX_OK
    qo[:] = -5
    do[:] = 1 << 40
    ctx.sync()
    assert not exact_fails("C ABI", (out_s.cpu().numpy(), out_i.cpu().numpy()), want)
    blocks = sum((c[0] + 63) // 64 for c in counts)
    assert lib.svx_scratch_bytes(ctx.h) >= 2 * 8 * (len(counts) + 1) + 8 * blocks   # the scratch is counted
    # queries without any database row: all (-inf, -1)
    D, I = FlatIndex(d=d, storage="fp16").search_groups(qd[:70], k, [0, 30, 70], [0, 0, 0])
    assert np.isneginf(host((D, I))[0]).all() and (host((D, I))[1] == -1).all()
    # a zero query ties everywhere: the lowest ids of its group win
    qz = qd.clone()
    qz[3] = 0
    D, I = idx.search_groups(qz, k, q_off, db_off)
    assert not host((D, I))[0][3].any() and np.array_equal(host((D, I))[1][3], np.arange(k))
    D, I = idx.search_groups(qz[70:], k, q_off[1:] - 70, db_off[1:] - 40)   # (other ranges of the same index)
    assert tuple(D.shape) == (69, k)
    # no queries
    D0, I0 = idx.search_groups(qd[:0], k, [0], [0])
    assert tuple(D0.shape) == tuple(I0.shape) == (0, k) and I0.dtype == torch.int64
    # the Python mirror
    for bad_q, bad_db, text in ((q_off[:-1], db_off[:-1], "q_off ends at"), (q_off, db_off + 1, "the index holds"), (q_off, db_off[:-1], "entries"),
                                (q_off.astype(np.float32), db_off, "integers"), (q_off.reshape(1, -1), db_off, "vector")):
        with pytest.raises(ValueError, match=text):
            idx.search_groups(qd, k, bad_q, bad_db)
    with pytest.raises(_lib.SvxError, match="decrease"):
        idx.search_groups(qd, k, dec, db_off)
    with pytest.raises(_lib.SvxError, match=r"supported 1\.\.64"):
        idx.search_groups(qd, 65, q_off, db_off)
    with pytest.raises(ValueError, match="unit rows"):
        FlatIndex.over(qd)
